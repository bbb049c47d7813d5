// wire_out_ents_asan.cpp — the entry encoder, the coverage rule and the payload copy plan of
// etcd_amd/csrc/hipbatch_wire_out.h on the host under AddressSanitizer + UBSan
// (tests/test_wire_out_ents.py builds and runs it).
//
// 1. Reads tests/golden/wire_out/wire_out_ents_vectors.npz (written by
//    tests/golden/make_wire_out_ents_vectors.py with the bytes of tests/wire_util._entry and
//    gogo_marshal) and checks wo_entry_size, wo_entry_head_len and wo_entry_head of every entry
//    (the head into a heap buffer of exactly its size), and every whole message: its size from
//    wo_size_split and wo_ents_covered's run, its bytes from wo_write_prefix, the entries (head,
//    then the Data bytes) and wo_write_suffix into a heap buffer of exactly the message's size.
// 2. wo_ents_covered on a table of window and range cases: every boundary of the rule, and
//    that no per-entry word outside [0, n_ent) is read (the arrays are exactly sized).
// 3. wo_copy_lane, lane by lane for 64 emulated lanes, for all 16 x 16 source and destination
//    phases and the lengths 0-80, 4,095-4,097 and 70,000; both buffers end exactly at the last
//    byte (one byte more and ASan aborts), the bytes before the first are checked to be untouched.
//
//   wire_out_ents_asan <path to wire_out_ents_vectors.npz>

// the npz reader of wire_out_asan.cpp (die, Npy, read_npz); its main is not this program's
#define main wire_out_asan_main
#include "wire_out_asan.cpp"
#undef main

namespace {

std::vector<uint64_t> words(const Npy& a) {
  if (a.descr != "<u8" || a.raw.size() % 8) die("fixture dtypes");
  std::vector<uint64_t> v(a.raw.size() / 8);
  std::memcpy(v.data(), a.raw.data(), a.raw.size());
  return v;
}
std::string at(const char* what, uint64_t i) { return std::string(what) + " " + std::to_string(i); }

void check_entries_and_messages(std::map<std::string, Npy>& z) {
  for (const char* k : {"ents", "esize", "hoff", "hdata", "pdata", "msgs", "moff", "mdata"})
    if (!z.count(k)) die(std::string("fixture lacks ") + k);
  const std::vector<uint64_t> ents = words(z["ents"]), esize = words(z["esize"]), hoff = words(z["hoff"]),
                              msgs = words(z["msgs"]), moff = words(z["moff"]);
  const Npy &HD = z["hdata"], &PD = z["pdata"], &MD = z["mdata"];
  if (HD.descr != "|u1" || PD.descr != "|u1" || MD.descr != "|u1") die("fixture dtypes");
  const uint64_t E = esize.size(), M = msgs.size() / 8;
  if (ents.size() != E * 4 || hoff.size() != E + 1 || moff.size() != M + 1 || msgs.size() != M * 8) die("fixture shapes");
  if (hoff[E] != HD.raw.size() || moff[M] != MD.raw.size()) die("fixture data size");
  uint32_t vl_seen = 0, head_max = 0;
  bool type1 = false, nil = false, empty = false;
  for (uint64_t i = 0; i < E; ++i) {
    const uint32_t desc = (uint32_t)ents[i * 4];
    const uint64_t term = ents[i * 4 + 1], index = ents[i * 4 + 2], poff = ents[i * 4 + 3];
    if (ents[i * 4] >> 32) die(at("descriptor of entry", i));
    if (hb::wo_desc_has_data(desc) && poff + hb::wo_desc_len(desc) > PD.raw.size()) die(at("payload of entry", i));
    if (hb::wo_entry_size(desc, term, index) != esize[i]) die(at("wo_entry_size of entry", i));
    const uint64_t hl = hoff[i + 1] - hoff[i];
    if (hb::wo_entry_head_len(desc, term, index) != hl || hl > hb::WO_ENTRY_HEAD_MAX) die(at("wo_entry_head_len of entry", i));
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(hl));  // exactly sized: ASan guards byte hl
    if (!buf) die("malloc");
    if (hb::wo_entry_head(buf, desc, term, index) != hl || std::memcmp(buf, &HD.raw[hoff[i]], hl) != 0)
      die(at("wo_entry_head of entry", i));
    std::free(buf);
    vl_seen |= 1u << hb::wo_varint_len(term) | 1u << hb::wo_varint_len(index);
    head_max = hl > head_max ? (uint32_t)hl : head_max;
    type1 |= hb::wo_desc_type(desc) == 1;
    nil |= !hb::wo_desc_has_data(desc);
    empty |= hb::wo_desc_has_data(desc) && hb::wo_desc_len(desc) == 0;
  }
  if (vl_seen != 0x7FE) die("the fixture lacks a varint length of 1 to 10 bytes");
  if (!type1 || !nil || !empty) die("the fixture lacks Type 1, nil Data or empty Data");
  if (head_max < 1 + 3 + 2 + 10 + 10 + 4) die("the fixture lacks a long head");

  const uint32_t MSG_APP = 3;
  uint64_t most = 0, longest = 0;
  for (uint64_t m = 0; m < M; ++m) {
    const uint64_t* v = &msgs[m * 8];  // to, from, term, logTerm, index, commit, e0, e1
    const uint64_t e0 = v[6], e1 = v[7], n = e1 - e0, full = moff[m + 1] - moff[m];
    if (e0 > e1 || e1 > E) die(at("entry rows of message", m));
    // the window table of one group that holds exactly this message's entries (exactly sized arrays)
    std::vector<uint64_t> eterm(n), edata(n);
    std::vector<uint32_t> edesc(n);
    for (uint64_t k = 0; k < n; ++k) {
      edesc[k] = (uint32_t)ents[(e0 + k) * 4];
      eterm[k] = ents[(e0 + k) * 4 + 1];
      edata[k] = ents[(e0 + k) * 4 + 3];
      if (ents[(e0 + k) * 4 + 2] != v[4] + 1 + k) die(at("entry indices of message", m));
    }
    uint64_t pos = 99, ne = 99, run = 0;
    const bool cov = hb::wo_ents_covered(v[4], v[4] + n, v[4] + 1, (uint32_t)n, 0, n, eterm.data(), edesc.data(),
                                         edata.data(), PD.raw.size(), &pos, &ne, &run);
    if (cov != (n > 0) || (cov && (pos != 0 || ne != n))) die(at("wo_ents_covered of message", m));
    const uint64_t size = hb::wo_size_split(MSG_APP, v[0], v[1], v[2], v[3], v[4], v[5]) + run;
    if (size != full) die(at("size of message", m) + ": " + std::to_string(size) + " expected " + std::to_string(full));
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(size));  // exactly sized
    if (!buf) die("malloc");
    uint64_t i = hb::wo_write_prefix(buf, MSG_APP, v[0], v[1], v[2], v[3], v[4]);
    if (i != hb::wo_prefix_len(MSG_APP, v[0], v[1], v[2], v[3], v[4])) die(at("wo_write_prefix of message", m));
    for (uint64_t k = 0; k < n; ++k) {
      i += hb::wo_entry_head(buf + i, edesc[k], eterm[k], v[4] + 1 + k);
      if (hb::wo_desc_has_data(edesc[k])) {
        // the payload, through the copy plan (one emulated lane after another)
        for (uint32_t lane = 0; lane < 64; ++lane)
          hb::wo_copy_lane(PD.raw.data() + edata[k], buf + i, hb::wo_desc_len(edesc[k]), lane, 64);
        i += hb::wo_desc_len(edesc[k]);
      }
    }
    const uint32_t suf = hb::wo_write_suffix(buf + i, v[5]);
    if (suf > hb::WO_SUFFIX_MAX || i + suf != full) die(at("length of message", m));
    if (std::memcmp(buf, &MD.raw[moff[m]], full) != 0) die(at("bytes of message", m));
    // prefix ‖ suffix is the split record
    uint8_t split[hb::WO_MAX];
    const uint32_t ss = hb::wo_write_split(split, MSG_APP, v[0], v[1], v[2], v[3], v[4], v[5]);
    const uint32_t pre = hb::wo_prefix_len(MSG_APP, v[0], v[1], v[2], v[3], v[4]);
    if (ss != pre + suf || std::memcmp(split, buf, pre) != 0 || std::memcmp(split + pre, buf + i, suf) != 0)
      die(at("prefix and suffix of message", m));
    std::free(buf);
    most = n > most ? n : most;
    longest = full > longest ? full : longest;
  }
  if (most != 300 || longest < 16383 + 16384 + 70000) die("the fixture lacks the 300-entry or the long message");
  std::printf("entries ok: %llu entries, %llu messages\n", (unsigned long long)E, (unsigned long long)M);
}

// one window case: entries (index, hint] against the window (first, count, start) of arrays of n_ent elements
struct CovCase {
  const char* name;
  uint64_t index, hint, first;
  uint32_t count;
  uint64_t start, n_ent;
  int64_t edata_delta;  // added to the last carried entry's edata (payloads end at data_len exactly)
  bool want;
};
void check_coverage() {
  const uint64_t N = 12, LEN = 16, DL = N * LEN, U = ~0ull;
  const CovCase cases[] = {
      {"exact fit", 10, 13, 11, 3, 4, N, 0, true},
      {"inside a longer window", 10, 12, 9, 6, 2, N, 0, true},
      {"one entry", 10, 11, 11, 1, 0, N, 0, true},
      {"count 0", 10, 11, 11, 0, 0, N, 0, false},
      {"hint == index", 10, 10, 11, 3, 0, N, 0, false},
      {"hint < index", 10, 9, 5, 8, 0, N, 0, false},
      {"window starts at index + 2", 10, 13, 12, 3, 0, N, 0, false},
      {"window starts at index + 1", 10, 13, 11, 3, 0, N, 0, true},
      {"window ends at hint - 1", 10, 13, 11, 2, 0, N, 0, false},
      {"window ends at hint - 1 (skip)", 10, 13, 9, 4, 0, N, 0, false},
      {"window ends at hint (skip)", 10, 13, 9, 5, 0, N, 0, true},
      {"start + count == n_ent", 10, 13, 11, 3, N - 3, N, 0, true},
      {"start + count == n_ent + 1", 10, 13, 11, 3, N - 2, N, 0, false},
      {"start past n_ent", 10, 11, 11, 1, N + 5, N, 0, false},
      {"start near 2^64", 10, 11, 11, 1, U, N, 0, false},
      {"n_ent 0", 10, 11, 11, 1, 0, 0, 0, false},
      {"edata + len == data_len", 10, 13, 11, 3, N - 3, N, 0, true},
      {"edata + len == data_len + 1", 10, 13, 11, 3, N - 3, N, 1, false},
      {"edata past data_len", 10, 13, 11, 3, N - 3, N, 1000, false},
      {"edata near 2^64", 10, 13, 11, 3, N - 3, N, -(int64_t)(DL - LEN) - 1, false},
      {"index 2^64 - 2", U - 1, U, U, 1, 0, N, 0, true},
      {"index 2^64 - 1", U, U, 0, 12, 0, N, 0, false},
      {"first 0, index 0", 0, 12, 0, 12, 0, N, 0, false},
      {"first 1, index 0", 0, 12, 1, 12, 0, N, 0, true},
      {"range wider than any count", 0, U, 1, 0xFFFFFFFFu, 0, N, 0, false},
  };
  for (const CovCase& c : cases) {
    // exactly sized arrays: a read outside [0, n_ent) aborts under ASan
    uint64_t* eterm = static_cast<uint64_t*>(std::malloc(c.n_ent ? c.n_ent * 8 : 1));
    uint64_t* edata = static_cast<uint64_t*>(std::malloc(c.n_ent ? c.n_ent * 8 : 1));
    uint32_t* edesc = static_cast<uint32_t*>(std::malloc(c.n_ent ? c.n_ent * 4 : 1));
    if (!eterm || !edata || !edesc) die("malloc");
    for (uint64_t k = 0; k < c.n_ent; ++k) {
      eterm[k] = 5;
      edesc[k] = (uint32_t)LEN | 0x80000000u;
      edata[k] = k * LEN;  // entry k's payload: the last one ends at data_len
    }
    uint64_t pos = 0, ne = 0, run = 0;
    if (c.edata_delta && hb::wo_ents_window(c.index, c.hint, c.first, c.count, c.start, c.n_ent, &pos, &ne))
      edata[pos + ne - 1] += (uint64_t)c.edata_delta;
    pos = ne = run = 0;
    const bool got = hb::wo_ents_covered(c.index, c.hint, c.first, c.count, c.start, c.n_ent, eterm, edesc, edata, DL,
                                         &pos, &ne, &run);
    if (got != c.want) die(std::string("coverage case: ") + c.name);
    if (got) {
      if (pos != c.start + (c.index + 1 - c.first) || ne != c.hint - c.index) die(std::string("coverage position: ") + c.name);
      uint64_t want_run = 0;
      for (uint64_t k = 0; k < ne; ++k) {
        const uint64_t es = hb::wo_entry_size(edesc[pos + k], 5, c.index + 1 + k);
        want_run += 1 + hb::wo_varint_len(es) + es;
      }
      if (run != want_run) die(std::string("coverage run: ") + c.name);
    }
    std::free(eterm);
    std::free(edata);
    std::free(edesc);
  }
  // entries without Data: edata is not looked at
  uint64_t eterm[2] = {1, 1}, edata[2] = {~0ull, ~0ull}, pos, ne, run;
  uint32_t edesc[2] = {0, 0x40000000u};
  if (!hb::wo_ents_covered(7, 9, 8, 2, 0, 2, eterm, edesc, edata, 0, &pos, &ne, &run) || run != 2 * (2 + 6))
    die("coverage: entries without Data");
  std::printf("coverage ok: %zu cases\n", sizeof(cases) / sizeof(cases[0]));
}

void check_copy_plan() {
  std::vector<uint64_t> lens;
  for (uint64_t l = 0; l <= 80; ++l) lens.push_back(l);
  for (uint64_t l : {4095ull, 4096ull, 4097ull, 70000ull}) lens.push_back(l);
  uint64_t cases = 0;
  uint32_t widths = 0;
  for (uint64_t len : lens)
    for (uint32_t sp = 0; sp < 16; ++sp)
      for (uint32_t dp = 0; dp < 16; ++dp) {
        // 16-byte aligned blocks that end exactly at the last byte; phase = the bytes skipped in front
        void *sv = nullptr, *dv = nullptr;
        if (posix_memalign(&sv, 16, sp + len + (sp + len == 0)) || posix_memalign(&dv, 16, dp + len + (dp + len == 0))) die("memalign");
        uint8_t *sb = static_cast<uint8_t*>(sv), *db = static_cast<uint8_t*>(dv);
        for (uint64_t i = 0; i < sp + len; ++i) sb[i] = (uint8_t)(i * 7 + sp + 1);
        for (uint64_t i = 0; i < dp + len; ++i) db[i] = 0xEE;
        const uint8_t* src = sb + sp;
        uint8_t* dst = db + dp;
        const hb::wo_chunk_plan p = hb::wo_plan_copy(reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst), len);
        if (p.head + p.body * hb::WO_CHUNK + p.tail != len || p.head >= hb::WO_CHUNK || p.tail >= hb::WO_CHUNK) die("plan sums");
        const uint32_t diff = (sp - dp) & 15;
        const uint32_t want_w = diff == 0 ? 16 : (diff & (~diff + 1));
        if (p.width != want_w) die("plan width");
        if (p.body && ((reinterpret_cast<uintptr_t>(src) + p.head) % p.width || (reinterpret_cast<uintptr_t>(dst) + p.head) % hb::WO_CHUNK))
          die("plan alignment");
        widths |= p.width;
        for (uint32_t lane = 0; lane < 64; ++lane) hb::wo_copy_lane(src, dst, len, lane, 64);
        if (len && std::memcmp(src, dst, len) != 0) die("copied bytes");
        for (uint32_t i = 0; i < dp; ++i)
          if (db[i] != 0xEE) die("a byte before the destination was written");
        std::free(sv);
        std::free(dv);
        ++cases;
      }
  if (widths != 31) die("not every chunk width was planned");
  std::printf("copy plan ok: %llu cases\n", (unsigned long long)cases);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: wire_out_ents_asan <wire_out_ents_vectors.npz>");
  auto z = read_npz(argv[1]);
  check_entries_and_messages(z);
  check_coverage();
  check_copy_plan();
  std::printf("wire_out_ents ok\n");
  return 0;
}
