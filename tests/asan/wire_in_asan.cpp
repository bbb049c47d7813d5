// wire_in_asan.cpp — the canonical-shape parser of etcd_amd/csrc/hipbatch_wire_in.h on the
// host under AddressSanitizer + UBSan (tests/test_wire_in.py builds and runs it).
//
// Reads tests/golden/wire_in/wire_in_vectors.npz (written by
// tests/golden/make_wire_in_vectors.py with the bytes of tests/wire_util.gogo_marshal).
// Every record is parsed from a heap buffer of exactly its length (one byte more and
// ASan aborts).  A canonical vector must give its generating header, tail and
// entries, through wi_message and through the second walk hb_decode_follow makes
// (wi_header, then wi_entry per entry); a vector marked not canonical must be
// refused.  Every truncation of the first dozen canonical records (and of the
// long ones' first 200 bytes) must be refused too, without a read past the buffer.
//
//   wire_in_asan <path to wire_in_vectors.npz>

#include "npz_reader.h"  // die, Npy, read_npz

#include "../../etcd_amd/csrc/hipbatch_wire_in.h"

namespace {

struct Heap {  // exactly n bytes on the heap (n = 0: a one-byte block nobody may read)
  uint8_t* p;
  Heap(const uint8_t* src, size_t n) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))) {
    if (!p) die("malloc");
    if (n) std::memcpy(p, src, n);
  }
  ~Heap() { std::free(p); }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
};

template <class T>
std::vector<T> column(const Npy& a, const char* descr, const char* name) {
  if (a.descr != descr || a.raw.size() % sizeof(T)) die(std::string("fixture dtype of ") + name);
  std::vector<T> v(a.raw.size() / sizeof(T));
  if (!v.empty()) std::memcpy(v.data(), a.raw.data(), a.raw.size());
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: wire_in_asan <wire_in_vectors.npz>");
  auto z = read_npz(argv[1]);
  for (const char* k : {"fields", "off", "data", "eoff", "eterm", "edesc", "epos"})
    if (!z.count(k)) die(std::string("fixture lacks ") + k);
  const Npy& F = z["fields"];
  if (F.shape.size() != 2 || F.shape[1] != 10) die("fixture shapes");
  const uint64_t n = F.shape[0];
  const auto fields = column<uint64_t>(F, "<u8", "fields");
  const auto off = column<uint64_t>(z["off"], "<u8", "off");
  const auto eoff = column<uint64_t>(z["eoff"], "<u8", "eoff");
  const auto eterm = column<uint64_t>(z["eterm"], "<u8", "eterm");
  const auto edesc = column<uint32_t>(z["edesc"], "<u4", "edesc");
  const auto epos = column<uint64_t>(z["epos"], "<u8", "epos");
  const std::vector<uint8_t>& D = z["data"].raw;
  if (z["data"].descr != "|u1" || fields.size() != n * 10 || off.size() != n + 1 || eoff.size() != n + 1 ||
      off[n] != D.size() || eoff[n] != eterm.size() || edesc.size() != eterm.size() || epos.size() != eterm.size())
    die("fixture sizes");
  uint64_t canon = 0, refused = 0, cuts = 0, most = 0, longest = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* v = &fields[i * 10];  // type, to, from, term, log_term, index, commit, hint, entries, canon
    if (off[i + 1] < off[i] || off[i + 1] > off[n] || eoff[i + 1] < eoff[i] || eoff[i + 1] > eoff[n]) die("fixture offsets");
    const uint64_t l = off[i + 1] - off[i];
    const std::string at = "vector " + std::to_string(i);
    Heap rec(D.data() + off[i], l);
    hb::WiHeader h;
    hb::WiTail t;
    uint32_t ne = 0;
    const bool ok = hb::wi_message(rec.p, l, &h, &t, &ne);
    if (!v[9]) {
      if (ok) die(at + ": accepted, but it is not canonical");
      ++refused;
      continue;
    }
    if (!ok) die(at + ": refused");
    ++canon;
    if (h.type != v[0] || h.to != v[1] || h.from != v[2] || h.term != v[3] || h.log_term != v[4] || h.index != v[5] ||
        t.commit != v[6] || t.hint != v[7] || ne != v[8] || ne != eoff[i + 1] - eoff[i])
      die(at + ": header, tail or entry count");
    // the second walk: the header, then one wi_entry per entry
    hb::WiHeader h2;
    if (!hb::wi_header(rec.p, l, &h2) || h2.ents != h.ents || h2.index != h.index) die(at + ": wi_header");
    uint64_t p = h2.ents;
    for (uint32_t k = 0; k < ne; ++k) {
      hb::WiEntry e;
      const uint64_t x = eoff[i] + k;
      if (p >= l || rec.p[p] != 0x3a || !hb::wi_entry(rec.p, l, p, h.index + 1 + k, &e)) die(at + ": wi_entry");
      if (e.term != eterm[x] || e.desc != edesc[x] || e.data != epos[x]) die(at + ": entry " + std::to_string(k));
      const uint64_t dl = e.desc & hb::WI_ENT_MAX_DATA;
      if (e.data ? e.data + dl > l : dl != 0) die(at + ": Data outside the record");
      longest = dl > longest ? dl : longest;
    }
    hb::WiTail t2;
    if (!hb::wi_tail(rec.p, l, p, &t2) || t2.commit != t.commit || t2.hint != t.hint || t2.reject != t.reject)
      die(at + ": wi_tail after the walk");
    most = ne > most ? ne : most;
    // truncations: the first dozen canonical records at every length, the others' first 200 bytes
    const uint64_t upto = canon <= 12 ? l : (l < 200 ? l : 200);
    for (uint64_t c = 0; c < upto; ++c) {
      Heap cut(rec.p, c);
      uint32_t ne2 = 0;
      if (hb::wi_message(cut.p, c, &h2, &t2, &ne2)) die(at + ": accepted when cut to " + std::to_string(c));
      ++cuts;
    }
  }
  if (canon < 5 * 19 || refused < 10) die("too few vectors");
  if (most != 300 || longest != 70000) die("the fixture lacks the 300-entry record or the 70,000-byte payload");
  std::printf("wire_in ok: %llu canonical, %llu refused, %llu truncations\n", (unsigned long long)canon,
              (unsigned long long)refused, (unsigned long long)cuts);
  return 0;
}
