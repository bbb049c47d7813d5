// wire_out_app_asan.cpp — the split MsgApp records of etcd_amd/csrc/hipbatch_wire_out.h on
// the host under AddressSanitizer + UBSan (tests/test_wire_out_app.py builds and runs it).
//
// Reads tests/golden/wire_out/wire_out_app_vectors.npz (written by
// tests/golden/make_wire_out_app_vectors.py with the bytes of
// tests/wire_util.gogo_marshal, entries included) and checks for every vector
// that wo_size_split is the message's length without its entries, that
// wo_write_split writes into a heap buffer of exactly that size (one byte more
// and ASan aborts), that wo_prefix_len is the expected prefix length, and that
// prefix ‖ entries ‖ suffix is the whole message.
//
//   wire_out_app_asan <path to wire_out_app_vectors.npz>

// the npz reader of wire_out_asan.cpp (die, Npy, read_npz); its main is not this program's
#define main wire_out_asan_main
#include "wire_out_asan.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 2) die("usage: wire_out_app_asan <wire_out_app_vectors.npz>");
  auto z = read_npz(argv[1]);
  for (const char* k : {"fields", "off", "data", "eoff", "edata"})
    if (!z.count(k)) die(std::string("fixture lacks ") + k);
  const Npy &F = z["fields"], &O = z["off"], &D = z["data"], &EO = z["eoff"], &ED = z["edata"];
  if (F.descr != "<u8" || O.descr != "<u8" || EO.descr != "<u8" || D.descr != "|u1" || ED.descr != "|u1") die("fixture dtypes");
  if (F.shape.size() != 2 || F.shape[1] != 8 || O.shape.size() != 1 || O.shape[0] != F.shape[0] + 1 ||
      EO.shape.size() != 1 || EO.shape[0] != O.shape[0])
    die("fixture shapes");
  const uint64_t n = F.shape[0];
  if (F.raw.size() != n * 64 || O.raw.size() != (n + 1) * 8 || EO.raw.size() != (n + 1) * 8) die("fixture sizes");
  std::vector<uint64_t> fields(n * 8), off(n + 1), eoff(n + 1);
  std::memcpy(fields.data(), F.raw.data(), F.raw.size());
  std::memcpy(off.data(), O.raw.data(), O.raw.size());
  std::memcpy(eoff.data(), EO.raw.data(), EO.raw.size());
  if (off[n] != D.raw.size() || eoff[n] != ED.raw.size()) die("fixture data size");
  if (n < 6 * 19) die("too few vectors");  // six fields x the 19 edges
  const uint32_t MSG_APP = 3;
  const uint32_t top = hb::WO_MIN + 6 * (hb::WO_VARINT_MAX - 1);  // all six varints at 10 bytes, RejectHint 0
  uint32_t lo = ~0u, hi = 0, with[4] = {0, 0, 0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* v = &fields[i * 8];  // to, from, term, logTerm, index, commit, entries, prefix
    if (off[i + 1] < off[i] || off[i + 1] > off[n] || eoff[i + 1] < eoff[i] || eoff[i + 1] > eoff[n]) die("fixture offsets");
    const uint64_t full = off[i + 1] - off[i], run = eoff[i + 1] - eoff[i];
    if (v[6] > 3 || (v[6] == 0) != (run == 0) || run > full) die("vector " + std::to_string(i) + ": entries");
    ++with[v[6]];
    const uint32_t sz = hb::wo_size_split(MSG_APP, v[0], v[1], v[2], v[3], v[4], v[5]);
    if (sz != full - run) die("wo_size_split of vector " + std::to_string(i) + ": " + std::to_string(sz));
    if (sz < hb::WO_MIN || sz > top || sz > hb::WO_MAX) die("size outside a record's bounds");
    const uint32_t pre = hb::wo_prefix_len(MSG_APP, v[0], v[1], v[2], v[3], v[4]);
    if (pre != v[7] || pre > hb::WO_PREFIX_MAX || pre >= sz) die("wo_prefix_len of vector " + std::to_string(i));
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(sz));  // exactly sized: ASan guards byte sz
    if (!buf) die("malloc");
    const uint32_t wrote = hb::wo_write_split(buf, MSG_APP, v[0], v[1], v[2], v[3], v[4], v[5]);
    if (wrote != sz) die("wo_write_split length of vector " + std::to_string(i));
    // the same bytes as the payload-free record with Reject = 0 and RejectHint = 0
    uint8_t* ref = static_cast<uint8_t*>(std::malloc(sz));
    if (!ref) die("malloc");
    if (hb::wo_write(ref, MSG_APP, v[0], v[1], v[2], v[3], v[4], v[5], false, 0) != sz || std::memcmp(buf, ref, sz) != 0)
      die("wo_write_split differs from wo_write at vector " + std::to_string(i));
    std::free(ref);
    // prefix ‖ entries ‖ suffix
    std::vector<uint8_t> msg(buf, buf + pre);
    msg.insert(msg.end(), ED.raw.begin() + eoff[i], ED.raw.begin() + eoff[i + 1]);
    msg.insert(msg.end(), buf + pre, buf + sz);
    if (msg.size() != full || std::memcmp(msg.data(), &D.raw[off[i]], full) != 0) die("spliced bytes of vector " + std::to_string(i));
    std::free(buf);
    lo = sz < lo ? sz : lo;
    hi = sz > hi ? sz : hi;
  }
  if (lo != hb::WO_MIN || hi != top) die("the fixture lacks the smallest or the longest record");
  if (!with[0] || !with[1] || !with[3]) die("the fixture lacks 0, 1 or 3 entries");
  std::printf("wire_out_app ok: %llu vectors, %u..%u bytes\n", (unsigned long long)n, lo, hi);
  return 0;
}
