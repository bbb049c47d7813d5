// wire_out_vote_asan.cpp — the MsgVote records of etcd_amd/csrc/hipbatch_wire_out.h on
// the host under AddressSanitizer + UBSan (tests/test_wire_out_vote.py builds and runs it).
//
// Reads tests/golden/wire_out/wire_out_vote_vectors.npz (the layout of
// wire_out_vectors.npz; written by tests/golden/make_wire_out_vote_vectors.py with
// the bytes of tests/wire_util.gogo_marshal) and checks for every vector that
// wo_size is the expected length and that wo_write writes the expected bytes
// into a heap buffer of exactly wo_size bytes: one byte more and ASan aborts.
//
//   wire_out_vote_asan <path to wire_out_vote_vectors.npz>

// the npz reader of wire_out_asan.cpp (die, Npy, read_npz); its main is not this program's
#define main wire_out_asan_main
#include "wire_out_asan.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 2) die("usage: wire_out_vote_asan <wire_out_vote_vectors.npz>");
  auto z = read_npz(argv[1]);
  if (!z.count("fields") || !z.count("off") || !z.count("data")) die("fixture lacks fields / off / data");
  const Npy &F = z["fields"], &O = z["off"], &D = z["data"];
  if (F.descr != "<u8" || O.descr != "<u8" || D.descr != "|u1") die("fixture dtypes");
  if (F.shape.size() != 2 || F.shape[1] != 9 || O.shape.size() != 1 || O.shape[0] != F.shape[0] + 1) die("fixture shapes");
  const uint64_t n = F.shape[0];
  if (F.raw.size() != n * 72 || O.raw.size() != (n + 1) * 8) die("fixture sizes");
  std::vector<uint64_t> fields(n * 9), off(n + 1);
  std::memcpy(fields.data(), F.raw.data(), F.raw.size());
  std::memcpy(off.data(), O.raw.data(), O.raw.size());
  if (off[n] != D.raw.size()) die("fixture data size");
  if (n < 5 * 19) die("too few vectors");  // five fields x the 19 edges
  const uint32_t top = hb::WO_MIN + 5 * (hb::WO_VARINT_MAX - 1);  // to, from, term, logTerm, index at 10 bytes
  uint32_t lo = ~0u, hi = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* v = &fields[i * 9];
    if (v[0] != 5 || v[6] != 0 || v[7] != 0 || v[8] != 0) die("vector " + std::to_string(i) + " is no MsgVote of campaign");
    if (off[i + 1] < off[i] || off[i + 1] > off[n]) die("fixture offsets");
    const uint32_t want = (uint32_t)(off[i + 1] - off[i]);
    const uint32_t sz = hb::wo_size(5, v[1], v[2], v[3], v[4], v[5], 0, false, 0);
    if (sz != want) die("wo_size of vector " + std::to_string(i) + ": " + std::to_string(sz) + ", expected " + std::to_string(want));
    if (sz < hb::WO_MIN || sz > top) die("size outside a MsgVote's bounds");
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(sz));  // exactly sized: ASan guards byte sz
    if (!buf) die("malloc");
    const uint32_t wrote = hb::wo_write(buf, 5, v[1], v[2], v[3], v[4], v[5], 0, false, 0);
    if (wrote != sz) die("wo_write length of vector " + std::to_string(i));
    if (std::memcmp(buf, &D.raw[off[i]], sz) != 0) die("wo_write bytes of vector " + std::to_string(i));
    std::free(buf);
    lo = sz < lo ? sz : lo;
    hi = sz > hi ? sz : hi;
  }
  if (lo != hb::WO_MIN || hi != top) die("the fixture lacks the smallest or the largest MsgVote");
  std::printf("wire_out_vote ok: %llu vectors, %u..%u bytes\n", (unsigned long long)n, lo, hi);
  return 0;
}
