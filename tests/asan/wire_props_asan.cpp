// wire_props_asan.cpp — the forwarded-proposal rule of etcd_amd/csrc/hipbatch_wire_in.h on the
// host under AddressSanitizer + UBSan (tests/test_wire_props.py builds and runs it).
//
// Reads tests/golden/wire_in/wire_props_vectors.npz (tests/golden/make_wire_props_vectors.py:
// one MsgProp per rule of hb_decode_follow's HB_WIRE_PROPS_IN contract, on both sides of
// each).  Every record is parsed from a heap buffer of exactly its length (one byte more
// and ASan aborts).  An accepted vector must give its sender, entry count and entries,
// through wi_message(props) and through the second walk hb_decode_follow makes (wi_header,
// then wi_prop_entry per entry); any other vector must be refused.  Every truncation of the
// accepted records (the long one's first 200 bytes) must be refused too, without a read
// past the buffer.  Then tests/golden/wire_in/wire_in_vectors.npz: the follower rule is
// unchanged, and the knob does not move a record that is no MsgProp.
//
//   wire_props_asan <wire_props_vectors.npz> <wire_in_vectors.npz>

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

void proposals(const char* path) {
  auto z = read_npz(path);
  for (const char* k : {"accept", "frm", "off", "data", "eoff", "edesc", "epos"})
    if (!z.count(k)) die(std::string("fixture lacks ") + k);
  const auto accept = column<uint8_t>(z["accept"], "|u1", "accept");
  const auto frm = column<uint64_t>(z["frm"], "<u8", "frm");
  const auto off = column<uint64_t>(z["off"], "<u8", "off");
  const auto eoff = column<uint64_t>(z["eoff"], "<u8", "eoff");
  const auto edesc = column<uint32_t>(z["edesc"], "<u4", "edesc");
  const auto epos = column<uint64_t>(z["epos"], "<u8", "epos");
  const std::vector<uint8_t>& D = z["data"].raw;
  const uint64_t n = accept.size();
  if (z["data"].descr != "|u1" || frm.size() != n || off.size() != n + 1 || eoff.size() != n + 1 || off[n] != D.size() ||
      eoff[n] != edesc.size() || epos.size() != edesc.size())
    die("fixture sizes");
  uint64_t taken = 0, refused = 0, cuts = 0, most = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (off[i + 1] < off[i] || off[i + 1] > off[n] || eoff[i + 1] < eoff[i] || eoff[i + 1] > eoff[n]) die("fixture offsets");
    const uint64_t l = off[i + 1] - off[i];
    const std::string at = "proposal vector " + std::to_string(i);
    Heap rec(D.data() + off[i], l);
    hb::WiHeader h;
    hb::WiTail t;
    uint32_t ne = 0;
    const bool ok = hb::wi_message(rec.p, l, &h, &t, &ne, true);
    if (!accept[i]) {
      if (ok) die(at + ": accepted, but a rule refuses it");
      ++refused;
      continue;
    }
    if (!ok) die(at + ": refused");
    ++taken;
    if (h.type != hb::WI_MSG_PROP || h.from != frm[i] || h.term || h.log_term || h.index || t.commit || t.hint || t.reject ||
        ne == 0 || ne != eoff[i + 1] - eoff[i])
      die(at + ": header, tail or entry count");
    // without the knob the record is no follower-class message: its entries carry Index 0, not 1
    hb::WiHeader h0;
    hb::WiTail t0;
    uint32_t ne0 = 0;
    if (hb::wi_message(rec.p, l, &h0, &t0, &ne0, false) || hb::wi_message(rec.p, l, &h0, &t0, &ne0))
      die(at + ": canonical for the follower rule");
    // the second walk: the header, then one wi_prop_entry per entry
    hb::WiHeader h2;
    if (!hb::wi_header(rec.p, l, &h2) || h2.ents != h.ents || !hb::wi_is_prop(h2, true) || hb::wi_is_prop(h2, false))
      die(at + ": wi_header");
    uint64_t p = h2.ents;
    for (uint32_t k = 0; k < ne; ++k) {
      hb::WiEntry e;
      const uint64_t x = eoff[i] + k;
      if (p >= l || rec.p[p] != 0x3a || !hb::wi_prop_entry(rec.p, l, p, &e)) die(at + ": wi_prop_entry");
      if (e.term != 0 || e.desc != edesc[x] || e.data != epos[x]) die(at + ": entry " + std::to_string(k));
      const uint64_t dl = e.desc & hb::WI_ENT_MAX_DATA;
      if ((e.desc >> 30) & 1u) die(at + ": an entry type");
      if (e.data ? e.data + dl > l : dl != 0) die(at + ": Data outside the record");
    }
    hb::WiTail t2;
    if (!hb::wi_tail(rec.p, l, p, &t2) || t2.commit != 0 || t2.hint != 0 || t2.reject) die(at + ": wi_tail after the walk");
    most = ne > most ? ne : most;
    const uint64_t upto = l < 400 ? l : 200;
    for (uint64_t c = 0; c < upto; ++c) {
      Heap cut(rec.p, c);
      uint32_t ne2 = 0;
      if (hb::wi_message(cut.p, c, &h2, &t2, &ne2, true)) die(at + ": accepted when cut to " + std::to_string(c));
      ++cuts;
    }
  }
  if (taken < 6 || refused < 25 || most != 300 || cuts < 200) die("too few proposal vectors");
  std::printf("wire_props: %llu accepted, %llu refused, %llu truncations\n", (unsigned long long)taken,
              (unsigned long long)refused, (unsigned long long)cuts);
}

// The follower rule over its own fixture: the same verdict and values with the knob off and on.
void followers(const char* path) {
  auto z = read_npz(path);
  for (const char* k : {"fields", "off", "data", "eoff"})
    if (!z.count(k)) die(std::string("fixture lacks ") + k);
  const Npy& F = z["fields"];
  if (F.shape.size() != 2 || F.shape[1] != 10) die("fixture shapes");
  const uint64_t n = F.shape[0];
  const auto fields = column<uint64_t>(F, "<u8", "fields");
  const auto off = column<uint64_t>(z["off"], "<u8", "off");
  const auto eoff = column<uint64_t>(z["eoff"], "<u8", "eoff");
  const std::vector<uint8_t>& D = z["data"].raw;
  if (fields.size() != n * 10 || off.size() != n + 1 || eoff.size() != n + 1 || off[n] != D.size()) die("fixture sizes");
  uint64_t canon = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* v = &fields[i * 10];  // type, to, from, term, log_term, index, commit, hint, entries, canon
    if (off[i + 1] < off[i] || off[i + 1] > off[n]) die("fixture offsets");
    const uint64_t l = off[i + 1] - off[i];
    const std::string at = "follower vector " + std::to_string(i);
    Heap rec(D.data() + off[i], l);
    for (int props = 0; props < 2; ++props) {
      hb::WiHeader h;
      hb::WiTail t;
      uint32_t ne = 0;
      const bool ok = hb::wi_message(rec.p, l, &h, &t, &ne, props != 0);
      if (ok != (v[9] != 0)) die(at + ": verdict with props = " + std::to_string(props));
      if (!ok) continue;
      if (h.type != v[0] || h.to != v[1] || h.from != v[2] || h.term != v[3] || h.log_term != v[4] || h.index != v[5] ||
          t.commit != v[6] || t.hint != v[7] || ne != v[8] || ne != eoff[i + 1] - eoff[i])
        die(at + ": header, tail or entry count with props = " + std::to_string(props));
      canon += props;
    }
  }
  if (canon < 5 * 19) die("too few follower vectors");
  std::printf("wire_in unchanged: %llu canonical\n", (unsigned long long)canon);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: wire_props_asan <wire_props_vectors.npz> <wire_in_vectors.npz>");
  proposals(argv[1]);
  followers(argv[2]);
  std::printf("wire_props ok\n");
  return 0;
}
