// npz_reader.h — the stored members of an np.savez file, for the stand-alone sanitizer programs
// (no library: a zip's central directory, then each .npy member's header and raw data).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <vector>

namespace {

[[noreturn]] void die(const std::string& what) {
  std::fprintf(stderr, "npz_reader: %s\n", what.c_str());
  std::exit(1);
}

struct Npy {
  std::string descr;
  std::vector<uint64_t> shape;
  std::vector<uint8_t> raw;
};

uint64_t rd(const std::vector<uint8_t>& b, size_t at, int n) {
  if (at + n > b.size()) die("npz truncated");
  uint64_t v = 0;
  for (int i = 0; i < n; ++i) v |= (uint64_t)b[at + i] << (8 * i);
  return v;
}

// A .npy member: magic, version, header dict ('descr', 'shape'), raw data.
Npy parse_npy(const uint8_t* p, size_t n) {
  if (n < 10 || std::memcmp(p, "\x93NUMPY", 6) != 0) die("not an npy member");
  const size_t hl = p[6] == 1 ? (size_t)(p[8] | p[9] << 8) : (size_t)(p[8] | p[9] << 8 | p[10] << 16 | (uint32_t)p[11] << 24);
  const size_t h0 = p[6] == 1 ? 10 : 12;
  if (h0 + hl > n) die("npy header truncated");
  const std::string hdr(reinterpret_cast<const char*>(p + h0), hl);
  Npy a;
  size_t d = hdr.find("'descr'");
  if (d == std::string::npos) die("npy header lacks descr");
  d = hdr.find('\'', d + 7);
  a.descr = hdr.substr(d + 1, hdr.find('\'', d + 1) - d - 1);
  if (hdr.find("'fortran_order': False") == std::string::npos) die("fortran order");
  size_t s = hdr.find("'shape'");
  s = hdr.find('(', s);
  const size_t e = hdr.find(')', s);
  for (size_t i = s + 1; i < e;) {
    while (i < e && (hdr[i] < '0' || hdr[i] > '9')) ++i;
    if (i >= e) break;
    uint64_t v = 0;
    while (i < e && hdr[i] >= '0' && hdr[i] <= '9') v = v * 10 + (uint64_t)(hdr[i++] - '0');
    a.shape.push_back(v);
  }
  a.raw.assign(p + h0 + hl, p + n);
  return a;
}

// The stored (uncompressed) members of a zip, through its central directory.
std::map<std::string, Npy> read_npz(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die("cannot open " + path);
  const std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (b.size() < 22) die("npz too short");
  size_t eocd = b.size() - 22;
  while (rd(b, eocd, 4) != 0x06054b50) {
    if (eocd == 0) die("no end-of-central-directory record");
    --eocd;
  }
  uint64_t count = rd(b, eocd + 10, 2), cd = rd(b, eocd + 16, 4);
  if (cd == 0xFFFFFFFFull || count == 0xFFFF) {  // zip64: the locator sits before the record
    if (eocd < 20 || rd(b, eocd - 20, 4) != 0x07064b50) die("zip64 locator missing");
    const size_t e64 = (size_t)rd(b, eocd - 20 + 8, 8);
    if (rd(b, e64, 4) != 0x06064b50) die("zip64 record missing");
    count = rd(b, e64 + 32, 8);
    cd = rd(b, e64 + 48, 8);
  }
  std::map<std::string, Npy> out;
  size_t at = (size_t)cd;
  for (uint64_t k = 0; k < count; ++k) {
    if (rd(b, at, 4) != 0x02014b50) die("bad central directory entry");
    if (rd(b, at + 10, 2) != 0) die("compressed member (np.savez writes stored ones)");
    uint64_t size = rd(b, at + 24, 4), lho = rd(b, at + 42, 4);
    const size_t nl = (size_t)rd(b, at + 28, 2), xl = (size_t)rd(b, at + 30, 2), cl = (size_t)rd(b, at + 32, 2);
    const uint64_t csize = rd(b, at + 20, 4);
    const std::string name(reinterpret_cast<const char*>(&b[at + 46]), nl);
    for (size_t x = at + 46 + nl; x + 4 <= at + 46 + nl + xl;) {  // zip64 extra: the 0xFFFFFFFF fields, in order
      const uint64_t id = rd(b, x, 2), len = rd(b, x + 2, 2);
      if (id == 1) {
        size_t y = x + 4;
        if (size == 0xFFFFFFFFull) {  // uncompressed size (a stored member: its size in the file)
          size = rd(b, y, 8);
          y += 8;
        }
        if (csize == 0xFFFFFFFFull) y += 8;
        if (lho == 0xFFFFFFFFull) lho = rd(b, y, 8);
      }
      x += 4 + (size_t)len;
    }
    if (rd(b, (size_t)lho, 4) != 0x04034b50) die("bad local header");
    const size_t data = (size_t)lho + 30 + (size_t)rd(b, (size_t)lho + 26, 2) + (size_t)rd(b, (size_t)lho + 28, 2);
    if (data + size > b.size()) die("member past the end");
    std::string key = name;
    if (key.size() > 4 && key.substr(key.size() - 4) == ".npy") key.resize(key.size() - 4);
    out[key] = parse_npy(&b[data], (size_t)size);
    at += 46 + nl + xl + cl;
  }
  return out;
}

}  // namespace
