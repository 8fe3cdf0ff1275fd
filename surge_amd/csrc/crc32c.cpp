// crc32c.cpp — CRC-32C (Castagnoli), the checksum of a Kafka record batch: surge_crc32c and surge_crc32c_portable
// (include/surge_ingest.h).  The host framer (ingest.cpp) and the snapshot writer reach it through those two exports; nothing
// else needs the tables or the instruction path.
#include <cstdint>
#include <cstring>

#include "../../include/surge_ingest.h"

namespace {

struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;  // Castagnoli, reflected
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xff];
  }
};

const CrcTables& crc_tables() {
  static const CrcTables tables;  // initialised once, thread-safe (one decoder per partition thread)
  return tables;
}

#if defined(__x86_64__)
// The CRC32 instruction computes exactly this polynomial, 8 bytes per instruction with a latency of 3 cycles and a
// throughput of one per cycle: ONE dependent chain leaves two thirds of the unit idle (4.3 GB/s measured).  So a long
// buffer is cut into three equal blocks whose CRCs run interleaved in one loop; block A's register is then advanced
// over the length of B ("crc of A followed by |B| zero bytes", a linear map applied through four 256-entry tables built
// once from the byte table) and xor-ed into B's, likewise into C's — the classic three-way scheme of Intel's white paper
// / Mark Adler's crc32c.c, restated.
constexpr int64_t kCrcLong = 8192, kCrcShort = 256;

struct CrcShift {
  uint32_t t[4][256];
  // t[k][n]: the register value (n << 8k) after `len` zero bytes
  explicit CrcShift(int64_t len) {
    const CrcTables& T = crc_tables();
    for (int k = 0; k < 4; ++k)
      for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n << (8 * k);
        for (int64_t i = 0; i < len; ++i) c = (c >> 8) ^ T.t[0][c & 0xff];
        t[k][n] = c;
      }
  }
  uint32_t apply(uint32_t c) const { return t[0][c & 0xff] ^ t[1][(c >> 8) & 0xff] ^ t[2][(c >> 16) & 0xff] ^ t[3][c >> 24]; }
};

// three interleaved chains over data[0 .. 3 block), joined; returns the register after all three blocks
__attribute__((target("sse4.2"))) uint64_t crc32c_three_way(uint64_t c0, const uint8_t* data, int64_t block, const CrcShift& sh) {
  uint64_t c1 = 0, c2 = 0;
  const uint8_t* a = data;
  const uint8_t* b = data + block;
  const uint8_t* c = data + 2 * block;
  for (int64_t i = 0; i < block; i += 8) {
    uint64_t va, vb, vc;
    std::memcpy(&va, a + i, 8);
    std::memcpy(&vb, b + i, 8);
    std::memcpy(&vc, c + i, 8);
    c0 = __builtin_ia32_crc32di(c0, va);
    c1 = __builtin_ia32_crc32di(c1, vb);
    c2 = __builtin_ia32_crc32di(c2, vc);
  }
  c0 = sh.apply((uint32_t)c0) ^ c1;
  c0 = sh.apply((uint32_t)c0) ^ c2;
  return c0;
}

__attribute__((target("sse4.2"))) uint32_t crc32c_hw(const uint8_t* data, int64_t len) {
  static const CrcShift shift_long(kCrcLong), shift_short(kCrcShort);
  uint64_t c0 = 0xffffffffu;
  for (; len >= 3 * kCrcLong; data += 3 * kCrcLong, len -= 3 * kCrcLong) c0 = crc32c_three_way(c0, data, kCrcLong, shift_long);
  for (; len >= 3 * kCrcShort; data += 3 * kCrcShort, len -= 3 * kCrcShort) c0 = crc32c_three_way(c0, data, kCrcShort, shift_short);
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t v;
    std::memcpy(&v, data + i, 8);
    c0 = __builtin_ia32_crc32di(c0, v);
  }
  uint32_t c32 = (uint32_t)c0;
  for (; i < len; ++i) c32 = __builtin_ia32_crc32qi(c32, data[i]);
  return c32 ^ 0xffffffffu;
}
#endif

}  // namespace

extern "C" {

uint32_t surge_crc32c(const uint8_t* data, int64_t len) {
#if defined(__x86_64__)
  static const bool have_hw = __builtin_cpu_supports("sse4.2");
  if (have_hw) return crc32c_hw(data, len);
#endif
  const CrcTables& T = crc_tables();
  uint32_t c = 0xffffffffu;
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) {  // slicing-by-8
    const uint32_t lo = c ^ ((uint32_t)data[i] | ((uint32_t)data[i + 1] << 8) | ((uint32_t)data[i + 2] << 16) | ((uint32_t)data[i + 3] << 24));
    c = T.t[7][lo & 0xff] ^ T.t[6][(lo >> 8) & 0xff] ^ T.t[5][(lo >> 16) & 0xff] ^ T.t[4][lo >> 24] ^
        T.t[3][data[i + 4]] ^ T.t[2][data[i + 5]] ^ T.t[1][data[i + 6]] ^ T.t[0][data[i + 7]];
  }
  for (; i < len; ++i) c = (c >> 8) ^ T.t[0][(c ^ data[i]) & 0xff];
  return c ^ 0xffffffffu;
}

/* table walk only (tests compare it with the instruction path) */
uint32_t surge_crc32c_portable(const uint8_t* data, int64_t len) {
  const CrcTables& T = crc_tables();
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < len; ++i) c = (c >> 8) ^ T.t[0][(c ^ data[i]) & 0xff];
  return c ^ 0xffffffffu;
}

}  // extern "C"
