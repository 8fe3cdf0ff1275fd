// shard_utf8.h — the shard map of an id given as UTF-8: abs(MurmurHash3.stringHash(s) % n) of the string the JVM sees after
// new String(bytes, UTF_8), without the string ever being built.  One routine for both compilers: the host export
// (shard_utf8.cpp, built by any C++17 compiler) and the device kernel (shard_utf8.hip) include this file and nothing else.
//
// The bytes are transcoded to UTF-16 code units on the fly — a code point below 0x10000 is one unit, any other the surrogate
// pair 0xD800 + ((cp - 0x10000) >> 10), 0xDC00 + ((cp - 0x10000) & 0x3FF) — and the units are hashed exactly as K4
// (state_kernels.hip) hashes them: seed 0xf7ca7fd2, pairs (u[k] << 16) + u[k + 1], a last odd unit alone, the length mixed in
// is the number of UNITS, the finaliser, the truncated % and abs.
//
// Only well-formed UTF-8 is hashed (the Unicode table of well-formed byte sequences; what a strict decoder accepts):
//   00..7F | C2..DF 80..BF | E0 A0..BF 80..BF | E1..EC 80..BF 80..BF | ED 80..9F 80..BF | EE..EF 80..BF 80..BF |
//   F0 90..BF 80..BF 80..BF | F1..F3 80..BF x 3 | F4 80..8F 80..BF 80..BF
// Anything else in the hashed span — a lone continuation byte, an over-long form, an encoded surrogate, a value above
// U+10FFFF, F5..FF, a sequence cut by the span's end — makes the id MALFORMED: the result is -1.  (The JVM would substitute
// U+FFFD; which bytes one substitution covers cannot be pinned without a JVM, so such ids are refused, not guessed.)
//
// CUT = true: the hashed span ends in front of the first byte 0x3A (PartitionStringUpToColon.partitionBy; ':' is never part
// of a multi-byte sequence).  The bytes behind it are neither hashed nor validated — the JVM's cut discards them too.
//
// s[i] is read for 0 <= i < len only: a sequence the end of the id cuts is malformed before its missing bytes are looked for.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SURGE_SHARD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SURGE_SHARD_HD inline
#endif

namespace surge {

SURGE_SHARD_HD uint32_t shard_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

SURGE_SHARD_HD uint32_t shard_mix_k(uint32_t d) {
  d *= 0xcc9e2d51u;
  d = shard_rotl(d, 15);
  return d * 0x1b873593u;
}

// The running hash of a stream of UTF-16 units: `pend` holds the first unit of a pair until its second one arrives.
struct ShardUnits {
  uint32_t h = 0xf7ca7fd2u;
  uint32_t pend = 0;
  uint32_t units = 0;

  SURGE_SHARD_HD void put(uint32_t u) {
    if (units & 1u) {
      h ^= shard_mix_k((pend << 16) + u);
      h = shard_rotl(h, 13);
      h = h * 5u + 0xe6546b64u;
    } else {
      pend = u;
    }
    ++units;
  }

  SURGE_SHARD_HD int32_t partition(int32_t n_partitions) const {
    uint32_t x = h;
    if (units & 1u) x ^= shard_mix_k(pend);
    x ^= units;
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    const int32_t r = (int32_t)x % n_partitions;  // truncated, like the JVM
    return r < 0 ? -r : r;
  }
};

// P: anything indexable that yields bytes (const uint8_t* into host memory, global memory or LDS).  n_partitions > 0.
template <bool CUT, class P>
SURGE_SHARD_HD int32_t shard_partition_utf8(P s, int64_t len, int32_t n_partitions) {
  ShardUnits acc;
  int64_t i = 0;
  while (i < len) {
    const uint32_t c = (uint8_t)s[i];
    if (CUT && c == 0x3Au) break;
    if (c < 0x80u) {
      acc.put(c);
      ++i;
      continue;
    }
    int follow;
    uint32_t cp, lo = 0x80u, hi = 0xBFu;  // the range of the FIRST following byte; every later one is 80..BF
    if (c >= 0xC2u && c <= 0xDFu) {
      follow = 1;
      cp = c & 0x1Fu;
    } else if ((c & 0xF0u) == 0xE0u) {
      follow = 2;
      cp = c & 0x0Fu;
      if (c == 0xE0u) lo = 0xA0u;  // no over-long form
      if (c == 0xEDu) hi = 0x9Fu;  // no encoded surrogate
    } else if (c >= 0xF0u && c <= 0xF4u) {
      follow = 3;
      cp = c & 0x07u;
      if (c == 0xF0u) lo = 0x90u;  // no over-long form
      if (c == 0xF4u) hi = 0x8Fu;  // nothing above U+10FFFF
    } else {
      return -1;  // 80..BF alone, C0, C1, F5..FF
    }
    if (len - i <= follow) return -1;  // cut by the id's end: the next id's bytes never complete it
    uint32_t b = (uint8_t)s[i + 1];
    if (b < lo || b > hi) return -1;
    cp = (cp << 6) | (b & 0x3Fu);
    for (int k = 2; k <= follow; ++k) {
      b = (uint8_t)s[i + k];
      if (b < 0x80u || b > 0xBFu) return -1;
      cp = (cp << 6) | (b & 0x3Fu);
    }
    i += follow + 1;
    if (cp < 0x10000u) {
      acc.put(cp);
    } else {
      cp -= 0x10000u;
      acc.put(0xD800u + (cp >> 10));
      acc.put(0xDC00u + (cp & 0x3FFu));
    }
  }
  return acc.partition(n_partitions);
}

}  // namespace surge
