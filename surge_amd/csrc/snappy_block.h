// snappy_block.h — the snappy formats a Kafka records section may be written in, once, for the host and the device: the raw
// block (format_description.txt of the snappy project) and the framing kafka-clients puts around blocks (snappy-java's
// SnappyOutputStream).  Header only and inline throughout: the host framer (ingest.cpp, ingest_group.cpp) decompresses
// through it without a call into another translation unit, snappy_frame.cpp wraps it for the C exports, ingest_snappy.hip
// plans sections with walk_chunks and its parse kernel decodes elements with header_bytes / element.
//
// A raw block: the uncompressed length as a little-endian base-128 varint (1 - 5 bytes, at most 2^32 - 1; an over-long
// spelling such as 80 00 is read, as the reference decoder reads it), then elements, each begun by a tag byte whose low two
// bits name its kind:
//   0  literal    length - 1 in the tag's upper six bits when below 60; 60 .. 63: in the 1 .. 4 bytes that follow
//                 (little-endian); then the bytes themselves
//   1  copy-1     length 4 .. 11 (tag bits 2 - 4), offset 0 .. 2047 (tag bits 5 - 7, then one byte)
//   2  copy-2     length 1 .. 64 (upper six bits), offset in two bytes, little-endian
//   3  copy-4     length 1 .. 64, offset in four bytes
// A copy repeats `length` bytes from `offset` bytes back in the output; offset < length repeats a period.
//
// The framing: 8 magic bytes 82 53 4E 41 50 50 59 00, two big-endian int32 (version, compatible version: 1, 1), then chunks
// [int32 BE compressed length][raw block] until the section ends, each holding at most the writer's block size (32 KiB by
// default) of output.  A section that does not begin with the magic is ONE raw block — what clients other than the Java one
// write, and what SnappyInputStream accepts.
//
// The decoder never reads at or beyond src + len and never writes beyond the capacity it is given; what does not decode is
// refused with a status that names the reason, never wrapped or guessed at.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SURGE_SNAPPY_HD __host__ __device__
#else
#define SURGE_SNAPPY_HD
#endif

namespace surge {
namespace snappy {

enum Status : int32_t {
  SN_OK = 0,
  SN_NO_SPACE = 1,             // the output does not fit the capacity given: nothing wrong with the input
  SN_PREAMBLE_TRUNCATED = 2,   // the length varint runs past the input
  SN_PREAMBLE_TOO_LARGE = 3,   // ... spells more than 2^32 - 1, or does not end within 5 bytes
  SN_TAG_PAST_INPUT = 4,       // a tag's extension or offset bytes run past the input
  SN_LITERAL_PAST_INPUT = 5,   // a literal's bytes run past the input
  SN_OFFSET_ZERO = 6,
  SN_OFFSET_BEYOND_OUTPUT = 7, // a copy reaches in front of the bytes produced so far in its block
  SN_OUTPUT_BEYOND_PREAMBLE = 8,
  SN_OUTPUT_SHORT = 9,         // the elements end before the preamble's length is reached
  SN_CHUNK_NEGATIVE = 10,      // framing: a chunk's length word is negative
  SN_CHUNK_PAST_INPUT = 11,    // ... or larger than what is left of the section
  SN_VERSION = 12,             // ... the header is cut short or names a version pair other than 1, 1
  SN_TRAILING_BYTES = 13,      // ... bytes behind the last chunk that hold no whole length word
  SN_TOO_LARGE = 14,           // a section that expands beyond 2 GiB
  SN_STATUS_COUNT
};

inline const char* status_name(int32_t s) {
  switch (s) {
    case SN_OK: return "ok";
    case SN_NO_SPACE: return "snappy: the output does not fit the space given";
    case SN_PREAMBLE_TRUNCATED: return "bad snappy block in record batch: the uncompressed-length varint runs past the input";
    case SN_PREAMBLE_TOO_LARGE: return "bad snappy block in record batch: the uncompressed-length varint spells more than 2^32 - 1";
    case SN_TAG_PAST_INPUT: return "bad snappy block in record batch: a tag's extension or offset bytes run past the input";
    case SN_LITERAL_PAST_INPUT: return "bad snappy block in record batch: a literal runs past the input";
    case SN_OFFSET_ZERO: return "bad snappy block in record batch: a copy with offset 0";
    case SN_OFFSET_BEYOND_OUTPUT: return "bad snappy block in record batch: a copy reaches in front of the block's output";
    case SN_OUTPUT_BEYOND_PREAMBLE: return "bad snappy block in record batch: more output than the block's preamble names";
    case SN_OUTPUT_SHORT: return "bad snappy block in record batch: less output than the block's preamble names";
    case SN_CHUNK_NEGATIVE: return "bad snappy framing in record batch: negative chunk length";
    case SN_CHUNK_PAST_INPUT: return "bad snappy framing in record batch: a chunk runs past the section";
    case SN_VERSION: return "bad snappy framing in record batch: header cut short or unknown version pair";
    case SN_TRAILING_BYTES: return "bad snappy framing in record batch: trailing bytes that form no whole chunk";
    case SN_TOO_LARGE: return "snappy batch expands beyond 2 GiB";
    default: return "snappy: unknown status";
  }
}

// ---- the element grammar (host and device) ----------------------------------------------------------------------------------
struct Element {
  uint32_t header;  // bytes of the tag with its extension / offset bytes: 1 .. 5
  uint32_t n1;      // length - 1 (a literal with a 4-byte extension may spell 2^32 - 1 here: compare, never add 1 in 32 bits)
  uint32_t offset;  // of a copy
  bool copy;
};

// bytes a tag occupies with what follows it in front of any literal bytes: known from the tag alone
SURGE_SNAPPY_HD inline uint32_t header_bytes(uint32_t tag) {
  const uint32_t kind = tag & 3u, n = tag >> 2;
  return kind == 0u ? (n < 60u ? 1u : n - 58u) : kind == 1u ? 2u : kind == 2u ? 3u : 5u;
}

// the element a tag begins; `ext`: the four bytes behind the tag, little-endian — only header_bytes(tag) - 1 of them are
// looked at, so bytes past the input may hold anything once the caller has checked that the header fits
SURGE_SNAPPY_HD inline Element element(uint32_t tag, uint32_t ext) {
  Element e;
  const uint32_t kind = tag & 3u, n = tag >> 2;
  e.header = header_bytes(tag);
  e.copy = kind != 0u;
  e.offset = 0u;
  if (kind == 0u) {
    e.n1 = n < 60u ? n : (n == 63u ? ext : ext & ((1u << (8u * (n - 59u))) - 1u));
  } else if (kind == 1u) {
    e.n1 = 3u + (n & 7u);
    e.offset = ((tag >> 5) << 8) | (ext & 0xffu);
  } else {
    e.n1 = n;
    e.offset = kind == 2u ? (ext & 0xffffu) : ext;
  }
  return e;
}

// the preamble at src[0 .. len): *value, *bytes (1 .. 5)
SURGE_SNAPPY_HD inline Status read_preamble(const uint8_t* src, int64_t len, uint32_t* value, int32_t* bytes) {
  uint64_t v = 0;
  for (int32_t k = 0; k < 5; ++k) {
    if (k >= len) return SN_PREAMBLE_TRUNCATED;
    const uint32_t b = src[k];
    v |= (uint64_t)(b & 0x7fu) << (7 * k);
    if (!(b & 0x80u)) {
      if (v > 0xffffffffull) return SN_PREAMBLE_TOO_LARGE;
      *value = (uint32_t)v;
      *bytes = k + 1;
      return SN_OK;
    }
  }
  return SN_PREAMBLE_TOO_LARGE;
}

// ---- the host decoder ------------------------------------------------------------------------------------------------------
inline uint32_t ext_bytes(const uint8_t* p, uint32_t n) {  // n <= 4 bytes from p, little-endian
  uint32_t v = 0;
  for (uint32_t k = 0; k < n; ++k) v |= (uint32_t)p[k] << (8 * k);
  return v;
}

// One raw block src[0 .. len) into dst[0 .. cap): *out_len = the preamble's length when everything checked out.
inline Status uncompress_block(const uint8_t* src, int64_t len, uint8_t* dst, int64_t cap, int64_t* out_len) {
  uint32_t want32 = 0;
  int32_t pre = 0;
  const Status ps = read_preamble(src, len, &want32, &pre);
  if (ps != SN_OK) return ps;
  const int64_t want = (int64_t)want32;
  if (want > cap) return SN_NO_SPACE;
  int64_t ip = pre, op = 0;
  while (ip < len) {
    const uint32_t tag = src[ip];
    const int64_t hdr = (int64_t)header_bytes(tag);
    if (hdr > len - ip) return SN_TAG_PAST_INPUT;
    const Element e = element(tag, ext_bytes(src + ip + 1, (uint32_t)hdr - 1u));
    const int64_t n = (int64_t)e.n1 + 1;
    ip += hdr;
    if (!e.copy) {
      if (n > len - ip) return SN_LITERAL_PAST_INPUT;
      if (n > want - op) return SN_OUTPUT_BEYOND_PREAMBLE;
      memcpy(dst + op, src + ip, (size_t)n);
      ip += n;
    } else {
      const int64_t off = (int64_t)e.offset;
      if (off == 0) return SN_OFFSET_ZERO;
      if (off > op) return SN_OFFSET_BEYOND_OUTPUT;
      if (n > want - op) return SN_OUTPUT_BEYOND_PREAMBLE;
      if (off >= n) {
        memcpy(dst + op, dst + op - off, (size_t)n);
      } else {  // the period is the data
        for (int64_t k = 0; k < n; ++k) dst[op + k] = dst[op + k - off];
      }
    }
    op += n;
  }
  if (op != want) return SN_OUTPUT_SHORT;
  *out_len = want;
  return SN_OK;
}

constexpr uint8_t kMagic[8] = {0x82, 0x53, 0x4E, 0x41, 0x50, 0x50, 0x59, 0x00};
constexpr int64_t kFrameHeader = 16;

inline bool framed(const uint8_t* src, int64_t len) { return len >= 8 && memcmp(src, kMagic, 8) == 0; }

inline int32_t be32(const uint8_t* p) { return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]); }

// The raw blocks of a records section, framed or not, in order: each(block_off, block_len, preamble) for every one whose
// length word and preamble check out — nothing per byte.  `each` returns SN_OK to go on.
template <typename F>
inline Status walk_chunks(const uint8_t* src, int64_t len, F&& each) {
  uint32_t want = 0;
  int32_t pre = 0;
  if (!framed(src, len)) {
    const Status ps = read_preamble(src, len, &want, &pre);
    return ps != SN_OK ? ps : each((int64_t)0, len, want);
  }
  if (len < kFrameHeader || be32(src + 8) != 1 || be32(src + 12) != 1) return SN_VERSION;
  int64_t p = kFrameHeader;
  while (p < len) {
    if (len - p < 4) return SN_TRAILING_BYTES;
    const int64_t clen = (int64_t)be32(src + p);
    p += 4;
    if (clen < 0) return SN_CHUNK_NEGATIVE;
    if (clen > len - p) return SN_CHUNK_PAST_INPUT;
    const Status ps = read_preamble(src + p, clen, &want, &pre);
    if (ps != SN_OK) return ps;
    const Status es = each(p, clen, want);
    if (es != SN_OK) return es;
    p += clen;
  }
  return SN_OK;
}

// what a records section decompresses to by its preambles: nothing is decoded
inline Status frame_bound(const uint8_t* src, int64_t len, int64_t* total) {
  int64_t sum = 0;
  const Status s = walk_chunks(src, len, [&](int64_t, int64_t clen, uint32_t want) {
    // (the densest element is a 3-byte copy of 64 bytes: a preamble beyond 32 x the block is never reached, and a damaged one
    // must not size a buffer)
    if ((int64_t)want > clen * 32) return SN_OUTPUT_SHORT;
    sum += (int64_t)want;
    return sum > (1ll << 31) ? SN_TOO_LARGE : SN_OK;
  });
  *total = sum;
  return s;
}

// a records section into dst[0 .. cap)
inline Status frame_decompress(const uint8_t* src, int64_t len, uint8_t* dst, int64_t cap, int64_t* out_len) {
  int64_t op = 0;
  const Status s = walk_chunks(src, len, [&](int64_t at, int64_t clen, uint32_t) {
    int64_t got = 0;
    const Status bs = uncompress_block(src + at, clen, dst + op, cap - op, &got);
    op += got;
    return bs;
  });
  *out_len = op;
  return s;
}

}  // namespace snappy
}  // namespace surge
