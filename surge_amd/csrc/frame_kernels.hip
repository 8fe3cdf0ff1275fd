// frame_kernels.hip — the state-topic record batches of a bulk publish, framed on the GPU.
//
// What it replaces: snapshot_writer.cpp's append loop on the host.  A publish of config C5 (0.95 M changed aggregates of
// 10 M, 85 MB of record batches every 30 micro-batches) spent 40 of its 52 ms there — one host thread per partition
// pushing varints and bytes into vectors — while the states, their JSON text and their keys were already in HBM.  Here
// the GPU writes the records where they go and only what the host is better at stays on the host: the CRC-32C of each
// finished batch (the crc32 instruction: 11 GB/s per thread) over the bytes after they arrived in page-locked memory.
//
// The output is BYTE-IDENTICAL to surge_snapshot_writer_append + flush on the same input (tests/test_frame_gpu.py):
// same record order (per partition, aggregate index order), same batch cuts (a batch closes with the record that makes
// it reach max_records or max_bytes), same header fields.  A record is
//     varint(body) | attributes 0 | varint(timestampDelta = 0) | varint(offsetDelta) | varint(klen) key | varint(vlen | -1) value | varint(0 headers)
// and the only field that depends on where a batch starts is offsetDelta (1 byte below 64, 2 below 8192, 3 below 2^20)
// — and through it the size of the length prefix.  So with v = 1, 2, 3 the record's size is known up to that choice:
//     size_v(i) = varint_size(base_i + v) + base_i + v,        base_i = everything but the offsetDelta
// and three prefix sums C_v over the records of a partition give the bytes of ANY run [s, s + m) in closed form:
//     bytes(s, m) = C_1[s .. s+min(m,64)) + C_2[s+64 .. s+min(m,8192)) + C_3[s+8192 .. s+m)
// which makes the greedy cut a binary search per batch (one thread per partition walks its few batches) and gives every
// record its byte position without any sequential pass over the records.
//
// Steps (all on the framer's stream): select the changed aggregates (rocPRIM select) -> their partition + base size ->
// stable radix sort by partition -> the three scans -> batches per partition (count, then emit at scanned offsets) ->
// one thread per record writes its bytes, one per batch its 61-byte header -> one device -> host copy -> host CRCs.
//
// LZ4 mode (surge_device_framer_set_compression): what the reference's producer writes (compression.type = lz4).  The
// batch cuts, offsets and counts are those of the uncompressed framing — they are decided on the uncompressed sizes, as
// the host writer decides them —; the records section of every batch then becomes ONE LZ4 frame as kafka-clients writes
// it (magic, FLG 0x60, BD 0x40, HC 0x82, independent blocks of 64 KiB of input, EndMark; no checksums), attributes = 3,
// and the CRC covers the compressed batch.  After the write kernel has put the records into the uncompressed buffer:
//     block table (batch, block) -> frame_lz4_block_kernel, ONE WAVE PER BLOCK, into a scratch slot per block ->
//     scan of the block sizes -> every batch's frame size and final place -> frame_lz4_pack_kernel moves size words and
//     block bytes (from the scratch slot, or from the uncompressed buffer for a block that did not shrink: stored) ->
//     header kernel -> device -> host copy of the COMPRESSED bytes -> host CRCs.
// The output is not the host compressor's byte for byte (a wave looks at 64 positions at once and sees the hash table
// differently); it decodes to the same records and is about as small (tests/test_frame_lz4_gpu.py).
// Device memory at the peak of an LZ4 publish of U uncompressed batch bytes: the uncompressed buffer (U), the scratch
// slots (U: a slot is as long as its block, a block that would not shrink is abandoned before it outgrows it) and the
// final buffer (at most U + 11 bytes per batch + 4 per block) — about 3 U, beside the tables of the uncompressed mode.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/surge_ingest.h"  // surge_crc32c
#include "../../include/surge_replay.h"  // SURGE_SNAP_*
#include "../../include/surge_snapshot.h"

namespace {

constexpr int32_t OK = 0, E_INVALID = -1, E_DEVICE = -3, E_NOMEM = -4, E_RANGE = -6;
constexpr int kHeader = 61;
constexpr int64_t kD1 = 64, kD2 = 8192, kD3 = 1 << 20;  // offsetDelta below these takes 1 / 2 / 3 bytes

struct Batch {          // device + host
  int64_t out_off;      // first byte of the batch (its header) in the output
  int64_t first;        // index of its first record in partition-sorted order
  int64_t base_offset;  // Kafka offset of its first record
  int32_t count;
  int32_t partition;
  int64_t records_bytes;
};

__host__ __device__ inline int varint_size(int64_t x) {
  uint64_t z = ((uint64_t)x << 1) ^ (uint64_t)(x >> 63);
  int n = 1;
  while (z >= 0x80) { z >>= 7; ++n; }
  return n;
}

__device__ inline uint8_t* put_varint(uint8_t* p, int64_t x) {
  uint64_t z = ((uint64_t)x << 1) ^ (uint64_t)(x >> 63);
  while (z >= 0x80) {
    *p++ = (uint8_t)(z | 0x80);
    z >>= 7;
  }
  *p++ = (uint8_t)z;
  return p;
}

// a record's key / value, 8 bytes at a time: neither end is aligned, which global memory on gfx9+ does not ask for (the
// byte loop this replaces made the write kernel 1.9 ms of an 85 MB publish)
__device__ inline void copy_bytes(uint8_t* dst, const uint8_t* src, int64_t n) {
  int64_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t v;
    __builtin_memcpy(&v, src + i, 8);
    __builtin_memcpy(dst + i, &v, 8);
  }
  for (; i < n; ++i) dst[i] = src[i];
}

__device__ inline void put_be(uint8_t* p, uint64_t x, int n) {
  for (int i = 0; i < n; ++i) p[i] = (uint8_t)(x >> (8 * (n - 1 - i)));
}

// per selected record r (aggregate sel[r]): its partition and the size of its body without the offsetDelta; bad[0] is
// set when a partition is out of range, a span is negative or a kind is unknown
__global__ void frame_size_kernel(const int64_t* __restrict__ sel, int64_t n_sel, const uint8_t* __restrict__ kind, const int32_t* __restrict__ part,
                                  int32_t n_part, const int64_t* __restrict__ key_off, const int64_t* __restrict__ val_off, bool have_keys,
                                  bool have_values, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ base,
                                  uint32_t* __restrict__ bad) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_sel) return;
  const int64_t a = sel[r];
  const uint8_t k = kind[a];
  const int32_t p = part[a];
  const bool value = k == SURGE_SNAP_VALUE;
  const int64_t klen = key_off[a + 1] - key_off[a];
  const int64_t vlen = value && val_off ? val_off[a + 1] - val_off[a] : -1;
  if ((!value && k != SURGE_SNAP_TOMBSTONE) || p < 0 || p >= n_part || klen < 0 || (value && (!val_off || vlen < 0)) || klen > (1 << 28) ||
      vlen > (1 << 28) || (klen > 0 && !have_keys) || (vlen > 0 && !have_values))
    atomicOr(bad, 1u);
  keys[r] = (uint32_t)(p < 0 ? 0 : p);
  vals[r] = (uint32_t)r;
  base[r] = (uint32_t)(1 + 1 + varint_size(klen) + klen + varint_size(vlen) + (vlen > 0 ? vlen : 0) + 1);
}

// j = position in partition order: c_v[j] = size of record order[j] if its offsetDelta takes v bytes (scanned afterwards)
__global__ void frame_sizes3_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ base, int64_t n_sel, int64_t* __restrict__ c1,
                                    int64_t* __restrict__ c2, int64_t* __restrict__ c3) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n_sel) return;
  if (j == n_sel) {  // the element the exclusive scans leave the totals in
    c1[j] = c2[j] = c3[j] = 0;
    return;
  }
  const int64_t b = base[order[j]];
  c1[j] = varint_size(b + 1) + b + 1;
  c2[j] = varint_size(b + 2) + b + 2;
  c3[j] = varint_size(b + 3) + b + 3;
}

// first position of every partition in the sorted order (pstart[n_part] = n_sel)
__global__ void frame_pstart_kernel(const uint32_t* __restrict__ sorted_part, int64_t n_sel, int32_t n_part, int64_t* __restrict__ pstart) {
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n_part) return;
  int64_t lo = 0, hi = n_sel;  // first j with sorted_part[j] >= p
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted_part[mid] < (uint32_t)p) lo = mid + 1; else hi = mid;
  }
  pstart[p] = lo;
}

__device__ inline int64_t run_bytes(const int64_t* c1, const int64_t* c2, const int64_t* c3, int64_t s, int64_t m) {
  const int64_t m1 = m < kD1 ? m : kD1;
  int64_t b = c1[s + m1] - c1[s];
  if (m > kD1) b += c2[s + (m < kD2 ? m : kD2)] - c2[s + kD1];
  if (m > kD2) b += c3[s + m] - c3[s + kD2];
  return b;
}

// One thread per partition walks its batches.  emit == false: nb[p] / pbytes[p] only; emit == true: the batches are
// written at batch index nb_off[p] and byte offset pbytes_off[p] (the exclusive scans of the first pass).
__global__ void frame_batches_kernel(const int64_t* __restrict__ pstart, int32_t n_part, const int64_t* __restrict__ c1, const int64_t* __restrict__ c2,
                                     const int64_t* __restrict__ c3, int32_t max_records, int64_t max_bytes, const int64_t* __restrict__ next_offset,
                                     bool emit, int64_t* __restrict__ nb, int64_t* __restrict__ pbytes, Batch* __restrict__ batches) {
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_part) return;
  int64_t s = pstart[p];
  const int64_t e = pstart[p + 1];
  int64_t count = 0, bytes = 0;
  int64_t bi = emit ? nb[p] : 0, at = emit ? pbytes[p] : 0;
  while (s < e) {
    int64_t m = e - s < max_records ? e - s : max_records;  // the batch closes at max_records at the latest
    if (run_bytes(c1, c2, c3, s, m) >= max_bytes) {         // ... or with the first record that brings it to max_bytes
      int64_t lo = 1, hi = m;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (run_bytes(c1, c2, c3, s, mid) >= max_bytes) hi = mid; else lo = mid + 1;
      }
      m = lo;
    }
    const int64_t rb = run_bytes(c1, c2, c3, s, m);
    if (emit) {
      Batch b;
      b.out_off = at + bytes;
      b.first = s;
      b.base_offset = next_offset[p] + (s - pstart[p]);
      b.count = (int32_t)m;
      b.partition = p;
      b.records_bytes = rb;
      batches[bi + count] = b;
    }
    bytes += kHeader + rb;
    count += 1;
    s += m;
  }
  if (!emit) {
    nb[p] = count;
    pbytes[p] = bytes;
  }
}

// one thread per record (partition order): find its batch, its place in it, write it
__global__ void frame_write_kernel(const Batch* __restrict__ batches, int64_t n_batches, const uint32_t* __restrict__ order, const int64_t* __restrict__ sel,
                                   int64_t n_sel, const uint8_t* __restrict__ kind, const uint32_t* __restrict__ base, const int64_t* __restrict__ c1,
                                   const int64_t* __restrict__ c2, const int64_t* __restrict__ c3, const uint8_t* __restrict__ keys_utf8,
                                   const int64_t* __restrict__ key_off, const uint8_t* __restrict__ values, const int64_t* __restrict__ val_off,
                                   uint8_t* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_sel) return;
  int64_t lo = 0, hi = n_batches;  // last batch whose first record is <= j
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (batches[mid].first <= j) lo = mid; else hi = mid;
  }
  const Batch b = batches[lo];
  const int64_t d = j - b.first;
  const uint32_t r = order[j];
  const int64_t a = sel[r];
  const int v = d < kD1 ? 1 : (d < kD2 ? 2 : 3);
  const int64_t body = (int64_t)base[r] + v;
  uint8_t* p = out + b.out_off + kHeader + run_bytes(c1, c2, c3, b.first, d);
  p = put_varint(p, body);
  *p++ = 0;  // attributes
  *p++ = 0;  // timestampDelta 0: every record of a publish carries the publish's timestamp
  p = put_varint(p, d);
  const int64_t k0 = key_off[a], klen = key_off[a + 1] - k0;
  p = put_varint(p, klen);
  copy_bytes(p, keys_utf8 + k0, klen);
  p += klen;
  if (kind[a] == SURGE_SNAP_VALUE) {
    const int64_t v0 = val_off[a], vlen = val_off[a + 1] - v0;
    p = put_varint(p, vlen);
    copy_bytes(p, values + v0, vlen);
    p += vlen;
  } else {
    p = put_varint(p, -1);  // null value: a tombstone
  }
  *p = 0;  // no headers
}

__global__ void frame_header_kernel(const Batch* __restrict__ batches, int64_t n_batches, int64_t timestamp_ms, int32_t codec, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_batches) return;
  const Batch b = batches[i];
  uint8_t* o = out + b.out_off;
  put_be(o, (uint64_t)b.base_offset, 8);
  put_be(o + 8, (uint64_t)(kHeader - 12 + b.records_bytes), 4);  // batchLength: everything after this field
  put_be(o + 12, 0, 4);                                           // partitionLeaderEpoch
  o[16] = 2;                                                      // magic
  put_be(o + 17, 0, 4);                                           // crc: the host fills it in
  put_be(o + 21, (uint64_t)codec, 2);                             // attributes: the codec, CreateTime, not transactional
  put_be(o + 23, (uint64_t)(b.count - 1), 4);                     // lastOffsetDelta
  put_be(o + 27, (uint64_t)timestamp_ms, 8);                      // baseTimestamp
  put_be(o + 35, (uint64_t)timestamp_ms, 8);                      // maxTimestamp
  put_be(o + 43, ~0ull, 8);                                       // producerId -1
  put_be(o + 51, 0xffffull, 2);                                   // producerEpoch -1
  put_be(o + 53, 0xffffffffull, 4);                               // baseSequence -1
  put_be(o + 57, (uint64_t)b.count, 4);
}

// ---- LZ4 mode -------------------------------------------------------------------------------------------------------
constexpr int32_t kLzBlock = 65536;     // input bytes per block: the device decoder places block k at k * 64 KiB
constexpr int kLzFrameHeader = 7;       // magic, FLG, BD, HC
constexpr int32_t kLzSmall = 4096;      // blocks up to this size are compressed with the small hash table
constexpr int kLzHashLogSmall = 11, kLzHashLog = 13;  // 4 KiB / 16 KiB of LDS per wave

struct LzBlock {
  int64_t src_off;  // first byte of the block in the uncompressed buffer (and of its slot in the scratch buffer)
  int32_t n;        // input bytes: 65536 for all but a frame's last block
  int32_t batch;
};

__global__ void frame_lz4_count_kernel(const Batch* __restrict__ batches, int64_t n_batches, int64_t* __restrict__ nblk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_batches) return;
  nblk[i] = i == n_batches ? 0 : (batches[i].records_bytes + kLzBlock - 1) / kLzBlock;
}

// one thread per block: find its batch in blk_first (the exclusive scan of the counts; every batch has a block, so it
// rises strictly), its place in it, write its entry
__global__ void frame_lz4_blocks_kernel(const Batch* __restrict__ batches, int64_t n_batches, const int64_t* __restrict__ blk_first, int64_t n_blocks,
                                        LzBlock* __restrict__ blocks) {
  const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= n_blocks) return;
  int64_t lo = 0, hi = n_batches;  // last batch whose first block is <= blk
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (blk_first[mid] <= blk) lo = mid; else hi = mid;
  }
  const Batch b = batches[lo];
  const int64_t k = blk - blk_first[lo];
  const int64_t rest = b.records_bytes - k * kLzBlock;
  LzBlock e;
  e.src_off = b.out_off + kHeader + k * kLzBlock;
  e.n = (int32_t)(rest < kLzBlock ? rest : kLzBlock);
  e.batch = (int32_t)lo;
  blocks[blk] = e;
}

__device__ inline uint32_t load32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// bytes of the 255-continued length that follows a saturated token nibble
__device__ inline int32_t lz4_len_bytes(int32_t len) { return len >= 15 ? (len - 15) / 255 + 1 : 0; }

__device__ inline void lz4_put_len(uint8_t* dst, int32_t len, int lane) {  // the whole wave; len >= 15
  const int32_t v = len - 15, nb = v / 255 + 1;
  for (int32_t i = lane; i < nb; i += 64) dst[i] = i < nb - 1 ? (uint8_t)255 : (uint8_t)(v % 255);
}

// One wave compresses one block (LZ4 block format) into the block's scratch slot; bsz[blk] = 4 + its compressed size, or
// 4 + n when it is to be stored.  Launched once per size class (n_lo < n <= n_hi) with a hash table to match, so that
// the many small batches of a many-partition publish do not each hold the LDS a 64 KiB block wants.
//
// The wave looks at the 64 positions ip .. ip + 63: every lane hashes its 4 bytes, reads its candidate from the table and
// tests it; the lowest matching lane f wins, the wave extends its match 64 bytes per step, emits the sequence together
// and goes on behind the match; with no match in the window it moves on by 64.  Two rules that a lane-for-lane
// simulation of this scheme showed to matter:
//   * only the lanes up to and including f insert their position into the table (all of them when nothing matched).
//     Were all 64 to insert before the decision, the positions behind a short match would overwrite the very entries
//     the next window needs, and then point at themselves: the ratio on Counter state records fell from 2.54 to 1.23;
//   * a candidate must lie strictly BEFORE the lane's position.  The table starts as all zeros (position 0 is a valid
//     candidate for every later position: what counts is that the bytes are equal) and a 16-bit entry has no value to
//     spare for "empty", so a lane at position 0 meets itself; one compare keeps the offset in 1 .. 65535.
// A third rule is for what the window scheme cannot see: all 64 lanes read their candidates before any of them inserts, so
// a repeat that begins inside a window of new content is found one window late -- and in the block's LAST window
// (ip + 64 > n - 12) not at all.  There, when the table gave no hit, every lane takes the nearest earlier lane of the
// window with the same 4 bytes as its candidate: one shuffle per active lane of that window, in every block whose last
// window has no table hit -- every incompressible block, and every small block without a repeat, of which a
// many-partition publish has many (200 000 blocks of 35 to 75 random bytes: 232 us for the launch, 73 us without the
// search, in a publish of 25 ms).  Without it no block below 76 bytes could shrink unless it repeated its own first
// bytes, and a batch of one small record of zeros was stored.
// The table holds 16-bit positions (a block is at most 64 KiB), the block's bytes are read from global memory (the write
// kernel has just put them there) — 16 KiB of LDS per wave leaves room for ten waves per CU.
// Writes: a sequence is emitted only if the output stays BELOW n bytes with it; otherwise the block is given up as
// stored (the output only grows, so it would have ended up stored anyway).  So whatever the input, nothing is written
// beyond the n bytes of the block's own slot, and table indices are hash values of HASH_LOG bits.
template <int HASH_LOG>
__global__ __launch_bounds__(64) void frame_lz4_block_kernel(const LzBlock* __restrict__ blocks, int64_t n_blocks, int32_t n_lo, int32_t n_hi,
                                                             const uint8_t* __restrict__ src_base, uint8_t* __restrict__ tmp_base,
                                                             int64_t* __restrict__ bsz) {
  __shared__ uint16_t table[1 << HASH_LOG];
  const int64_t blk = blockIdx.x;
  if (blk >= n_blocks) return;
  const LzBlock B = blocks[blk];
  const int32_t n = B.n;
  if (n <= n_lo || n > n_hi) return;
  const int lane = threadIdx.x;
  const uint8_t* __restrict__ src = src_base + B.src_off;
  uint8_t* __restrict__ dst = tmp_base + B.src_off;
  for (int i = lane; i < (1 << HASH_LOG); i += 64) table[i] = 0;
  __syncthreads();
  const int32_t mflimit = n - 12;    // no match starts after this position ...
  const int32_t matchlimit = n - 5;  // ... and none reaches this one: the last 5 bytes are literals
  int32_t ip = 0, anchor = 0, op = 0;
  while (ip <= mflimit) {  // (a block below 13 bytes is one literal run, longer than its input: stored)
    const int32_t pos = ip + lane;
    const bool active = pos <= mflimit;
    const uint32_t v = active ? load32(src + pos) : 0u;
    const uint32_t h = (v * 2654435761u) >> (32 - HASH_LOG);
    int32_t cand = active ? (int32_t)table[h] : 0;
    bool hit = active && cand < pos && load32(src + cand) == v;
    uint64_t hits = __ballot(hit);
    if (!hits && ip + 64 > mflimit) {  // the block's last window: nearest earlier lane with the same 4 bytes
      const int live = mflimit - ip + 1;  // its active lanes, 1 .. 64: the same for the whole wave
      for (int d = 1; d < live; ++d) {
        const uint32_t w = __shfl_up(v, d);
        if (!hit && active && lane >= d && w == v) {
          hit = true;
          cand = pos - d;
        }
      }
      hits = __ballot(hit);
    }
    const int f = hits ? __ffsll((long long)hits) - 1 : 63;
    if (active && lane <= f) table[h] = (uint16_t)pos;
    __syncthreads();  // one wave: orders this window's inserts before the next window's reads
    if (!hits) {
      ip += 64;
      continue;
    }
    const int32_t mpos = ip + f;
    const int32_t off = mpos - __shfl(cand, f);
    int32_t len = 4;
    for (;;) {
      const int32_t q = mpos + len + lane;
      const bool same = q < matchlimit && src[q] == src[q - off];
      const uint64_t diff = __ballot(!same);
      if (diff) {
        len += __ffsll((long long)diff) - 1;
        break;
      }
      len += 64;
    }
    const int32_t lit = mpos - anchor, ml = len - 4;
    const int32_t lit_lb = lz4_len_bytes(lit), ml_lb = lz4_len_bytes(ml);
    const int32_t need = 1 + lit_lb + lit + 2 + ml_lb;
    if (op + need >= n) {
      if (lane == 0) bsz[blk] = 4 + (int64_t)n;
      return;
    }
    uint8_t* o = dst + op;
    if (lane == 0) o[0] = (uint8_t)((lit >= 15 ? 15 : lit) << 4 | (ml >= 15 ? 15 : ml));
    if (lit >= 15) lz4_put_len(o + 1, lit, lane);
    o += 1 + lit_lb;
    for (int32_t i = lane; i < lit; i += 64) o[i] = src[anchor + i];
    o += lit;
    if (lane == 0) {
      o[0] = (uint8_t)off;
      o[1] = (uint8_t)(off >> 8);
    }
    if (ml >= 15) lz4_put_len(o + 2, ml, lane);
    op += need;
    ip = mpos + len;
    anchor = ip;
  }
  const int32_t lit = n - anchor;  // the last sequence is literals only
  const int32_t lit_lb = lz4_len_bytes(lit);
  const int32_t need = 1 + lit_lb + lit;
  if (op + need >= n) {
    if (lane == 0) bsz[blk] = 4 + (int64_t)n;
    return;
  }
  uint8_t* o = dst + op;
  if (lane == 0) o[0] = (uint8_t)((lit >= 15 ? 15 : lit) << 4);
  if (lit >= 15) lz4_put_len(o + 1, lit, lane);
  o += 1 + lit_lb;
  for (int32_t i = lane; i < lit; i += 64) o[i] = src[anchor + i];
  if (lane == 0) bsz[blk] = 4 + (int64_t)(op + need);
}

// per batch (and one entry beyond): bytes of the compressed batch, from the scanned block sizes (bscan[b] = bytes of
// the size words and blocks before block b)
__global__ void frame_lz4_batch_size_kernel(int64_t n_batches, const int64_t* __restrict__ blk_first, const int64_t* __restrict__ bscan,
                                            int64_t* __restrict__ bbytes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_batches) return;
  bbytes[i] = i == n_batches ? 0 : kHeader + kLzFrameHeader + (bscan[blk_first[i + 1]] - bscan[blk_first[i]]) + 4;
}

// the partitions' spans in the compressed output: nb[p] = first batch of partition p, new_off = scanned batch bytes
__global__ void frame_lz4_spans_kernel(int32_t n_part, const int64_t* __restrict__ nb, const int64_t* __restrict__ new_off, int64_t* __restrict__ pspan) {
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n_part) return;
  pspan[p] = new_off[nb[p]];
}

// One workgroup per block moves it to its final place: size word + bytes; the batch's first block also writes the frame
// header, its last the EndMark.  Reads blocks[].src_off (the uncompressed layout), so it runs before the batches are
// re-addressed.
__global__ __launch_bounds__(256) void frame_lz4_pack_kernel(const LzBlock* __restrict__ blocks, const int64_t* __restrict__ blk_first,
                                                             const int64_t* __restrict__ bscan, const int64_t* __restrict__ new_off,
                                                             const uint8_t* __restrict__ src_base, const uint8_t* __restrict__ tmp_base,
                                                             uint8_t* __restrict__ out) {
  const int64_t blk = blockIdx.x;
  const LzBlock B = blocks[blk];
  const int64_t first = blk_first[B.batch], last = blk_first[B.batch + 1] - 1;
  const int64_t csize = bscan[blk + 1] - bscan[blk] - 4;
  const bool stored = csize >= B.n;
  uint8_t* frame = out + new_off[B.batch] + kHeader;
  uint8_t* o = frame + kLzFrameHeader + (bscan[blk] - bscan[first]);
  const int t = threadIdx.x;
  if (t < 4) {
    const uint32_t word = stored ? ((uint32_t)B.n | 0x80000000u) : (uint32_t)csize;
    o[t] = (uint8_t)(word >> (8 * t));
  }
  if (blk == first && t >= 32 && t < 32 + kLzFrameHeader) {
    const uint8_t head[kLzFrameHeader] = {0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82};  // HC = (XXH32(FLG BD) >> 8) & 0xff
    frame[t - 32] = head[t - 32];
  }
  if (blk == last && t >= 64 && t < 68) o[4 + csize + (t - 64)] = 0;  // EndMark
  const uint8_t* s = (stored ? src_base : tmp_base) + B.src_off;
  o += 4;
  for (int64_t i = (int64_t)t * 8; i < csize; i += 256 * 8) {
    if (i + 8 <= csize) {
      uint64_t v;
      __builtin_memcpy(&v, s + i, 8);
      __builtin_memcpy(o + i, &v, 8);
    } else {
      for (int64_t k = i; k < csize; ++k) o[k] = s[k];
    }
  }
}

// the batches in the compressed layout: what the header kernel, the copy and the host CRCs work from
__global__ void frame_lz4_readdress_kernel(Batch* __restrict__ batches, int64_t n_batches, const int64_t* __restrict__ new_off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_batches) return;
  batches[i].out_off = new_off[i];
  batches[i].records_bytes = new_off[i + 1] - new_off[i] - kHeader;
}

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    const size_t want = cap * 2 > bytes ? cap * 2 : bytes;
    void* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, want);
    if (e != hipSuccess) return e;
    if (p) (void)hipFree(p);
    p = fresh;
    cap = want;
    return hipSuccess;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

thread_local std::string g_frame_err;

}  // namespace

struct surge_device_framer {
  int device = 0;
  hipStream_t stream = nullptr;
  int32_t n_part = 0, max_records = 10000;
  int64_t max_bytes = 1 << 20;
  int32_t codec = SURGE_SNAPSHOT_CODEC_NONE;
  int64_t uncompressed_bytes = 0;  // of the last publish's batches
  std::string err;
  std::vector<int64_t> next_offset, part_byte_off;
  std::vector<Batch> h_batches;
  Buf sel, n_sel, keys_a, keys_b, vals_a, vals_b, base, c, pstart, nb, pbytes, d_next, batches, out, bad, temp;
  Buf lz_nblk, lz_blocks, lz_bsz, lz_bbytes, lz_tmp, lz_out;  // LZ4 mode only
  uint8_t* pinned = nullptr;
  size_t pinned_cap = 0;
};

namespace {

int32_t ffail(surge_device_framer* f, int32_t code, const std::string& m) {
  if (f) f->err = m;
  g_frame_err = m;
  return code;
}

#define FCHK(f, call)                                                                                                       \
  do {                                                                                                                      \
    const hipError_t e_ = (call);                                                                                           \
    if (e_ != hipSuccess) return ffail(f, e_ == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct Guard {
  int prev = -1;
  explicit Guard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
  ~Guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline unsigned grid(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int32_t surge_device_framer_create(int32_t device_id, void* hip_stream, int32_t n_partitions, int32_t max_records_per_batch, int64_t max_batch_bytes,
                                   surge_device_framer** out) {
  if (!out) return ffail(nullptr, E_INVALID, "out is NULL");
  *out = nullptr;
  if (n_partitions <= 0 || n_partitions > (1 << 20) || max_records_per_batch < 0 || max_records_per_batch > kD3 || max_batch_bytes < 0)
    return ffail(nullptr, E_INVALID, "bad argument (partitions in 1 .. 2^20, at most 2^20 records per batch)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device_id < 0 || device_id >= n_dev)
    return ffail(nullptr, E_DEVICE, "no usable HIP device (the device framer has no CPU fallback: use surge_snapshot_writer_append)");
  surge_device_framer* f = new (std::nothrow) surge_device_framer();
  if (!f) return ffail(nullptr, E_NOMEM, "out of host memory");
  f->device = device_id;
  f->stream = (hipStream_t)hip_stream;
  f->n_part = n_partitions;
  if (max_records_per_batch > 0) f->max_records = max_records_per_batch;
  if (max_batch_bytes > 0) f->max_bytes = max_batch_bytes;
  try {
    f->next_offset.assign((size_t)n_partitions, 0);
    f->part_byte_off.assign((size_t)n_partitions + 1, 0);
  } catch (const std::bad_alloc&) {
    delete f;
    return ffail(nullptr, E_NOMEM, "out of host memory");
  }
  *out = f;
  return OK;
}

int32_t surge_device_framer_destroy(surge_device_framer* f) {
  if (!f) return OK;
  Guard g(f->device);
  (void)hipStreamSynchronize(f->stream);
  for (Buf* b : {&f->sel, &f->n_sel, &f->keys_a, &f->keys_b, &f->vals_a, &f->vals_b, &f->base, &f->c, &f->pstart, &f->nb, &f->pbytes, &f->d_next,
                 &f->batches, &f->out, &f->bad, &f->temp, &f->lz_nblk, &f->lz_blocks, &f->lz_bsz, &f->lz_bbytes, &f->lz_tmp, &f->lz_out})
    b->release();
  if (f->pinned) (void)hipHostFree(f->pinned);
  delete f;
  return OK;
}

const char* surge_device_framer_last_error(const surge_device_framer* f) { return f ? f->err.c_str() : g_frame_err.c_str(); }

int32_t surge_device_framer_set_compression(surge_device_framer* f, int32_t codec) {
  if (!f) return ffail(nullptr, E_INVALID, "framer is NULL");
  if (codec != SURGE_SNAPSHOT_CODEC_NONE && codec != SURGE_SNAPSHOT_CODEC_LZ4)
    return ffail(f, E_INVALID, "unknown codec (the device framer writes uncompressed or LZ4 batches)");
  f->codec = codec;
  return OK;
}

int32_t surge_device_framer_next_offsets(const surge_device_framer* f, int64_t* out) {
  if (!f || !out) return ffail(nullptr, E_INVALID, "bad argument");
  std::memcpy(out, f->next_offset.data(), f->next_offset.size() * 8);
  return OK;
}

int64_t surge_device_framer_uncompressed_bytes(const surge_device_framer* f) { return f ? f->uncompressed_bytes : -1; }

int32_t surge_device_framer_frame(surge_device_framer* f, int64_t n_aggregates, const uint8_t* d_kind, const int32_t* d_partition,
                                  const uint8_t* d_keys_utf8, const int64_t* d_key_off, const uint8_t* d_values, const int64_t* d_val_off,
                                  int64_t timestamp_ms, const uint8_t** bytes_out, const int64_t** part_byte_off_out, int64_t* n_records_out,
                                  int64_t* n_batches_out) {
  if (!f) return ffail(nullptr, E_INVALID, "framer is NULL");
  if (n_aggregates < 0 || n_aggregates > (1ll << 32) - 2 || !bytes_out || !part_byte_off_out)
    return ffail(f, E_INVALID, "bad argument");
  if (n_aggregates > 0 && (!d_kind || !d_partition || !d_key_off)) return ffail(f, E_INVALID, "NULL device buffer");
  Guard g(f->device);
  hipStream_t st = f->stream;
  const int32_t P = f->n_part;
  const int64_t n = n_aggregates;
  std::fill(f->part_byte_off.begin(), f->part_byte_off.end(), 0);
  struct SpanReset {  // on an error nothing advances, and no partition has a span: whichever return it is
    std::vector<int64_t>& spans;
    bool done = false;
    ~SpanReset() { if (!done) std::fill(spans.begin(), spans.end(), 0); }
  } span_reset{f->part_byte_off};
  *bytes_out = f->pinned;
  *part_byte_off_out = f->part_byte_off.data();
  if (n_records_out) *n_records_out = 0;
  if (n_batches_out) *n_batches_out = 0;
  f->uncompressed_bytes = 0;
  if (n == 0) return OK;

  // 1. the changed aggregates, in index order
  FCHK(f, f->sel.reserve((size_t)n * 8));
  FCHK(f, f->n_sel.reserve(16));
  FCHK(f, f->bad.reserve(16));
  size_t tb_select = 0, tb_sort = 0, tb_scan = 0;
  FCHK(f, rocprim::select(nullptr, tb_select, rocprim::counting_iterator<int64_t>(0), d_kind, (int64_t*)f->sel.p, (int64_t*)f->n_sel.p, (size_t)n, st));
  FCHK(f, f->temp.reserve(tb_select));
  FCHK(f, hipMemsetAsync(f->bad.p, 0, 4, st));
  FCHK(f, rocprim::select(f->temp.p, tb_select, rocprim::counting_iterator<int64_t>(0), d_kind, (int64_t*)f->sel.p, (int64_t*)f->n_sel.p, (size_t)n, st));
  int64_t n_sel = 0;
  FCHK(f, hipMemcpyAsync(&n_sel, f->n_sel.p, 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  if (n_sel == 0) return OK;
  if (n_sel > 0xfffffff0ll) return ffail(f, E_RANGE, "more than 2^32 records in one publish");

  // 2. partition + base size per record, stable sort by partition
  unsigned bits = 1;
  while ((1ll << bits) < P) ++bits;
  using SortConfig = rocprim::default_config;  // (merge sort up to 2^20 records; a lower limit was measured for K3's group-by and dropped: stream_kernels.hip)
  FCHK(f, rocprim::radix_sort_pairs<SortConfig>(nullptr, tb_sort, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                (size_t)n_sel, 0u, bits, st));
  FCHK(f, rocprim::exclusive_scan(nullptr, tb_scan, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)n_sel + 1, rocprim::plus<int64_t>(), st));
  FCHK(f, f->temp.reserve(tb_sort > tb_scan ? tb_sort : tb_scan));
  for (Buf* b : {&f->keys_a, &f->keys_b, &f->vals_a, &f->vals_b, &f->base}) FCHK(f, b->reserve((size_t)n_sel * 4));
  FCHK(f, f->c.reserve((size_t)(n_sel + 1) * 8 * 3));
  FCHK(f, f->pstart.reserve((size_t)(P + 1) * 8));
  FCHK(f, f->nb.reserve((size_t)(P + 1) * 8));
  FCHK(f, f->pbytes.reserve((size_t)(P + 1) * 8));
  FCHK(f, f->d_next.reserve((size_t)P * 8));
  hipLaunchKernelGGL(frame_size_kernel, dim3(grid(n_sel)), dim3(256), 0, st, (const int64_t*)f->sel.p, n_sel, d_kind, d_partition, P, d_key_off, d_val_off,
                     d_keys_utf8 != nullptr, d_values != nullptr, (uint32_t*)f->keys_a.p, (uint32_t*)f->vals_a.p, (uint32_t*)f->base.p, (uint32_t*)f->bad.p);
  FCHK(f, rocprim::radix_sort_pairs<SortConfig>(f->temp.p, tb_sort, (const uint32_t*)f->keys_a.p, (uint32_t*)f->keys_b.p, (const uint32_t*)f->vals_a.p,
                                                (uint32_t*)f->vals_b.p, (size_t)n_sel, 0u, bits, st));
  const uint32_t* order = (const uint32_t*)f->vals_b.p;
  int64_t* c1 = (int64_t*)f->c.p;
  int64_t* c2 = c1 + (n_sel + 1);
  int64_t* c3 = c2 + (n_sel + 1);
  hipLaunchKernelGGL(frame_sizes3_kernel, dim3(grid(n_sel + 1)), dim3(256), 0, st, order, (const uint32_t*)f->base.p, n_sel, c1, c2, c3);
  for (int64_t* cv : {c1, c2, c3})
    FCHK(f, rocprim::exclusive_scan(f->temp.p, tb_scan, (const int64_t*)cv, cv, (int64_t)0, (size_t)n_sel + 1, rocprim::plus<int64_t>(), st));
  hipLaunchKernelGGL(frame_pstart_kernel, dim3(grid(P + 1)), dim3(256), 0, st, (const uint32_t*)f->keys_b.p, n_sel, P, (int64_t*)f->pstart.p);

  // 3. the batches of every partition: count, scan, emit
  FCHK(f, hipMemcpyAsync(f->d_next.p, f->next_offset.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(frame_batches_kernel, dim3(grid(P)), dim3(256), 0, st, (const int64_t*)f->pstart.p, P, c1, c2, c3, f->max_records, f->max_bytes,
                     (const int64_t*)f->d_next.p, false, (int64_t*)f->nb.p, (int64_t*)f->pbytes.p, (Batch*)nullptr);
  FCHK(f, hipMemsetAsync((int64_t*)f->nb.p + P, 0, 8, st));
  FCHK(f, hipMemsetAsync((int64_t*)f->pbytes.p + P, 0, 8, st));
  size_t tb_small = tb_scan;  // P + 1 <= 2^20 + 1 elements: the scratch sized for n_sel + 1 may be smaller
  {
    size_t need = 0;
    FCHK(f, rocprim::exclusive_scan(nullptr, need, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)P + 1, rocprim::plus<int64_t>(), st));
    if (need > f->temp.cap) {
      FCHK(f, hipStreamSynchronize(st));  // the scans above still use the scratch
      FCHK(f, f->temp.reserve(need));
    }
    tb_small = need;
  }
  FCHK(f, rocprim::exclusive_scan(f->temp.p, tb_small, (const int64_t*)f->nb.p, (int64_t*)f->nb.p, (int64_t)0, (size_t)P + 1, rocprim::plus<int64_t>(), st));
  FCHK(f, rocprim::exclusive_scan(f->temp.p, tb_small, (const int64_t*)f->pbytes.p, (int64_t*)f->pbytes.p, (int64_t)0, (size_t)P + 1, rocprim::plus<int64_t>(), st));
  int64_t totals[2] = {0, 0};
  FCHK(f, hipMemcpyAsync(&totals[0], (int64_t*)f->nb.p + P, 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipMemcpyAsync(&totals[1], (int64_t*)f->pbytes.p + P, 8, hipMemcpyDeviceToHost, st));
  uint32_t bad = 0;
  FCHK(f, hipMemcpyAsync(&bad, f->bad.p, 4, hipMemcpyDeviceToHost, st));
  FCHK(f, hipMemcpyAsync(f->part_byte_off.data(), f->pbytes.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  if (bad)
    return ffail(f, E_RANGE, "a changed aggregate has an unknown kind, a partition outside [0, n_partitions), a negative key / value span, or bytes in a table that was passed as NULL");
  const int64_t n_batches = totals[0];
  const bool lz4 = f->codec == SURGE_SNAPSHOT_CODEC_LZ4;
  int64_t n_bytes = totals[1];  // of the uncompressed layout; LZ4 mode replaces it below
  FCHK(f, f->batches.reserve((size_t)n_batches * sizeof(Batch)));
  FCHK(f, f->out.reserve((size_t)n_bytes));
  try {
    f->h_batches.resize((size_t)n_batches);
  } catch (const std::bad_alloc&) {
    return ffail(f, E_NOMEM, "out of host memory");
  }
  hipLaunchKernelGGL(frame_batches_kernel, dim3(grid(P)), dim3(256), 0, st, (const int64_t*)f->pstart.p, P, c1, c2, c3, f->max_records, f->max_bytes,
                     (const int64_t*)f->d_next.p, true, (int64_t*)f->nb.p, (int64_t*)f->pbytes.p, (Batch*)f->batches.p);

  // 4. the bytes
  hipLaunchKernelGGL(frame_write_kernel, dim3(grid(n_sel)), dim3(256), 0, st, (const Batch*)f->batches.p, n_batches, order, (const int64_t*)f->sel.p, n_sel,
                     d_kind, (const uint32_t*)f->base.p, c1, c2, c3, d_keys_utf8, d_key_off, d_values, d_val_off, (uint8_t*)f->out.p);
  const uint8_t* d_final = (const uint8_t*)f->out.p;
  if (lz4) {
    // 4b. every batch's records section -> one LZ4 frame, the batches packed at their compressed sizes
    auto scan = [&](int64_t* v, size_t count) -> int32_t {  // exclusive, in place
      size_t need = 0;
      FCHK(f, rocprim::exclusive_scan(nullptr, need, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, count, rocprim::plus<int64_t>(), st));
      if (need > f->temp.cap) {
        FCHK(f, hipStreamSynchronize(st));  // earlier scans may still use the scratch
        FCHK(f, f->temp.reserve(need));
      }
      FCHK(f, rocprim::exclusive_scan(f->temp.p, need, (const int64_t*)v, v, (int64_t)0, count, rocprim::plus<int64_t>(), st));
      return OK;
    };
    FCHK(f, f->lz_nblk.reserve((size_t)(n_batches + 1) * 8));
    FCHK(f, f->lz_bbytes.reserve((size_t)(n_batches + 1) * 8));
    FCHK(f, f->lz_tmp.reserve((size_t)n_bytes));
    int64_t* blk_first = (int64_t*)f->lz_nblk.p;
    int64_t* new_off = (int64_t*)f->lz_bbytes.p;
    hipLaunchKernelGGL(frame_lz4_count_kernel, dim3(grid(n_batches + 1)), dim3(256), 0, st, (const Batch*)f->batches.p, n_batches, blk_first);
    if (const int32_t rc = scan(blk_first, (size_t)n_batches + 1)) return rc;
    int64_t n_blocks = 0;
    FCHK(f, hipMemcpyAsync(&n_blocks, blk_first + n_batches, 8, hipMemcpyDeviceToHost, st));
    FCHK(f, hipStreamSynchronize(st));
    if (n_blocks < n_batches || n_blocks > 0x7fffffffll)  // (every batch has a block; LzBlock.batch and the grids are 32 bits wide)
      return ffail(f, E_RANGE, n_blocks < n_batches ? "the LZ4 block count is inconsistent with the batches" : "more than 2^31 LZ4 blocks in one publish");
    FCHK(f, f->lz_blocks.reserve((size_t)n_blocks * sizeof(LzBlock)));
    FCHK(f, f->lz_bsz.reserve((size_t)(n_blocks + 1) * 8));
    const LzBlock* blocks = (const LzBlock*)f->lz_blocks.p;
    int64_t* bscan = (int64_t*)f->lz_bsz.p;
    hipLaunchKernelGGL(frame_lz4_blocks_kernel, dim3(grid(n_blocks)), dim3(256), 0, st, (const Batch*)f->batches.p, n_batches, (const int64_t*)blk_first,
                       n_blocks, (LzBlock*)f->lz_blocks.p);
    FCHK(f, hipMemsetAsync(bscan + n_blocks, 0, 8, st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(frame_lz4_block_kernel<kLzHashLogSmall>), dim3((unsigned)n_blocks), dim3(64), 0, st, blocks, n_blocks, 0, kLzSmall,
                       (const uint8_t*)f->out.p, (uint8_t*)f->lz_tmp.p, bscan);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(frame_lz4_block_kernel<kLzHashLog>), dim3((unsigned)n_blocks), dim3(64), 0, st, blocks, n_blocks, kLzSmall, kLzBlock,
                       (const uint8_t*)f->out.p, (uint8_t*)f->lz_tmp.p, bscan);
    if (const int32_t rc = scan(bscan, (size_t)n_blocks + 1)) return rc;
    hipLaunchKernelGGL(frame_lz4_batch_size_kernel, dim3(grid(n_batches + 1)), dim3(256), 0, st, n_batches, (const int64_t*)blk_first, (const int64_t*)bscan,
                       new_off);
    if (const int32_t rc = scan(new_off, (size_t)n_batches + 1)) return rc;
    // (nb is the scanned batch index of every partition, pbytes is free again: the spans of the compressed output)
    hipLaunchKernelGGL(frame_lz4_spans_kernel, dim3(grid(P + 1)), dim3(256), 0, st, P, (const int64_t*)f->nb.p, (const int64_t*)new_off, (int64_t*)f->pbytes.p);
    FCHK(f, hipGetLastError());
    FCHK(f, hipMemcpyAsync(f->part_byte_off.data(), f->pbytes.p, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, st));
    FCHK(f, hipStreamSynchronize(st));
    n_bytes = f->part_byte_off[(size_t)P];
    FCHK(f, f->lz_out.reserve((size_t)n_bytes));
    hipLaunchKernelGGL(frame_lz4_pack_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, blocks, (const int64_t*)blk_first, (const int64_t*)bscan,
                       (const int64_t*)new_off, (const uint8_t*)f->out.p, (const uint8_t*)f->lz_tmp.p, (uint8_t*)f->lz_out.p);
    hipLaunchKernelGGL(frame_lz4_readdress_kernel, dim3(grid(n_batches)), dim3(256), 0, st, (Batch*)f->batches.p, n_batches, (const int64_t*)new_off);
    d_final = (const uint8_t*)f->lz_out.p;
  }
  if ((size_t)n_bytes > f->pinned_cap) {
    if (f->pinned) (void)hipHostFree(f->pinned);
    f->pinned = nullptr;
    f->pinned_cap = 0;
    const size_t want = (size_t)n_bytes + (size_t)n_bytes / 4;
    void* hp = nullptr;
    FCHK(f, hipHostMalloc(&hp, want, hipHostMallocDefault));
    f->pinned = (uint8_t*)hp;
    f->pinned_cap = want;
  }
  hipLaunchKernelGGL(frame_header_kernel, dim3(grid(n_batches)), dim3(256), 0, st, (const Batch*)f->batches.p, n_batches, timestamp_ms, f->codec,
                     (uint8_t*)d_final);
  FCHK(f, hipGetLastError());
  FCHK(f, hipMemcpyAsync(f->pinned, d_final, (size_t)n_bytes, hipMemcpyDeviceToHost, st));
  FCHK(f, hipMemcpyAsync(f->h_batches.data(), f->batches.p, (size_t)n_batches * sizeof(Batch), hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));

  // 5. CRC-32C of every batch (attributes .. end), on the host's crc32 instruction, batches spread over a few threads
  {
    (void)surge_crc32c((const uint8_t*)"", 0);  // initialise the dispatch before threads race for it
    uint8_t* base = f->pinned;
    const std::vector<Batch>& hb = f->h_batches;
    std::atomic<int64_t> next{0};
    auto work = [&]() {
      for (int64_t i = next.fetch_add(1); i < n_batches; i = next.fetch_add(1)) {
        uint8_t* o = base + hb[(size_t)i].out_off;
        const uint32_t crc = surge_crc32c(o + 21, (int64_t)(kHeader - 21) + hb[(size_t)i].records_bytes);
        o[17] = (uint8_t)(crc >> 24); o[18] = (uint8_t)(crc >> 16); o[19] = (uint8_t)(crc >> 8); o[20] = (uint8_t)crc;
      }
    };
    unsigned hw = std::thread::hardware_concurrency();
    int n_threads = (int)(hw ? hw : 1);
    if (n_threads > 8) n_threads = 8;
    if ((int64_t)n_threads > n_batches) n_threads = (int)n_batches;
    if (n_bytes < (4 << 20)) n_threads = 1;
    std::vector<std::thread> th;
    try {
      for (int t = 1; t < n_threads; ++t) th.emplace_back(work);
    } catch (...) {  // the threads that did start, and this one, do the work
    }
    work();
    for (std::thread& t : th) t.join();
  }
  for (const Batch& b : f->h_batches) f->next_offset[(size_t)b.partition] += b.count;
  f->uncompressed_bytes = totals[1];
  span_reset.done = true;
  *bytes_out = f->pinned;
  if (n_records_out) *n_records_out = n_sel;
  if (n_batches_out) *n_batches_out = n_batches;
  return OK;
}

}  // extern "C"
