// frame_records.hip — the uncompressed framing of the device framer: its six kernels and their launchers, and the select / sort /
// scan steps (the one unit of the framer that includes rocPRIM).
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
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/surge_replay.h"  // SURGE_SNAP_*
#include "frame_device.h"

namespace surge {
namespace frame {
namespace {

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

}  // namespace

hipError_t select_changed(void* temp, size_t& temp_bytes, const uint8_t* kind, int64_t* sel, int64_t* n_sel, int64_t n, hipStream_t st) {
  return rocprim::select(temp, temp_bytes, rocprim::counting_iterator<int64_t>(0), kind, sel, n_sel, (size_t)n, st);
}

hipError_t sort_by_partition(void* temp, size_t& temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                             int64_t n_sel, unsigned bits, hipStream_t st) {
  using SortConfig = rocprim::default_config;  // (merge sort up to 2^20 records; a lower limit was measured for K3's group-by and dropped: stream_kernels.hip)
  return rocprim::radix_sort_pairs<SortConfig>(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n_sel, 0u, bits, st);
}

hipError_t scan_exclusive(void* temp, size_t& temp_bytes, int64_t* v, size_t count, hipStream_t st) {
  return rocprim::exclusive_scan(temp, temp_bytes, (const int64_t*)v, v, (int64_t)0, count, rocprim::plus<int64_t>(), st);
}

void launch_frame_size(const int64_t* sel, int64_t n_sel, const uint8_t* kind, const int32_t* part, int32_t n_part, const int64_t* key_off,
                       const int64_t* val_off, bool have_keys, bool have_values, uint32_t* keys, uint32_t* vals, uint32_t* base, uint32_t* bad,
                       hipStream_t st) {
  hipLaunchKernelGGL(frame_size_kernel, dim3(grid(n_sel)), dim3(256), 0, st, sel, n_sel, kind, part, n_part, key_off, val_off, have_keys, have_values, keys,
                     vals, base, bad);
}

void launch_frame_sizes3(const uint32_t* order, const uint32_t* base, int64_t n_sel, int64_t* c1, int64_t* c2, int64_t* c3, hipStream_t st) {
  hipLaunchKernelGGL(frame_sizes3_kernel, dim3(grid(n_sel + 1)), dim3(256), 0, st, order, base, n_sel, c1, c2, c3);
}

void launch_frame_pstart(const uint32_t* sorted_part, int64_t n_sel, int32_t n_part, int64_t* pstart, hipStream_t st) {
  hipLaunchKernelGGL(frame_pstart_kernel, dim3(grid(n_part + 1)), dim3(256), 0, st, sorted_part, n_sel, n_part, pstart);
}

void launch_frame_batches(const int64_t* pstart, int32_t n_part, const int64_t* c1, const int64_t* c2, const int64_t* c3, int32_t max_records,
                          int64_t max_bytes, const int64_t* next_offset, bool emit, int64_t* nb, int64_t* pbytes, Batch* batches, hipStream_t st) {
  hipLaunchKernelGGL(frame_batches_kernel, dim3(grid(n_part)), dim3(256), 0, st, pstart, n_part, c1, c2, c3, max_records, max_bytes, next_offset, emit, nb,
                     pbytes, batches);
}

void launch_frame_write(const Batch* batches, int64_t n_batches, const uint32_t* order, const int64_t* sel, int64_t n_sel, const uint8_t* kind,
                        const uint32_t* base, const int64_t* c1, const int64_t* c2, const int64_t* c3, const uint8_t* keys_utf8, const int64_t* key_off,
                        const uint8_t* values, const int64_t* val_off, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(frame_write_kernel, dim3(grid(n_sel)), dim3(256), 0, st, batches, n_batches, order, sel, n_sel, kind, base, c1, c2, c3, keys_utf8,
                     key_off, values, val_off, out);
}

void launch_frame_header(const Batch* batches, int64_t n_batches, int64_t timestamp_ms, int32_t codec, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(frame_header_kernel, dim3(grid(n_batches)), dim3(256), 0, st, batches, n_batches, timestamp_ms, codec, out);
}

}  // namespace frame
}  // namespace surge
