// ingest_order.hip — the device decoder's key table in KEY ORDER: a permutation of the dense indices sorted by the keys' bytes as
// unsigned bytes, a proper prefix in front of the longer key ("a" < "a\0" < "a\0\0" < "a\x01": Kafka's Bytes comparator, and for
// valid UTF-8 Python's sorted() on str).  The hash table and the arena (first-delivered order) know nothing of it; range reads do.
//   chunk      one thread per position: bytes [4p, 4p + 4) of its key, big-endian, zero behind the key's end, with the bytes the
//              key has left from 4p on clipped to 0..4 — (group << 35 | chunk << 3 | left) is the pass's sort key.  `left` is what
//              keeps "a" in front of "a\0": zero padding alone makes them one key.
//   sort       (rocPRIM) a stable radix sort of (sort key, index) over the bits in use
//   flag+scan  a position whose sort key differs from the one in front of it opens a group; the groups are re-numbered by a
//              (rocPRIM) inclusive scan of the flags
//   bounds     two threads: lower_bound(from) and upper_bound(to) over the order, bytes compared with the arena
//   gather     the ids of a row list, back to back: lengths (a row outside the table raises a flag), a scan, the copy
// The pass loop — most significant chunk first, until every group is one key — is the host object's (ingest_reads.hip): this
// unit launches what it is told to and waits for nothing.  Keys are unique, so a group of several keys holds only keys that go
// on behind the bytes compared so far: the loop ends after at most ceil(max_len / 4) + 1 passes.  Keys that are alone in their
// group stay in the later passes (they sort by their group alone): see DESIGN §7.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ingest_device.h"

namespace surge {
namespace ingest {
namespace {

// four bytes from p on as the number that orders them: the first byte the most significant
__device__ __forceinline__ uint32_t load4_be(const uint8_t* p) { return __builtin_bswap32(load4(p)); }
// ... of which only the first `left` (1..3) count
__device__ __forceinline__ uint32_t first_bytes(uint32_t be, int64_t left) { return be & ~(0xffffffffu >> (8 * (int)left)); }

__global__ void __launch_bounds__(256) order_init_kernel(uint32_t* __restrict__ idx, uint32_t* __restrict__ grp, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  idx[j] = (uint32_t)j;
  grp[j] = 0u;
}

// Reads the arena at most 7 bytes behind a key's last byte (load4): the arena is readable 16 bytes behind its end.  A key that
// has no byte left is not read at all.  *live becomes 1 when some key has a byte in this pass (every writer writes the same 1).
__global__ void __launch_bounds__(256) order_chunk_kernel(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ grp, int64_t n, const uint8_t* __restrict__ arena,
                                                         const int64_t* __restrict__ key_off, int64_t at, unsigned long long* __restrict__ sort_key,
                                                         uint32_t* __restrict__ live) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = idx[j];
  const int64_t a0 = key_off[k];
  int64_t left = key_off[k + 1] - a0 - at;
  left = left < 0 ? 0 : left > 4 ? 4 : left;
  uint32_t chunk = 0u;
  if (left > 0) {
    chunk = load4_be(arena + a0 + at);
    if (left < 4) chunk = first_bytes(chunk, left);
    if (*live == 0u) *live = 1u;
  }
  sort_key[j] = ((unsigned long long)grp[j] << 35) | ((unsigned long long)chunk << 3) | (unsigned long long)left;
}

__global__ void __launch_bounds__(256) order_flag_kernel(const unsigned long long* __restrict__ sorted_key, int64_t n, uint32_t* __restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  flag[j] = j > 0 && sorted_key[j] != sorted_key[j - 1] ? 1u : 0u;
}

__global__ void __launch_bounds__(256) order_finish_kernel(const uint32_t* __restrict__ idx, int64_t n, int64_t* __restrict__ ord) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) ord[j] = (int64_t)idx[j];
}

// key a (in the arena) against the bound b: < 0, 0, > 0.  Unsigned, four bytes a load; both are readable behind their ends.
__device__ __forceinline__ int compare_key(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
  const int64_t m = la < lb ? la : lb;
  for (int64_t i = 0; i < m; i += 4) {
    uint32_t x = load4_be(a + i), y = load4_be(b + i);
    if (m - i < 4) {
      x = first_bytes(x, m - i);
      y = first_bytes(y, m - i);
    }
    if (x != y) return x < y ? -1 : 1;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// thread 0: out[0] = the first position whose key is >= from; thread 1: out[1] = the first position whose key is > to.  A bound of
// negative length is none: 0 / n_keys.  Each search reads ord and key_off inside [0, n_keys) only (lo <= mid < hi <= n_keys).
__global__ void __launch_bounds__(64) order_bounds_kernel(const int64_t* __restrict__ ord, int64_t n_keys, const uint8_t* __restrict__ arena,
                                                         const int64_t* __restrict__ key_off, const uint8_t* __restrict__ bounds, int64_t from_len, int64_t to_at,
                                                         int64_t to_len, int64_t* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= 2) return;
  const bool upper = t == 1;
  const int64_t len = upper ? to_len : from_len;
  const uint8_t* b = bounds + (upper ? to_at : 0);
  if (len < 0) {
    out[t] = upper ? n_keys : 0;
    return;
  }
  int64_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int64_t k = ord[mid];
    const int64_t a0 = key_off[k];
    const int c = compare_key(arena + a0, key_off[k + 1] - a0, b, len);
    if (upper ? c <= 0 : c < 0) lo = mid + 1; else hi = mid;
  }
  out[t] = lo;
}

// len[q] = bytes of the id of rows[q] (entry n: 0, the scan's total lands there); a row outside [0, n_keys) sets *bad
__global__ void __launch_bounds__(256) key_len_kernel(const int64_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ key_off, int64_t n_keys,
                                                     unsigned long long* __restrict__ len, uint32_t* __restrict__ bad) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > n) return;
  unsigned long long l = 0ull;
  if (q < n) {
    const int64_t r = rows[q];
    if (r < 0 || r >= n_keys) *bad = 1u;
    else l = (unsigned long long)(key_off[r + 1] - key_off[r]);
  }
  len[q] = l;
}

// behind the checks (every row is inside the table, out holds at[n] bytes): the offsets, and each id's bytes from the arena
__global__ void __launch_bounds__(256) key_gather_kernel(const int64_t* __restrict__ rows, int64_t n, const uint8_t* __restrict__ arena, const int64_t* __restrict__ key_off,
                                                        const unsigned long long* __restrict__ at, uint8_t* __restrict__ out, int64_t* __restrict__ off_out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > n) return;
  const int64_t dst = (int64_t)at[q];
  off_out[q] = dst;
  if (q == n) return;
  const int64_t r = rows[q];
  const int64_t a0 = key_off[r], l = key_off[r + 1] - a0;
  for (int64_t b = 0; b < l; ++b) out[dst + b] = arena[a0 + b];
}

#define LAUNCH_1D(kernel, n, st, ...) hipLaunchKernelGGL(kernel, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)

}  // namespace

hipError_t order_temp_bytes(int64_t n, size_t* bytes, hipStream_t st) {
  size_t tb_sort = 0, tb_scan = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, tb_sort, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (size_t)n, 0u, 64u, st);
  if (e == hipSuccess) e = rocprim::inclusive_scan(nullptr, tb_scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, rocprim::plus<uint32_t>(), st);
  *bytes = tb_sort > tb_scan ? tb_sort : tb_scan;
  return e;
}

hipError_t key_gather_temp_bytes(int64_t n, size_t* bytes, hipStream_t st) {
  return rocprim::exclusive_scan(nullptr, *bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), st);
}

hipError_t launch_order_init(const OrderScratch& sc, int64_t n, hipStream_t st) {
  LAUNCH_1D(order_init_kernel, n, st, sc.idx_in, sc.grp, n);
  return hipGetLastError();
}

hipError_t launch_order_pass(const KeyTable& k, int64_t pass, int group_bits, OrderScratch& sc, hipStream_t st) {
  const int64_t n = k.n_keys;
  hipError_t e = hipMemsetAsync(sc.live, 0, 4, st);
  if (e != hipSuccess) return e;
  LAUNCH_1D(order_chunk_kernel, n, st, (const uint32_t*)sc.idx_in, (const uint32_t*)sc.grp, n, (const uint8_t*)k.arena, (const int64_t*)k.key_off, 4 * pass, sc.key_in, sc.live);
  size_t tb = sc.temp_bytes;
  e = rocprim::radix_sort_pairs(sc.temp, tb, (const unsigned long long*)sc.key_in, sc.key_out, (const uint32_t*)sc.idx_in, sc.idx_out, (size_t)n, 0u,
                                (unsigned)(35 + group_bits), st);
  if (e != hipSuccess) return e;
  LAUNCH_1D(order_flag_kernel, n, st, (const unsigned long long*)sc.key_out, n, sc.flag);
  tb = sc.temp_bytes;
  e = rocprim::inclusive_scan(sc.temp, tb, (const uint32_t*)sc.flag, sc.grp, (size_t)n, rocprim::plus<uint32_t>(), st);
  uint32_t* was = sc.idx_in;  // the next pass — or the finish — reads the indices this one sorted
  sc.idx_in = sc.idx_out;
  sc.idx_out = was;
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_order_finish(const OrderScratch& sc, int64_t n, int64_t* ord, hipStream_t st) {
  LAUNCH_1D(order_finish_kernel, n, st, (const uint32_t*)sc.idx_in, n, ord);
  return hipGetLastError();
}

hipError_t launch_order_bounds(const KeyTable& k, const int64_t* ord, const uint8_t* bounds, int64_t from_len, int64_t to_at, int64_t to_len, int64_t* lo_hi, hipStream_t st) {
  hipLaunchKernelGGL(order_bounds_kernel, dim3(1), dim3(64), 0, st, ord, k.n_keys, (const uint8_t*)k.arena, (const int64_t*)k.key_off, bounds, from_len, to_at, to_len, lo_hi);
  return hipGetLastError();
}

hipError_t launch_key_lengths(const KeyTable& k, const int64_t* rows, int64_t n, const KeyGatherScratch& sc, hipStream_t st) {
  hipError_t e = hipMemsetAsync(sc.bad, 0, 4, st);
  if (e != hipSuccess) return e;
  LAUNCH_1D(key_len_kernel, n + 1, st, rows, n, (const int64_t*)k.key_off, k.n_keys, sc.len, sc.bad);
  size_t tb = sc.temp_bytes;
  e = rocprim::exclusive_scan(sc.temp, tb, (const unsigned long long*)sc.len, sc.at, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), st);
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_key_gather(const KeyTable& k, const int64_t* rows, int64_t n, const KeyGatherScratch& sc, uint8_t* out, int64_t* off_out, hipStream_t st) {
  LAUNCH_1D(key_gather_kernel, n + 1, st, rows, n, (const uint8_t*)k.arena, (const int64_t*)k.key_off, (const unsigned long long*)sc.at, out, off_out);
  return hipGetLastError();
}

}  // namespace ingest
}  // namespace surge
