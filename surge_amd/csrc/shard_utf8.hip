// shard_utf8.hip — the shard map straight from UTF-8 ids in device memory (surge_replay_partition_hash_utf8_device): what lets a
// key table that never left the GPU (surge_device_decoder_key_table) be partitioned there.  The routine is shard_utf8.h, the
// one the host export runs; this unit adds the transport.
//
// One lane per id, 256 ids per workgroup.  Ids are short (13 - 40 bytes) and lie back to back, so a workgroup's ids are one
// contiguous span of the arena: it is staged into LDS with aligned 16-byte loads (the unaligned head and tail byte by byte:
// nothing outside [str_off[first], str_off[last + 1]) is ever read, so the caller owes no slack) and every lane parses its
// id out of LDS.  A workgroup whose span does not fit the stage (one long id among its 256 is enough) reads from global
// memory, byte by byte, each lane inside its own id.
#include "engine_internal.h"
#include "shard_utf8.h"

namespace surge {
namespace {

constexpr int kShBlock = 256;
constexpr int kShStageBytes = 16 * 1024;  // 64 bytes an id; with it eight workgroups (every wave slot) fit a CU's 160 KiB

enum { SH_BAD = 0, SH_FIRST_BAD = 1, SH_N_COUNTS = 2 };

template <bool CUT>
__global__ void __launch_bounds__(kShBlock) partition_hash_utf8_kernel(const uint8_t* __restrict__ utf8, const int64_t* __restrict__ str_off,
                                                                       int64_t n, int32_t n_partitions, int32_t* __restrict__ part_out,
                                                                       unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kShStageBytes];
  const int64_t r0 = (int64_t)blockIdx.x * kShBlock;
  const int64_t r = r0 + threadIdx.x;
  const int64_t r1 = (r0 + kShBlock < n) ? r0 + kShBlock : n;
  const int64_t base = str_off[r0], end = str_off[r1];
  const uint32_t shift = (uint32_t)((uintptr_t)(utf8 + base) & 15u);
  const bool staged = end >= base && (end - base) + shift <= kShStageBytes;  // block-uniform
  if (staged) {
    const uint32_t total = (uint32_t)(end - base);
    const uint8_t* g = utf8 + base - shift;         // 16-byte aligned; LDS offset i <-> g[i]
    const uint32_t lo = shift, hi = shift + total;  // the valid span in that frame: only g[lo .. hi) is read
    const uint32_t body_lo = (lo + 15u) & ~15u, body_hi = hi & ~15u;
    if (body_lo <= body_hi) {
      for (uint32_t i = lo + threadIdx.x; i < body_lo; i += kShBlock) stage[i] = g[i];
      for (uint32_t i = body_lo + threadIdx.x * 16u; i < body_hi; i += kShBlock * 16u) *(uint4*)(stage + i) = *(const uint4*)(g + i);
      for (uint32_t i = body_hi + threadIdx.x; i < hi; i += kShBlock) stage[i] = g[i];
    } else {
      for (uint32_t i = lo + threadIdx.x; i < hi; i += kShBlock) stage[i] = g[i];
    }
    __syncthreads();
  }
  bool bad = false;
  if (r < n) {
    const int64_t o0 = str_off[r], o1 = str_off[r + 1];
    int32_t part = -1;
    if (o0 >= base && o1 <= end && o1 >= o0) {  // (offsets that are not monotone: nothing of the id is read)
      if (staged) part = shard_partition_utf8<CUT>((const uint8_t*)stage + shift + (uint32_t)(o0 - base), o1 - o0, n_partitions);
      else part = shard_partition_utf8<CUT>(utf8 + o0, o1 - o0, n_partitions);
    }
    part_out[r] = part;
    bad = part < 0;
  }
  // one atomic per wave with a malformed id in it (called by every lane of the block)
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & (warpSize - 1)) == (unsigned)(__ffsll((long long)m) - 1)) {
    atomicAdd(&counts[SH_BAD], (unsigned long long)__popcll(m));
    atomicMin(&counts[SH_FIRST_BAD], (unsigned long long)r);  // the wave's lowest: lanes are in row order
  }
}

// counts: SH_N_COUNTS u64 (zeroed here, SH_FIRST_BAD to ~0)
hipError_t launch_partition_hash_utf8(const uint8_t* utf8, const int64_t* str_off, int64_t n, int32_t n_partitions, int32_t* part_out,
                                      bool up_to_colon, unsigned long long* counts, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(counts, 0, 8, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(counts + SH_FIRST_BAD, 0xFF, 8, stream);
  if (e != hipSuccess || n <= 0) return e;
  const dim3 grid((unsigned)((n + kShBlock - 1) / kShBlock)), block(kShBlock);
  if (up_to_colon) hipLaunchKernelGGL(partition_hash_utf8_kernel<true>, grid, block, 0, stream, utf8, str_off, n, n_partitions, part_out, counts);
  else hipLaunchKernelGGL(partition_hash_utf8_kernel<false>, grid, block, 0, stream, utf8, str_off, n, n_partitions, part_out, counts);
  return hipGetLastError();
}

}  // namespace
}  // namespace surge

using namespace surge;

extern "C" int32_t surge_replay_partition_hash_utf8_device(surge_replay_handle* h, const uint8_t* d_utf8, const int64_t* d_str_off, int64_t n,
                                                           int32_t n_partitions, int32_t up_to_colon, int32_t* d_part_out,
                                                           int64_t* first_bad_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n < 0 || n_partitions <= 0) return fail(h, SURGE_E_INVALID, "bad n or n_partitions");
  if (n > (int64_t)0x7fffffff * kShBlock) return fail(h, SURGE_E_INVALID, "more ids than one launch takes");
  if (n == 0) {
    if (first_bad_out) *first_bad_out = -1;
    return SURGE_OK;
  }
  if (!d_utf8 || !d_str_off || !d_part_out) return fail(h, SURGE_E_INVALID, "NULL buffer");
  DeviceGuard g(h->device);
  HIPCHK(h, h->shard_counts.reserve(SH_N_COUNTS * 8));
  unsigned long long* d_counts = (unsigned long long*)h->shard_counts.ptr;
  HIPCHK(h, launch_partition_hash_utf8(d_utf8, d_str_off, n, n_partitions, d_part_out, up_to_colon != 0, d_counts, h->stream));
  unsigned long long c[SH_N_COUNTS] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(c, d_counts, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (first_bad_out) *first_bad_out = c[SH_BAD] ? (int64_t)c[SH_FIRST_BAD] : -1;
  if (c[SH_BAD])
    return fail(h, SURGE_E_CORRUPT, std::to_string(c[SH_BAD]) + " of " + std::to_string(n) + " ids are not well-formed UTF-8 (the first: id " +
                                        std::to_string(c[SH_FIRST_BAD]) + "); their partition is -1");
  return SURGE_OK;
}
