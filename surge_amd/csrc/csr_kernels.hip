// csr_kernels.hip — the CSR of a bound log or a micro-batch made ready for a fold; nothing here folds an event.
//   plan     : the flat kernel's wave tasks, contiguous ranges of whole segments of about task_events events each
//   analyze  : what the engine chooses a kernel by (empty / longest / uniform segments, the span of the offsets)
//   compact  : the kernel-facing CSR of a log with empty segments (the lane kernels want none), stable
//   fill     : the states of the aggregates without events (their prior snapshot, or None)
#include "replay_internal.h"

namespace surge {
namespace {

// first s in [0, n_seg] with off[s] >= target
__device__ __forceinline__ int64_t first_at_least(const int64_t* __restrict__ off, int64_t n_seg, int64_t target) {
  int64_t lo = 0, hi = n_seg;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- plan: task k owns segments [lower_bound(off, off[0] + k*T), lower_bound(off, off[0] + (k+1)*T)) ----
__global__ void plan_kernel(const int64_t* __restrict__ off, int64_t n_seg, int64_t task_events,
                            int64_t n_tasks, int64_t* __restrict__ plan) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_tasks) return;
  if (k == n_tasks) { plan[k] = n_seg; return; }
  plan[k] = first_at_least(off, n_seg, off[0] + k * task_events);
}

// the same plan over a segment count that only the device knows yet (micro-batches: the group count the device group-by
// has just produced — no host round trip between the group-by and the fold)
__global__ void plan_dev_kernel(const int64_t* __restrict__ off, const uint32_t* __restrict__ d_n_seg, int64_t task_events,
                                int64_t n_tasks, int64_t* __restrict__ plan) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_tasks) return;
  const int64_t n_seg = (int64_t)d_n_seg[0];
  if (k == n_tasks || n_seg == 0) { plan[k] = n_seg; return; }  // no segments: every task is empty
  plan[k] = first_at_least(off, n_seg, off[0] + k * task_events);
}

__global__ void analyze_csr_kernel(const int64_t* __restrict__ off, int64_t n_seg, CsrAnalysis* res) {
  __shared__ unsigned long long s_empty;
  __shared__ long long s_max;
  __shared__ int s_bad, s_nonuni;
  if (threadIdx.x == 0) { s_empty = 0; s_max = 0; s_bad = 0; s_nonuni = 0; }
  __syncthreads();
  const int64_t len0 = n_seg > 0 ? off[1] - off[0] : 0;
  unsigned long long empty = 0;
  long long mx = 0;
  int bad = 0, nonuni = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_seg; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t len = off[s + 1] - off[s];
    if (len < 0) bad = 1;
    if (len == 0) ++empty;
    if (len != len0) nonuni = 1;
    if (len > mx) mx = len;
  }
  if (empty) atomicAdd(&s_empty, empty);
  if (mx) atomicMax(&s_max, mx);
  if (bad) atomicOr(&s_bad, 1);
  if (nonuni) atomicOr(&s_nonuni, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_empty) atomicAdd((unsigned long long*)&res->n_empty, s_empty);
    if (s_max) atomicMax((long long*)&res->max_len, s_max);
    if (s_bad) atomicOr(&res->bad, 1);
    if (s_nonuni) atomicOr(&res->nonuniform, 1);
    if (blockIdx.x == 0) {
      res->len0 = len0;
      res->first = off[0];
      res->last = off[n_seg];
    }
  }
}

// Aggregates without events keep their prior snapshot (or stay None).
__global__ void fill_empty_kernel(const int64_t* __restrict__ off, int64_t n_seg, const uint4* __restrict__ init,
                                  uint4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 16 B quarter of a state per thread
  const int64_t s = i >> 2;
  if (s >= n_seg) return;
  if (off[s + 1] != off[s]) return;
  uint4 v;
  v.x = v.y = v.z = v.w = 0u;
  if (init) v = init[i];
  out[i] = v;
}

constexpr int kCompactBlock = 1024;

__global__ void __launch_bounds__(kCompactBlock) compact_count_kernel(const int64_t* __restrict__ off, int64_t n_seg,
                                                                       int64_t* __restrict__ block_counts) {
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int64_t s = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
  const bool nz = s < n_seg && off[s + 1] != off[s];
  const int c = __popcll(__ballot(nz));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s_cnt;
}

// single block: exclusive scan of block_counts[0..nb) in place, total appended at [nb]
__global__ void __launch_bounds__(1024) compact_scan_kernel(int64_t* block_counts, int64_t nb) {
  __shared__ int64_t s_part[1024];
  const int tid = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024;
  const int64_t b0 = tid * per, b1 = (b0 + per < nb) ? b0 + per : nb;
  int64_t sum = 0;
  for (int64_t b = b0; b < b1; ++b) sum += block_counts[b];
  s_part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int i = 0; i < 1024; ++i) { const int64_t v = s_part[i]; s_part[i] = run; run += v; }
    block_counts[nb] = run;
  }
  __syncthreads();
  int64_t run = s_part[tid];
  for (int64_t b = b0; b < b1; ++b) { const int64_t v = block_counts[b]; block_counts[b] = run; run += v; }
}

__global__ void __launch_bounds__(kCompactBlock) compact_scatter_kernel(const int64_t* __restrict__ off, int64_t n_seg,
                                                                         const int64_t* __restrict__ block_counts,
                                                                         int64_t* __restrict__ nz_off,
                                                                         int64_t* __restrict__ nz_map) {
  __shared__ int s_wave[kCompactBlock / 64];
  const int64_t s = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
  const bool nz = s < n_seg && off[s + 1] != off[s];
  const unsigned long long bal = __ballot(nz);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  if (nz) {
    const int64_t r = block_counts[blockIdx.x] + base + __popcll(bal & ((1ull << lane) - 1ull));
    nz_off[r] = off[s];
    nz_map[r] = s;
  }
  const int64_t nb = (n_seg + kCompactBlock - 1) / kCompactBlock;
  if (blockIdx.x == 0 && threadIdx.x == 0) nz_off[block_counts[nb]] = off[n_seg];
}

}  // namespace

hipError_t launch_plan(const int64_t* off, int64_t n_seg, int64_t task_events, int64_t n_tasks, int64_t* plan,
                       hipStream_t stream) {
  const int64_t n = n_tasks + 1;
  hipLaunchKernelGGL(plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, off, n_seg, task_events,
                     n_tasks, plan);
  return hipGetLastError();
}

hipError_t launch_plan_dev(const int64_t* off, const uint32_t* d_n_seg, int64_t task_events, int64_t n_tasks, int64_t* plan,
                           hipStream_t stream) {
  const int64_t n = n_tasks + 1;
  hipLaunchKernelGGL(plan_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, off, d_n_seg, task_events, n_tasks, plan);
  return hipGetLastError();
}

hipError_t launch_analyze_csr(const int64_t* off, int64_t n_seg, CsrAnalysis* d_result, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(d_result, 0, sizeof(CsrAnalysis), stream);
  if (e != hipSuccess) return e;
  int64_t blocks = (n_seg + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(analyze_csr_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, off, n_seg, d_result);
  return hipGetLastError();
}

hipError_t launch_fill_empty(const int64_t* off, int64_t n_seg, const uint4* init, uint4* out, hipStream_t stream) {
  if (n_seg <= 0) return hipSuccess;
  const int64_t n = n_seg * 4;
  hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, off, n_seg, init, out);
  return hipGetLastError();
}

hipError_t launch_exclusive_scan_i64(int64_t* v, int64_t n, hipStream_t stream) {
  if (n < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, stream, v, n);
  return hipGetLastError();
}

hipError_t launch_compact_nonempty(const int64_t* off, int64_t n_seg, int64_t* d_block_counts, int64_t* nz_off,
                                   int64_t* nz_map, hipStream_t stream) {
  if (n_seg <= 0) return hipSuccess;
  const int64_t nb = (n_seg + kCompactBlock - 1) / kCompactBlock;
  hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb), dim3(kCompactBlock), 0, stream, off, n_seg, d_block_counts);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, stream, d_block_counts, nb);
  hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)nb), dim3(kCompactBlock), 0, stream, off, n_seg,
                     d_block_counts, nz_off, nz_map);
  return hipGetLastError();
}

}  // namespace surge
