// state_strings.hip — the string fields of serialized state values -> a side string column on the device
// (surge_replay_merge_state_strings): what surge_replay_decode_json_states validates and reports as still-escaped spans
// becomes, per SURGE_JP_STR column, the CSR column surge_replay_set_encode_strings takes.
//
// A load names some aggregates; the others keep the string they had.  Per aggregate a:
//   winner   the highest record with status OK that names a (win1[a] = record + 1; 0 = none)  -> the unescaped bytes of
//            its span (sp_unescape, state_parse.h: the rules the decoder validated the span with), nothing for a tombstone
//   kept     no winner and a < n_prev                                                         -> the previous string
//   else     empty
// Two passes around the encoder's exclusive scan, as surge_replay_encode_json: lengths into out_off, then bytes.
// Record side (ss_new_kernel): one lane per record, 256 per block; a block's values are contiguous, so they are staged in
// LDS with 16-byte loads exactly as state_decode_kernel stages them (LDS offset == global address mod 16, head and tail
// by bytes, nothing outside the span read) and a winner's lane unescapes its span out of LDS; a block whose values
// exceed the stage reads them from global (block-uniform choice).
// Aggregate side (ss_kept_*): kept strings of consecutive aggregates are consecutive in the previous column AND in the new
// one, so a block of 256 aggregates copies its output span in aligned 16-byte pieces, each from one unaligned 16-byte
// read of the previous column; a piece that touches a winner's bytes, a break in the previous column or the span's
// ends goes byte by byte and skips the bytes that are not kept.  (ingest_intern.hip's value_gather_kernel copies EVERY
// record of a run and reads up to 7 bytes behind a value, into the slack of the decoder's staged bytes: a column has
// neither, so it is not launched here.)
// Every byte either side stores lies inside [out_off[a], out_off[a + 1]) of the aggregate it belongs to.
#include "replay_internal.h"
#include "state_parse.h"

namespace surge {
namespace {

constexpr int kSsBlock = 256;
constexpr int kSsStageBytes = 32 * 1024;

__global__ void __launch_bounds__(kSsBlock) ss_winner_kernel(const int64_t* __restrict__ agg_idx, const uint8_t* __restrict__ status, int64_t n_records,
                                                             int64_t n_agg, unsigned long long* __restrict__ win1, unsigned long long* __restrict__ bad) {
  const int64_t r = (int64_t)blockIdx.x * kSsBlock + threadIdx.x;
  if (r >= n_records) return;
  const int64_t a = agg_idx ? agg_idx[r] : r;
  if (a < 0 || a >= n_agg) {
    atomicAdd(bad, 1ull);
    return;
  }
  if (status[r] == SURGE_STATE_DECODE_OK) atomicMax(&win1[a], (unsigned long long)r + 1ull);
}

// lengths of the aggregates without a winner (a winner's length is its record's lane's to write)
__global__ void __launch_bounds__(kSsBlock) ss_kept_len_kernel(const StateStringsParams p) {
  const int64_t a = (int64_t)blockIdx.x * kSsBlock + threadIdx.x;
  if (a >= p.n_agg || (p.win1 && p.win1[a])) return;
  int64_t len = 0;
  if (a < p.n_prev && p.prev) {
    len = p.prev_off[a + 1] - p.prev_off[a];
    if (len < 0) len = 0;
  }
  p.out_off[a] = len;
}

// WRITE == false: out_off[a] = the unescaped length of the winner's span; true: the bytes, behind the scan
template <bool WRITE>
__global__ void __launch_bounds__(kSsBlock) ss_new_kernel(const StateStringsParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ss_stage[];
  const int64_t r0 = (int64_t)blockIdx.x * kSsBlock;
  const int64_t r = r0 + threadIdx.x;
  const int64_t r1 = (r0 + kSsBlock < p.n_records) ? r0 + kSsBlock : p.n_records;
  const int64_t base = p.value_off[r0], end = p.value_off[r1];
  const uint32_t shift = (uint32_t)((uintptr_t)(p.values + base) & 15u);
  const bool staged = p.values && end > base && (end - base) + shift <= kSsStageBytes;  // block-uniform
  if (staged) {
    const uint32_t total = (uint32_t)(end - base);
    const uint8_t* g = p.values + base - shift;     // 16-byte aligned; LDS offset i <-> g[i]
    const uint32_t lo = shift, hi = shift + total;  // the valid span in that frame
    const uint32_t body_lo = (lo + 15u) & ~15u, body_hi = hi & ~15u;
    if (body_lo <= body_hi) {
      for (uint32_t i = lo + threadIdx.x; i < body_lo; i += kSsBlock) ss_stage[i] = g[i];
      for (uint32_t i = body_lo + threadIdx.x * 16u; i < body_hi; i += kSsBlock * 16u) *(uint4*)(ss_stage + i) = *(const uint4*)(g + i);
      for (uint32_t i = body_hi + threadIdx.x; i < hi; i += kSsBlock) ss_stage[i] = g[i];
    } else {
      for (uint32_t i = lo + threadIdx.x; i < hi; i += kSsBlock) ss_stage[i] = g[i];
    }
    __syncthreads();
  }
  if (r >= p.n_records || p.status[r] != SURGE_STATE_DECODE_OK) return;
  const int64_t a = p.agg_idx ? p.agg_idx[r] : r;  // in range: ss_winner_kernel counted the ones that are not, and nothing ran
  if (p.win1[a] != (unsigned long long)r + 1ull) return;
  // the span, only if it lies inside the record's value and that inside the block's (anything else reads as empty)
  const int64_t o0 = p.value_off[r], o1 = p.value_off[r + 1];
  const uint8_t* raw = nullptr;
  int64_t raw_len = 0;
  if (p.values && o0 >= base && o1 <= end && o1 > o0) {
    const int64_t* sp = p.spans + r * (2 * SURGE_JSON_STRING_COLUMNS) + 2 * p.column;
    const int64_t so = sp[0], sl = sp[1];
    if (so >= 0 && sl > 0 && so <= o1 - o0 && sl <= o1 - o0 - so) {
      raw = (staged ? ss_stage + shift + (o0 - base) : p.values + o0) + so;
      raw_len = sl;
    }
  }
  int64_t n = 0;
  if (!WRITE) {
    if (raw_len > 0 && sp_unescape(raw, raw_len, nullptr, 0, &n) != SURGE_STATE_DECODE_OK) n = 0;
    p.out_off[a] = n;
  } else {
    const int64_t d0 = p.out_off[a], cap = p.out_off[a + 1] - d0;  // == the length pass's n: sp_unescape never writes beyond it
    if (raw_len > 0 && cap > 0) (void)sp_unescape(raw, raw_len, p.out + d0, cap, &n);
  }
}

// the aggregate of the block whose bytes hold output offset q (off[0] <= q < off[n]): the first whose end lies behind q
__device__ __forceinline__ int32_t ss_find(const int64_t* off, int32_t n, int64_t q) {
  int32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > q) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kSsBlock) ss_kept_bytes_kernel(const StateStringsParams p) {
  __shared__ int64_t off[kSsBlock + 1];   // out_off of the block's aggregates
  __shared__ int32_t wc[kSsBlock + 1];    // winners among the block's aggregates [0, k)
  __shared__ int32_t wave_total[kSsBlock / 64];
  const int t = threadIdx.x;
  const int64_t a0 = (int64_t)blockIdx.x * kSsBlock;
  const int32_t n = p.n_agg - a0 < kSsBlock ? (int32_t)(p.n_agg - a0) : kSsBlock;
  if (t < n) off[t] = p.out_off[a0 + t];
  if (t == 0) off[n] = p.out_off[a0 + n];
  const bool w = t < n && p.win1 && p.win1[a0 + t];
  const unsigned long long m = __ballot(w);
  if ((t & 63) == 0) wave_total[t >> 6] = __popcll(m);
  __syncthreads();
  int32_t before = __popcll(m & ((1ull << (t & 63)) - 1ull));
  for (int k = 0; k < (t >> 6); ++k) before += wave_total[k];
  wc[t] = before;
  if (t == kSsBlock - 1) wc[kSsBlock] = before + (w ? 1 : 0);
  __syncthreads();
  const int64_t d0 = off[0], d1 = off[n];
  if (d1 <= d0 || wc[n] == n) return;  // no bytes, or every aggregate has a winner
  // pieces: [q, q + 16) with d_out + q 16-byte aligned; the first and the last may stick out of [d0, d1)
  const int64_t q0 = d0 - (int64_t)((uintptr_t)(p.out + d0) & 15u);
  const int64_t n_pieces = (d1 - q0 + 15) >> 4;
  for (int64_t j = t; j < n_pieces; j += kSsBlock) {
    const int64_t q = q0 + 16 * j;
    const int64_t lo = q < d0 ? d0 : q, hi = q + 16 > d1 ? d1 : q + 16;
    const int32_t k_lo = ss_find(off, n, lo), k_hi = ss_find(off, n, hi - 1);
    if (hi - lo == 16 && wc[k_hi + 1] == wc[k_lo]) {  // a whole piece of kept strings (k_lo, k_hi hold bytes: both < n_prev)
      const int64_t s_lo = p.prev_off[a0 + k_lo] + (lo - off[k_lo]), s_hi = p.prev_off[a0 + k_hi] + (hi - 1 - off[k_hi]);
      if (s_hi - s_lo == 15) {  // ... that are consecutive in the previous column too
        uint4 x;
        __builtin_memcpy(&x, p.prev + s_lo, 16);
        *(uint4*)(p.out + lo) = x;
        continue;
      }
    }
    int32_t k = k_lo;
    for (int64_t b = lo; b < hi; ++b) {
      while (off[k + 1] <= b) ++k;
      if (wc[k + 1] == wc[k]) p.out[b] = p.prev[p.prev_off[a0 + k] + (b - off[k])];
    }
  }
}

}  // namespace

// p.win1: n_agg u64 of scratch (zeroed here); *bad (zeroed here) += the records whose index lies outside [0, n_agg)
hipError_t launch_state_strings_winners(const StateStringsParams& p, unsigned long long* bad, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(bad, 0, 8, stream);
  if (e == hipSuccess) e = hipMemsetAsync(p.win1, 0, (size_t)p.n_agg * 8, stream);
  if (e != hipSuccess || p.n_records <= 0) return e;
  hipLaunchKernelGGL(ss_winner_kernel, dim3((unsigned)((p.n_records + kSsBlock - 1) / kSsBlock)), dim3(kSsBlock), 0, stream, p.agg_idx, p.status, p.n_records,
                     p.n_agg, p.win1, bad);
  return hipGetLastError();
}

// write == false: out_off[0 .. n_agg) = every aggregate's length (the caller scans them); true: the bytes
hipError_t launch_state_strings_pass(const StateStringsParams& p, bool write, hipStream_t stream) {
  if (p.n_agg <= 0) return hipSuccess;
  const unsigned agg_blocks = (unsigned)((p.n_agg + kSsBlock - 1) / kSsBlock), rec_blocks = (unsigned)((p.n_records + kSsBlock - 1) / kSsBlock);
  if (!write) {
    hipLaunchKernelGGL(ss_kept_len_kernel, dim3(agg_blocks), dim3(kSsBlock), 0, stream, p);
    if (p.n_records > 0) hipLaunchKernelGGL(ss_new_kernel<false>, dim3(rec_blocks), dim3(kSsBlock), kSsStageBytes + 16, stream, p);
  } else {
    if (p.n_prev > 0 && p.prev) hipLaunchKernelGGL(ss_kept_bytes_kernel, dim3(agg_blocks), dim3(kSsBlock), 0, stream, p);
    if (p.n_records > 0) hipLaunchKernelGGL(ss_new_kernel<true>, dim3(rec_blocks), dim3(kSsBlock), kSsStageBytes + 16, stream, p);
  }
  return hipGetLastError();
}

}  // namespace surge
