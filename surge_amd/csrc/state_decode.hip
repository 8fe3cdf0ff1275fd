// state_decode.hip — serialized state values -> fixed 64-byte states on the device (surge_replay_decode_json_states):
// the inverse of json_encode_kernel<true> (state_kernels.hip), with the parser the host runs (state_parse.h).
//
// Pass 1 (only with an aggregate index per record): last[agg] = the highest record that names agg (atomic max; stored
// + 1, so that 0 is "no record"), and the count of indices outside [0, n_agg) — pass 2 does nothing when there is one.
// Pass 2: one lane per record, 256 per block.  A block's values are contiguous in d_values, so the block copies their
// span into LDS with 16-byte loads (placed so that LDS offset == global address mod 16; head and tail by bytes, so
// nothing outside the span is read) and every lane parses out of LDS; a block whose span exceeds the stage parses
// straight from global (block-uniform choice).  A lane composes its row in LDS and stores it with four 16-byte stores
// once the whole value has parsed; a value that does not parse leaves the row alone.
// state_decode_kernel<true> is the same kernel for values in the multilanguage module's protobuf State envelope
// (surge_replay_decode_protobuf_states; state_parse_protobuf_state in state_parse.h): chosen at the launch, the envelope
// being the same for every record of it.  state_decode_kernel<*, true> reads in the lenient mode (surge_replay_set_decode_mode;
// state_parse_json_lenient): the parse call is the one thing that differs, and the template's field table is one more argument.
#include "replay_internal.h"
#include "state_parse.h"

#include <type_traits>

namespace surge {
namespace {

constexpr int kSdBlock = 256;
constexpr int kSdStageBytes = 32 * 1024;
constexpr int kSdRowBytes = kSdBlock * 64;

__global__ void __launch_bounds__(kSdBlock) state_last_record_kernel(const int64_t* __restrict__ agg_idx, int64_t n_records, int64_t n_agg,
                                                                     unsigned long long* __restrict__ last1,
                                                                     unsigned long long* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * kSdBlock + threadIdx.x;
  if (r >= n_records) return;
  const int64_t a = agg_idx[r];
  if (a < 0 || a >= n_agg) {
    atomicAdd(&counts[SD_BAD_INDEX], 1ull);
    return;
  }
  atomicMax(&last1[a], (unsigned long long)r + 1ull);
}

// += the number of lanes of this wave with `pred` (one atomic per wave; called by every lane of the block)
__device__ __forceinline__ void count_lanes(bool pred, unsigned long long* counter) {
  const unsigned long long m = __ballot(pred);
  if (m && (threadIdx.x & (warpSize - 1)) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(counter, (unsigned long long)__popcll(m));
}

struct SdNoFields {};  // what a strict instantiation takes where a lenient one takes the field table

template <bool ENVELOPE, bool LENIENT>
__global__ void __launch_bounds__(kSdBlock) state_decode_kernel(const surge_json_template t, const StateDecodeParams p,
                                                                const std::conditional_t<LENIENT, StateFieldTable, SdNoFields> fields) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sd_lds[];
  uint8_t* const rows = sd_lds;                 // 256 x 64 B: every lane's row while it parses
  uint8_t* const stage = sd_lds + kSdRowBytes;  // the block's values
  if (p.counts[SD_BAD_INDEX]) return;           // (written by pass 1, which is complete: the same for every block)
  const int64_t r0 = (int64_t)blockIdx.x * kSdBlock;
  const int64_t r = r0 + threadIdx.x;
  const bool live = r < p.n_records;
  const int64_t r1 = (r0 + kSdBlock < p.n_records) ? r0 + kSdBlock : p.n_records;
  const int64_t base = p.value_off[r0], end = p.value_off[r1];
  const uint32_t shift = (uint32_t)((uintptr_t)(p.values + base) & 15u);
  const bool staged = end >= base && (end - base) + shift <= kSdStageBytes;  // block-uniform
  if (staged) {
    const uint32_t total = (uint32_t)(end - base);
    const uint8_t* g = p.values + base - shift;     // 16-byte aligned; LDS offset i <-> g[i]
    const uint32_t lo = shift, hi = shift + total;  // the valid span in that frame
    const uint32_t body_lo = (lo + 15u) & ~15u, body_hi = hi & ~15u;
    if (body_lo <= body_hi) {
      for (uint32_t i = lo + threadIdx.x; i < body_lo; i += kSdBlock) stage[i] = g[i];
      for (uint32_t i = body_lo + threadIdx.x * 16u; i < body_hi; i += kSdBlock * 16u) *(uint4*)(stage + i) = *(const uint4*)(g + i);
      for (uint32_t i = body_hi + threadIdx.x; i < hi; i += kSdBlock) stage[i] = g[i];
    } else {
      for (uint32_t i = lo + threadIdx.x; i < hi; i += kSdBlock) stage[i] = g[i];
    }
    __syncthreads();
  }
  int rc = SURGE_STATE_DECODE_SKIPPED;
  bool wrote = false, tomb = false;
  if (live) {
    const int64_t a = p.agg_idx ? p.agg_idx[r] : r;  // in range: pass 1 / the launcher checked
    const bool winner = !p.agg_idx || p.last1[a] == (unsigned long long)r + 1ull;
    if (winner) {
      const int64_t o0 = p.value_off[r], o1 = p.value_off[r + 1];
      uint4* out = p.states + a * 4;
      if (o0 < base || o1 > end || o1 < o0) {
        rc = SURGE_STATE_DECODE_LITERAL;  // offsets that are not monotone: nothing of it is read
      } else if (o1 == o0) {              // a null value: the aggregate was deleted
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        out[0] = z; out[1] = z; out[2] = z; out[3] = z;
        rc = SURGE_STATE_DECODE_OK;
        tomb = true;
      } else {
        const uint8_t* v = staged ? stage + shift + (o0 - base) : p.values + o0;
        const uint8_t* key = p.keys ? p.keys + p.key_off[a] : nullptr;
        const int64_t key_len = p.key_off ? p.key_off[a + 1] - p.key_off[a] : -1;
        uint8_t* row = rows + threadIdx.x * 64;
        int64_t* span = p.spans ? p.spans + r * (2 * SURGE_JSON_STRING_COLUMNS) : nullptr;
        if constexpr (LENIENT) {
          if constexpr (ENVELOPE) rc = state_parse_protobuf_state_lenient<false>(t, fields, v, o1 - o0, key, key_len, p.ptab, row, span);
          else rc = state_parse_json_lenient<false>(t, fields, v, o1 - o0, key, key_len, p.ptab, row, span);
        } else {
          if constexpr (ENVELOPE) rc = state_parse_protobuf_state<false>(t, v, o1 - o0, key, key_len, p.ptab, row, span);
          else rc = state_parse_json<false>(t, v, o1 - o0, key, key_len, p.ptab, row, span);
        }
        if (rc == SURGE_STATE_DECODE_OK) {
          const uint4* lr = (const uint4*)row;
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // | the bytes the template does not name (surge_replay_set_decode_base; zeros by default)
            const uint4 x = lr[q], b = p.base[q];
            out[q] = make_uint4(x.x | b.x, x.y | b.y, x.z | b.z, x.w | b.w);
          }
          wrote = true;
        }
      }
    }
    if (p.status) p.status[r] = (uint8_t)rc;
  }
  const bool ambiguous = rc == SURGE_STATE_DECODE_AMBIGUOUS;
  const bool refused = rc != SURGE_STATE_DECODE_OK && rc != SURGE_STATE_DECODE_SKIPPED && !ambiguous;
  count_lanes(wrote, &p.counts[SD_WRITTEN]);
  count_lanes(tomb, &p.counts[SD_TOMBSTONES]);
  count_lanes(refused, &p.counts[SD_REFUSED]);
  count_lanes(ambiguous, &p.counts[SD_AMBIGUOUS]);
  if (refused) atomicMin(&p.counts[SD_FIRST_REFUSED], (unsigned long long)r);
}

constexpr size_t kSdLdsBytes = (size_t)kSdRowBytes + kSdStageBytes + 16;

}  // namespace

// p.counts: SD_N_COUNTS u64 (zeroed here, SD_FIRST_REFUSED to ~0); p.last1: n_agg u64 of scratch when p.agg_idx is given
// fields: the template's field table (state_field_table), read when p.lenient
hipError_t launch_state_decode(const surge_json_template& tmpl, const StateDecodeParams& p, hipStream_t stream, const StateFieldTable* fields) {
  if (p.lenient && !fields) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(p.counts, 0, SD_N_COUNTS * 8, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(p.counts + SD_FIRST_REFUSED, 0xFF, 8, stream);
  if (e != hipSuccess || p.n_records <= 0) return e;
  const unsigned blocks = (unsigned)((p.n_records + kSdBlock - 1) / kSdBlock);
  if (p.agg_idx) {
    e = hipMemsetAsync(p.last1, 0, (size_t)p.n_agg * 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(state_last_record_kernel, dim3(blocks), dim3(kSdBlock), 0, stream, p.agg_idx, p.n_records, p.n_agg, p.last1, p.counts);
  }
  if (p.lenient) {
    if (p.envelope) hipLaunchKernelGGL((state_decode_kernel<true, true>), dim3(blocks), dim3(kSdBlock), kSdLdsBytes, stream, tmpl, p, *fields);
    else hipLaunchKernelGGL((state_decode_kernel<false, true>), dim3(blocks), dim3(kSdBlock), kSdLdsBytes, stream, tmpl, p, *fields);
  } else {
    if (p.envelope) hipLaunchKernelGGL((state_decode_kernel<true, false>), dim3(blocks), dim3(kSdBlock), kSdLdsBytes, stream, tmpl, p, SdNoFields{});
    else hipLaunchKernelGGL((state_decode_kernel<false, false>), dim3(blocks), dim3(kSdBlock), kSdLdsBytes, stream, tmpl, p, SdNoFields{});
  }
  return hipGetLastError();
}

}  // namespace surge
