// ingest_strings.hip — the string fields of events on the device (surge_device_decoder_keep_event_strings, include/surge_ingest.h):
// what stands in front of the merge of state_strings.hip for an EVENTS decoder.  A 16-byte event has no room for
// BankAccountCreated's accountOwner and securityCode; a decoder that was told which class carries which string runs, behind a
// push's interning (ingest_stage2.hip says when):
//   select  one lane per record: the kept records (keep[i]) whose decoded event type belongs to a class that names a column,
//           compacted per block of 256 records by wave ballot and block total, in record order — topic order survives; the count
//           goes to the cell the push's finish reads.  A push that selected nothing costs this kernel and nothing else.
//   list    (n_sel > 0) the blocks' segments joined into one list behind an exclusive scan of the block counts, with the
//           selected values' lengths
//   spans   one lane per selected record walks its value where stage 1 left it — RecMeta::val_off / val_len into the push's
//           staged, decompressed bytes — by the rule of event_strings_parse.h (an enveloped template through sp_envelope_spans),
//           and writes spans and one status byte per column; a refusal is reported through ErrorCell / report as RS_STRING and
//           fails the push before anything of it is committed
//   gather  one wave per selected record copies its value behind what earlier pushes kept (CSR offsets, rows beside them):
//           bytes up to the destination's next 16-byte boundary, aligned 16-byte stores each put together from four load4 (the
//           source is where it is: every alignment), the last bytes one by one.  Only these few records are copied.  load4 reads
//           at most 7 bytes behind the byte it is asked for, and is asked for nothing behind value + len - 4: the staged bytes'
//           16 bytes of slack (ingest_device.h).  Nothing outside [off[q], off[q + 1]) is written.
// The merge itself is state_strings.hip's (launch_state_strings_winners / _pass per named column with that column's status
// array: SURGE_EVENT_STRING_ABSENT is not OK, so such a record is never a winner).  It rewrites a whole column — once per fetch
// would be quadratic on a 10^7-aggregate topic — so the gathered records ACCUMULATE across pushes and the merge runs when the
// columns are asked for (surge_device_decoder_state_strings, the end of a recovery) or when more than the bound of
// records are pending (EventStringsState::Pending::bound, 2^20: at BankAccount's ~100 bytes a value 100 MB of device memory; SURGE_INGEST_EVENT_STRINGS_PENDING
// sets another bound, the tests a low one).  clear drops what is pending; a re-seed or a growth of the key table does not touch
// it: rows do not move.
#include "event_strings_parse.h"
#include "ingest_device.h"
#include "replay_internal.h"

namespace surge {
namespace ingest {

namespace {

__global__ void __launch_bounds__(kStringsBlock) strings_select_kernel(const uint32_t* __restrict__ keep, const uint4* __restrict__ ev_tmp, int64_t n_rec, const EvsTypes types,
                                                                       uint32_t* __restrict__ seg, uint32_t* __restrict__ block_count, StringsCell* __restrict__ cell) {
  __shared__ uint32_t wave_total[kStringsBlock / 64];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kStringsBlock + t;
  bool sel = false;
  if (i < n_rec && keep[i]) {
    const uint32_t type = ev_tmp[i].x;  // surge_event16.type
    for (uint32_t k = 0; k < types.n; ++k) sel = sel || type == types.type[k];
  }
  const unsigned long long m = __ballot(sel);
  if ((t & 63) == 0) wave_total[t >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = (uint32_t)__popcll(m & ((1ull << (t & 63)) - 1ull)), total = 0;
  for (int w = 0; w < kStringsBlock / 64; ++w) {
    if (w < (t >> 6)) before += wave_total[w];
    total += wave_total[w];
  }
  if (sel) seg[(int64_t)blockIdx.x * kStringsBlock + before] = (uint32_t)i;
  if (t == 0) {
    block_count[blockIdx.x] = total;
    if (total) atomicAdd(&cell->n_sel, total);
  }
}

// block_base = the exclusive scan of block_count: one workgroup, a chunk of kStringsBlock counts at a time
__global__ void __launch_bounds__(kStringsBlock) strings_base_kernel(const uint32_t* __restrict__ block_count, int64_t n_blocks, uint32_t* __restrict__ block_base) {
  __shared__ uint32_t part[kStringsBlock];
  __shared__ uint32_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n_blocks; c0 += kStringsBlock) {
    const uint32_t mine = c0 + t < n_blocks ? block_count[c0 + t] : 0u;
    part[t] = mine;
    __syncthreads();
    for (int d = 1; d < kStringsBlock; d <<= 1) {  // inclusive scan of the chunk
      const uint32_t add = t >= d ? part[t - d] : 0u;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    if (c0 + t < n_blocks) block_base[c0 + t] = carry + part[t] - mine;
    __syncthreads();
    if (t == 0) carry += part[kStringsBlock - 1];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kStringsBlock) strings_list_kernel(const RecMeta* __restrict__ meta, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ block_count,
                                                                     const uint32_t* __restrict__ block_base, uint32_t* __restrict__ sel, int64_t* __restrict__ lens) {
  const int t = threadIdx.x;
  if ((uint32_t)t >= block_count[blockIdx.x]) return;
  const uint32_t rec = seg[(int64_t)blockIdx.x * kStringsBlock + t];
  const int64_t k = (int64_t)block_base[blockIdx.x] + t;
  const int32_t len = meta[rec].val_len;
  sel[k] = rec;
  lens[k] = len > 0 ? len : 0;
}

__global__ void __launch_bounds__(kStringsBlock) strings_spans_kernel(const EvsRule* __restrict__ rule, const RecMeta* __restrict__ meta, const uint8_t* __restrict__ bytes,
                                                                      const uint32_t* __restrict__ sel, int64_t n_sel, const StringsPending p, ErrorCell* err) {
  const int64_t k = (int64_t)blockIdx.x * kStringsBlock + threadIdx.x;
  if (k >= n_sel) return;
  const uint32_t rec = sel[k];
  const RecMeta m = meta[rec];
  int64_t span[2 * SURGE_JSON_STRING_COLUMNS];
  uint8_t status[SURGE_JSON_STRING_COLUMNS];
  const int rc = evs_string_spans(*rule, bytes + m.val_off, m.val_len > 0 ? m.val_len : 0, span, status);
  const int64_t q = p.n + k;
#pragma unroll
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
    p.spans[q * (2 * SURGE_JSON_STRING_COLUMNS) + 2 * c] = span[2 * c];
    p.spans[q * (2 * SURGE_JSON_STRING_COLUMNS) + 2 * c + 1] = span[2 * c + 1];
    p.status[c][q] = status[c];
  }
  if (rc != SURGE_EVENT_STRING_OK) report(err, rec, RS_STRING);
}

// one wave per selected record
__global__ void __launch_bounds__(kStringsBlock) strings_gather_kernel(const RecMeta* __restrict__ meta, const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ sel,
                                                                       const int64_t* __restrict__ lens, int64_t n_sel, int64_t total, const uint32_t* __restrict__ keep_pos,
                                                                       const int64_t* __restrict__ agg, const StringsPending p) {
  const int64_t k = (int64_t)blockIdx.x * (kStringsBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= n_sel) return;
  const uint32_t rec = sel[k];
  const RecMeta m = meta[rec];
  const int64_t len = m.val_len > 0 ? m.val_len : 0;
  const int64_t d0 = p.bytes + lens[k];  // (lens: scanned, the bytes of the selected values in front of this one)
  if (lane == 0) {
    p.off[p.n + k] = d0;
    p.rows[p.n + k] = agg[keep_pos[rec]];
    if (k == n_sel - 1) p.off[p.n + n_sel] = p.bytes + total;
  }
  const uint8_t* src = bytes + m.val_off;
  uint8_t* dst = p.values + d0;
  int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
  if (head > len) head = len;
  const int64_t n_pieces = (len - head) >> 4;
  for (int64_t b = lane; b < head; b += 64) dst[b] = src[b];
  for (int64_t j = lane; j < n_pieces; j += 64) {
    const uint8_t* s = src + head + 16 * j;
    *(uint4*)(dst + head + 16 * j) = make_uint4(load4(s), load4(s + 4), load4(s + 8), load4(s + 12));
  }
  for (int64_t b = head + 16 * n_pieces + lane; b < len; b += 64) dst[b] = src[b];
}

}  // namespace

hipError_t launch_strings_select(const uint32_t* keep, const uint4* ev_tmp, int64_t n_rec, const EvsTypes& types, const StringsSelect& s, hipStream_t st) {
  if (n_rec <= 0) return hipSuccess;
  const unsigned n_blocks = (unsigned)((n_rec + kStringsBlock - 1) / kStringsBlock);
  hipLaunchKernelGGL(strings_select_kernel, dim3(n_blocks), dim3(kStringsBlock), 0, st, keep, ev_tmp, n_rec, types, s.seg, s.block_count, s.cell);
  return hipGetLastError();
}

hipError_t launch_strings_list(const RecMeta* meta, int64_t n_rec, const StringsSelect& s, uint32_t* sel, int64_t* lens, hipStream_t st) {
  if (n_rec <= 0) return hipSuccess;
  const int64_t n_blocks = (n_rec + kStringsBlock - 1) / kStringsBlock;
  hipLaunchKernelGGL(strings_base_kernel, dim3(1), dim3(kStringsBlock), 0, st, (const uint32_t*)s.block_count, n_blocks, s.block_base);
  hipLaunchKernelGGL(strings_list_kernel, dim3((unsigned)n_blocks), dim3(kStringsBlock), 0, st, meta, (const uint32_t*)s.seg, (const uint32_t*)s.block_count,
                     (const uint32_t*)s.block_base, sel, lens);
  return hipGetLastError();
}

hipError_t launch_strings_spans(const void* rule, const RecMeta* meta, const uint8_t* bytes, const uint32_t* sel, int64_t n_sel, const StringsPending& p, ErrorCell* err,
                                hipStream_t st) {
  if (n_sel <= 0) return hipSuccess;
  hipLaunchKernelGGL(strings_spans_kernel, dim3((unsigned)((n_sel + kStringsBlock - 1) / kStringsBlock)), dim3(kStringsBlock), 0, st, (const EvsRule*)rule, meta, bytes, sel,
                     n_sel, p, err);
  return hipGetLastError();
}

hipError_t launch_strings_gather(const RecMeta* meta, const uint8_t* bytes, const uint32_t* sel, const int64_t* lens, int64_t n_sel, int64_t total, const uint32_t* keep_pos,
                                 const int64_t* agg, const StringsPending& p, hipStream_t st) {
  if (n_sel <= 0) return hipSuccess;
  constexpr int per_block = kStringsBlock / 64;
  hipLaunchKernelGGL(strings_gather_kernel, dim3((unsigned)((n_sel + per_block - 1) / per_block)), dim3(kStringsBlock), 0, st, meta, bytes, sel, lens, n_sel, total, keep_pos,
                     agg, p);
  return hipGetLastError();
}

hipError_t launch_strings_scan(int64_t* lens, int64_t n, int64_t* totals, hipStream_t st) { return launch_scan_lengths_i64(lens, n, totals, st); }

hipError_t strings_merge_column(const StringsPending& pend, int column, int64_t n_agg, const StringsColumn& col, unsigned long long* win1, unsigned long long* bad,
                                int64_t* totals, int64_t* total_out, hipStream_t st) {
  StateStringsParams p{};
  p.values = pend.values; p.value_off = pend.off; p.n_records = pend.n;
  p.agg_idx = pend.rows; p.status = pend.status[column]; p.spans = pend.spans; p.column = column;
  p.win1 = pend.n > 0 ? win1 : nullptr;
  p.n_agg = n_agg;
  p.prev = col.prev; p.prev_off = col.prev_off; p.n_prev = col.n_prev;
  p.out = col.out; p.out_off = col.out_off;
  hipError_t e = hipSuccess;
  if (pend.n > 0) e = launch_state_strings_winners(p, bad, st);  // (the rows are the decoder's own: none lies outside [0, n_agg))
  int64_t total = 0;
  if (e == hipSuccess && n_agg > 0) {
    e = launch_state_strings_pass(p, false, st);
    if (e == hipSuccess) e = launch_scan_lengths_i64(col.out_off, n_agg, totals, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, totals + (n_agg + 1023) / 1024, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(col.out_off + n_agg, &total, 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && total > 0) e = launch_state_strings_pass(p, true, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // (`total` is read by the copy above until here)
  *total_out = total;
  return e;
}

}  // namespace ingest
}  // namespace surge
