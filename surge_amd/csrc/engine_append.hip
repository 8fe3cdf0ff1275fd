// engine_append.hip — micro-batches onto the resident state (surge_replay_append_fold / append_events and their _device
// forms), the staging log and the packer that turns it into a bound log.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "engine_internal.h"

using namespace surge;

namespace surge {

// A micro-batch whose aggregate indices were out of range is skipped on the device (stream_kernels.hip) and reported
// here, at the host's next synchronisation point, once.
int32_t report_skipped_batches(surge_replay_handle* h) {
  if (!h->host_flags) return SURGE_OK;
  const uint32_t skipped = h->host_flags[2];
  if (skipped == h->skipped_seen) return SURGE_OK;
  const uint32_t n = skipped - h->skipped_seen;
  h->skipped_seen = skipped;
  return fail(h, SURGE_E_RANGE, std::to_string(n) + " micro-batch(es) carried an aggregate index out of range and were skipped (agg_idx out of range)");
}

}  // namespace surge

extern "C" {

int32_t surge_replay_append_fold_device(surge_replay_handle* h, const int64_t* d_group_agg, const int64_t* d_group_off,
                                        int64_t n_groups, const void* d_events, int64_t n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "append_fold before load_csr/bind_device_csr");
  if (n_groups < 0 || n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_groups == 0 || n_events == 0) return SURGE_OK;
  if (!d_group_agg || !d_group_off || !d_events) return fail(h, SURGE_E_INVALID, "NULL batch buffer");
  if ((uintptr_t)d_events & 15) return fail(h, SURGE_E_INVALID, "events must be 16-byte aligned");
  DeviceGuard g(h->device);
  FoldParams p;
  fill_params(h, p);
  p.events = (const uint4*)d_events;
  p.n_events = n_events;
  p.init = h->d_state;  // fold onto the resident state, in place
  p.out = h->d_state;
  p.out_map = d_group_agg;
  SURGE_TRY(fold_begin(h));
  if (h->v2) std::memset(p.table, 0, sizeof(p.table));
  SURGE_TRY(h->v2 ? run_slots(h, p, d_group_off, n_groups, false) : run_flat(h, p, d_group_off, n_groups, n_events));
  if (h->v2) h->perm_valid = false;  // the length order of the micro-batch replaced the bound log's
  return fold_end(h, h->v2 ? SURGE_ALGO_SLOTS : SURGE_ALGO_FLAT);
}

int32_t surge_replay_append_fold(surge_replay_handle* h, const int64_t* group_agg, const int64_t* group_off,
                                 int64_t n_groups, const void* events, int64_t n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "append_fold before load_csr/bind_device_csr");
  if (n_groups < 0 || n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_groups == 0 || n_events == 0) return SURGE_OK;
  if (!group_agg || !group_off || !events) return fail(h, SURGE_E_INVALID, "NULL batch buffer");
  if (group_off[0] != 0 || group_off[n_groups] != n_events)
    return fail(h, SURGE_E_INVALID, "group_off must span [0, n_events]");
  for (int64_t gidx = 0; gidx < n_groups; ++gidx) {
    if (group_off[gidx + 1] <= group_off[gidx]) return fail(h, SURGE_E_INVALID, "batch groups must be non-empty and ordered");
    if (group_agg[gidx] < 0 || group_agg[gidx] >= h->n_agg) return fail(h, SURGE_E_RANGE, "group_agg out of range");
  }
  try {
    // an aggregate may appear in one group only: two groups would race on the same resident state
    std::vector<int64_t> seen(group_agg, group_agg + n_groups);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
      return fail(h, SURGE_E_INVALID, "an aggregate appears in more than one group of the batch");
  } catch (const std::bad_alloc&) {
    return fail(h, SURGE_E_NOMEM, "out of host memory while validating the micro-batch");
  }
  DeviceGuard g(h->device);
  HIPCHK(h, h->batch_group_agg.reserve_roomy((size_t)n_groups * 8));
  HIPCHK(h, h->batch_group_off.reserve_roomy((size_t)(n_groups + 1) * 8));
  HIPCHK(h, h->batch_events.reserve_roomy((size_t)n_events * 16));
  HIPCHK(h, hipEventRecord(h->ev_h0, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->batch_group_agg.ptr, group_agg, (size_t)n_groups * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->batch_group_off.ptr, group_off, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->batch_events.ptr, events, (size_t)n_events * 16, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev_h1, h->stream));
  h->h2d_valid = true;
  return surge_replay_append_fold_device(h, (const int64_t*)h->batch_group_agg.ptr, (const int64_t*)h->batch_group_off.ptr,
                                         n_groups, h->batch_events.ptr, n_events);
}

int32_t surge_replay_append_events_device(surge_replay_handle* h, const int64_t* d_agg_idx, const void* d_events, int64_t n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "append_events before load_csr/bind_device_csr");
  if (n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_events == 0) return SURGE_OK;
  if (!d_agg_idx || !d_events) return fail(h, SURGE_E_INVALID, "NULL batch buffer");
  if (n_events > 0xffffffffll) return fail(h, SURGE_E_UNSUPPORTED, "micro-batches are limited to 2^32 - 1 events");
  if (h->n_agg > 0xffffffffll) return fail(h, SURGE_E_UNSUPPORTED, "the device group-by needs fewer than 2^32 aggregates");
  if ((uintptr_t)d_events & 15) return fail(h, SURGE_E_INVALID, "events must be 16-byte aligned");
  DeviceGuard g(h->device);
  const uint32_t n = (uint32_t)n_events;
  unsigned bits = 1;
  while (bits < 32 && (h->n_agg >> bits) != 0) ++bits;
  size_t temp = 0;
  HIPCHK(h, groupby_temp_bytes(n, bits, &temp));
  HIPCHK(h, h->gb_temp.reserve_roomy(temp));
  HIPCHK(h, h->gb_u32.reserve_roomy((size_t)n * 4 * 6));
  HIPCHK(h, h->gb_flags.reserve(16));
  HIPCHK(h, h->batch_group_agg.reserve_roomy((size_t)n * 8));
  HIPCHK(h, h->batch_group_off.reserve_roomy((size_t)(n + 1) * 8));
  HIPCHK(h, h->batch_events.reserve_roomy((size_t)n * 16));
  uint32_t* u = (uint32_t*)h->gb_u32.ptr;
  if (!h->host_flags) {
    HIPCHK(h, hipHostMalloc((void**)&h->host_flags, 16, hipHostMallocDefault));
    std::memset(h->host_flags, 0, 16);
    HIPCHK(h, hipMemsetAsync(h->gb_flags.ptr, 0, 16, h->stream));  // the sticky "skipped batches" word starts at 0
  }
  HIPCHK(h, launch_groupby(d_agg_idx, (const uint4*)d_events, n, h->n_agg, bits, h->gb_temp.ptr, temp, u, u + n, u + 2 * (size_t)n,
                           u + 3 * (size_t)n, u + 4 * (size_t)n, u + 5 * (size_t)n, (uint4*)h->batch_events.ptr,
                           (int64_t*)h->batch_group_agg.ptr, (int64_t*)h->batch_group_off.ptr, (uint32_t*)h->gb_flags.ptr, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->host_flags, h->gb_flags.ptr, 12, hipMemcpyDeviceToHost, h->stream));
  if (h->v2) {
    // the slot kernel's launch (length sort of the groups, one lane per group) is sized on the host: wait for the count
    HIPCHK(h, hipStreamSynchronize(h->stream));
    SURGE_TRY(report_skipped_batches(h));
    if (h->host_flags[0] == 0u) return SURGE_OK;
    return surge_replay_append_fold_device(h, (const int64_t*)h->batch_group_agg.ptr, (const int64_t*)h->batch_group_off.ptr,
                                           (int64_t)h->host_flags[0], h->batch_events.ptr, n_events);
  }
  // v1: no host round trip — the plan kernel reads the group count where the group-by left it, the fold's grid depends on
  // the event count only, and a batch with a bad index has zero groups (reported at the next synchronisation point)
  FoldParams p;
  fill_params(h, p);
  p.events = (const uint4*)h->batch_events.ptr;
  p.n_events = n_events;
  p.init = h->d_state;  // fold onto the resident state, in place
  p.out = h->d_state;
  p.out_map = (const int64_t*)h->batch_group_agg.ptr;
  SURGE_TRY(fold_begin(h));
  SURGE_TRY(run_flat(h, p, (const int64_t*)h->batch_group_off.ptr, 0, n_events, (const uint32_t*)h->gb_flags.ptr));
  return fold_end(h, SURGE_ALGO_FLAT);
}

int32_t surge_replay_append_events(surge_replay_handle* h, const int64_t* agg_idx, const void* events, int64_t n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "append_events before load_csr/bind_device_csr");
  if (n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_events == 0) return SURGE_OK;
  if (!agg_idx || !events) return fail(h, SURGE_E_INVALID, "NULL batch buffer");
  if (n_events > 0xffffffffll) return fail(h, SURGE_E_UNSUPPORTED, "micro-batches are limited to 2^32 - 1 events");
  DeviceGuard g(h->device);
  // the indices are on the host here: check them before anything is enqueued (immediate SURGE_E_RANGE, batch not applied)
  for (int64_t i = 0; i < n_events; ++i)
    if (agg_idx[i] < 0 || agg_idx[i] >= h->n_agg) return fail(h, SURGE_E_RANGE, "agg_idx out of range");
  // Host buffers (pageable: a JNI direct buffer, a numpy array) go through pinned staging so the H2D copy runs at PCIe
  // speed; two staging areas alternate, so filling the next batch overlaps the copy and the fold of the previous one and
  // the host never waits for the whole stream (double-buffered H2D).  Grouping happens on the device.
  const size_t need = (size_t)n_events * 24;
  const int k = h->pinned_next;
  h->pinned_next ^= 1;
  if (!h->ev_staged[k]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_staged[k], hipEventDisableTiming));
  if (h->staged_busy[k]) {  // the copies out of this area (two batches ago) must be done before it is overwritten
    HIPCHK(h, hipEventSynchronize(h->ev_staged[k]));
    h->staged_busy[k] = false;
  }
  if (need > h->pinned_cap[k]) {
    if (h->pinned[k]) (void)hipHostFree(h->pinned[k]);
    h->pinned[k] = nullptr;
    h->pinned_cap[k] = 0;
    const size_t cap = need < (4u << 20) ? (4u << 20) : need + need / 2;
    HIPCHK(h, hipHostMalloc(&h->pinned[k], cap, hipHostMallocDefault));
    h->pinned_cap[k] = cap;
  }
  // the device-side landing buffers are reused by every batch: stream order keeps a batch's copies behind the previous
  // batch's kernels; growing them must wait for those kernels
  if ((size_t)n_events * 8 > h->gb_agg_idx.cap || (size_t)n_events * 16 > h->gb_events.cap) HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, h->gb_agg_idx.reserve_roomy((size_t)n_events * 8));
  HIPCHK(h, h->gb_events.reserve_roomy((size_t)n_events * 16));
  std::memcpy(h->pinned[k], agg_idx, (size_t)n_events * 8);
  std::memcpy((char*)h->pinned[k] + (size_t)n_events * 8, events, (size_t)n_events * 16);
  HIPCHK(h, hipEventRecord(h->ev_h0, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->gb_agg_idx.ptr, h->pinned[k], (size_t)n_events * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->gb_events.ptr, (char*)h->pinned[k] + (size_t)n_events * 8, (size_t)n_events * 16, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev_h1, h->stream));
  HIPCHK(h, hipEventRecord(h->ev_staged[k], h->stream));
  h->staged_busy[k] = true;
  h->h2d_valid = true;
  return surge_replay_append_events_device(h, (const int64_t*)h->gb_agg_idx.ptr, h->gb_events.ptr, n_events);
}

static int32_t stage_grow(surge_replay_handle* h, int64_t want) {
  if (want <= h->stage_cap) return SURGE_OK;
  if (want > 0xffffffffll) return fail(h, SURGE_E_UNSUPPORTED, "the staging log holds fewer than 2^32 events per pack");
  int64_t cap = h->stage_cap * 2 > want ? h->stage_cap * 2 : want;
  cap = cap < (1 << 16) ? (1 << 16) : (cap > 0xffffffffll ? 0xffffffffll : cap);
  void *nk = nullptr, *ne = nullptr;
  HIPCHK(h, hipMalloc(&nk, (size_t)cap * 4));
  hipError_t e = hipMalloc(&ne, (size_t)cap * 16);
  if (e == hipSuccess && h->staged_n > 0) {
    e = hipMemcpyAsync(nk, h->stage_keys.ptr, (size_t)h->staged_n * 4, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ne, h->stage_events.ptr, (size_t)h->staged_n * 16, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  if (e != hipSuccess) {
    (void)hipFree(nk);
    if (ne) (void)hipFree(ne);
    return fail_hip(h, e, "growing the staging log");
  }
  h->stage_keys.release();
  h->stage_events.release();
  h->stage_keys.ptr = nk; h->stage_keys.cap = (size_t)cap * 4;
  h->stage_events.ptr = ne; h->stage_events.cap = (size_t)cap * 16;
  h->stage_cap = cap;
  return SURGE_OK;
}

int32_t surge_replay_stage_reserve(surge_replay_handle* h, int64_t n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  DeviceGuard g(h->device);
  return stage_grow(h, n_events);
}

int32_t surge_replay_stage_events_device(surge_replay_handle* h, const int64_t* d_agg_idx, const void* d_events, int64_t n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (h->v2) return fail(h, SURGE_E_UNSUPPORTED, "the packer serves v1 handles");
  if (n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_events == 0) return SURGE_OK;
  if (!d_agg_idx || !d_events) return fail(h, SURGE_E_INVALID, "NULL batch buffer");
  DeviceGuard g(h->device);
  SURGE_TRY(stage_grow(h, h->staged_n + n_events));
  HIPCHK(h, launch_pack_stage(d_agg_idx, (uint32_t)n_events, (uint32_t*)h->stage_keys.ptr + h->staged_n, h->stream));
  HIPCHK(h, hipMemcpyAsync((char*)h->stage_events.ptr + (size_t)h->staged_n * 16, d_events, (size_t)n_events * 16, hipMemcpyDeviceToDevice, h->stream));
  h->staged_n += n_events;
  return SURGE_OK;
}

int32_t surge_replay_staged(surge_replay_handle* h, int64_t* n_events_out) {
  if (!h || !n_events_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  *n_events_out = h->staged_n;
  return SURGE_OK;
}

int32_t surge_replay_pack_staged(surge_replay_handle* h, int64_t n_agg) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (h->v2) return fail(h, SURGE_E_UNSUPPORTED, "the packer serves v1 handles");
  if (n_agg < 0 || n_agg > 0xfffffffell) return fail(h, SURGE_E_INVALID, "n_agg out of range");
  DeviceGuard g(h->device);
  const uint32_t n = (uint32_t)h->staged_n;
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)(n_agg > 0 ? n_agg : 1) >> bits) != 0) ++bits;  // the key bits an index below n_agg needs
  size_t temp = 0;
  HIPCHK(h, pack_temp_bytes(n > 0 ? n : 1, bits, &temp));
  DevBuf scratch, seg, evs;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t rows = n > 0 ? n : 1;
  const size_t o_kb = up(temp), o_va = o_kb + up(rows * 4), o_vb = o_va + up(rows * 4), o_bad = o_vb + up(rows * 4), total = o_bad + 256;
  hipError_t e = scratch.reserve(total);
  if (e == hipSuccess) e = seg.reserve((size_t)(n_agg + 1) * 8);
  if (e == hipSuccess) e = evs.reserve(rows * 16);
  char* sb = (char*)scratch.ptr;
  if (e == hipSuccess)
    e = launch_pack((const uint32_t*)h->stage_keys.ptr, (const uint4*)h->stage_events.ptr, n, n_agg, bits, sb, temp, (uint32_t*)(sb + o_kb), (uint32_t*)(sb + o_va),
                    (uint32_t*)(sb + o_vb), (int64_t*)seg.ptr, (uint4*)evs.ptr, (uint32_t*)(sb + o_bad), h->stream);
  uint32_t bad = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, sb + o_bad, 4, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  scratch.release();
  if (e != hipSuccess) {
    seg.release();
    evs.release();
    return fail_hip(h, e, "packing the staged events");
  }
  if (bad) {
    seg.release();
    evs.release();
    return fail(h, SURGE_E_RANGE, "a staged event names an aggregate index >= n_agg (nothing bound, the staging log kept)");
  }
  // the packed log becomes the handle's own bound log
  h->bound = false;
  h->own_seg_off.release();
  h->own_events.release();
  h->own_init.release();
  h->own_seg_off = seg;
  h->own_events = evs;
  seg.ptr = nullptr; seg.cap = 0; evs.ptr = nullptr; evs.cap = 0;
  h->stage_keys.release();
  h->stage_events.release();
  h->staged_n = h->stage_cap = 0;
  return surge_replay_bind_device_csr(h, (const int64_t*)h->own_seg_off.ptr, n_agg, h->own_events.ptr, (int64_t)n, nullptr, nullptr);
}

int32_t surge_replay_bound_log(surge_replay_handle* h, const int64_t** d_seg_off, const void** d_events, int64_t* n_agg, int64_t* n_events) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "bound_log before load_csr/bind_device_csr/pack_staged");
  if (d_seg_off) *d_seg_off = h->d_seg_off;
  if (d_events) *d_events = h->d_events;
  if (n_agg) *n_agg = h->n_agg;
  if (n_events) *n_events = h->n_events;
  return SURGE_OK;
}

}  // extern "C"
