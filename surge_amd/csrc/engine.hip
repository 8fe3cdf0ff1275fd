// engine.hip — host side of libsurge_replay.so: the handle's life (create / destroy / stream / errors), binding a log and
// its CSR analysis, stats, the partition hash and the stream probe.  The other extern "C" entry points of
// include/surge_replay.h live in engine_fold.hip, engine_append.hip, engine_states.hip and engine_comm.hip; what the units
// share is engine_internal.h.  No torch types, no CPU fold: if HIP is unusable every entry point reports SURGE_E_DEVICE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "engine_internal.h"

using namespace surge;

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace surge {

int32_t fail(surge_replay_handle* h, int32_t code, const std::string& msg) {
  if (h) {
    std::lock_guard<std::mutex> lk(h->err_mu);
    h->err = msg;
  }
  g_last_error = msg;  // thread-local: what surge_replay_last_error(NULL) returns to the failing thread
  return code;
}

int32_t fail_hip(surge_replay_handle* h, hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  const int32_t code = (e == hipErrorOutOfMemory) ? SURGE_E_NOMEM : SURGE_E_DEVICE;
  return fail(h, code, m);
}

int32_t validate_schema(const surge_replay_schema* s) {
  if (!s) return fail(nullptr, SURGE_E_INVALID, "schema is NULL");
  if (s->abi_version != SURGE_REPLAY_ABI_VERSION) return fail(nullptr, SURGE_E_UNSUPPORTED, "schema.abi_version mismatch");
  if (s->state_size != 64 || s->event_size != 16)
    return fail(nullptr, SURGE_E_UNSUPPORTED, "only 64-byte states and 16-byte events are supported");
  if (s->n_types < 1 || s->n_types > SURGE_MAX_EVENT_TYPES) return fail(nullptr, SURGE_E_INVALID, "schema.n_types out of range");
  const uint32_t known = SURGE_CLS_MASK | SURGE_D_POISON | SURGE_D_COUNT_MASK | SURGE_D_VERSION_SET | SURGE_D_SUM_MASK |
                         SURGE_D_BALANCE_SET | SURGE_D_MIN_ARG | SURGE_D_MAX_ARG | SURGE_D_EVCOUNT_INC;
  for (uint32_t i = 0; i < s->n_types; ++i) {
    if (s->desc[i] & ~known) return fail(nullptr, SURGE_E_UNSUPPORTED, "schema descriptor uses unknown bits");
    if ((s->desc[i] & SURGE_D_SUM_MASK) == SURGE_D_SUM_MASK) return fail(nullptr, SURGE_E_UNSUPPORTED, "invalid sum64 op");
  }
  return SURGE_OK;
}

int32_t validate_schema_v2(const surge_replay_schema_v2* sc) {
  if (!sc) return fail(nullptr, SURGE_E_INVALID, "schema is NULL");
  if (sc->abi_version != SURGE_REPLAY_ABI_VERSION_2) return fail(nullptr, SURGE_E_UNSUPPORTED, "schema.abi_version is not 2");
  if (sc->state_size != 64 || sc->event_size != 16) return fail(nullptr, SURGE_E_UNSUPPORTED, "only 64-byte states and 16-byte events are supported");
  if (sc->n_types < 1 || sc->n_types > SURGE_MAX_EVENT_TYPES) return fail(nullptr, SURGE_E_INVALID, "schema.n_types out of range");
  if (sc->n_slots < 1 || sc->n_slots > SURGE_MAX_SLOTS) return fail(nullptr, SURGE_E_INVALID, "schema.n_slots out of range");
  if (sc->flags & ~SURGE_V2_COUNT_EVENTS) return fail(nullptr, SURGE_E_UNSUPPORTED, "schema.flags uses unknown bits");
  for (uint32_t i = 0; i < sc->n_slots; ++i) {
    if (sc->slot[i].type < SURGE_SLOT_I32 || sc->slot[i].type > SURGE_SLOT_F64) return fail(nullptr, SURGE_E_UNSUPPORTED, "unknown slot type");
    if (sc->slot[i].source > SURGE_SRC_ONE) return fail(nullptr, SURGE_E_UNSUPPORTED, "unknown operand source");
  }
  for (uint32_t t = 0; t < sc->n_types; ++t) {
    if (sc->cls[t] & ~(SURGE_CLS_MASK | SURGE_D_POISON)) return fail(nullptr, SURGE_E_UNSUPPORTED, "cls uses unknown bits");
    for (uint32_t i = 0; i < 8; ++i) {
      const uint32_t op = (sc->ops[t] >> (4 * i)) & 15u;
      if (op > SURGE_OP_MAX) return fail(nullptr, SURGE_E_UNSUPPORTED, "unknown slot operation");
      if (i >= sc->n_slots && op != SURGE_OP_KEEP) return fail(nullptr, SURGE_E_INVALID, "operation on a slot the schema does not declare");
    }
  }
  return SURGE_OK;
}

}  // namespace surge

namespace {

// Analyse the bound CSR once: monotone? empty segments? uniform length?  Synchronous (load time).
int32_t analyze_bound(surge_replay_handle* h) {
  HIPCHK(h, h->d_analysis.reserve(sizeof(CsrAnalysis)));
  h->n_nz = h->n_agg;
  std::memset(&h->an, 0, sizeof(h->an));
  if (h->n_agg == 0) return SURGE_OK;
  HIPCHK(h, launch_analyze_csr(h->d_seg_off, h->n_agg, (CsrAnalysis*)h->d_analysis.ptr, h->stream));
  HIPCHK(h, hipMemcpyAsync(&h->an, h->d_analysis.ptr, sizeof(CsrAnalysis), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->an.bad) return fail(h, SURGE_E_INVALID, "seg_off is not monotone non-decreasing");
  if (h->an.first < 0 || h->an.last > h->n_events)
    return fail(h, SURGE_E_INVALID, "seg_off range exceeds the events buffer");
  if (h->an.n_empty > 0) {
    // kernel-facing CSR without empty segments (+ rank -> aggregate map)
    const int64_t nb = (h->n_agg + 1023) / 1024;
    h->n_nz = h->n_agg - h->an.n_empty;
    HIPCHK(h, h->block_counts.reserve((size_t)(nb + 1) * 8));
    HIPCHK(h, h->nz_off.reserve((size_t)(h->n_nz + 1) * 8));
    HIPCHK(h, h->nz_map.reserve((size_t)(h->n_nz > 0 ? h->n_nz : 1) * 8));
    HIPCHK(h, launch_compact_nonempty(h->d_seg_off, h->n_agg, (int64_t*)h->block_counts.ptr, (int64_t*)h->nz_off.ptr,
                                      (int64_t*)h->nz_map.ptr, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return SURGE_OK;
}

int64_t algorithmic_bytes(int64_t n_events, int64_t n_agg, bool has_init) {
  return 16 * n_events + 8 * (n_agg + 1) + 64 * n_agg * (has_init ? 2 : 1);
}

}  // namespace

extern "C" {

int32_t surge_replay_default_schema(surge_replay_schema* out) {
  if (!out) return fail(nullptr, SURGE_E_INVALID, "out is NULL");
  std::memset(out, 0, sizeof(*out));
  out->abi_version = SURGE_REPLAY_ABI_VERSION;
  out->state_size = 64;
  out->event_size = 16;
  out->n_types = 7;
  const uint32_t extras = SURGE_D_MIN_ARG | SURGE_D_MAX_ARG | SURGE_D_EVCOUNT_INC;
  out->desc[SURGE_EVT_NOOP] = SURGE_CLS_MATERIALIZE;
  out->desc[SURGE_EVT_INC] = SURGE_CLS_MATERIALIZE | SURGE_D_COUNT_ADD | SURGE_D_VERSION_SET | SURGE_D_SUM_ADD | extras;
  out->desc[SURGE_EVT_DEC] = SURGE_CLS_MATERIALIZE | SURGE_D_COUNT_SUB | SURGE_D_VERSION_SET | SURGE_D_SUM_SUB | extras;
  out->desc[SURGE_EVT_CREATE] = SURGE_CLS_CREATE | SURGE_D_BALANCE_SET | SURGE_D_EVCOUNT_INC;
  out->desc[SURGE_EVT_SET_BALANCE] = SURGE_CLS_REQUIRE | SURGE_D_BALANCE_SET | SURGE_D_EVCOUNT_INC;
  out->desc[SURGE_EVT_DELETE] = SURGE_CLS_DELETE;
  out->desc[SURGE_EVT_THROW] = SURGE_D_POISON;
  out->default_state.min_arg = 0x7fffffff;
  out->default_state.max_arg = (int32_t)0x80000000;
  out->default_state.flags = SURGE_STATE_PRESENT;
  return SURGE_OK;
}

int32_t surge_replay_create(const surge_replay_schema* schema, int32_t device_id, surge_replay_handle** out) {
  if (!out) return fail(nullptr, SURGE_E_INVALID, "out is NULL");
  *out = nullptr;
  SURGE_TRY(validate_schema(schema));
  int n_dev = 0;
  hipError_t e = hipGetDeviceCount(&n_dev);
  if (e != hipSuccess || n_dev <= 0)
    return fail(nullptr, SURGE_E_DEVICE, "no usable HIP device (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= n_dev) return fail(nullptr, SURGE_E_INVALID, "device_id out of range");
  surge_replay_handle* h = new (std::nothrow) surge_replay_handle();
  if (!h) return fail(nullptr, SURGE_E_NOMEM, "out of host memory");
  h->device = device_id;
  h->schema = *schema;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) h->n_cus = cus;
  }
  DeviceGuard g(device_id);
  if (!g.ok) {
    delete h;
    return fail(nullptr, SURGE_E_DEVICE, "hipSetDevice failed");
  }
  hipEvent_t* evs[] = {&h->ev_total0, &h->ev_total1, &h->ev_h0, &h->ev_h1, &h->ev_i0, &h->ev_i1, &h->ev_r0, &h->ev_r1};
  for (hipEvent_t* ev : evs) {
    e = hipEventCreate(ev);
    if (e != hipSuccess) {
      const int32_t rc = fail_hip(nullptr, e, "hipEventCreate");
      surge_replay_destroy(h);
      return rc;
    }
  }
  h->st.n_poisoned = -1;
  *out = h;
  return SURGE_OK;
}

int32_t surge_replay_create_v2(const surge_replay_schema_v2* sc, int32_t device_id, surge_replay_handle** out) {
  if (!out) return fail(nullptr, SURGE_E_INVALID, "out is NULL");
  *out = nullptr;
  SURGE_TRY(validate_schema_v2(sc));
  surge_replay_schema v1;
  surge_replay_default_schema(&v1);  // the handle's v1 half is inert; every fold of a v2 handle goes through the slot kernel
  SURGE_TRY(surge_replay_create(&v1, device_id, out));
  (*out)->v2 = true;
  (*out)->schema2 = *sc;
  slot_params_from_schema(*sc, (SlotParams*)(*out)->slot_params);
  {
    // the schema never changes: compile the slot kernels for it (hiprtc, ~1 s the first time a process sees the schema);
    // any failure leaves the generic interpreter in charge and is reported by surge_replay_kernel_info, not here
    DeviceGuard g(device_id);
    surge_replay_handle* h = *out;
    h->spec.tried = true;
    h->spec.have = slot_kernels_acquire(*(const SlotParams*)h->slot_params, device_id, &h->spec.k, &h->spec.why);
    if (h->spec.have) h->spec.why = std::string("compiled by ") + rtc_library_path();
  }
  return SURGE_OK;
}

int32_t surge_replay_destroy(surge_replay_handle* h) {
  if (!h) return SURGE_OK;
  DeviceGuard g(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->comm) comm_destroy(h->comm);
  h->comm = nullptr;
  for (int k = 0; k < 2; ++k) {
    if (h->pinned[k]) (void)hipHostFree(h->pinned[k]);
    h->pinned[k] = nullptr;
    if (h->ev_staged[k]) (void)hipEventDestroy(h->ev_staged[k]);
    h->ev_staged[k] = nullptr;
  }
  if (h->host_flags) (void)hipHostFree(h->host_flags);
  h->host_flags = nullptr;
  h->cidx.release();
  h->tidx.release();
  DevBuf* bufs[] = {&h->gb_temp, &h->gb_u32, &h->gb_flags, &h->gb_agg_idx, &h->gb_events, &h->published, &h->gathered[0], &h->gathered[1], &h->f64_tables, &h->nan_count, &h->sd_ptab, &h->sd_counts, &h->sd_last, &h->sd_status, &h->shard_counts, &h->ix_arena, &h->ix_cnt, &h->stage_keys, &h->stage_events, &h->t_tiles, &h->t_gsub, &h->perm, &h->counter, &h->own_seg_off, &h->own_events, &h->own_init, &h->own_state, &h->d_analysis, &h->nz_off,
                    &h->nz_map, &h->block_counts, &h->plan, &h->batch_group_agg, &h->batch_group_off,
                    &h->batch_events, &h->poison_count, &h->gather_idx, &h->gather_out, &h->scan_totals, &h->rows_off};
  for (DevBuf* b : bufs) b->release();
  hipEvent_t evs[] = {h->ev_total0, h->ev_total1, h->ev_h0, h->ev_h1, h->ev_i0, h->ev_i1, h->ev_r0, h->ev_r1};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& pr : h->fold_events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  delete h;
  return SURGE_OK;
}

const char* surge_replay_last_error(const surge_replay_handle* h) {
  return h ? h->err.c_str() : g_last_error.c_str();
}

int32_t surge_replay_set_stream(surge_replay_handle* h, void* hip_stream) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  h->stream = (hipStream_t)hip_stream;
  return SURGE_OK;
}

int32_t surge_replay_get_stream(surge_replay_handle* h, void** hip_stream_out) {
  if (!h || !hip_stream_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  *hip_stream_out = (void*)h->stream;
  return SURGE_OK;
}

int32_t surge_replay_synchronize(surge_replay_handle* h) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  DeviceGuard g(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return report_skipped_batches(h);
}

int32_t surge_replay_bind_device_csr(surge_replay_handle* h, const int64_t* d_seg_off, int64_t n_agg,
                                     const void* d_events, int64_t n_events, const void* d_init_state,
                                     void* d_state_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n_agg < 0 || n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (!d_seg_off) return fail(h, SURGE_E_INVALID, "seg_off is NULL");
  if (n_events > 0 && !d_events) return fail(h, SURGE_E_INVALID, "events is NULL");
  if (((uintptr_t)d_events & 15) || ((uintptr_t)d_init_state & 15) || ((uintptr_t)d_state_out & 15) ||
      ((uintptr_t)d_seg_off & 7))
    return fail(h, SURGE_E_INVALID, "device buffers must be 16-byte aligned (seg_off: 8)");
  DeviceGuard g(h->device);
  h->bound = false;
  h->perm_valid = false;
  h->cidx.T = 0;
  h->tidx.T = 0;
  h->tiled_valid = false;
  h->index_timed = h->relayout_timed = false;
  h->index_algo = 0;
  h->d_seg_off = d_seg_off;
  h->d_events = (const uint4*)d_events;
  h->d_init = (const uint4*)d_init_state;
  h->n_agg = n_agg;
  h->n_events = n_events;
  if (d_state_out) {
    h->d_state = (uint4*)d_state_out;
  } else {
    HIPCHK(h, h->own_state.reserve((size_t)n_agg * 64));
    h->d_state = (uint4*)h->own_state.ptr;
  }
  SURGE_TRY(analyze_bound(h));
  h->bound = true;
  h->log_valid = true;
  h->st.n_aggregates = n_agg;
  h->st.n_events = h->an.last - h->an.first;
  h->st.algorithmic_bytes = algorithmic_bytes(h->st.n_events, n_agg, d_init_state != nullptr);
  h->fold_epoch.fetch_add(1);
  return SURGE_OK;
}

int32_t surge_replay_load_csr(surge_replay_handle* h, const int64_t* seg_off, int64_t n_agg, const void* events,
                              int64_t n_events, const void* init_state) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n_agg < 0 || n_events < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (!seg_off) return fail(h, SURGE_E_INVALID, "seg_off is NULL");
  if (n_events > 0 && !events) return fail(h, SURGE_E_INVALID, "events is NULL");
  // cheap host-side validation before touching the device
  for (int64_t a = 0; a < n_agg; ++a)
    if (seg_off[a + 1] < seg_off[a]) return fail(h, SURGE_E_INVALID, "seg_off is not monotone non-decreasing");
  if (seg_off[0] < 0 || seg_off[n_agg] > n_events) return fail(h, SURGE_E_INVALID, "seg_off range exceeds the events buffer");
  DeviceGuard g(h->device);
  h->bound = false;
  HIPCHK(h, h->own_seg_off.reserve((size_t)(n_agg + 1) * 8));
  HIPCHK(h, h->own_events.reserve((size_t)n_events * 16));
  if (init_state) HIPCHK(h, h->own_init.reserve((size_t)n_agg * 64));
  HIPCHK(h, hipEventRecord(h->ev_h0, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->own_seg_off.ptr, seg_off, (size_t)(n_agg + 1) * 8, hipMemcpyHostToDevice, h->stream));
  if (n_events > 0)
    HIPCHK(h, hipMemcpyAsync(h->own_events.ptr, events, (size_t)n_events * 16, hipMemcpyHostToDevice, h->stream));
  if (init_state && n_agg > 0)
    HIPCHK(h, hipMemcpyAsync(h->own_init.ptr, init_state, (size_t)n_agg * 64, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev_h1, h->stream));
  h->h2d_valid = true;
  return surge_replay_bind_device_csr(h, (const int64_t*)h->own_seg_off.ptr, n_agg, h->own_events.ptr, n_events,
                                      init_state ? h->own_init.ptr : nullptr, nullptr);
}

/* CPU variant of the shard map (R15).  This is product code (host-side routing needs it without a
 * GPU round trip), written independently of oracle/. */
static inline uint32_t rotl32_host(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

static int32_t partition_hash_host(const uint16_t* utf16, const int64_t* str_off, int64_t n, int32_t n_partitions,
                                   int32_t* part_out, bool up_to_colon) {
  if (n < 0 || n_partitions <= 0) return fail(nullptr, SURGE_E_INVALID, "bad n or n_partitions");
  if (n == 0) return SURGE_OK;
  if (!str_off || !part_out) return fail(nullptr, SURGE_E_INVALID, "NULL buffer");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = str_off[i], e = str_off[i + 1];
    if (e < b) return fail(nullptr, SURGE_E_INVALID, "str_off is not monotone");
    int64_t len = e - b;
    if (up_to_colon) {  // PartitionStringUpToColon.partitionBy (KafkaPartitioner.scala:38-42)
      len = 0;
      while (b + len < e && utf16[b + len] != (uint16_t)':') ++len;
    }
    uint32_t hsh = 0xf7ca7fd2u;
    int64_t k = 0;
    for (; k + 1 < len; k += 2) {
      uint32_t d = ((uint32_t)utf16[b + k] << 16) + (uint32_t)utf16[b + k + 1];
      d *= 0xcc9e2d51u; d = rotl32_host(d, 15); d *= 0x1b873593u;
      hsh ^= d; hsh = rotl32_host(hsh, 13); hsh = hsh * 5u + 0xe6546b64u;
    }
    if (k < len) {
      uint32_t d = (uint32_t)utf16[b + k];
      d *= 0xcc9e2d51u; d = rotl32_host(d, 15); d *= 0x1b873593u;
      hsh ^= d;
    }
    hsh ^= (uint32_t)len;
    hsh ^= hsh >> 16; hsh *= 0x85ebca6bu; hsh ^= hsh >> 13; hsh *= 0xc2b2ae35u; hsh ^= hsh >> 16;
    const int32_t r = (int32_t)hsh % n_partitions;
    part_out[i] = r < 0 ? -r : r;
  }
  return SURGE_OK;
}

int32_t surge_replay_partition_hash(const uint16_t* utf16, const int64_t* str_off, int64_t n, int32_t n_partitions,
                                    int32_t* part_out) {
  return partition_hash_host(utf16, str_off, n, n_partitions, part_out, false);
}

int32_t surge_replay_partition_hash_up_to_colon(const uint16_t* utf16, const int64_t* str_off, int64_t n,
                                                int32_t n_partitions, int32_t* part_out) {
  return partition_hash_host(utf16, str_off, n, n_partitions, part_out, true);
}

static int32_t partition_hash_dev(surge_replay_handle* h, const uint16_t* d_utf16, const int64_t* d_str_off, int64_t n,
                                  int32_t n_partitions, int32_t* d_part_out, bool up_to_colon) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n < 0 || n_partitions <= 0) return fail(h, SURGE_E_INVALID, "bad n or n_partitions");
  if (n == 0) return SURGE_OK;
  if (!d_str_off || !d_part_out) return fail(h, SURGE_E_INVALID, "NULL buffer");
  DeviceGuard g(h->device);
  HIPCHK(h, launch_partition_hash(d_utf16, d_str_off, n, n_partitions, d_part_out, up_to_colon, h->stream));
  return SURGE_OK;
}

int32_t surge_replay_partition_hash_device(surge_replay_handle* h, const uint16_t* d_utf16, const int64_t* d_str_off,
                                           int64_t n, int32_t n_partitions, int32_t* d_part_out) {
  return partition_hash_dev(h, d_utf16, d_str_off, n, n_partitions, d_part_out, false);
}

int32_t surge_replay_partition_hash_up_to_colon_device(surge_replay_handle* h, const uint16_t* d_utf16,
                                                       const int64_t* d_str_off, int64_t n, int32_t n_partitions,
                                                       int32_t* d_part_out) {
  return partition_hash_dev(h, d_utf16, d_str_off, n, n_partitions, d_part_out, true);
}

int32_t surge_replay_stats(surge_replay_handle* h, surge_replay_stats_t* out) {
  if (!h || !out) return fail(h, SURGE_E_INVALID, "NULL argument");
  DeviceGuard g(h->device);
  if (h->timing_valid) {
    HIPCHK(h, hipEventSynchronize(h->ev_total1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev_k0, h->ev_k1));
    h->st.last_fold_kernel_ms = ms;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev_total0, h->ev_total1));
    h->st.last_fold_total_ms = ms;
    const size_t n = h->folds_since_reset < kMaxTimedFolds ? h->folds_since_reset : kMaxTimedFolds;
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) {
      HIPCHK(h, hipEventElapsedTime(&ms, h->fold_events[i].first, h->fold_events[i].second));
      sum += ms;
    }
    h->st.sum_fold_kernel_ms = sum;
    h->st.timed_folds = (int64_t)n;
  }
  if (h->h2d_valid) {
    HIPCHK(h, hipEventSynchronize(h->ev_h1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev_h0, h->ev_h1));
    h->st.h2d_ms = ms;
  }
  if (h->bound && h->st.n_folds > 0 && h->st.n_poisoned < 0) {
    HIPCHK(h, h->poison_count.reserve(8));
    HIPCHK(h, launch_count_poisoned(h->d_state, h->n_agg, (unsigned long long*)h->poison_count.ptr, h->stream));
    unsigned long long c = 0;
    HIPCHK(h, hipMemcpyAsync(&c, h->poison_count.ptr, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->st.n_poisoned = (int64_t)c;
  }
  *out = h->st;
  return SURGE_OK;
}

int32_t surge_replay_fold_times(surge_replay_handle* h, double* ms_out, int64_t cap, int64_t* n_out) {
  if (!h || !n_out || cap < 0 || (!ms_out && cap > 0)) return fail(h, SURGE_E_INVALID, "bad argument");
  *n_out = 0;
  if (!h->timing_valid) return SURGE_OK;
  DeviceGuard g(h->device);
  HIPCHK(h, hipEventSynchronize(h->ev_total1));
  size_t n = h->folds_since_reset < kMaxTimedFolds ? h->folds_since_reset : kMaxTimedFolds;
  if ((int64_t)n > cap) n = (size_t)cap;
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->fold_events[i].first, h->fold_events[i].second));
    ms_out[i] = ms;
  }
  *n_out = (int64_t)n;
  return SURGE_OK;
}

int32_t surge_replay_stats_reset(surge_replay_handle* h) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  DeviceGuard g(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->folds_since_reset = 0;
  h->timing_valid = false;
  h->st.sum_fold_kernel_ms = 0.0;
  h->st.timed_folds = 0;
  return SURGE_OK;
}

int32_t surge_replay_grow(surge_replay_handle* h, int64_t new_n_agg) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "grow before load_csr/bind_device_csr");
  if (new_n_agg <= h->n_agg) return SURGE_OK;
  if (h->d_state != (uint4*)h->own_state.ptr)
    return fail(h, SURGE_E_UNSUPPORTED, "the state buffer belongs to the caller (bind_device_csr / set_state_out): grow it there");
  DeviceGuard g(h->device);
  std::unique_lock<std::shared_mutex> lk(h->mu);
  if ((size_t)new_n_agg * 64 > h->own_state.cap) {
    // amortised: at least double, so a stream of new aggregates reallocates O(log n) times
    size_t want = h->own_state.cap * 2;
    if (want < (size_t)new_n_agg * 64) want = (size_t)new_n_agg * 64;
    void* fresh = nullptr;
    HIPCHK(h, hipMalloc(&fresh, want));
    hipError_t e = hipMemcpyAsync(fresh, h->own_state.ptr, (size_t)h->n_agg * 64, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      (void)hipFree(fresh);
      return fail_hip(h, e, "copying the resident state");
    }
    (void)hipFree(h->own_state.ptr);
    h->own_state.ptr = fresh;
    h->own_state.cap = want;
    h->d_state = (uint4*)fresh;
  }
  // new aggregates are None (all-zero, the canonical encoding)
  HIPCHK(h, hipMemsetAsync((char*)h->d_state + (size_t)h->n_agg * 64, 0, (size_t)(new_n_agg - h->n_agg) * 64, h->stream));
  h->n_agg = new_n_agg;
  h->st.n_aggregates = new_n_agg;
  h->log_valid = false;
  h->fold_epoch.fetch_add(1);
  return SURGE_OK;
}

int32_t surge_replay_stream_probe(surge_replay_handle* h, const void* d_src, int64_t n_bytes, double* ms_out) {
  if (!h || !d_src || !ms_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  if (n_bytes < 16 || (n_bytes & 15) || ((uintptr_t)d_src & 15)) return fail(h, SURGE_E_INVALID, "n_bytes/pointer must be 16-byte multiples");
  DeviceGuard g(h->device);
  HIPCHK(h, h->poison_count.reserve(8));
  if (std::getenv("SURGE_DBG_PROBE_TILES") && h->tiled_valid) {  // experiments: stream the handle's own tile-major copy
    d_src = h->t_tiles.ptr;
    n_bytes = h->t_n_sub * (int64_t)kTileSubBytes;
  }
  float best = 0.f;
  for (int variant = 0; variant < 6; ++variant) {  // plain / non-temporal loads, the LDS-DMA tile stream at 9 / 6 / 4 waves per CU, register tiles: report the fastest
    HIPCHK(h, hipEventRecord(h->ev_h0, h->stream));
    HIPCHK(h, launch_stream_probe((const uint4*)d_src, n_bytes / 16, (uint32_t*)h->poison_count.ptr, variant, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_h1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_h1));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, h->ev_h0, h->ev_h1));
    if (variant == 0 || t < best) best = t;
  }
  const float ms = best;
  *ms_out = ms;
  h->h2d_valid = false;  // ev_h0/ev_h1 were reused
  return SURGE_OK;
}

}  // extern "C"
