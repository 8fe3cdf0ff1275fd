// engine_internal.h — what the units of the host engine share (engine.hip, engine_fold.hip, engine_append.hip,
// engine_states.hip, engine_comm.hip): the handle, device memory, error reporting and the few helpers that cross units.
// Host only; not part of the C ABI (that is include/surge_replay.h).
#pragma once

#include <atomic>
#include <cstdint>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <utility>
#include <vector>

#include "replay_internal.h"

namespace surge {

struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&ptr, bytes ? bytes : 16);
    if (e == hipSuccess) cap = bytes ? bytes : 16;
    return e;
  }
  // for the buffers of a stream of micro-batches: the next batch is a few per cent larger or smaller than this one, and a
  // buffer that grows is freed — hipFree waits for the whole device (3 - 6 ms spikes per fetch on the bytes -> states path)
  hipError_t reserve_roomy(size_t bytes) { return bytes <= cap ? hipSuccess : reserve(bytes + bytes / 4 + 4096); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// One run-time compiled program of a handle (K: V1Kernels, SlotKernels): its kernels once acquired, else why the
// ahead-of-time ones run (what surge_replay_kernel_info reports).
template <class K>
struct Compiled {
  K k;  // (k.compile_ms stays 0 when nothing was compiled)
  bool have = false, tried = false;
  std::string why;
  const K* get() const { return have ? &k : nullptr; }
};

}  // namespace surge

struct surge_replay_handle {
  using DevBuf = surge::DevBuf;
  int device = 0;
  int n_cus = 256;
  hipStream_t stream = nullptr;
  surge_replay_schema schema{};
  bool v2 = false;                     // ABI v2 slot schema: folds only through fold_slots.hip
  surge_replay_schema_v2 schema2{};
  alignas(16) unsigned char slot_params[surge::kSlotParamsBytes] = {};
  // the kernels compiled for this handle's schema (process-wide modules, rtc_module.hip); `why`: which libhiprtc compiled them,
  // or why the ahead-of-time kernels run instead
  surge::Compiled<surge::SlotKernels> spec;  // v2: acquired when the handle is created; none = the interpreter
  surge::Compiled<surge::V1Kernels> spec1;   // v1: the flat kernel (acquired at the first flat fold)
  surge::Compiled<surge::V1Kernels> lanes1;  // v1: the lane-per-row kernels, SORTED / CHUNKED / ROWS (first lane fold / prepare)
  std::string err;
  std::mutex err_mu;  // concurrent point readers may fail at the same time

  // the bound log (owned copies or borrowed device pointers)
  DevBuf own_seg_off, own_events, own_init, own_state;
  const int64_t* d_seg_off = nullptr;
  const uint4* d_events = nullptr;
  const uint4* d_init = nullptr;
  uint4* d_state = nullptr;
  int64_t n_agg = 0, n_events = 0;
  bool bound = false;
  bool log_valid = false;  // false once the resident state was grown past the bound CSR (append_* only until the next load)

  // analysis of the bound CSR (computed at load/bind time)
  surge::CsrAnalysis an{};
  DevBuf d_analysis, nz_off, nz_map, block_counts;
  int64_t n_nz = 0;
  // what the kernels fold: with empty segments the compacted arrays (+ rank -> aggregate map), otherwise the bound ones
  surge::KernelCsr csr() const {
    if (an.n_empty > 0) return {(const int64_t*)nz_off.ptr, n_nz, (const int64_t*)nz_map.ptr};
    return {d_seg_off, n_agg, nullptr};
  }
  DevBuf perm, counter;  // SORTED: segments by descending length (built lazily, per bound log)
  // scratch of the index builds (index_kernels.hip): rocPRIM temp, sort keys / values, the chunk table's counts and its
  // rows in aggregate order; released once the bound log's index stands
  // (two allocations, carved: a hipMalloc costs 50 - 300 us and a hipFree waits for the device — ten of each were most of
  // the chunk table's 3 - 7 ms in round 5)
  DevBuf ix_arena, ix_cnt;
  bool perm_valid = false;
  // CHUNKED / TILED: the chunk table (built lazily, per bound log), the chunk summaries and the list of cut aggregates
  struct ChunkIndex {
    surge::DevBuf arena;      // one allocation; the pointers below are views into it
    surge::ChunkRows rows;
    surge::StitchTable cut;
    uint32_t T = 0;  // the chunk target the table was built for (0 = none built)
    void release() {
      arena.release();
      rows = {};
      cut = {};
      T = 0;
    }
  };
  ChunkIndex cidx;              // CHUNKED: rows tiled from their 128-byte lines in the CSR log
  ChunkIndex tidx;              // TILED: rows copied to tile boundaries
  DevBuf t_tiles, t_gsub;  // TILED: the tile-major copy of the log, first subtile of every group
  int64_t t_n_sub = 0;          // subtiles (8 KiB each) of the tile-major copy
  bool tiled_valid = false;
  // one-off costs of the bound log's index (device time between HIP events), reported by surge_replay_layout_info
  hipEvent_t ev_i0 = nullptr, ev_i1 = nullptr, ev_r0 = nullptr, ev_r1 = nullptr;
  bool index_timed = false, relayout_timed = false;
  int32_t index_algo = 0;

  // per-fold scratch
  DevBuf plan, batch_group_agg, batch_group_off, batch_events, poison_count, gather_idx, gather_out, scan_totals;

  hipEvent_t ev_total0 = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_total1 = nullptr, ev_h0 = nullptr,
             ev_h1 = nullptr;
  bool timing_valid = false, h2d_valid = false;
  surge_replay_stats_t st{};
  // one HIP-event pair per fold since the last stats_reset (kernel time of the dominant kernel)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> fold_events;
  size_t folds_since_reset = 0;

  // append_events: device group-by scratch (stream_kernels.hip) and pinned H2D staging of host batches
  DevBuf gb_temp, gb_u32, gb_flags, gb_agg_idx, gb_events;
  // hipHostMalloc'ed staging of host batches (agg_idx then events), two areas used in turn: the host fills one while the
  // copy engine still drains the other; ev_staged[k] = "the H2D copies out of area k are done"
  void* pinned[2] = {nullptr, nullptr};
  size_t pinned_cap[2] = {0, 0};
  hipEvent_t ev_staged[2] = {nullptr, nullptr};
  bool staged_busy[2] = {false, false};
  int pinned_next = 0;
  uint32_t* host_flags = nullptr;  // pinned: {groups, bad, skipped batches} of the last device group-by, copied back async
  uint32_t skipped_seen = 0;       // skipped batches already reported to the host

  // the packer's staging log (surge_replay_stage_events_device): aggregate indices (u32) and events (16 B) in topic order
  DevBuf stage_keys, stage_events;
  int64_t staged_n = 0, stage_cap = 0;

  DevBuf published;                      // the last committed snapshot (surge_replay_snapshot_delta), n_agg x 64 B
  int64_t published_n = 0;
  const uint8_t* encode_filter = nullptr;  // surge_replay_set_encode_filter
  surge::JsonSide json_side{};           // Double-text tables (device copy, made on first use), side string columns
  DevBuf f64_tables, nan_count;
  DevBuf rows_off;                       // surge_replay_encode_json_rows: lengths, then offsets, of the rows asked for
  alignas(16) uint8_t decode_base[64] = {};       // surge_replay_set_decode_base: what a decoded row's unnamed bytes hold
  int32_t decode_mode = SURGE_STATE_READ_STRICT;  // surge_replay_set_decode_mode
  DevBuf sd_ptab, sd_counts, sd_last, sd_status;  // surge_replay_decode_json_states: parse table, counters, last record per aggregate, statuses
  DevBuf shard_counts;  // surge_replay_partition_hash_utf8_device: {malformed ids, the lowest of them}

  surge::CommState* comm = nullptr;  // the snapshot exchange (comm.hip), created by surge_replay_comm_init
  DevBuf gathered[2];         // handle-owned output of allgather_snapshot(d_out = NULL), per slot
  int64_t gathered_rows[2] = {0, 0};
  int32_t comm_world = 1;

  // host mirror for point reads (S2)
  std::shared_mutex mu;  // readers share it against the published mirror; snapshot / device reads take it exclusively
  std::vector<uint8_t> mirror;
  std::atomic<int64_t> fold_epoch{0};
  int64_t delta_epoch = -1, delta_n = -1;  // fold epoch / aggregate count the last snapshot_delta's kinds describe
  int64_t mirror_epoch = -1;
};

namespace surge {

// engine.hip.  The message also becomes the failing thread's surge_replay_last_error(NULL), whichever unit failed.
int32_t fail(surge_replay_handle* h, int32_t code, const std::string& msg);
int32_t fail_hip(surge_replay_handle* h, hipError_t e, const char* what);

#define HIPCHK(h, call)                                   \
  do {                                                    \
    hipError_t e_ = (call);                               \
    if (e_ != hipSuccess) return fail_hip(h, e_, #call); \
  } while (0)

// a SURGE_* status that is not SURGE_OK ends the caller with it (whoever produced it has set the message)
#define SURGE_TRY(call)                 \
  do {                                  \
    const int32_t rc_ = (call);         \
    if (rc_ != SURGE_OK) return rc_;    \
  } while (0)

int32_t validate_schema(const surge_replay_schema* s);
int32_t validate_schema_v2(const surge_replay_schema_v2* sc);
constexpr size_t kMaxTimedFolds = 256;  // HIP-event pairs (one per fold) a handle keeps since the last stats_reset

// engine_fold.hip
void fill_params(const surge_replay_schema& schema, FoldParams& p);
void fill_params(const surge_replay_handle* h, FoldParams& p);
// Every fold is framed by this pair: ev_total0 and st.n_tasks = 0, then ev_total1 and what a finished fold leaves in the stats.
int32_t fold_begin(surge_replay_handle* h);
int32_t fold_end(surge_replay_handle* h, int32_t algo);
// plan + flat fold over an arbitrary kernel-facing CSR.  d_n_seg: a micro-batch whose group count only the device knows
// (where the group-by left it; n_seg = 0), nullptr: the host's n_seg counts
int32_t run_flat(surge_replay_handle* h, FoldParams& p, const int64_t* off, int64_t n_seg, int64_t span_events, const uint32_t* d_n_seg = nullptr);
// v2: length-sort the kernel-facing segments (once per bound log / per micro-batch), then one lane per segment
int32_t run_slots(surge_replay_handle* h, FoldParams& p, const int64_t* off, int64_t n_seg, bool cache_perm);

// engine_append.hip
int32_t report_skipped_batches(surge_replay_handle* h);

}  // namespace surge
