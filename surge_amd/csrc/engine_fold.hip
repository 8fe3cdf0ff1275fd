// engine_fold.hip — folding the bound log: which kernel (plan_fold), the per-log index it needs, and the launch of each
// algorithm.  Every fold launch is timed the same way (timed_launch) inside the same frame (fold_begin / fold_end).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"

using namespace surge;

namespace {

// The kernels for this handle's op table: compiled (hiprtc, ~1 s) the first time a process folds with the table, shared by
// every handle with the same table; nullptr = the ahead-of-time kernels (why: surge_replay_kernel_info).  V1_FLAT: the flat
// kernel.  V1_LANES: the lane-per-row kernels (SORTED / CHUNKED / ROWS), compiled at surge_replay_prepare or the first such
// fold — like the per-log index, before the fold's timing events, never between them.
const V1Kernels* v1_spec(surge_replay_handle* h, const FoldParams& p, int kind) {
  Compiled<V1Kernels>& c = kind == V1_FLAT ? h->spec1 : h->lanes1;
  if (!c.tried) {
    c.tried = true;
    c.have = v1_kernels_acquire(p.table, h->device, kind, &c.k, &c.why);
    if (c.have) c.why = kind == V1_FLAT ? std::string("flat kernel compiled for the op table by ") + rtc_library_path() : "compiled for the op table";
  }
  return c.get();
}

// Wave-task size in events: a multiple of one tile (64 * lane_events events), about kTaskBytes of
// events at most, small enough that short logs still spread over the chip.
int64_t choose_task_events(int64_t n_events, int lane_events) {
  const int64_t tile = (int64_t)kWave * lane_events;
  int64_t task_bytes = kTaskBytes;
  if (const char* v = std::getenv("SURGE_REPLAY_TASK_KB")) task_bytes = (int64_t)std::atoi(v) * 1024;
  const int64_t max_tiles = task_bytes / (tile * 16) > 0 ? task_bytes / (tile * 16) : 1;
  int64_t target = kTargetTasks;
  if (const char* v = std::getenv("SURGE_REPLAY_TARGET_TASKS")) target = std::atoi(v) > 0 ? std::atoi(v) : target;
  int64_t tiles = (n_events / target + tile - 1) / tile;
  if (tiles < 1) tiles = 1;
  if (tiles > max_tiles) tiles = max_tiles;
  return tiles * tile;
}

// Events per lane per tile for each kernel (8 -> 8 KiB tiles and twice the resident waves, 16 -> 16 KiB
// tiles and half the per-tile scan overhead).  Tunable through the environment for experiments.
int env_lane_events(const char* name, int dflt) {
  const char* v = std::getenv(name);
  if (!v) return dflt;
  const int x = std::atoi(v);
  return (x == 8 || x == 16 || x == 32) ? x : dflt;
}

// Event pair bracketing the dominant kernel of this fold; pairs are kept per fold (up to
// kMaxTimedFolds since the last stats_reset) so a benchmark can average them without syncing per step.
int32_t next_fold_events(surge_replay_handle* h, hipEvent_t* e0, hipEvent_t* e1) {
  size_t i = h->folds_since_reset < kMaxTimedFolds ? h->folds_since_reset : kMaxTimedFolds - 1;
  while (h->fold_events.size() <= i) {
    hipEvent_t a = nullptr, b = nullptr;
    HIPCHK(h, hipEventCreate(&a));
    hipError_t e = hipEventCreate(&b);
    if (e != hipSuccess) {
      (void)hipEventDestroy(a);
      return fail_hip(h, e, "hipEventCreate");
    }
    h->fold_events.emplace_back(a, b);
  }
  *e0 = h->fold_events[i].first;
  *e1 = h->fold_events[i].second;
  h->ev_k0 = *e0;
  h->ev_k1 = *e1;
  h->folds_since_reset += 1;
  return SURGE_OK;
}

// The one way a fold's dominant kernel is launched: between the fold's next event pair, nothing else.  `launch` enqueues
// the kernel(s) and returns a SURGE_* status (nothing at all for a log with nothing to fold).  Whoever needs kernels
// compiled at run time (v1_spec) acquires them BEFORE calling this: a process's first fold with an op table
// compiles it (hiprtc, ~1 s), and that must land before the timed region, not inside it.
template <class Launch>
int32_t timed_launch(surge_replay_handle* h, int64_t n_tasks, Launch launch) {
  hipEvent_t e0, e1;
  SURGE_TRY(next_fold_events(h, &e0, &e1));
  HIPCHK(h, hipEventRecord(e0, h->stream));
  SURGE_TRY(launch());
  HIPCHK(h, hipEventRecord(e1, h->stream));
  h->st.n_tasks = (int32_t)n_tasks;
  return SURGE_OK;
}

// The persistent kernels: one wave per group of 64 rows, but no more waves than stay resident on the chip at per_cu a CU
// (env: the knob that overrides per_cu in experiments, or nullptr).
int64_t resident_waves(const surge_replay_handle* h, int64_t rows, int64_t per_cu, const char* env) {
  if (const char* v = env ? std::getenv(env) : nullptr) per_cu = std::atoi(v) > 0 ? std::atoi(v) : per_cu;
  const int64_t groups = (rows + kWave - 1) / kWave, slots = (int64_t)h->n_cus * per_cu;
  return groups < slots ? groups : slots;
}

// The persistent kernels pull groups from an atomic ticket counter that the last wave of every launch re-arms; the
// host only zeroes it when it is allocated.
int32_t dispenser_begin(surge_replay_handle* h, FoldParams& p) {
  if (!h->counter.ptr) {
    HIPCHK(h, h->counter.reserve(16));
    HIPCHK(h, hipMemset(h->counter.ptr, 0, 16));
  }
  p.counter = (unsigned long long*)h->counter.ptr;
  return SURGE_OK;
}

// scratch for ordering n rows by length (vals_b only when the caller does not supply its own output).  max_key: the largest
// key among them — below kCountSortMaxBins the hand-written counting sort orders them (its histograms are the only scratch),
// else rocPRIM's radix sort (temp + key / value double buffers).  min_temp: bytes the caller wants of `temp` besides.
int32_t index_scratch(surge_replay_handle* h, int64_t n, bool need_vals_b, int64_t max_key, size_t min_temp, IndexScratch* sc, size_t extra_bytes = 0,
                      void** extra = nullptr) {
  const size_t rows = (size_t)(n > 0 ? n : 1);
  const char* sort_env = std::getenv("SURGE_REPLAY_INDEX_SORT");  // "radix": rocPRIM's radix sort whatever the keys (the test that compares the two orders)
  const bool force_radix = sort_env && std::strcmp(sort_env, "radix") == 0;
  sc->counting = !force_radix && max_key >= 0 && max_key < kCountSortMaxBins;
  sc->max_key = (uint32_t)(max_key > 0 ? max_key : 0);
  sc->n_cus = h->n_cus;
  size_t tb = 0;
  if (sc->counting) tb = count_sort_scratch_bytes(n, sc->max_key, h->n_cus);
  else HIPCHK(h, index_temp_bytes(n, &tb));
  tb = tb > min_temp ? tb : min_temp;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_keys_a = up(tb), o_keys_b = o_keys_a + up(rows * 4), o_vals_a = o_keys_b + (sc->counting ? 0 : up(rows * 4)),
               o_vals_b = o_vals_a + (sc->counting ? 0 : up(rows * 8)), o_extra = o_vals_b + (need_vals_b ? up(rows * 8) : 0);
  HIPCHK(h, h->ix_arena.reserve(o_extra + extra_bytes));
  char* base = (char*)h->ix_arena.ptr;
  sc->temp = base;
  sc->temp_bytes = tb;
  sc->keys_a = (uint32_t*)(base + o_keys_a);
  sc->keys_b = sc->counting ? nullptr : (uint32_t*)(base + o_keys_b);
  sc->vals_a = sc->counting ? nullptr : (int64_t*)(base + o_vals_a);
  sc->vals_b = need_vals_b ? (int64_t*)(base + o_vals_b) : nullptr;
  if (extra) *extra = base + o_extra;
  return SURGE_OK;
}

// a bound log's index stands: give the build scratch back (a 10 M-aggregate log's is ~0.6 GB); micro-batch sorts keep theirs
void index_scratch_release(surge_replay_handle* h) {
  h->ix_arena.release();
  h->ix_cnt.release();
}

// the length order of these segments, into h->perm.  max_len: the longest of them (a bound log's longest aggregate), or -1
// where the host does not know it (a micro-batch's longest group: the radix sort).  timed: part of the bound log's index
int32_t build_length_order(surge_replay_handle* h, const int64_t* off, int64_t n_seg, int64_t max_len, bool timed) {
  HIPCHK(h, h->perm.reserve((size_t)(n_seg > 0 ? n_seg : 1) * 8));
  IndexScratch sc;
  SURGE_TRY(index_scratch(h, n_seg, false, max_len, 0, &sc));
  if (timed) HIPCHK(h, hipEventRecord(h->ev_i0, h->stream));
  HIPCHK(h, launch_sort_by_length(off, n_seg, sc, (int64_t*)h->perm.ptr, h->stream));
  if (timed) HIPCHK(h, hipEventRecord(h->ev_i1, h->stream));
  return SURGE_OK;
}

}  // namespace

namespace surge {

void fill_params(const surge_replay_schema& schema, FoldParams& p) {
  std::memset(&p, 0, sizeof(p));
  for (int i = 0; i < kTableEntries; ++i) {
    const uint32_t d = ((uint32_t)i < schema.n_types && i < SURGE_MAX_EVENT_TYPES) ? schema.desc[i] : SURGE_D_POISON;
    uint32_t* w = p.table[i];
    const uint32_t cop = d & SURGE_D_COUNT_MASK, sop = d & SURGE_D_SUM_MASK, cls = d & SURGE_CLS_MASK;
    if (d & SURGE_D_POISON) {
      w[TW_POISON] = ~0u;  // everything else stays zero: a throwing event has no effect on the fields
      w[TW_FLAGS] = 1u;
      if (i == kTableEntries - 1) {  // [17]: the null event that pads the last tile — identity on every state
        w[TW_POISON] = 0u;
        w[TW_FLAGS] = 0u;
      }
      continue;
    }
    if (cls == SURGE_CLS_DELETE) {
      w[TW_DELETE] = ~0u;  // a tombstone has no field ops
      w[TW_NOT_REQUIRE] = ~0u;
      w[TW_FLAGS] = 1u << 16;
      continue;
    }
    w[TW_CNT_NZ] = (cop == SURGE_D_COUNT_ADD || cop == SURGE_D_COUNT_SUB) ? ~0u : 0u;
    w[TW_CNT_NEG] = (cop == SURGE_D_COUNT_SUB) ? ~0u : 0u;
    w[TW_CNT_SET] = (cop == SURGE_D_COUNT_SET) ? ~0u : 0u;
    w[TW_VER_SET] = (d & SURGE_D_VERSION_SET) ? ~0u : 0u;
    w[TW_SUM_NZ] = (sop == SURGE_D_SUM_ADD || sop == SURGE_D_SUM_SUB) ? ~0u : 0u;
    w[TW_SUM_NEG] = (sop == SURGE_D_SUM_SUB) ? ~0u : 0u;
    w[TW_BAL_SET] = (d & SURGE_D_BALANCE_SET) ? ~0u : 0u;
    w[TW_EVC] = (d & SURGE_D_EVCOUNT_INC) ? 1u : 0u;
    w[TW_MATERIALIZES] = (cls == SURGE_CLS_MATERIALIZE || cls == SURGE_CLS_CREATE) ? ~0u : 0u;
    w[TW_NOT_REQUIRE] = (cls != SURGE_CLS_REQUIRE) ? ~0u : 0u;
    w[TW_CREATE] = (cls == SURGE_CLS_CREATE) ? ~0u : 0u;
    w[TW_MIN] = (d & SURGE_D_MIN_ARG) ? ~0u : 0u;
    w[TW_MAX] = (d & SURGE_D_MAX_ARG) ? ~0u : 0u;
    w[TW_FLAGS] = 0u;  // bit0 poison, bit16 delete; materializes goes in its own accumulator (TW_MATERIALIZES & 1)
  }
  const surge_state64& d = schema.default_state;
  p.d_count = d.count;
  p.d_version = d.version;
  p.d_sum = d.sum64;
  std::memcpy(&p.d_balance, &d.balance, 8);
  p.d_min = d.min_arg;
  p.d_max = d.max_arg;
  p.d_evcount = d.event_count;
}

void fill_params(const surge_replay_handle* h, FoldParams& p) { fill_params(h->schema, p); }

int32_t fold_begin(surge_replay_handle* h) {
  HIPCHK(h, hipEventRecord(h->ev_total0, h->stream));
  h->st.n_tasks = 0;
  return SURGE_OK;
}

int32_t fold_end(surge_replay_handle* h, int32_t algo) {
  HIPCHK(h, hipEventRecord(h->ev_total1, h->stream));
  h->timing_valid = true;
  h->st.last_algo = algo;
  h->st.n_folds += 1;
  h->st.n_poisoned = -1;
  h->fold_epoch.fetch_add(1);
  return SURGE_OK;
}

int32_t run_flat(surge_replay_handle* h, FoldParams& p, const int64_t* off, int64_t n_seg, int64_t span_events, const uint32_t* d_n_seg) {
  // short rows (a head in almost every lane): 8 KiB tiles — three waves per SIMD instead of two hide the per-head state
  // stores better than the halved scan overhead of 16 KiB tiles pays (uniform 1..32 events: 0.48 -> 0.53 of peak at 20 M
  // aggregates, 0.36 -> 0.42 at 2 M; Zipf(1..4096), mean 460: 16 KiB tiles stay ahead)
  const int le = env_lane_events("SURGE_REPLAY_LE_FLAT", (n_seg > 0 && span_events / n_seg < 64) ? 8 : 16);
  const int64_t task_events = choose_task_events(span_events, le);
  const int64_t n_tasks = (span_events + task_events - 1) / task_events;
  if (d_n_seg) {
    HIPCHK(h, h->plan.reserve_roomy((size_t)(n_tasks + 1) * 8));
    HIPCHK(h, launch_plan_dev(off, d_n_seg, task_events, n_tasks, (int64_t*)h->plan.ptr, h->stream));
  } else {
    HIPCHK(h, h->plan.reserve((size_t)(n_tasks + 1) * 8));
    HIPCHK(h, launch_plan(off, n_seg, task_events, n_tasks, (int64_t*)h->plan.ptr, h->stream));
  }
  p.seg_off = off;
  p.plan = (const int64_t*)h->plan.ptr;
  p.n_seg = n_seg;  // (0 with d_n_seg: FLAT takes its segments from the plan)
  const V1Kernels* spec = v1_spec(h, p, V1_FLAT);  // (a process's first fold with this op table compiles it: before the timed region, not inside it)
  return timed_launch(h, n_tasks, [&]() -> int32_t {
    HIPCHK(h, launch_fold_flat(p, spec, n_tasks, le, h->stream));
    return SURGE_OK;
  });
}

int32_t run_slots(surge_replay_handle* h, FoldParams& p, const int64_t* off, int64_t n_seg, bool cache_perm) {
  if (!cache_perm || !h->perm_valid) {
    SURGE_TRY(build_length_order(h, off, n_seg, cache_perm ? h->an.max_len : -1, false));
    h->perm_valid = cache_perm;
  }
  p.seg_off = off;
  p.plan = (const int64_t*)h->perm.ptr;
  SURGE_TRY(dispenser_begin(h, p));
  p.n_seg = n_seg;
  // the interpreter is VALU-bound and light on registers (93 VGPRs): 8 KiB tiles and as many resident waves as LDS
  // allows; the schema-specialised kernels keep their tile in registers like the v1 sorted-rows kernel: 16 KiB tiles, 8 waves
  const int le = env_lane_events("SURGE_REPLAY_LE_SLOTS", h->spec.have ? 16 : 8) == 16 ? 16 : 8;
  const int64_t n_waves = resident_waves(h, n_seg, le == 8 ? (h->spec.have ? 12 : 14) : 8, "SURGE_REPLAY_SLOTS_WAVES");
  return timed_launch(h, n_waves, [&]() -> int32_t {
    HIPCHK(h, launch_fold_slots(p, *(const SlotParams*)h->slot_params, h->spec.get(), n_waves, le, h->stream));
    return SURGE_OK;
  });
}

}  // namespace surge

namespace {

struct FoldPlan {
  int32_t use = SURGE_ALGO_FLAT;
  bool uniform = false;
  uint32_t chunk_T = 0;   // CHUNKED / TILED: aggregates longer than this are cut
  int64_t span = 0;
};

int32_t plan_fold(surge_replay_handle* h, int32_t algo, FoldPlan& pl) {
  if (!h->bound) return fail(h, SURGE_E_STATE, "fold before load_csr/bind_device_csr");
  if (!h->log_valid) return fail(h, SURGE_E_STATE, "the resident state was grown past the bound log (surge_replay_grow): load a log again");
  if (algo < SURGE_ALGO_AUTO || algo > SURGE_ALGO_SHORT) return fail(h, SURGE_E_INVALID, "unknown algo");
  if (h->v2 != (algo == SURGE_ALGO_SLOTS) && !(h->v2 && (algo == SURGE_ALGO_AUTO || algo == SURGE_ALGO_TILED)))
    return fail(h, SURGE_E_UNSUPPORTED, h->v2 ? "a v2 slot schema folds with SURGE_ALGO_AUTO / SURGE_ALGO_SLOTS / SURGE_ALGO_TILED only"
                                               : "SURGE_ALGO_SLOTS needs a handle created with surge_replay_create_v2");
  if (h->v2) {
    // one lane per WHOLE aggregate whatever the transport: the tile-major copy is built with nothing cut
    pl.use = algo == SURGE_ALGO_TILED ? SURGE_ALGO_TILED : SURGE_ALGO_SLOTS;
    pl.span = h->an.last - h->an.first;
    pl.chunk_T = 0x7ffffff8u;
    if (pl.use == SURGE_ALGO_TILED && h->an.max_len >= (1ll << 31))
      return fail(h, SURGE_E_UNSUPPORTED, "ALGO_SORTED / ALGO_CHUNKED / ALGO_TILED need segments shorter than 2^31 events");
    return SURGE_OK;
  }
  const int64_t span = h->an.last - h->an.first;
  pl.span = span;
  const bool uniform = h->n_agg > 0 && !h->an.nonuniform && h->an.n_empty == 0 && h->an.len0 > 0 &&
                       (h->an.len0 % 16) == 0 && h->an.len0 < (1ll << 31) && h->an.first == 0;
  pl.uniform = uniform;
  if ((algo == SURGE_ALGO_FIXED || algo == SURGE_ALGO_ROWS) && !uniform)
    return fail(h, SURGE_E_UNSUPPORTED, "ALGO_FIXED / ALGO_ROWS need equal segment lengths that are a multiple of 16");
  const bool rows_ok = uniform && h->an.len0 <= (1 << 20);  // 64 rows x L x 16 B must fit a 31-bit buffer offset
  if (algo == SURGE_ALGO_ROWS && !rows_ok) return fail(h, SURGE_E_UNSUPPORTED, "ALGO_ROWS needs L <= 2^20");
  // one lane per aggregate only pays when 64-aggregate groups alone can fill the chip: measured crossover
  // with FIXED between 512 groups (FIXED 20-50 % faster) and 1024 groups (ROWS 10-18 % faster, L = 64..1024)
  const bool rows_auto = rows_ok && h->n_agg / kWave >= 1024;
  const bool sorted_ok = h->an.max_len < (1ll << 31);
  if ((algo == SURGE_ALGO_SORTED || algo == SURGE_ALGO_CHUNKED || algo == SURGE_ALGO_TILED) && !sorted_ok)
    return fail(h, SURGE_E_UNSUPPORTED, "ALGO_SORTED / ALGO_CHUNKED / ALGO_TILED need segments shorter than 2^31 events");
  // Measured on MI355X (C3: 10 M aggregates, Zipf 1..4096): FLAT 16.2 ms (4.6 TB/s); SORTED (line-aligned
  // 256 B row pieces, 8 resident waves per CU) 12.1-12.7 ms (5.9-6.2 TB/s).  One lane per aggregate pays only when
  // rows are long enough to fill their 256-byte pieces (mean >= 64 events: at <= 32 events per aggregate the
  // lane-per-aggregate kernels measured 2-4x slower than the linear-stream FLAT kernel, at ~64 they tie).
  const double mean_len = h->n_nz > 0 ? (double)span / (double)h->n_nz : 0.0;
  // CHUNKED bounds the critical path: no wave walks more than ~T events alone.  T grows with the log (the longest
  // chunk's walk should stay a small fraction of the kernel; measured optimum on Zipf(1..4096) logs of 2–15 GB with the
  // final kernels: T ~ algorithmic bytes / 4 MB — 0.5 M aggregates 925, 0.8 M 1475, 1.25 M 2320; the optimum is flat
  // to the right and falls off quickly to the left of it) and cut aggregates get at most 256 chunks (the stitch kernel
  // walks them one by one).
  // When T reaches the longest aggregate nothing is cut and the plain sorted-rows kernel runs instead.
  uint32_t chunk_T = 0;
  {
    double t = (double)h->st.algorithmic_bytes / 4.0e6;
    const double t_min = (double)h->an.max_len / 256.0;
    t = t < t_min ? t_min : t;
    t = t < 256.0 ? 256.0 : (t > 65528.0 ? 65528.0 : t);
    chunk_T = ((uint32_t)t + 7u) & ~7u;
    if (const char* v = std::getenv("SURGE_REPLAY_CHUNK_T")) chunk_T = (uint32_t)std::atoi(v);
    chunk_T = chunk_T < 16u ? 16u : (chunk_T > 65528u ? 65528u : chunk_T);
    chunk_T &= ~7u;
  }
  pl.chunk_T = chunk_T;
  const bool nothing_to_cut = (int64_t)chunk_T >= h->an.max_len + 7;
  // one lane per aggregate / chunk pays from ~1.5 GB of log and a mean of 64 events per aggregate (shorter aggregates
  // run 2-4x faster on the linear-stream FLAT kernel; at 0.2 M Zipf aggregates = 1.5 GB CHUNKED and FLAT tie)
  const bool lanes_auto = sorted_ok && mean_len >= 64.0 && (double)h->st.algorithmic_bytes >= 1.5e9;
  // many short rows (a packed events topic whose aggregates published a handful of events each): one lane per row straight from
  // the CSR arrays.  Measured on the e2e topic's packed log (10 M aggregates, 1.4 events each): FLAT 0.29 of 8 TB/s.
  const bool short_auto = h->n_agg >= 65536 && h->an.max_len <= 64 && mean_len < 16.0 && h->an.max_len > 0;
  int32_t use = algo;
  if (algo == SURGE_ALGO_AUTO && short_auto && !uniform) {
    use = SURGE_ALGO_SHORT;
  } else if (algo == SURGE_ALGO_AUTO) {
    // AUTO never picks TILED: the tile-major copy costs about four folds and doubles the log's footprint, which only a
    // caller that replays the bound log repeatedly (or binds it long before it needs the states) wants to pay
    if (uniform)
      use = rows_auto ? SURGE_ALGO_ROWS : SURGE_ALGO_FIXED;
    else if (lanes_auto)
      use = nothing_to_cut ? SURGE_ALGO_SORTED : SURGE_ALGO_CHUNKED;
    else
      use = SURGE_ALGO_FLAT;
  }
  pl.use = use;
  return SURGE_OK;
}

// chunk table of the kernel-facing CSR for chunk target T (align: rows tiled from their 128-byte lines — CHUNKED)
int32_t build_chunk_index(surge_replay_handle* h, surge_replay_handle::ChunkIndex& ci, const KernelCsr& csr, uint32_t T, bool align) {
  const int64_t n_seg = csr.n_seg;
  // a virtual row is at most T + 7 slots long (an aggregate in one piece: at most T; a chunk: span / c rounded to lines)
  const int64_t max_row = (int64_t)T + 7 < h->an.max_len + 7 ? (int64_t)T + 7 : h->an.max_len + 7;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  // phase 1: the three counts per aggregate and their scans (one allocation: counts, then the scans' block sums)
  const size_t cnt_bytes = up((size_t)(n_seg + 1) * 3 * 8);
  HIPCHK(h, h->ix_cnt.reserve(cnt_bytes + scan_i64_scratch_bytes(n_seg + 1, 3)));
  int64_t* cnt = (int64_t*)h->ix_cnt.ptr;
  HIPCHK(h, launch_chunk_count(csr.off, n_seg, T, align, cnt, (char*)h->ix_cnt.ptr + cnt_bytes, h->stream));
  int64_t totals[3] = {0, 0, 0};  // virtual rows, cut aggregates, side slots
  for (int k = 0; k < 3; ++k)
    HIPCHK(h, hipMemcpyAsync(&totals[k], cnt + (int64_t)k * (n_seg + 1) + n_seg, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ci.rows.n_vrows = totals[0];
  ci.cut.n_cut = totals[1];
  // phase 2: the table itself (one allocation) ...
  const size_t rows = (size_t)(totals[0] > 0 ? totals[0] : 1), cut = (size_t)(totals[1] > 0 ? totals[1] : 1), slots = (size_t)(totals[2] > 0 ? totals[2] : 1);
  // the four arrays of `rows` virtual rows, carved from b: starts, destinations, lengths, infos
  auto carve_rows = [&](char* b, ChunkRows& r) {
    r.v_start = (int64_t*)b; r.v_dest = (int64_t*)(b + up(rows * 8)); r.v_len = (uint32_t*)(b + 2 * up(rows * 8));
    r.v_info = (uint32_t*)(b + 2 * up(rows * 8) + up(rows * 4));
  };
  const size_t rows_bytes = 2 * up(rows * 8) + 2 * up(rows * 4);
  {
    const size_t o_side = rows_bytes, o_slot0 = o_side + up(slots * 80), o_out = o_slot0 + up(cut * 8), o_c = o_out + up(cut * 8), total = o_c + up(cut * 4);
    HIPCHK(h, ci.arena.reserve(total));
    char* b = (char*)ci.arena.ptr;
    carve_rows(b, ci.rows);
    ci.rows.side = ci.cut.side = (uint32_t*)(b + o_side);
    ci.cut.r_slot0 = (int64_t*)(b + o_slot0); ci.cut.r_out = (int64_t*)(b + o_out); ci.cut.r_c = (uint32_t*)(b + o_c);
  }
  // ... and the scratch of its build (one allocation): the sort's, then the rows in aggregate order
  IndexScratch sc;
  void* extra = nullptr;
  SURGE_TRY(index_scratch(h, ci.rows.n_vrows, true, max_row, 0, &sc, rows_bytes, &extra));  // the rows (>= aggregates) are what gets sorted
  ChunkRows u;
  carve_rows((char*)extra, u);
  HIPCHK(h, launch_chunk_table(csr, T, align, cnt, sc, u, ci.rows, ci.cut, h->stream));
  ci.T = T;
  return SURGE_OK;
}

// Build (once per bound log) whatever index the chosen kernel needs: the length order (SORTED), the chunk table
// (CHUNKED), the chunk table + the tile-major copy of the log (TILED).  Timed with HIP events; see
// surge_replay_layout_info.
int32_t ensure_index(surge_replay_handle* h, const FoldPlan& pl) {
  if (h->n_agg <= 0 || pl.span <= 0) return SURGE_OK;
  const KernelCsr csr = h->csr();
  if (pl.use == SURGE_ALGO_SORTED && !h->perm_valid) {
    SURGE_TRY(build_length_order(h, csr.off, csr.n_seg, h->an.max_len, true));
    h->perm_valid = true;
    h->index_timed = true;
    h->relayout_timed = false;
    h->index_algo = SURGE_ALGO_SORTED;
  } else if (pl.use == SURGE_ALGO_CHUNKED && h->cidx.T != pl.chunk_T) {
    HIPCHK(h, hipEventRecord(h->ev_i0, h->stream));
    SURGE_TRY(build_chunk_index(h, h->cidx, csr, pl.chunk_T, true));
    HIPCHK(h, hipEventRecord(h->ev_i1, h->stream));
    h->index_timed = true;
    h->relayout_timed = false;
    h->index_algo = SURGE_ALGO_CHUNKED;
  } else if (pl.use == SURGE_ALGO_TILED && (!h->tiled_valid || h->tidx.T != pl.chunk_T)) {
    h->tiled_valid = false;
    HIPCHK(h, hipEventRecord(h->ev_i0, h->stream));
    SURGE_TRY(build_chunk_index(h, h->tidx, csr, pl.chunk_T, false));
    const ChunkRows& rows = h->tidx.rows;
    const int64_t n_groups = (rows.n_vrows + kWave - 1) / kWave;
    HIPCHK(h, h->t_gsub.reserve((size_t)(n_groups + 1) * 8));
    HIPCHK(h, launch_tile_index(rows.v_len, rows.n_vrows, (int64_t*)h->t_gsub.ptr, h->stream));
    HIPCHK(h, launch_exclusive_scan_i64((int64_t*)h->t_gsub.ptr, n_groups, h->stream));
    int64_t n_sub = 0;
    HIPCHK(h, hipMemcpyAsync(&n_sub, (int64_t*)h->t_gsub.ptr + n_groups, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_i1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->t_n_sub = n_sub;
    HIPCHK(h, h->t_tiles.reserve((size_t)n_sub * kTileSubBytes));
    HIPCHK(h, hipEventRecord(h->ev_r0, h->stream));
    HIPCHK(h, launch_relayout(h->d_events, rows.v_start, rows.v_len, rows.n_vrows, (const int64_t*)h->t_gsub.ptr, n_sub, (uint4*)h->t_tiles.ptr, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_r1, h->stream));
    if (std::getenv("SURGE_DBG_PRINT"))
      std::fprintf(stderr, "[surge dbg] tiles %p (%lld subtiles) v_len %p v_info %p v_dest %p g_sub %p state %p events %p\n", h->t_tiles.ptr,
                   (long long)n_sub, (void*)rows.v_len, (void*)rows.v_info, (void*)rows.v_dest, h->t_gsub.ptr, (void*)h->d_state, (const void*)h->d_events);
    h->tiled_valid = true;
    h->index_timed = h->relayout_timed = true;
    h->index_algo = SURGE_ALGO_TILED;
  } else {
    return SURGE_OK;  // nothing was built
  }
  index_scratch_release(h);  // (hipFree waits for the build's kernels)
  return SURGE_OK;
}

// ---- one function per fold of the bound log (beside run_flat and run_slots above): each sets its parameters, acquires its
// compiled kernels before the timed region and launches between the fold's event pair ---------------------------------------

int32_t run_rows(surge_replay_handle* h, FoldParams& p) {
  const int le = env_lane_events("SURGE_REPLAY_LE_ROWS", 8);
  // a task = G groups of 64 aggregates, about kTaskBytes of events
  // Measured on MI355X: this access pattern runs fastest as ONE resident generation of waves (no
  // re-dispatch, every wave streams from start to end): G groups of 64 aggregates per wave so that
  // the grid just fits the chip's wave slots (CUs x 16 waves at 8 KiB tiles, x 9 at 16 KiB tiles).
  const int64_t groups = (h->n_agg + kWave - 1) / kWave;
  const int64_t slots = (int64_t)h->n_cus * (le == 8 ? 16 : (le == 16 ? 9 : 4));
  int64_t G = (groups + slots - 1) / slots;
  if (const char* v = std::getenv("SURGE_REPLAY_ROWS_GROUPS")) G = std::atoi(v);
  if (G < 1) G = 1;
  const int64_t per_task = G * kWave;
  const int64_t n_tasks = (h->n_agg + per_task - 1) / per_task;
  p.n_seg = h->n_agg;
  p.fixed_len = h->an.len0;
  p.segs_per_task = per_task;
  const V1Kernels* lanes = v1_spec(h, p, V1_LANES);
  return timed_launch(h, n_tasks, [&]() -> int32_t {
    HIPCHK(h, launch_fold_rows(p, lanes, n_tasks, le, h->stream));
    return SURGE_OK;
  });
}

int32_t run_fixed(surge_replay_handle* h, FoldParams& p, int64_t span) {
  const int le = env_lane_events("SURGE_REPLAY_LE_FIXED", 16);
  const int64_t L = h->an.len0;
  const int64_t task_events = choose_task_events(span, le);
  int64_t G = task_events / L;
  if (G < 1) G = 1;
  const int64_t n_tasks = (h->n_agg + G - 1) / G;
  p.n_seg = h->n_agg;
  p.fixed_len = L;
  p.segs_per_task = G;
  return timed_launch(h, n_tasks, [&]() -> int32_t {
    HIPCHK(h, launch_fold_fixed(p, n_tasks, le, h->stream));
    return SURGE_OK;
  });
}

int32_t run_short(surge_replay_handle* h, FoldParams& p) {
  p.seg_off = h->d_seg_off;  // every aggregate is a row, the empty ones too
  p.n_seg = h->n_agg;
  return timed_launch(h, (h->n_agg + 63) / 64, [&]() -> int32_t {
    HIPCHK(h, launch_fold_short(p, h->stream));
    return SURGE_OK;
  });
}

int32_t run_sorted(surge_replay_handle* h, FoldParams& p, const KernelCsr& csr) {
  const int le = env_lane_events("SURGE_REPLAY_LE_SORTED", 16);
  p.out_map = csr.out_map;
  p.seg_off = csr.off;
  p.plan = (const int64_t*)h->perm.ptr;
  SURGE_TRY(dispenser_begin(h, p));
  p.n_seg = csr.n_seg;
  // resident waves per CU = min(LDS, registers): 8 KiB tiles 12 (136 VGPRs), 16 KiB tiles 8 (18.6 KB LDS), 32 KiB tiles 4
  const int64_t n_waves = resident_waves(h, csr.n_seg, le == 8 ? 12 : (le == 16 ? 8 : 4), "SURGE_REPLAY_SORTED_WAVES");  // (experiments)
  const V1Kernels* lanes = v1_spec(h, p, V1_LANES);
  // round 5: the walk that fetches the next group's first tile during this group's last one (fold_sorted_pf_kernel);
  // SURGE_REPLAY_SORTED_KERNEL=plain keeps fold_sorted_kernel for a same-box comparison, and 32-event lanes are its only
  static const bool plain = [] { const char* v = std::getenv("SURGE_REPLAY_SORTED_KERNEL"); return v && std::strcmp(v, "plain") == 0; }();
  return timed_launch(h, n_waves, [&]() -> int32_t {
    if (plain || (le == 32 && !lanes)) HIPCHK(h, launch_fold_sorted(p, n_waves, le, h->stream));
    else HIPCHK(h, launch_fold_sorted_pf(p, lanes, n_waves, le, h->stream));
    return SURGE_OK;
  });
}

int32_t run_chunked(surge_replay_handle* h, FoldParams& p, const KernelCsr& csr) {
  const int le = env_lane_events("SURGE_REPLAY_LE_CHUNKED", 16) == 8 ? 8 : 16;
  const auto& ci = h->cidx;
  SURGE_TRY(dispenser_begin(h, p));
  p.n_seg = csr.n_seg;
  // resident waves per CU: 16 KiB tiles 8 (2 per SIMD, 8 x 18.7 KB of LDS), 8 KiB tiles 12 (3 per SIMD)
  const int64_t n_waves = resident_waves(h, ci.rows.n_vrows, le == 8 ? 12 : 8, nullptr);
  const V1Kernels* lanes = v1_spec(h, p, V1_LANES);
  return timed_launch(h, n_waves, [&]() -> int32_t {  // the stitch kernel is timed with the fold: it is part of it
    HIPCHK(h, launch_fold_chunked(p, ci.rows, ci.cut, lanes, n_waves, le, h->stream));
    return SURGE_OK;
  });
}

// TILED, v1 and v2 (whose rows are whole aggregates, never cut) alike: the fold over the tile-major copy
int32_t run_tiled(surge_replay_handle* h, FoldParams& p, const KernelCsr& csr) {
  const auto& ci = h->tidx;
  if (h->v2) p.out_map = csr.out_map;
  int subs = 2;  // subtiles (8 events per lane) per step: 16 KiB in flight per wave
  if (const char* v = std::getenv("SURGE_REPLAY_TILED_SUBS")) subs = std::atoi(v) == 1 ? 1 : 2;
  SURGE_TRY(dispenser_begin(h, p));
  p.n_seg = csr.n_seg;
  // resident waves per CU.  Measured (round 3, same handle, Zipf(1..4096) logs of 9 / 30 / 74 GB and config C2): with
  // 16 KiB steps 6 waves per CU beat 8 and 9 by 0.3-7 % and 4 by 0-5 %; 8 KiB steps are 0.5-4 % behind at any count
  const int64_t n_waves = resident_waves(h, ci.rows.n_vrows, subs == 1 ? 8 : 6, "SURGE_REPLAY_TILED_WAVES");
  TileTable t;  // (the one place the kernels' table is made: the chunk table's rows over the tile-major copy)
  t.tiles = (const uint4*)h->t_tiles.ptr; t.g_sub0 = (const int64_t*)h->t_gsub.ptr; t.v_len = ci.rows.v_len;
  t.v_info = ci.rows.v_info; t.v_dest = ci.rows.v_dest; t.n_vrows = ci.rows.n_vrows;
  t.side = h->v2 ? nullptr : ci.rows.side;
  return timed_launch(h, n_waves, [&]() -> int32_t {  // the stitch kernel is timed with the fold: it is part of it
    if (h->v2) {
      HIPCHK(h, launch_fold_slots_tiled(p, *(const SlotParams*)h->slot_params, h->spec.get(), t, n_waves, subs, h->stream));
      return SURGE_OK;
    }
    HIPCHK(h, launch_fold_tiled(p, t, n_waves, subs, h->stream));
    HIPCHK(h, launch_chunk_stitch(p, ci.cut, h->stream));
    return SURGE_OK;
  });
}

// surge_replay_compile_schema(_v2): the program through hiprtc for `arch`, the code object to the caller
int32_t compile_out(const std::string& source, const char* arch, void* code_out, int64_t capacity, int64_t* code_bytes) {
  std::vector<char> code;
  std::string log;
  double ms = 0.0;
  if (!rtc_compile(source, arch, &code, &log, &ms)) return fail(nullptr, SURGE_E_UNSUPPORTED, log);
  *code_bytes = (int64_t)code.size();
  if (code_out) {
    if (capacity < (int64_t)code.size()) return fail(nullptr, SURGE_E_INVALID, "code_out is too small (see *code_bytes)");
    std::memcpy(code_out, code.data(), code.size());
  }
  return SURGE_OK;
}

}  // namespace

extern "C" {

int32_t surge_replay_kernel_info(surge_replay_handle* h, surge_replay_kernel_info_t* out) {
  if (!h || !out) return fail(h, SURGE_E_INVALID, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  if (!h->v2) {  // v1: the flat kernel (K3 appends, AUTO on logs of few long rows) is the one compiled per op table
    DeviceGuard g(h->device);
    FoldParams p;
    fill_params(h, p);
    (void)v1_spec(h, p, V1_FLAT);
  }
  out->specialised = (h->v2 ? h->spec.have : h->spec1.have) ? 1 : 0;
  out->compile_ms = h->v2 ? h->spec.k.compile_ms : h->spec1.k.compile_ms;
  std::string d = h->v2 ? h->spec.why
                        : (h->spec1.have ? h->spec1.why : "v1 schema, ahead-of-time kernels interpret the op table: " + h->spec1.why);
  if (!h->v2 && h->lanes1.tried) d = "lane kernels " + (h->lanes1.have ? h->lanes1.why : "ahead of time (" + h->lanes1.why.substr(0, 60) + ")") + "; " + d;
  std::snprintf(out->detail, sizeof(out->detail), "%s", d.c_str());
  return SURGE_OK;
}

int32_t surge_replay_compile_schema(const surge_replay_schema* schema, const char* arch, void* code_out, int64_t capacity, int64_t* code_bytes) {
  if (!schema || !arch || !code_bytes) return fail(nullptr, SURGE_E_INVALID, "NULL argument");
  *code_bytes = 0;
  SURGE_TRY(validate_schema(schema));
  FoldParams p;
  fill_params(*schema, p);
  const std::string src = v1_spec_source(p.table, V1_FLAT);
  if (src.empty()) return fail(nullptr, SURGE_E_UNSUPPORTED, "the op table holds words the specialised build cannot express");
  if (const char* v = std::getenv("SURGE_REPLAY_RTC_LANES")) {
    if (std::atoi(v) != 0) {  // the lane kernels' program too (its code object goes to the disk cache, not to the caller)
      int64_t lanes_bytes = 0;
      SURGE_TRY(compile_out(v1_spec_source(p.table, V1_LANES), arch, nullptr, 0, &lanes_bytes));
    }
  }
  return compile_out(src, arch, code_out, capacity, code_bytes);
}

int32_t surge_replay_compile_schema_v2(const surge_replay_schema_v2* sc, const char* arch, void* code_out, int64_t capacity,
                                       int64_t* code_bytes) {
  if (!sc || !arch || !code_bytes) return fail(nullptr, SURGE_E_INVALID, "NULL argument");
  *code_bytes = 0;
  SURGE_TRY(validate_schema_v2(sc));
  alignas(16) unsigned char spb[kSlotParamsBytes] = {};
  slot_params_from_schema(*sc, (SlotParams*)spb);
  return compile_out(slots_spec_source(*(const SlotParams*)spb), arch, code_out, capacity, code_bytes);
}

int32_t surge_replay_prepare(surge_replay_handle* h, int32_t algo) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  DeviceGuard g(h->device);
  FoldPlan pl;
  SURGE_TRY(plan_fold(h, algo, pl));
  if (h->v2 && pl.use != SURGE_ALGO_TILED) return SURGE_OK;  // the slot kernel's length order is built by its first fold
  if (!h->v2 && (pl.use == SURGE_ALGO_SORTED || pl.use == SURGE_ALGO_CHUNKED || pl.use == SURGE_ALGO_ROWS)) {
    FoldParams p;
    fill_params(h, p);
    (void)v1_spec(h, p, V1_LANES);  // the kernels for this op table (hiprtc, or the code-object cache on disk)
  }
  return ensure_index(h, pl);
}

int32_t surge_replay_layout_info(surge_replay_handle* h, surge_replay_layout_info_t* out) {
  if (!h || !out) return fail(h, SURGE_E_INVALID, "NULL argument");
  if (!h->bound) return fail(h, SURGE_E_STATE, "layout_info before load_csr/bind_device_csr");
  DeviceGuard g(h->device);
  std::memset(out, 0, sizeof(*out));
  out->algo = h->index_algo;
  if (h->index_algo == SURGE_ALGO_CHUNKED) {
    out->virtual_rows = h->cidx.rows.n_vrows;
    out->cut_aggregates = h->cidx.cut.n_cut;
    out->chunk_events = h->cidx.T;
  } else if (h->index_algo == SURGE_ALGO_TILED) {
    out->virtual_rows = h->tidx.rows.n_vrows;
    out->cut_aggregates = h->tidx.cut.n_cut;
    out->chunk_events = h->tidx.T;
    out->tiled_bytes = h->t_n_sub * kTileSubBytes;
    out->padding_events = h->t_n_sub * (kTileSubBytes / 16) - (h->an.last - h->an.first);
  } else if (h->index_algo == SURGE_ALGO_SORTED) {
    out->virtual_rows = h->csr().n_seg;
  }
  if (h->index_timed) {
    HIPCHK(h, hipEventSynchronize(h->ev_i1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev_i0, h->ev_i1));
    out->index_build_ms = ms;
  }
  if (h->relayout_timed) {
    HIPCHK(h, hipEventSynchronize(h->ev_r1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev_r0, h->ev_r1));
    out->relayout_ms = ms;
  }
  return SURGE_OK;
}

int32_t surge_replay_index_order(surge_replay_handle* h, int32_t algo, int64_t* order_out, int64_t capacity, int64_t* n_out) {
  if (!h || !n_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  *n_out = 0;
  if (!h->bound) return fail(h, SURGE_E_STATE, "index_order before load_csr/bind_device_csr");
  if (capacity < 0 || (capacity > 0 && !order_out)) return fail(h, SURGE_E_INVALID, "bad capacity / buffer");
  DeviceGuard g(h->device);
  const void* src = nullptr;
  int64_t n = 0;
  if (algo == SURGE_ALGO_SORTED && h->perm_valid && !h->v2) {
    src = h->perm.ptr;
    n = h->csr().n_seg;
  } else if (algo == SURGE_ALGO_CHUNKED && h->cidx.T != 0) {
    src = h->cidx.rows.v_start;
    n = h->cidx.rows.n_vrows;
  } else {
    return fail(h, SURGE_E_STATE, "the bound log has no index of that kind (surge_replay_prepare / fold with SURGE_ALGO_SORTED or _CHUNKED first)");
  }
  *n_out = n;
  const int64_t take = n < capacity ? n : capacity;
  if (take > 0) {
    HIPCHK(h, hipMemcpyAsync(order_out, src, (size_t)take * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return SURGE_OK;
}

int32_t surge_replay_fold(surge_replay_handle* h, int32_t algo) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  DeviceGuard g(h->device);
  FoldPlan pl;
  SURGE_TRY(plan_fold(h, algo, pl));
  SURGE_TRY(ensure_index(h, pl));  // once per bound log (part of its index, like the empty-segment compaction)
  const int64_t span = pl.span;
  const int32_t use = pl.use;
  const KernelCsr csr = h->csr();

  FoldParams p;
  if (h->v2) std::memset(&p, 0, sizeof(p));  // a slot schema has no op table: the kernels take it from h->slot_params
  else fill_params(h, p);
  p.events = h->d_events;
  p.n_events = h->n_events;
  p.init = h->d_init;
  p.out = h->d_state;

  SURGE_TRY(fold_begin(h));
  if (h->n_agg > 0 && span > 0) {
    switch (use) {
      case SURGE_ALGO_ROWS: SURGE_TRY(run_rows(h, p)); break;
      case SURGE_ALGO_FIXED: SURGE_TRY(run_fixed(h, p, span)); break;
      case SURGE_ALGO_SHORT: SURGE_TRY(run_short(h, p)); break;
      case SURGE_ALGO_SORTED: SURGE_TRY(run_sorted(h, p, csr)); break;
      case SURGE_ALGO_CHUNKED: SURGE_TRY(run_chunked(h, p, csr)); break;
      case SURGE_ALGO_TILED: SURGE_TRY(run_tiled(h, p, csr)); break;
      case SURGE_ALGO_SLOTS:
        if (h->an.max_len >= (1ll << 31)) return fail(h, SURGE_E_UNSUPPORTED, "segments must be shorter than 2^31 events");
        p.out_map = csr.out_map;
        SURGE_TRY(run_slots(h, p, csr.off, csr.n_seg, true));
        break;
      default:
        p.out_map = csr.out_map;
        SURGE_TRY(run_flat(h, p, csr.off, csr.n_seg, span));
    }
  } else {
    SURGE_TRY(timed_launch(h, 0, [] { return (int32_t)SURGE_OK; }));  // nothing to fold: an empty timed region
  }
  if ((h->an.n_empty > 0 && !(use == SURGE_ALGO_SHORT && span > 0)) || span == 0)
    HIPCHK(h, launch_fill_empty(h->d_seg_off, h->n_agg, h->d_init, h->d_state, h->stream));
  return fold_end(h, use);
}

}  // extern "C"
