// replay_internal.h — shared between the HIP kernels and the host engine: what each unit offers the others, unit by unit.
// Not part of the C ABI (that is include/surge_replay.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/surge_replay.h"
#include "fold_layout.h"

namespace surge {

struct CsrAnalysis {
  int32_t bad;              // a negative segment length was seen
  int32_t nonuniform;       // lengths differ
  int64_t n_empty;
  int64_t len0;             // length of segment 0
  int64_t max_len;
  int64_t first, last;      // seg_off[0], seg_off[n]
};

// Every launch wrapper below is asynchronous on `stream`.

// ---- rtc.cpp: hiprtc (dlopen'ed) and the code-object cache on disk -----------------------------------------------
bool rtc_compile(const std::string& source, const char* arch, std::vector<char>* code, std::string* log, double* ms);
const char* rtc_library_path();
// ---- rtc_module.hip: the run-time compiled programs this process has loaded ----------------------------------------
struct RtcModule {
  hipModule_t module = nullptr;
  std::vector<hipFunction_t> fn;  // the entry points, in the order they were asked for
  double compile_ms = 0.0;
};
bool rtc_disabled(std::string* why);  // SURGE_REPLAY_RTC=0: nothing is compiled at run time (*why says so)
// The module of one program on one device: compiled (source() makes its text) and loaded the first time a process asks for
// `key`, the same object ever after; a key that failed once is not tried again.  Keys start with their program's kind.
// Never fails the caller: on any problem nullptr, and *why says what happened.
const RtcModule* rtc_module_acquire(const std::string& key, int device, const std::function<std::string()>& source,
                                    const std::vector<const char*>& entry_points, std::string* why);
// one wave-sized block per grid entry, the kernel's arguments as one block of bytes
hipError_t launch_module_kernel(hipFunction_t fn, int64_t grid, unsigned lds, hipStream_t stream, const void* args, size_t args_bytes);

// ---- fold_v1_spec.hip: the kernels compiled for one v1 op table (host only) ----------------------------------------
// Filled per handle from the process-wide module of the table; the launchers take nullptr for the ahead-of-time kernels
// that read the table from LDS.
enum { V1_FLAT = 0, V1_LANES = 1 };  // the two run-time compiled programs of a v1 op table
struct V1Kernels {
  hipFunction_t flat8 = nullptr, flat16 = nullptr;                                  // V1_FLAT
  hipFunction_t sorted8 = nullptr, sorted16 = nullptr, sorted32 = nullptr, chunked8 = nullptr, chunked16 = nullptr, rows8 = nullptr, rows16 = nullptr;  // V1_LANES
  double compile_ms = 0.0;
};
std::string v1_spec_source(const uint32_t (*table)[kTableWords], int kind);  // the program handed to hiprtc ("" = not expressible)
// never fails the caller: false, and *why says why the ahead-of-time kernels run
bool v1_kernels_acquire(const uint32_t (*table)[kTableWords], int device, int kind, V1Kernels* out, std::string* why);

// ---- fold_kernels.hip: the flat, fixed, rows, plain sorted and short-rows folds -------------------------------------
// The <events per lane, concrete walk> pair a lane-per-row kernel is instantiated for: f(LaneWalk<LE, CONC>{}) for 8 or
// (anything else) 16 events per lane and the walk SURGE_REPLAY_WALK selects (concrete_walk: read once per process).
template <int LE_, bool CONC_>
struct LaneWalk {
  static constexpr int LE = LE_;
  static constexpr bool CONC = CONC_;
};
bool concrete_walk();  // false: SURGE_REPLAY_WALK=transformer (the transformer walk everywhere, for comparisons)
template <class F>
void for_lane_walk(int lane_events, F&& f) {
  const bool conc = concrete_walk();
  if (lane_events == 8) {
    if (conc) f(LaneWalk<8, true>{}); else f(LaneWalk<8, false>{});
  } else {
    if (conc) f(LaneWalk<16, true>{}); else f(LaneWalk<16, false>{});
  }
}
hipError_t launch_fold_fixed(const FoldParams& p, int64_t n_tasks, int lane_events, hipStream_t stream);
hipError_t launch_fold_flat(const FoldParams& p, const V1Kernels* spec, int64_t n_tasks, int lane_events, hipStream_t stream);
// lanes: the V1_LANES kernels compiled for the handle's op table, or nullptr = the ahead-of-time kernels (op table in LDS)
hipError_t launch_fold_rows(const FoldParams& p, const V1Kernels* lanes, int64_t n_tasks, int lane_events, hipStream_t stream);
hipError_t launch_fold_sorted(const FoldParams& p, int64_t n_waves, int lane_events, hipStream_t stream);
hipError_t launch_fold_short(const FoldParams& p, hipStream_t stream);  // K1s: one lane per aggregate of a log of many short rows (p.seg_off over ALL aggregates, empty ones included)

// ---- csr_kernels.hip: the CSR of a bound log or a micro-batch made ready for a fold ---------------------------------
hipError_t launch_plan(const int64_t* off, int64_t n_seg, int64_t task_events, int64_t n_tasks,
                       int64_t* plan, hipStream_t stream);
hipError_t launch_plan_dev(const int64_t* off, const uint32_t* d_n_seg, int64_t task_events, int64_t n_tasks, int64_t* plan,
                           hipStream_t stream);
hipError_t launch_analyze_csr(const int64_t* off, int64_t n_seg, CsrAnalysis* d_result, hipStream_t stream);
hipError_t launch_fill_empty(const int64_t* off, int64_t n_seg, const uint4* init, uint4* out,
                             hipStream_t stream);
// Stable compaction of non-empty segments: nz_off[n_nz+1], nz_map[n_nz].  d_block_counts is scratch of
// ceil(n_seg/1024)+1 int64.
hipError_t launch_compact_nonempty(const int64_t* off, int64_t n_seg, int64_t* d_block_counts,
                                   int64_t* nz_off, int64_t* nz_map, hipStream_t stream);
// in-place exclusive scan of v[0..n) with the total appended at v[n] (single block: index-time use only)
hipError_t launch_exclusive_scan_i64(int64_t* v, int64_t n, hipStream_t stream);

// ---- fold_chunked.hip: SORTED pipelined across groups, CHUNKED and the stitch of cut aggregates ----------------------
// The chunk table of a bound log as the host holds it (the engine's ChunkIndex: views into one allocation).
struct ChunkRows {  // the virtual rows, longest first: what the kernels' ChunkTable / TileTable are made from
  int64_t* v_start = nullptr;   // first event slot of the row
  uint32_t* v_len = nullptr;    // event slots from there
  uint32_t* v_info = nullptr;   // VI_*
  int64_t* v_dest = nullptr;    // aggregate index (state array) or side-buffer slot
  int64_t n_vrows = 0;
  uint32_t* side = nullptr;     // the chunk summaries of cut aggregates, 80 bytes each
};
struct StitchTable {  // the cut aggregates: r_c[r] summaries from side slot r_slot0[r] on compose onto aggregate r_out[r]
  uint32_t* side = nullptr;
  int64_t* r_slot0 = nullptr;
  uint32_t* r_c = nullptr;
  int64_t* r_out = nullptr;
  int64_t n_cut = 0;
};
// the sorted-rows fold over whole aggregates (the chunked kernel's walk); 8 or 16 events per lane (32: compiled kernels only)
hipError_t launch_fold_sorted_pf(const FoldParams& p, const V1Kernels* lanes, int64_t n_waves, int lane_events, hipStream_t stream);
hipError_t launch_fold_chunked(const FoldParams& p, const ChunkRows& rows, const StitchTable& cut, const V1Kernels* lanes, int64_t n_waves,
                               int lane_events, hipStream_t stream);
hipError_t launch_chunk_stitch(const FoldParams& p, const StitchTable& cut, hipStream_t stream);

// ---- index_kernels.hip: the per-log indexes (length order, chunk table), built with rocPRIM sorts / scans -----------
struct KernelCsr {         // the kernel-facing CSR of the bound log (surge_replay_handle::csr)
  const int64_t* off;      // n_seg + 1 offsets, no empty segment among them
  int64_t n_seg;
  const int64_t* out_map;  // segment -> aggregate, or nullptr: segment i is aggregate i
};
struct IndexScratch {  // engine-owned device scratch, sized for the rows being ordered
  void* temp;          // the counting sort's histograms (counting) or rocPRIM temporary storage
  size_t temp_bytes;
  uint32_t *keys_a, *keys_b;  // n x u32 each (keys_b: rocPRIM path only)
  int64_t *vals_a, *vals_b;   // n x i64 each (vals_a: rocPRIM path only; launch_sort_by_length writes its result to `perm` instead of vals_b)
  bool counting;       // keys <= max_key < kCountSortMaxBins: the hand-written counting sort (length_sort.hip), else rocPRIM's radix sort
  uint32_t max_key;
  int n_cus;
};
hipError_t launch_sort_by_length(const int64_t* off, int64_t n_seg, const IndexScratch& sc, int64_t* perm, hipStream_t stream);
// CHUNKED / TILED: the chunk table of the kernel-facing CSR.  cnt: 3 x (n_seg + 1) int64.
hipError_t launch_chunk_count(const int64_t* off, int64_t n_seg, uint32_t T, bool align, int64_t* cnt, void* scan_scratch, hipStream_t stream);
// Phase 2: the rows in aggregate order (u: scratch of v.n_vrows rows), sorted by length into v; the cut aggregates into cut.
hipError_t launch_chunk_table(const KernelCsr& csr, uint32_t T, bool align, const int64_t* cnt, const IndexScratch& sc, const ChunkRows& u,
                              const ChunkRows& v, const StitchTable& cut, hipStream_t stream);
// ---- index_radix.hip: rocPRIM's radix sort (rows of 8192 events and more), in a unit of its own ----------------------------
hipError_t index_temp_bytes(int64_t n, size_t* bytes);
hipError_t launch_radix_sort_pairs_desc(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const int64_t* vals_in,
                                        int64_t* vals_out, int64_t n, hipStream_t stream);
// ---- length_sort.hip: the stable descending counting sort of the indexes, and the exclusive scans of the chunk counts ----------
constexpr int kCountSortMaxBins = 8192;
size_t count_sort_scratch_bytes(int64_t n, uint32_t max_key, int n_cus);
hipError_t launch_count_sort_desc(const uint32_t* keys, const int64_t* off, int64_t n, uint32_t max_key, int n_cus, void* scratch, int64_t* perm,
                                  hipStream_t stream);
size_t scan_i64_scratch_bytes(int64_t n, int k_arrays);
hipError_t launch_exclusive_scans_i64(int64_t* v, int64_t n, int64_t stride, int k_arrays, void* scratch, hipStream_t stream);
// ---- fold_tiled.hip: the chunk table's virtual rows copied once into group-major / tile-major order, then the fold
// over that copy.  g_sub: n_groups + 1 int64 (subtiles per group, scanned in place into offsets by the caller).
constexpr int kTileSubBytes = 8192;
hipError_t launch_tile_index(const uint32_t* v_len, int64_t n_vrows, int64_t* g_sub, hipStream_t stream);
hipError_t launch_relayout(const uint4* events, const int64_t* v_start, const uint32_t* v_len, int64_t n_vrows, const int64_t* g_sub0,
                           int64_t n_sub_total, uint4* tiles, hipStream_t stream);
hipError_t launch_fold_tiled(const FoldParams& p, const TileTable& t, int64_t n_waves, int subs, hipStream_t stream);
// ---- state_kernels.hip: partition hash, stream probe, the state encoders, snapshots ----------------------------------
hipError_t launch_partition_hash(const uint16_t* utf16, const int64_t* str_off, int64_t n,
                                 int32_t n_partitions, int32_t* part_out, bool up_to_colon, hipStream_t stream);
hipError_t launch_stream_probe(const uint4* src, int64_t n_vec, uint32_t* sink, int variant, hipStream_t stream);
struct F64Tables;
struct JsonSide {
  const F64Tables* f64;                              // device copy of the Double-text tables (f64_text.h); needed by SURGE_JP_F64
  const uint8_t* str[SURGE_JSON_STRING_COLUMNS];     // side string columns (SURGE_JP_STR), UTF-8
  const int64_t* str_off[SURGE_JSON_STRING_COLUMNS];
  unsigned long long* not_a_number;                  // += aggregates skipped because a Double of theirs is NaN / infinite
};
struct JsonRows {  // the encoders over a row list (surge_replay_encode_json_rows): output slot q is aggregate rows[q]
  const int64_t* rows;      // -1: a miss (zero bytes)
  int64_t n_agg;            // rows outside [-1, n_agg) are counted in *bad and never dereferenced
  uint8_t* kind;            // nullable: the write pass leaves each slot's SURGE_READ_* here
  unsigned long long* bad;
};
// rows == nullptr: the n resident aggregates in index order (d_len_off: n + 1 entries)
hipError_t launch_json_encode(const surge_json_template& tmpl, const uint4* states, int64_t n, const uint8_t* keys,
                              const int64_t* key_off, int64_t* d_len_off, int64_t* d_totals, uint8_t* out, bool write_pass,
                              uint32_t envelope, const uint8_t* filter, const JsonSide& side, hipStream_t stream, const JsonRows* rows = nullptr);
// ---- state_decode.hip: serialized state values -> 64-byte states (surge_replay_decode_json_states / _protobuf_states) ----
struct F64ParseTable;
enum { SD_WRITTEN = 0, SD_TOMBSTONES = 1, SD_REFUSED = 2, SD_AMBIGUOUS = 3, SD_FIRST_REFUSED = 4, SD_BAD_INDEX = 5, SD_N_COUNTS = 6 };
struct StateDecodeParams {
  const uint8_t* values;        // record r's text: values[value_off[r] .. value_off[r + 1])
  const int64_t* value_off;
  int64_t n_records;
  const uint8_t* keys;          // nullable pair: the ids the KEY strings must equal
  const int64_t* key_off;
  const int64_t* agg_idx;       // nullable: record r is aggregate r
  unsigned long long* last1;    // agg_idx only: n_agg entries of scratch (1 + the last record that names the aggregate)
  int64_t n_agg;
  uint4* states;
  uint4 base[4];                // ORed into every decoded row: zero wherever the template (or the flags word) writes
  uint8_t* status;              // nullable
  int64_t* spans;               // nullable
  const F64ParseTable* ptab;    // device copy of the Eisel-Lemire table (f64_parse.h)
  unsigned long long* counts;   // SD_N_COUNTS entries
  bool envelope;                // every value is a protobuf State message around the template's text (the same for the whole launch)
  bool lenient;                 // the lenient reading mode (surge_replay_set_decode_mode; likewise the same for the whole launch)
};
struct StateFieldTable;  // state_parse.h
hipError_t launch_state_decode(const surge_json_template& tmpl, const StateDecodeParams& p, hipStream_t stream, const StateFieldTable* fields = nullptr);
// ---- state_strings.hip: the STR spans of decoded state values -> a side string column (surge_replay_merge_state_strings) ----
struct StateStringsParams {
  const uint8_t* values;        // record r's text: values[value_off[r] .. value_off[r + 1])  (NULL: every value is empty)
  const int64_t* value_off;
  int64_t n_records;
  const int64_t* agg_idx;       // nullable: record r is aggregate r
  const uint8_t* status;        // as the decoder left them: only SURGE_STATE_DECODE_OK records contribute
  const int64_t* spans;         // per record 2 x SURGE_JSON_STRING_COLUMNS {offset into the value, length}
  int32_t column;
  unsigned long long* win1;     // n_agg entries of scratch: 1 + the highest OK record that names the aggregate (NULL with no records)
  int64_t n_agg;
  const uint8_t* prev;          // the column so far (nullable: every previous string is empty)
  const int64_t* prev_off;      // n_prev + 1
  int64_t n_prev;
  uint8_t* out;
  int64_t* out_off;             // n_agg + 1: lengths, then (scanned by the caller) offsets
};
hipError_t launch_state_strings_winners(const StateStringsParams& p, unsigned long long* bad, hipStream_t stream);
hipError_t launch_state_strings_pass(const StateStringsParams& p, bool write, hipStream_t stream);
// state_kernels.hip again: the encoders' exclusive scan of v[0 .. n) in place; d_totals: ceil(n / 1024) + 1 entries of scratch, the
// grand total lands in d_totals[ceil(n / 1024)]
hipError_t launch_scan_lengths_i64(int64_t* v, int64_t n, int64_t* d_totals, hipStream_t stream);
// kind[a] in SURGE_SNAP_*; d_counts: two u64 {values, tombstones}; commit: published := states where kind != SKIP
hipError_t launch_snapshot_invalidate(uint4* published, int64_t n, const uint8_t* kind, hipStream_t stream);
hipError_t launch_snapshot_commit(const uint4* states, uint4* published, int64_t n, const uint8_t* kind, hipStream_t stream);
hipError_t launch_snapshot_delta(const uint4* states, uint4* published, int64_t n, uint8_t* kind, unsigned long long* d_counts,
                                 bool commit, bool full64, hipStream_t stream);
// unpack == false: in = n x 64 B, out = n x 40 B; unpack == true: in = n x 40 B, out = n x 64 B
hipError_t launch_pack_states(const void* in, int64_t n, void* out, bool unpack, hipStream_t stream);
hipError_t launch_gather_states(const uint4* states, const int64_t* idx, int64_t n, uint4* out, hipStream_t stream);
hipError_t launch_count_poisoned(const uint4* states, int64_t n, unsigned long long* d_count,
                                 hipStream_t stream);

// ---- fold_slots.hip: the fold of ABI v2 slot schemas ------------------------------------------------------------
struct SlotParams;
constexpr size_t kSlotParamsBytes = 512;  // >= sizeof(SlotParams): the engine keeps it as opaque storage
void slot_params_from_schema(const surge_replay_schema_v2& sc, SlotParams* out);
// The slot kernels compiled for one schema (hiprtc), filled per handle from the process-wide module of the schema; the
// launchers take nullptr for the interpreter.
struct SlotKernels {
  hipFunction_t csr8 = nullptr, csr16 = nullptr, tiled1 = nullptr, tiled2 = nullptr;
  double compile_ms = 0.0;
};
std::string slots_spec_source(const SlotParams& sp);  // the program handed to hiprtc for this schema
// never fails the caller: false, and *why says why the interpreter runs
bool slot_kernels_acquire(const SlotParams& sp, int device, SlotKernels* out, std::string* why);
hipError_t launch_fold_slots(const FoldParams& p, const SlotParams& sp, const SlotKernels* spec, int64_t n_waves, int lane_events,
                             hipStream_t stream);
hipError_t launch_fold_slots_tiled(const FoldParams& p, const SlotParams& sp, const SlotKernels* spec, const TileTable& t, int64_t n_waves,
                                   int subs, hipStream_t stream);


// ---- stream_kernels.hip: K3 micro-batch group-by on the device ------------------------------------------------
hipError_t groupby_temp_bytes(uint32_t n, unsigned key_bits, size_t* bytes);
hipError_t launch_groupby(const int64_t* d_agg_idx, const uint4* d_events, uint32_t n, int64_t n_agg, unsigned key_bits, void* d_temp,
                          size_t temp_bytes, uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, uint32_t* head,
                          uint32_t* gid, uint4* d_sorted_events, int64_t* d_group_agg, int64_t* d_group_off, uint32_t* d_flags,
                          hipStream_t stream);

// the packer (surge_replay_pack_staged): staged (aggregate, event) pairs in topic order -> CSR
hipError_t launch_pack_stage(const int64_t* d_agg_idx, uint32_t n, uint32_t* keys, hipStream_t stream);
hipError_t pack_temp_bytes(uint32_t n, unsigned key_bits, size_t* bytes);
hipError_t launch_pack(const uint32_t* keys_a, const uint4* staged_events, uint32_t n, int64_t n_agg, unsigned key_bits, void* d_temp, size_t temp_bytes,
                       uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, int64_t* seg_off, uint4* out, uint32_t* d_bad, hipStream_t stream);

// ---- comm.hip: the snapshot exchange over RCCL (dlopen'ed) ----------------------------------------------------
struct CommState;
int32_t comm_unique_id(uint8_t* id_out, std::string* err);
int32_t comm_create(int device, int rank, int world, const uint8_t* id, CommState** out, std::string* err);
void comm_destroy(CommState* c);
int32_t comm_info(const CommState* c, int32_t* rank, int32_t* world, int32_t* version, const char** library);
// force: run the (collective) exchange even when counts for this n_local are cached — the public, documented-collective call
int32_t comm_counts(CommState* c, int64_t n_local, int64_t* counts_out, int64_t* max_count_out, bool force, std::string* err);
int32_t comm_allgather(CommState* c, hipStream_t compute, const void* d_states, int64_t n_local, void* d_out,
                       int64_t out_rows_per_rank, int slot, int mode, bool packed, std::string* err);
int32_t comm_wait(CommState* c, hipStream_t compute, int slot, bool host, std::string* err);
// in-process groups (one host process drives every rank; peer copies instead of RCCL)
int32_t comm_create_local(int device, int rank, int world, CommState** out, std::string* err);
bool comm_is_local(const CommState* c);
int32_t comm_allgather_local(CommState* const* cs, const hipStream_t* compute, const void* const* d_states, const int64_t* n_local,
                             void* const* d_out, int64_t out_rows_per_rank, int world, int slot, bool packed, std::string* err);

}  // namespace surge
