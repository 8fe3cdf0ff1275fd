// ingest_device.h — what the translation units of the device decoder share.  Internal, like replay_internal.h: not part of
// the C ABI.  Each stage is a unit of its own that knows the plain structs below and nothing of the decoder around it
// (the host object: ingest_decoder.hip and its units ingest_stage1.hip, ingest_stage2.hip, ingest_reads.hip, ingest_columns.hip,
// ingest_handover.hip, which share ingest_decoder_internal.h): ingest_crc.hip, ingest_lz4.hip, ingest_records.hip, ingest_intern.hip,
// ingest_order.hip, ingest_strings.hip.  Their launch_* functions enqueue on the stream they are given and return what the runtime
// said; none of them waits for the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/surge_ingest.h"
#include "f64_parse.h"

namespace surge {
namespace ingest {

// per-record status
enum : uint32_t {
  RS_OK = 0,
  RS_SKIP = 1,          // the producer's flush record (empty key, empty value): not an event
  RS_NULL = 2,          // null key or null value: not an event
  RS_MALFORMED = 3,     // varint / span runs past its record or batch
  RS_JSON = 4,          // value is not the JSON the template describes
  RS_TYPE = 5,          // unknown discriminator value
  RS_FIELD = 6,         // a field the template names is missing or is not the number it should be
  RS_SIZE = 7,          // fixed-16 topic: value is not 16 bytes
  RS_F64_HOST = 8,      // a Double the fast parser cannot decide: the host re-parses this value exactly
  RS_COLLISION = 9,     // two different keys with the same 64-bit hash
  RS_EMPTY_VALUE = 10,  // state mode: an empty, non-null value under a key (writeState never writes one; the loader reads empty as a tombstone)
  RS_ENVELOPE = 11,     // enveloped events (JsonCtx::envelope): the value is not `[aggregateId] [payload]` and nothing else (sp_envelope_spans, state_parse.h)
  RS_KEY_MISMATCH = 12, // ... its aggregateId is not the aggregate id of the record's key
  RS_BELOW = 13,        // below its section's floor (a consumer's start offset): passed over like RS_SKIP — not an error, never reported
  RS_STRING = 14,       // kept event strings (ingest_strings.hip): the record's class names a string field the value lacks, or that string is refused
  RS_COUNT,            // (how many there are: the host's text per status is checked against it, ingest_stage2.hip)
};

struct RecMeta {
  int64_t key_off, val_off, offset;
  uint64_t hash;
  int32_t key_len;   // aggregate id length (key up to ':')
  int32_t val_len;
  uint32_t slot;
  uint32_t status;
};

struct Section {  // = surge_batch_section + the batch's first record index in this push
  int64_t byte_off, byte_len, base_offset;
  int32_t n_records, reserved;
  int64_t rec_first;
};

struct ErrorCell {
  unsigned long long first_bad;  // min over (record index << 8 | status)
  unsigned int reserved, n_f64_host;
  unsigned int lz4_bad;          // the first section whose LZ4 frame did not decode (~0 = none)
  unsigned int crc_bad;          // the first section whose bytes do not give the batch's CRC-32C (~0 = none; SURGE_INGEST_DEVICE_CRC)
  unsigned int n_below;          // records below their section's floor (RS_BELOW)
  unsigned int snappy_bad;       // the first section with a snappy chunk that did not decode (~0 = none; ingest_snappy.hip)
};

__device__ __forceinline__ void report(ErrorCell* err, int64_t rec, uint32_t status) {
  atomicMin(&err->first_bad, ((unsigned long long)rec << 8) | status);
}

// a batch whose CRC-32C the device finishes (ingest_crc.hip)
struct CrcSpan {
  int64_t off;      // first byte the device still has to run the CRC over, in the staged bytes
  int32_t len;
  int32_t section;
  uint32_t expect;  // the batch's CRC-32C
  uint32_t state;   // the CRC register in front of `off`: after the 40 header bytes (the host ran those), or ~0 (in-place framing:
                    // off points at the header bytes, the device runs everything)
};

// one block of an LZ4 frame (ingest_lz4.hip)
struct Lz4Block {
  int64_t src_off;   // in the staged bytes
  int64_t dst_off;   // in the decompressed area
  int32_t src_len;   // bit 31: stored uncompressed
  int32_t section;   // the section this block belongs to
  int32_t last;      // the frame's last block: sets the section's length
  int32_t index;     // k: this block's number inside its frame
  int64_t seq_off;   // first entry of this block in the sequence table (two-pass decode); -1: the one-pass kernel takes it
};

// The scratch of the two-pass LZ4 decode, per push.  The caller allocates what lz4_scratch_bytes asks for and sets the four
// pointers; launch_lz4 clears the class counters and lays the class lists out behind them.
struct Lz4Work {
  int32_t dbg = 0;     // SURGE_DBG_DECODE (timing experiments only): 1 = image in, image out; 2 = the byte maps are built, never applied
  int32_t* state;      // per block: >= 0 decoded (its size), -1 malformed
  int32_t* n_seq;      // per block: entries written
  uint2* seq;          // the sequence table
  int32_t* cls_count;  // [kLz4Classes + 1]: blocks per LDS class; the last is "stored" (no LDS: copied as they are)
  int32_t* cls_list;   // [kLz4Classes + 1][n_blocks]
};
constexpr int kLz4Classes = 6;

struct Lz4ScratchBytes {  // bytes behind Lz4Block table, Lz4Work::state, ::n_seq, ::seq and ::cls_count (all 0: a push without LZ4 blocks)
  size_t blocks = 0, state = 0, n_seq = 0, seq = 0, cls = 0;
};

// The LZ4 work of one push, built up section by section by lz4_plan_section.
struct Lz4Plan {
  std::vector<Lz4Block> blocks;  // (the source of an asynchronous copy: it lives as long as the push)
  int64_t area = 0;              // bytes of the device-side decompressed area handed out so far (multiples of 64 KiB)
  int64_t n_seq = 0;             // sequence-table entries handed out (two-pass decode)
  void clear() { blocks.clear(); area = 0; n_seq = 0; }
};

enum Lz4Route {
  LZ4_ON_DEVICE,  // the frame's blocks joined the plan; its output starts at *area_off of the decompressed area
  LZ4_ON_HOST,    // a frame the device does not take block by block: decompressed here, appended to host_out
  LZ4_TOO_LARGE,  // ... which expands beyond 2 GiB
  LZ4_BAD_FRAME,  // ... which does not decode
};

typedef const __attribute__((address_space(3))) uint8_t* lds_ptr_t;

// Four bytes from p on, whatever its alignment, as ONE load instruction: the two aligned dwords that hold them
// (ds_read2_b32 / global_load_dwordx2), funnel-shifted into place.  Reads up to 7 bytes past p: the staged bytes and the
// LDS copies of a section end at least 16 bytes after their last byte.  (Round 5: the record and JSON walks read their bytes
// one ds_read_u8 at a time — ~200 dependent LDS reads per record; section_kernel waited 71 % of its wave cycles.)
// (the aligned pointer is derived from p by pointer arithmetic, not through an integer: the compiler keeps p's address space —
// global_load for the staged bytes, not flat_load)
__device__ __forceinline__ uint32_t load4(lds_ptr_t p) {
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  const __attribute__((address_space(3))) uint32_t* q = (const __attribute__((address_space(3))) uint32_t*)(p - sh);
  return __builtin_amdgcn_alignbyte(q[1], q[0], sh);
}
__device__ __forceinline__ uint32_t load4(const uint8_t* p) {
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* q = (const uint32_t*)(p - sh);
  return __builtin_amdgcn_alignbyte(q[1], q[0], sh);
}

// 64-bit hash of an aggregate id under the table's seed (a re-seed follows a detected collision); 0 marks an empty slot.
// (begin / end: the record parser hashes the id while it looks for its ':')
__device__ __forceinline__ uint64_t hash_key_begin(uint64_t seed) { return 0x9E3779B97F4A7C15ull + seed * 0xC2B2AE3D27D4EB4Full; }
__device__ __forceinline__ uint64_t hash_key_end(uint64_t h, int n, uint64_t seed) {
  h ^= (uint64_t)n * 0xFF51AFD7ED558CCDull;
  h ^= h >> 29;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  if (seed >> 63) h &= 0xffull;  // test hook (SURGE_INGEST_DEBUG_WEAK_HASH): collisions guaranteed until the first re-seed
  return h == 0ull ? 1ull : h;
}
template <typename P>
__device__ __forceinline__ uint64_t hash_key(P p, int n, uint64_t seed) {
  uint64_t h = hash_key_begin(seed);
  for (int i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
  return hash_key_end(h, n, seed);
}

// The template as the kernels use it: the distinct field names the decoder has to look for, with their lengths, and per
// event type which of them carry its sequence number / argument — so ONE pass over the object finds everything (round 3
// walked the text twice: once for the discriminator, once for the fields of the type it selected).
constexpr int kEvjNames = 1 + 2 * SURGE_EVJ_MAX_TYPES;
struct EvjDevice {
  uint32_t n_types, n_names;                  // names[0] is the discriminator ("" when the template has none)
  alignas(8) char names[kEvjNames][SURGE_EVJ_NAME];
  uint8_t name_len[kEvjNames];
  alignas(8) char type_name[SURGE_EVJ_MAX_TYPES][SURGE_EVJ_NAME];
  uint8_t type_name_len[SURGE_EVJ_MAX_TYPES];
  uint8_t seq_name[SURGE_EVJ_MAX_TYPES], arg_name[SURGE_EVJ_MAX_TYPES];  // index into names, 0xff = none
  uint32_t event_type[SURGE_EVJ_MAX_TYPES], arg_kind[SURGE_EVJ_MAX_TYPES];
};

constexpr int kEvjTrack = 8;  // numeric field names tracked in registers; templates with more use the generic lookup below

struct JsonCtx {  // what the value decoder needs besides the value
  const EvjDevice* tmpl;  // nullptr: 16-byte fixed events
  const surge::F64ParseTable* ptab;
  int32_t dbg = 0;  // SURGE_DBG_DECODE (timing experiments only, results are NOT the topic's): 1 = sections are staged, nothing else; 2 = staged and chained, no record decoded
  int16_t states = 0;  // state mode (surge_device_decoder_create_states): the id is the whole key, a null value is a tombstone, no value is decoded
  int16_t envelope = 0;  // SURGE_EVJ_ENVELOPE_* of the event template: what lies around the JSON text.  (Two halves of what was one int32: the
                         // struct is a kernel argument, and one that grows moves every argument behind it in section_kernel's instructions.)
#ifdef SURGE_EXPERIMENTS
  unsigned long long* ticks = nullptr;  // per workgroup: wall clock (10 ns) at start, after staging, after the chain, at the end
#endif
};

// ---- the key table (ingest_intern.hip) -------------------------------------------------------------------------------------
// One 16-byte slot per entry (round 5; three parallel arrays before): a probe, the flag pass and the final gather each touch
// ONE random line of the 2^25-slot table per record instead of two or three.
struct TableSlot {
  unsigned long long hash;  // 0 = empty
  uint32_t key_id;          // 0xffffffff = not assigned yet (inserted by the push in flight)
  uint32_t first_rec;       // of a slot inserted by the push in flight: its first record (0xffffffff otherwise)
};
static_assert(sizeof(TableSlot) == 16, "one slot = one 16-byte store");
struct Table {
  TableSlot* s;
  uint64_t mask;
};

struct KeyTable {  // the table with what stands behind its ids
  Table t;
  uint8_t* arena;                // the key bytes, one id after the other
  int64_t* key_off;              // [n_keys + 1] into the arena
  unsigned long long* key_hash;  // [n_keys] under the current seed
  int64_t n_keys, arena_bytes;
};

struct InternScratch {  // per push: (n_rec + 1) entries each, and rocPRIM's temporary storage
  unsigned long long *first, *first_scan;
  uint32_t *keep, *keep_pos;
  void* temp;
  size_t temp_bytes;
};

// ---- ingest_crc.hip: one wave per span over the staged bytes; a mismatch lowers err->crc_bad to the span's section ----------
hipError_t launch_crc(const uint8_t* bytes, const CrcSpan* spans, int32_t n_spans, ErrorCell* err, hipStream_t st);

// ---- ingest_lz4.hip ----------------------------------------------------------------------------------------------------------
// plans the section whose records are the LZ4 frame [frame, frame + frame_len), staged at src_off of the device bytes
Lz4Route lz4_plan_section(Lz4Plan& plan, const uint8_t* frame, int64_t frame_len, int64_t src_off, int32_t section, int64_t* area_off,
                          std::vector<uint8_t>& host_out);
Lz4ScratchBytes lz4_scratch_bytes(const Lz4Plan& plan);
// decodes the plan's blocks (d_blocks: their table on the device) from `bytes` into `area`; a frame's last block sets its
// section's byte_len, a frame that does not decode zeroes it and lowers err->lz4_bad
hipError_t launch_lz4(const Lz4Plan& plan, const uint8_t* bytes, uint8_t* area, const Lz4Block* d_blocks, Lz4Work w, Section* sections, ErrorCell* err, hipStream_t st);

// the second pass alone (lz4_exec_kernel, one launch per LDS class) over a block table whose first pass has run: entries, sizes
// and class lists in `w`.  It knows nothing of LZ4: ingest_snappy.hip runs it over the entries its own parse kernel wrote.
hipError_t launch_lz4_exec(const uint8_t* bytes, uint8_t* area, const Lz4Block* d_blocks, int64_t n_blocks, Lz4Work w, hipStream_t st);

// ---- ingest_snappy.hip: snappy sections (codec 2; the format: snappy_block.h) ------------------------------------------------------
// A section's chunks in a plan and a block table of their own, in the LZ4 stage's shapes: Lz4Block::index holds the chunk's
// output offset inside its section in units of 16 bytes (every chunk but a section's last is a multiple of 16 long, so chunk
// k's output lies right behind chunk k - 1's and every destination is 16-byte aligned), src_off / src_len name the raw block
// with its preamble, seq_off its room in the entry table (a copy takes at least 2 bytes: src_len / 2 + 2 entries).
// plans the section [sec, sec + len) staged at src_off; LZ4_ON_HOST: a chunk above 64 KiB, a chunk but the last off the 16-byte
// grid or a chunk longer than the parse kernel's LDS holds — decompressed here and appended to host_out; *why: the refusal's
// text for LZ4_BAD_FRAME
Lz4Route snappy_plan_section(Lz4Plan& plan, const uint8_t* sec, int64_t len, int64_t src_off, int32_t section, int64_t* area_off, std::vector<uint8_t>& host_out,
                             const char** why);
// parses the plan's chunks (snappy_parse_kernel: literals stored in place, one entry per copy), then applies the copies with the
// LZ4 stage's second pass; a section's last chunk sets its byte_len, a chunk that does not decode lowers err->snappy_bad
hipError_t launch_snappy(const Lz4Plan& plan, const uint8_t* bytes, uint8_t* area, const Lz4Block* d_blocks, Lz4Work w, Section* sections, ErrorCell* err, hipStream_t st);

// ---- ingest_records.hip: meta / ev_tmp / f64_host_list per record ---------------------------------------------------------------
// one workgroup per section, as wide as max_recs (the push's largest batch) needs; floors (nullable; events mode only): per section
// the offset below which its records are passed over, INT64_MIN for none
hipError_t launch_sections(const uint8_t* bytes, const Section* sections, int64_t n_sections, int32_t max_recs, uint64_t seed, JsonCtx jc, RecMeta* meta,
                           uint4* ev_tmp, uint32_t* f64_host_list, ErrorCell* err, const int64_t* floors, hipStream_t st);
// records that arrive already framed: the bytes hold the keys first, the values from val_base on
hipError_t launch_records(const uint8_t* bytes, const int64_t* key_off, const int64_t* val_off, const int64_t* offsets, int64_t val_base, int64_t n_rec,
                          uint64_t seed, JsonCtx jc, RecMeta* meta, uint4* ev_tmp, uint32_t* f64_host_list, ErrorCell* err, hipStream_t st);

// ---- ingest_intern.hip -------------------------------------------------------------------------------------------------------
hipError_t intern_temp_bytes(int64_t n_rec, size_t* bytes, hipStream_t st);  // of InternScratch::temp
void launch_table_build(const KeyTable& k, hipStream_t st);                  // a fresh table: every slot empty, then the known keys by their hashes
void launch_rekey_records(RecMeta* meta, int64_t n_rec, const uint8_t* bytes, uint64_t seed, hipStream_t st);  // the table was re-seeded after stage 1 hashed the keys
// probe + flag + the two scans: afterwards first_scan[n_rec] = new keys << 40 | their bytes, keep_pos[n_rec] = records delivered
hipError_t launch_intern_probe(RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const KeyTable& k, const InternScratch& sc, ErrorCell* err, hipStream_t st);
// a detected collision: the push's slots out, every known key and every record of the push re-hashed under `seed`, the table rebuilt
void launch_intern_reseed(RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const KeyTable& k, uint64_t seed, hipStream_t st);
// the commit: the n_new keys the push discovered get their ids and arena bytes, the delivered records go to the result arrays
void launch_intern_commit(const RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const KeyTable& k, const InternScratch& sc, int64_t n_new,
                          const uint4* ev_tmp, int64_t out_base, int64_t* agg_out, uint4* ev_out, int64_t* off_out, hipStream_t st);
void launch_intern_rollback(const RecMeta* meta, int64_t n_rec, const Table& t, hipStream_t st);  // a failed push takes the keys it probed out again
// read-only, no push in flight: idx_out[i] = the dense index of the id ids[id_off[i] .. id_off[i + 1]), compared byte for byte, or -1;
// `ids` must be readable 16 bytes behind its last id, as the arena is (keys_equal's loads)
hipError_t launch_lookup(const uint8_t* ids, const int64_t* id_off, int64_t n, const KeyTable& k, uint64_t seed, int64_t* idx_out, hipStream_t st);

// ---- ingest_order.hip: the key table in key order (unsigned bytes, a proper prefix first), and what reads through it ---------
constexpr int64_t kOrderMaxKeys = 1ll << 29;  // a pass sorts (group << 35 | chunk << 3 | bytes left) as one 64-bit key: 29 bits of group
struct OrderScratch {  // per build, n_keys entries each; freed behind it
  unsigned long long *key_in, *key_out;
  uint32_t *idx_in, *idx_out;  // (launch_order_pass swaps them: idx_in is always what the last pass sorted)
  uint32_t *grp, *flag;
  uint32_t* live;  // one word: did a key have a byte in the last pass
  void* temp;
  size_t temp_bytes;
};
hipError_t order_temp_bytes(int64_t n_keys, size_t* bytes, hipStream_t st);  // of OrderScratch::temp
hipError_t launch_order_init(const OrderScratch& sc, int64_t n_keys, hipStream_t st);  // idx_in = 0, 1, 2, ...; one group
// pass p: stable sort by (group, bytes [4p, 4p + 4) big-endian, bytes left clipped to 0..4) over 35 + group_bits bits, groups re-numbered:
// afterwards grp[n_keys - 1] + 1 = groups, *live = a key had a byte
hipError_t launch_order_pass(const KeyTable& k, int64_t pass, int group_bits, OrderScratch& sc, hipStream_t st);
hipError_t launch_order_finish(const OrderScratch& sc, int64_t n_keys, int64_t* ord, hipStream_t st);
// lo_hi[0] = lower_bound(from), lo_hi[1] = upper_bound(to) over ord; the bounds' bytes are bounds[0 .. from_len) and
// bounds[to_at .. to_at + to_len), each readable 16 bytes behind its end; a negative length: no bound (0 / n_keys)
hipError_t launch_order_bounds(const KeyTable& k, const int64_t* ord, const uint8_t* bounds, int64_t from_len, int64_t to_at, int64_t to_len, int64_t* lo_hi, hipStream_t st);
struct KeyGatherScratch {  // (n + 1) entries each
  unsigned long long *len, *at;
  uint32_t* bad;  // one word: a row outside [0, n_keys)
  void* temp;
  size_t temp_bytes;
};
hipError_t key_gather_temp_bytes(int64_t n, size_t* bytes, hipStream_t st);
// at[q] = bytes of the ids in front of rows[q] (at[n]: of all of them), *bad; nothing of the caller's is written
hipError_t launch_key_lengths(const KeyTable& k, const int64_t* rows, int64_t n, const KeyGatherScratch& sc, hipStream_t st);
// behind the checks: off_out[0 .. n] = at, the ids' bytes to out
hipError_t launch_key_gather(const KeyTable& k, const int64_t* rows, int64_t n, const KeyGatherScratch& sc, uint8_t* out, int64_t* off_out, hipStream_t st);

// ---- state mode (ingest_intern.hip): the kept records' VALUES move out of the push's staged bytes -------------------------------
constexpr int kGatherRecs = 256;          // kept records per workgroup of the value gather
constexpr int64_t kGatherOwn = 64 << 10;  // bytes of its run's span a workgroup copies itself; what lies beyond is split over a second, grid-wide launch
struct StateScratch {  // per push: vlen / vscan (n_rec + 1) entries, val_src one per delivered record, long_runs 1 + one per workgroup of the gather
  unsigned long long *vlen, *vscan;
  int64_t* val_src;
  uint32_t* long_runs;  // [0] = how many runs are listed behind it
};
// behind launch_intern_probe: vscan[i] = value bytes of the delivered records in front of record i (vscan[n_rec]: of all of them)
hipError_t launch_value_scan(const RecMeta* meta, int64_t n_rec, const InternScratch& sc, const StateScratch& ss, hipStream_t st);
// behind launch_intern_commit: value_off[out_base + k] (and the closing entry) = val_base + ..., the values' bytes to values[val_base ..)
hipError_t launch_value_gather(const RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const InternScratch& sc, const StateScratch& ss, int64_t kept, int64_t out_base,
                               int64_t val_base, int64_t* value_off, uint8_t* values, hipStream_t st);

// ---- ingest_strings.hip: the string fields of events (surge_device_decoder_keep_event_strings), behind a push's interning ------
struct EvsTypes {  // the surge_event16.type values of the classes that name a string column
  uint32_t n;
  uint32_t type[SURGE_EVJ_MAX_TYPES];
};
struct StringsCell {  // where a push's finish reads what the select found
  uint32_t n_sel, pad;
};
struct StringsSelect {  // per push: seg holds kStringsBlock entries per block of records, block_count / block_base one each
  uint32_t *seg, *block_count, *block_base;
  StringsCell* cell;
};
constexpr int kStringsBlock = 256;
// What a decoder keeps until the columns are merged: the selected records of every push since, in push order.  Record q's
// value is values[off[q] .. off[q + 1]), its aggregate rows[q], its spans spans[q * 2 * SURGE_JSON_STRING_COLUMNS ..), its
// status for column c status[c][q].
struct StringsPending {
  uint8_t* values;
  int64_t *off, *rows, *spans;
  uint8_t* status[4];
  int64_t n, bytes;
};
// select: one lane per record; the kept records (keep[i], behind launch_intern_probe) whose event type is one of `types`, compacted
// per block of kStringsBlock records in record order; cell->n_sel += their count (the caller zeroes the cell)
hipError_t launch_strings_select(const uint32_t* keep, const uint4* ev_tmp, int64_t n_rec, const EvsTypes& types, const StringsSelect& s, hipStream_t st);
// behind the wait that brought n_sel back (> 0): sel[0 .. n_sel) = the selected records in record order, lens[k] = record sel[k]'s value length
hipError_t launch_strings_list(const RecMeta* meta, int64_t n_rec, const StringsSelect& s, uint32_t* sel, int64_t* lens, hipStream_t st);
// spans: one lane per selected record walks its value where stage 1 left it (event_strings_parse.h; `rule`: a device EvsRule) and
// writes spans and statuses at pending entry p.n + k; a refusal is reported as RS_STRING
hipError_t launch_strings_spans(const void* rule, const RecMeta* meta, const uint8_t* bytes, const uint32_t* sel, int64_t n_sel, const StringsPending& p, ErrorCell* err,
                                hipStream_t st);
// gather, behind launch_intern_commit and the scan of lens: the selected records' values to p.values[p.bytes ..), their offsets
// (and the closing one, p.bytes + total) and rows (agg[keep_pos[record]]: the push's part of the result) to entries p.n ..
hipError_t launch_strings_gather(const RecMeta* meta, const uint8_t* bytes, const uint32_t* sel, const int64_t* lens, int64_t n_sel, int64_t total, const uint32_t* keep_pos,
                                 const int64_t* agg, const StringsPending& p, hipStream_t st);
// lens[0 .. n) scanned in place (exclusive; state_kernels.hip's scan); totals: ceil(n / 1024) + 1 entries, the sum lands in the last
hipError_t launch_strings_scan(int64_t* lens, int64_t n, int64_t* totals, hipStream_t st);
// One column of the merge over what is pending (state_strings.hip's kernels; the highest pending record with status OK wins, an
// aggregate without one keeps prev's string, a new one is empty): out_off gets n_agg + 1 offsets, out the bytes, *total_out their
// sum.  win1: n_agg u64 of scratch, bad: one u64, totals: ceil(n_agg / 1024) + 1 i64.  Waits for the stream (the total sizes
// nothing here — out holds prev's bytes + the pending values' — but the closing offset is the host's to write).
struct StringsColumn {
  const uint8_t* prev;
  const int64_t* prev_off;
  int64_t n_prev;
  uint8_t* out;
  int64_t* out_off;
};
hipError_t strings_merge_column(const StringsPending& p, int column, int64_t n_agg, const StringsColumn& col, unsigned long long* win1, unsigned long long* bad, int64_t* totals,
                                int64_t* total_out, hipStream_t st);

}  // namespace ingest
}  // namespace surge
