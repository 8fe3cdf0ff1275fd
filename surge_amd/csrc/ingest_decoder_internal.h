// ingest_decoder_internal.h — what the units of the device decoder's host object share (ingest_decoder.hip: lifecycle,
// slot queue, the push exports; ingest_stage1.hip; ingest_stage2.hip; ingest_reads.hip: the key table's reads between pushes;
// ingest_columns.hip: the kept string columns; ingest_handover.hip: the hand-overs to a replay handle): the object itself —
// every feature's state in a member struct that names the unit it belongs to — device memory, error reporting, the refusals
// every export words alike and the few helpers that cross units.  Host only and internal, like engine_internal.h: not part
// of the C ABI (that is include/surge_ingest.h).  The kernels and what launches them know none of this (ingest_device.h).
#pragma once

#include <sys/prctl.h>
#include <time.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/surge_ingest.h"
#include "../../include/surge_replay.h"
#include "ingest_device.h"

namespace surge {
namespace ingest {
namespace host __attribute__((visibility("hidden"))) {

constexpr int32_t OK = 0, E_INVALID = -1, E_DEVICE = -3, E_NOMEM = -4, E_UNSUPPORTED = -5;

struct Buf {  // device memory, owned: freed with the buffer, which must happen while its device is current (surge_device_decoder_destroy)
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~Buf() { release(); }
  hipError_t reserve(size_t bytes, bool keep, hipStream_t stream) {
    if (bytes <= cap) return hipSuccess;
    // room to spare: a fetch is a few per cent larger or smaller than the one before it, and a buffer that grows is freed —
    // hipFree waits for the whole device (1 - 3 ms with four pushes in flight: the spikes of round 4's per-fetch times)
    const size_t roomy = bytes + bytes / 4 + 4096;
    size_t want = cap * 2 > roomy ? cap * 2 : roomy;
    void* fresh = nullptr;
    hipError_t e = hipMalloc(&fresh, want);
    if (e != hipSuccess) return e;
    if (keep && p && cap) {
      e = hipMemcpyAsync(fresh, p, cap, hipMemcpyDeviceToDevice, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) { (void)hipFree(fresh); return e; }
    }
    if (p) (void)hipFree(p);
    p = fresh;
    cap = want;
    return hipSuccess;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Everything one push needs until it is finished.  A push has two halves: stage 1 does not touch the key table — copy to
// the device, LZ4, chain / parse / decode — and runs on the slot's own stream; stage 2 — interning, compaction, append —
// runs on the decoder's stream, one push after the other.  With several slots the host enqueues stage 1 of the next
// fetches (surge_device_decoder_push_async) while stage 2 and the fold of the current one run: the copy engine, the
// latency-bound LZ4 kernels and the compute-bound decode of different fetches overlap on the chip.
struct PushSlot {
  Buf lz4_blocks, lz4_sizes, lz4_nseq, lz4_seq, lz4_cls;
  Buf sn_blocks, sn_sizes, sn_nseq, sn_seq, sn_cls;  // the same five for the snappy chunks (ingest_snappy.hip)
  Buf d_bytes, d_sections, rec_a, rec_b, rec_c, meta, ev_tmp, f64_list, d_err;
  void* pinned = nullptr;  // page-locked staging, the slot's own (slot_pinned)
  size_t pinned_cap = 0;
  std::vector<Section> h_secs;      // (sources of asynchronous copies: they live as long as the slot is busy)
  Lz4Plan lz4;                      // the LZ4 frames' blocks (ingest_lz4.hip plans them)
  Lz4Plan snappy;                   // the snappy sections' chunks, in the same shapes (ingest_snappy.hip plans them)
  int64_t snappy_host_sections = 0; // ... and the sections of this push it decompressed on the host instead
  std::vector<CrcSpan> h_crc;       // sections whose CRC-32C this push finishes on the device
  Buf crc_spans;
  std::vector<int64_t> h_floors;    // per section the offset its records must reach (INT64_MIN: none); empty: a push without floors
  Buf d_floors;
  ErrorCell h_err;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;      // recorded on `stream` behind stage 1
  hipEvent_t released = nullptr;  // recorded on the decoder's stream behind stage 2: the slot's buffers may be written again
  bool released_valid = false;
  int64_t n_rec = 0;
  uint64_t seed = 0;   // the hash function stage 1 hashed the keys with
  bool busy = false, wire = false;
  ~PushSlot() { if (pinned) (void)hipHostFree(pinned); }
};
constexpr int kSlots = 5;

// ---- ingest_reads.hip: what the reads of the key table between pushes keep ---------------------------------------------------
struct ReadsState {
  struct Lookup { Buf ids, off, idx; } lookup;  // surge_device_decoder_lookup: the staged queries and their indices
  // the key order (ingest_order.hip): valid while keys == n_keys — a push that interns an id leaves it stale, the next read
  // rebuilds it whole; clear and a re-seed do not touch the keys' bytes, so they do not touch it
  struct Order {
    Buf idx;  // n_keys dense indices in key order
    int64_t keys = -1, passes = 0;
  } order;
  struct Range { Buf bounds, lo_hi; } range;      // surge_device_decoder_range_device: the staged bounds and their two positions
  struct Gather { Buf len, at, bad, temp; } gather;  // surge_device_decoder_gather_keys_device: lengths, their scan, the bad-row word
};

// ---- ingest_columns.hip: the kept string columns, a state decoder's (surge_device_decoder_keep_strings) and an events ---------
// decoder's (surge_device_decoder_keep_event_strings) alike
// One STR column: two buffers of bytes and of offsets, of which `cur` holds the column (-1: nothing has named it).  The rule
// of a merge, written once: it reads buffer cur and writes the OTHER one, which has n_keys + 1 offsets and room for the bytes
// of the column so far plus those that come in (an unescaped string is never longer than its span, and the spans lie inside
// the incoming values: the merge always fits) and 16 of slack; then the column flips to what was written.
struct StrColumn {
  Buf utf8[2], off[2];
  int cur = -1;
  int64_t n = 0, bytes = 0;
  int next() const { return cur < 0 ? 0 : 1 - cur; }
  int64_t next_capacity(int64_t incoming) const { return bytes + incoming + 16; }
  hipError_t reserve_next(int64_t n_keys, int64_t incoming, hipStream_t st) {
    const hipError_t e = off[next()].reserve((size_t)(n_keys + 1) * 8, false, st);
    return e != hipSuccess ? e : utf8[next()].reserve((size_t)next_capacity(incoming), false, st);
  }
  void flip(int64_t n_keys, int64_t total) {
    cur = next();
    n = n_keys;
    bytes = total;
  }
  const uint8_t* cur_utf8() const { return cur < 0 ? nullptr : (const uint8_t*)utf8[cur].p; }
  const int64_t* cur_off() const { return cur < 0 ? nullptr : (const int64_t*)off[cur].p; }
  int64_t cur_n() const { return cur < 0 ? 0 : n; }
};

// Events mode (ingest_strings.hip has the kernels; stage 2 selects, validates and gathers, ingest_columns.hip arms and merges):
// the rule on the device, the event types that select a record and the columns the rule names; a push's select / list / spans
// scratch; the selected records of the pushes since the last merge (values, n + 1 offsets, rows, spans, a status array per
// column), merged into the columns when they are asked for or more than `bound` records are pending; the merge's scratch
struct EventStringsState {
  bool armed = false;
  EvsTypes types{};
  bool named[SURGE_JSON_STRING_COLUMNS] = {};
  Buf rule;
  struct Select { Buf seg, count, base, cell, sel, lens, totals; } select;
  struct Pending {
    Buf val, off, rows, spans, status[SURGE_JSON_STRING_COLUMNS];
    int64_t n = 0, bytes = 0, bound = 1 << 20;
  } pend;
  struct Merge {
    Buf win, bad, totals;
    int64_t count = 0;  // merges that had records pending
  } merge;
  void drop_pending() { pend.n = pend.bytes = 0; }  // (what is pending and not merged goes with the records: clear)
  StringsPending pending() const {
    StringsPending p{(uint8_t*)pend.val.p, (int64_t*)pend.off.p, (int64_t*)pend.rows.p, (int64_t*)pend.spans.p, {}, pend.n, pend.bytes};
    for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) p.status[c] = (uint8_t*)pend.status[c].p;
    return p;
  }
};

struct StringsState {
  StrColumn col[SURGE_JSON_STRING_COLUMNS];
  EventStringsState ev;
};

}  // namespace host
}  // namespace ingest
}  // namespace surge

struct surge_device_decoder {
  using Buf = surge::ingest::host::Buf;
  using PushSlot = surge::ingest::host::PushSlot;
  static constexpr int kSlots = surge::ingest::host::kSlots;
  int device = 0;
  hipStream_t stream = nullptr;
  bool json = false;
  bool states = false;  // state mode (surge_device_decoder_create_states): values are kept (r_val / r_val_off), not decoded into events
  bool continued = false;  // was a state decoder (surge_device_decoder_continue_as_events): its key table and kept string columns are that decoder's
  // state mode, set by ingest_columns.hip (surge_device_decoder_keep_strings) and read by ingest_handover.hip's loads: every load
  // asks the decode for the string spans (st_spans) and has ingest_columns.hip merge the STR columns its template names into strings.col
  bool keep_strings = false;
  // Two host threads may drive one decoder: one enqueues stage 1 (push_async / push_parts_async), the other finishes pushes
  // (push_finish*, result, clear, append_decoded*).  `mu` covers what both touch: the slot queue and the error text.
  std::mutex mu;
  std::atomic<bool> poisoned{false};  // a device error left the tables in an unknown state: every later push is refused
  std::string err;
  Buf d_tmpl, d_ptab;
  surge_event_json_template h_tmpl;  // (host copy: Doubles the device cannot decide are re-parsed with it)
  PushSlot slots[kSlots];
  // Stage 1 streams.  Consecutive pushes take consecutive streams (PushSlot::stream is set when a push claims its slot): with four
  // pushes in flight three are in stage 1 at any time, so THREE streams are all the concurrency there is — and with the
  // stream stage 2 and the fold run on that makes four, the number of hardware queues the HIP runtime creates by default
  // (GPU_MAX_HW_QUEUES).  Round 4 gave each of the five slots a stream of its own: the fifth and sixth stream of the process
  // shared a hardware queue with another one, and every fifth fetch waited for a neighbour's stage 1 in front of its stage 2
  // (profiles/r05_e2e_k512_per_fetch_trace.txt: finish 1.1 - 1.5 ms instead of 0.4 on fetches 8, 13, 18, 23, 28).
  hipStream_t push_streams[kSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int n_push_streams = 0;
  int n_push_active = 0;       // of them in rotation (<= n_push_streams): one fewer once a consumer folds on a stream of its own (hardware queues, below)
  bool push_streams_pinned = false;  // SURGE_INGEST_PUSH_STREAMS said how many: never adjusted
  uint64_t push_seq = 0;
  int head = 0;
  std::atomic<int> n_pending{0};  // slots [head, head + n_pending) hold pushes whose stage 1 is enqueued (changes under `mu`)
  // stage 2 scratch
  Buf first, first_scan, keep, keep_pos, temp;
  Buf vlen, vscan, val_src, long_runs;  // state mode: the value scan and gather's scratch
  Buf st_status, st_spans;              // ... load_states' per-record statuses and, with keep_strings, the decode's string spans
  // hash table + key table
  Buf t_slots, arena, key_off, key_hash;
  uint64_t t_cap = 0;
  std::atomic<uint64_t> seed{0};  // (stage 1 reads it once per push; stage 2 of an earlier push may move it on: PushSlot::seed)
  int64_t n_keys = 0, arena_bytes = 0;
  // result
  Buf r_agg, r_ev, r_off;
  Buf r_val, r_val_off;   // state mode: the delivered records' value bytes, one after the other, and n_records + 1 offsets into them
  int64_t val_bytes = 0;  // ... bytes of r_val in use
  int64_t n_records = 0;
  int64_t state_loads = 0;  // state mode: loads so far (counted by ingest_handover.hip; ingest_columns.hip refuses keep_strings behind the first)
  uint64_t events_from_push = 0;  // push_seq when the decoder became an events decoder: arming kept event strings comes before the push behind it
  surge::ingest::host::ReadsState reads;      // ingest_reads.hip
  surge::ingest::host::StringsState strings;  // ingest_columns.hip (stage 2 fills strings.ev.pend; a state decoder's loads merge into strings.col)
  // hand-over of the result arrays to a consumer on another stream (surge_replay_append_decoded_async): `consumed` is
  // recorded on the consumer's stream behind its last read, the next stage 2 waits for it before it writes the arrays
  hipEvent_t ready = nullptr, consumed = nullptr;
  hipEvent_t sleeper = nullptr;  // hipEventBlockingSync: host waits of the consumer thread sleep on it instead of spinning
  bool block_waits = true;
  int64_t poll_ns = 0;  // > 0 (SURGE_INGEST_WAIT=poll): the waits query the event between naps of this length instead
  bool consumed_valid = false;
  int64_t counters[4] = {0, 0, 0, 0};  // records seen, delivered, flush records skipped, f64 values re-parsed on the host
  int64_t below_floor = 0;             // records passed over below their section's floor (surge_device_decoder_below_floor)
  int64_t chain_fallbacks = 0;         // batches whose records the one-lane walk chained after the parallel recognition declined (SURGE_EXPERIMENTS builds print it)
  int64_t reseeds = 0, pushes = 0;
  int64_t snappy_device_chunks = 0, snappy_host_sections = 0;  // of the pushes that delivered (surge_device_decoder_route_stats)
  bool slots_sized = false;  // the first wire push has sized every slot's buffers like its own
};

namespace surge {
namespace ingest {
namespace host __attribute__((visibility("hidden"))) {

inline thread_local std::string g_dec_err;

inline int32_t dfail(surge_device_decoder* d, int32_t code, const std::string& m) {
  if (d) {
    std::lock_guard<std::mutex> lk(d->mu);
    d->err = m;
  }
  g_dec_err = m;
  return code;
}

// The refusals most exports share, each worded in one place.  What is pending is refused with one of four endings: none
// (reserve), and the three below.
inline int32_t refuse_null_decoder() { return dfail(nullptr, E_INVALID, "decoder is NULL"); }
inline int32_t refuse_poisoned(surge_device_decoder* d) {
  return dfail(d, SURGE_E_STATE, "an earlier push failed on the device half way: destroy this decoder and create a new one");
}
constexpr const char* kPushOrder = ": finish them first (results are appended in push order)";
constexpr const char* kNoIdsYet = ": finish them first (their keys have no ids yet)";
constexpr const char* kFinishAndLoad = ": finish and load them first";
inline int32_t refuse_pending(surge_device_decoder* d, const char* ending = "") {
  return dfail(d, SURGE_E_STATE, std::string("asynchronous pushes are pending") + ending);
}

#define DCHK(d, call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return dfail(d, e_ == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ... behind the point where a push may have left its mark on the tables (stage 2 from its first launch on): the failure
// also poisons the decoder
inline int32_t poison(surge_device_decoder* d, int32_t rc) { d->poisoned = true; return rc; }
#define PCHK(d, call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return poison(d, dfail(d, e_ == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_))); \
  } while (0)

struct DeviceScope {  // the calling thread's device, restored on the way out
  int prev = 0;
  explicit DeviceScope(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
  ~DeviceScope() { (void)hipSetDevice(prev); }
};

inline KeyTable keys_of(surge_device_decoder* d) {
  return KeyTable{Table{(TableSlot*)d->t_slots.p, d->t_cap - 1}, (uint8_t*)d->arena.p, (int64_t*)d->key_off.p, (unsigned long long*)d->key_hash.p, d->n_keys, d->arena_bytes};
}

// capacity for n_keys + extra more keys at a load factor of at most 1/2 (rebuilt from the key hashes when it grows)
inline int32_t ensure_table(surge_device_decoder* d, int64_t extra) {
  uint64_t need = 1024;
  while (need < (uint64_t)(d->n_keys + extra) * 2) need *= 2;
  if (need <= d->t_cap) return OK;
  if (need > (1ull << 32)) return dfail(d, E_UNSUPPORTED, "more than 2^31 aggregate ids");
  Buf fresh;
  DCHK(d, fresh.reserve(need * sizeof(TableSlot), false, d->stream));
  d->t_slots = std::move(fresh);
  d->t_cap = need;
  launch_table_build(keys_of(d), d->stream);
  DCHK(d, hipGetLastError());
  return OK;
}

// the consumer thread's wait for `st`: naps between event queries (read_options; SURGE_INGEST_WAIT=block: asleep on
// the blocking event, =spin: hipStreamSynchronize)
inline hipError_t wait_stream(surge_device_decoder* d, hipStream_t st) {
  if (!d->block_waits) return hipStreamSynchronize(st);
  hipError_t e = hipEventRecord(d->sleeper, st);
  if (e != hipSuccess || d->poll_ns <= 0) return e != hipSuccess ? e : hipEventSynchronize(d->sleeper);
  // naps of poll_ns between queries; the thread's timer slack (50 us by default: it would triple a 25 us nap) is 1 us meanwhile
  const int slack = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
  if (slack > 1000) (void)prctl(PR_SET_TIMERSLACK, 1000ul, 0, 0, 0);
  const timespec nap{0, (long)d->poll_ns};
  while ((e = hipEventQuery(d->sleeper)) == hipErrorNotReady) (void)nanosleep(&nap, nullptr);
  (void)hipGetLastError();  // (hipErrorNotReady is remembered as the thread's last error: not one)
  if (slack > 1000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)slack, 0, 0, 0);
  return e;
}

// ---- ingest_stage1.hip: nothing here reads or writes the key table; everything is enqueued on the slot's stream ------------
int32_t stage1_wire(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                    const int64_t* n_sections, int64_t n_floors, const surge_section_floor* floors);
int32_t stage1_records(surge_device_decoder* d, PushSlot& s, const uint8_t* keys, const int64_t* key_off, const uint8_t* values, const int64_t* value_off,
                       const int64_t* offsets, int64_t n);
// ---- ingest_stage2.hip: interning, compaction, append on the decoder's stream; wait = false leaves the closing wait out -----
int32_t stage2(surge_device_decoder* d, PushSlot& s, bool wait);
// ---- ingest_columns.hip: what is pending of the kept event strings merged into the columns, every column brought to n_keys;
// and a state load's strings (the decode's spans in st_spans) merged into the columns its template names
int32_t merge_event_strings(surge_device_decoder* d);
int32_t merge_state_strings(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl);

}  // namespace host
}  // namespace ingest
}  // namespace surge
