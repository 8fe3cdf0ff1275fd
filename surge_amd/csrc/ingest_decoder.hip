// ingest_decoder.hip — SURVEY §8f N1 on the device: the records sections of Kafka record batches (message format v2,
// uncompressed or already decompressed by the host framer) -> (aggregate index, 16-byte event, offset) arrays and a key
// table, all resident in HBM, ready for surge_replay_append_events_device / a CSR build.  This unit is the host object
// (surge_device_decoder): the push slots, stage 1 and stage 2, the slot queue, the wait modes and the extern "C" exports.  The
// kernels and what launches them are the stage units ingest_crc / ingest_lz4 / ingest_records / ingest_intern .hip
// (ingest_device.h).
//
// Split of the work (include/surge_ingest.h, "device decode"): the HOST walks the 61-byte batch headers, verifies the
// CRC-32C (one instruction stream per partition thread), applies read_committed and undoes LZ4 — sequential, cheap per
// byte — and hands over the records sections as they are.  The DEVICE does everything that is per record: chains the
// varint-framed records of every batch, parses keys / values, interns the aggregate ids (key up to ':') in a hash table,
// decodes the event values (16-byte events as they are, or the reference's play-json text through the event template,
// surge_amd/csrc/event_decode.cpp's rules) and compacts away the producer's flush records.  The host decoder spends
// ≈ 90 ns (fixed-16) / 640 ns (JSON) per record and thread on exactly these steps.
// State mode (surge_device_decoder_create_states) reads the compacted STATE topic with the same stages: the id is the whole key,
// a null value is a delivered tombstone, no value is decoded — stage 2 gathers the delivered records' value bytes into one
// buffer behind value_off, and surge_device_decoder_load_states hands them to surge_replay_decode_json_states.
#include <sys/prctl.h>
#include <time.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/surge_ingest.h"
#include "../../include/surge_replay.h"
#include "ingest_device.h"

using namespace surge::ingest;

namespace {

constexpr int32_t OK = 0, E_INVALID = -1, E_DEVICE = -3, E_NOMEM = -4, E_UNSUPPORTED = -5;

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
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

thread_local std::string g_dec_err;

// Everything one push needs until it is finished.  A push has two halves: stage 1 does not touch the key table — copy to
// the device, LZ4, chain / parse / decode — and runs on the slot's own stream; stage 2 — interning, compaction, append —
// runs on the decoder's stream, one push after the other.  With several slots the host enqueues stage 1 of the next
// fetches (surge_device_decoder_push_async) while stage 2 and the fold of the current one run: the copy engine, the
// latency-bound LZ4 kernels and the compute-bound decode of different fetches overlap on the chip.
struct PushSlot {
  Buf lz4_blocks, lz4_sizes, lz4_nseq, lz4_seq, lz4_cls;
  Buf d_bytes, d_sections, rec_a, rec_b, rec_c, meta, ev_tmp, f64_list, d_err;
  void* pinned = nullptr;
  size_t pinned_cap = 0;
  std::vector<Section> h_secs;      // (sources of asynchronous copies: they live as long as the slot is busy)
  Lz4Plan lz4;                      // the LZ4 frames' blocks (ingest_lz4.hip plans them)
  std::vector<CrcSpan> h_crc;       // sections whose CRC-32C this push finishes on the device
  Buf crc_spans;
  ErrorCell h_err;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;      // recorded on `stream` behind stage 1
  hipEvent_t released = nullptr;  // recorded on the decoder's stream behind stage 2: the slot's buffers may be written again
  bool released_valid = false;
  int64_t n_rec = 0;
  uint64_t seed = 0;   // the hash function stage 1 hashed the keys with
  bool busy = false, wire = false;
};
constexpr int kSlots = 5;

}  // namespace

struct surge_device_decoder {
  int device = 0;
  hipStream_t stream = nullptr;
  bool json = false;
  bool states = false;  // state mode (surge_device_decoder_create_states): values are kept (r_val / r_val_off), not decoded into events
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
  Buf vlen, vscan, val_src, long_runs, st_status;  // state mode: the value scan and gather's scratch; load_states' per-record statuses
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
  // state mode, surge_device_decoder_keep_strings: the STR columns of the loaded states (surge_replay_merge_state_strings
  // writes buffer 1 - cur from buffer cur), and the decode's spans
  struct StrColumn {
    Buf utf8[2], off[2];
    int cur = -1;  // -1: no load has named the column
    int64_t n = 0, bytes = 0;
  };
  StrColumn str_cols[SURGE_JSON_STRING_COLUMNS];
  Buf st_spans;
  bool keep_strings = false;
  int64_t state_loads = 0;
  // hand-over of the result arrays to a consumer on another stream (surge_replay_append_decoded_async): `consumed` is
  // recorded on the consumer's stream behind its last read, the next stage 2 waits for it before it writes the arrays
  hipEvent_t ready = nullptr, consumed = nullptr;
  hipEvent_t sleeper = nullptr;  // hipEventBlockingSync: host waits of the consumer thread sleep on it instead of spinning
  bool block_waits = true;
  int64_t poll_ns = 0;  // > 0 (SURGE_INGEST_WAIT=poll): the waits query the event between naps of this length instead
  bool consumed_valid = false;
  int64_t counters[4] = {0, 0, 0, 0};  // records seen, delivered, flush records skipped, f64 values re-parsed on the host
  int64_t chain_fallbacks = 0;         // batches whose records the one-lane walk chained after the parallel recognition declined (SURGE_EXPERIMENTS builds print it)
  int64_t reseeds = 0, pushes = 0;
  bool slots_sized = false;  // the first wire push has sized every slot's buffers like its own
};

namespace {

int32_t dfail(surge_device_decoder* d, int32_t code, const std::string& m) {
  if (d) {
    std::lock_guard<std::mutex> lk(d->mu);
    d->err = m;
  }
  g_dec_err = m;
  return code;
}

#define DCHK(d, call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return dfail(d, e_ == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

KeyTable keys_of(surge_device_decoder* d) {
  return KeyTable{Table{(TableSlot*)d->t_slots.p, d->t_cap - 1}, (uint8_t*)d->arena.p, (int64_t*)d->key_off.p, (unsigned long long*)d->key_hash.p, d->n_keys, d->arena_bytes};
}

// capacity for n_keys + extra more keys at a load factor of at most 1/2 (rebuilt from the key hashes when it grows)
int32_t ensure_table(surge_device_decoder* d, int64_t extra) {
  uint64_t need = 1024;
  while (need < (uint64_t)(d->n_keys + extra) * 2) need *= 2;
  if (need <= d->t_cap) return OK;
  if (need > (1ull << 32)) return dfail(d, E_UNSUPPORTED, "more than 2^31 aggregate ids");
  Buf fresh;
  DCHK(d, fresh.reserve(need * sizeof(TableSlot), false, d->stream));
  d->t_slots.release();
  d->t_slots = fresh;
  d->t_cap = need;
  launch_table_build(keys_of(d), d->stream);
  DCHK(d, hipGetLastError());
  return OK;
}

}  // namespace

extern "C" {

static void* pinned_alloc(size_t n) {
  void* p = nullptr;
  return hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
static void pinned_release(void* p) { (void)hipHostFree(p); }

int32_t surge_ingest_use_pinned_arena(surge_ingest* g) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return dfail(nullptr, E_DEVICE, "no usable HIP device: the arena stays in pageable memory");
  return surge_ingest_set_allocator(g, pinned_alloc, pinned_release);
}

int32_t surge_ingest_group_use_pinned_slabs(surge_ingest_group* g) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return dfail(nullptr, E_DEVICE, "no usable HIP device: the slabs stay in pageable memory");
  return surge_ingest_group_set_allocator(g, pinned_alloc, pinned_release);
}

const char* surge_device_decoder_last_error(const surge_device_decoder* d) {
  if (d) {  // (a copy: the other thread of a two-thread host may be setting its own error text)
    std::lock_guard<std::mutex> lk(const_cast<surge_device_decoder*>(d)->mu);
    g_dec_err = d->err;
  }
  return g_dec_err.c_str();
}

static int32_t decoder_create(int32_t device_id, void* hip_stream, const surge_event_json_template* tmpl, bool states, surge_device_decoder** out) {
  if (!out) return dfail(nullptr, E_INVALID, "out is NULL");
  *out = nullptr;
  if (tmpl && surge_event_json_validate(tmpl) != 0) return dfail(nullptr, E_INVALID, std::string("event template: ") + surge_event_json_last_error());
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return dfail(nullptr, E_DEVICE, "no usable HIP device (the device decoder has no CPU fallback: use surge_ingest_drain_*)");
  if (device_id < 0 || device_id >= n_dev) return dfail(nullptr, E_INVALID, "device_id out of range");
  surge_device_decoder* d = new (std::nothrow) surge_device_decoder();
  if (!d) return dfail(nullptr, E_NOMEM, "out of host memory");
  d->device = device_id;
  d->stream = (hipStream_t)hip_stream;
  d->json = tmpl != nullptr;
  d->states = states;
  if (const char* v = std::getenv("SURGE_INGEST_DEBUG_WEAK_HASH"))
    if (v[0] == '1') d->seed = 1ull << 63;  // test hook: the table's first hash function keeps 8 bits, so keys collide and the re-seed runs
  int prev = 0;
  (void)hipGetDevice(&prev);
  int32_t rc = OK;
  auto init = [&]() -> int32_t {
    DCHK(d, hipSetDevice(device_id));
    {
      // Stage 1 rotates over THREE streams — with the decoder's own stream that makes four, the hardware queues the runtime
      // maps streams onto (GPU_MAX_HW_QUEUES).  A fifth stream shares a queue with another one, and a queue runs in order:
      // with the fold on a stream of its own every third push's interning sat behind a later push's whole stage 1 (2 ms
      // instead of 0.4: profiles/r06_e2e_consumer_waits_trace.txt).  So the hand-over calls (surge_replay_append_decoded_async,
      // surge_replay_stage_decoded) take one stream out of the rotation when the handle folds on another stream than the
      // decoder's.  Measured, fold on the decoder's stream: 3 streams 9.1 - 9.2e8, 2 streams 8.6 - 8.7e8 events/s
      // (profiles/r06_e2e_push_streams.txt); fold on its own stream: 3 streams 6.9 - 7.3e8, 2 streams 8.3 - 8.7e8.  A fourth
      // (low-priority) push stream: 6.8 - 7.0e8 with the 2.5 ms stalls back (profiles/r06_e2e_push_priority.txt).
      int n = 3;
      if (const char* v = std::getenv("SURGE_INGEST_PUSH_STREAMS")) {  // experiments: 5 = a stream per slot (round 4)
        n = std::atoi(v);
        d->push_streams_pinned = true;
      }
      n = n < 1 ? 1 : (n > kSlots ? kSlots : n);
      for (int i = 0; i < n; ++i) {
        // ... and at LOW priority: the runtime keeps a pool of hardware queues per priority, so the stage-1 streams cannot land on
        // the queue of the decoder's own stream or of the fold's whatever other streams the process has created (in bench.py's
        // default line, behind the legs that ran before it, one of three normal-priority push streams did: 7.4 instead of 9.1e8);
        // and stage 1 is the bulk work — interning and fold, the dependent chain, should win a tie (SURGE_INGEST_PUSH_PRIORITY=normal)
        int least = 0, greatest = 0;
        static const bool normal_prio = [] { const char* v = std::getenv("SURGE_INGEST_PUSH_PRIORITY"); return v && std::strcmp(v, "normal") == 0; }();
        if (!normal_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
          DCHK(d, hipStreamCreateWithPriority(&d->push_streams[i], hipStreamNonBlocking, least));
        else
          DCHK(d, hipStreamCreateWithFlags(&d->push_streams[i], hipStreamNonBlocking));
        d->n_push_streams = d->n_push_active = i + 1;
      }
    }
    for (PushSlot& s : d->slots) {
      DCHK(d, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
      DCHK(d, hipEventCreateWithFlags(&s.released, hipEventDisableTiming));
      DCHK(d, s.d_err.reserve(sizeof(ErrorCell), false, d->stream));
    }
    DCHK(d, hipEventCreateWithFlags(&d->ready, hipEventDisableTiming));
    DCHK(d, hipEventCreateWithFlags(&d->consumed, hipEventDisableTiming));
    // A consumer thread that waits for the device a few times per fetch spins a core away in hipStreamSynchronize (0.4 - 1.2 ms of
    // CPU per 10^6-record fetch, and — on a host whose CPUs the framing threads need — 5 - 15 % of the bytes -> states rate:
    // profiles/r06_e2e_host_budget.jsonl).  The runtime's blocking wait (hipEventBlockingSync) still spins for its first few
    // hundred microseconds — most of a wait here — before it sleeps on the interrupt.  So the waits NAP: the event is queried
    // between nanosleeps of SURGE_INGEST_POLL_US (10) microseconds — the consumer thread's CPU 1.28 -> 0.81 ms per fetch at the
    // same rate (profiles/r06_e2e_wait_modes.txt).  SURGE_INGEST_WAIT=block sleeps on the blocking event, =spin keeps
    // hipStreamSynchronize.
    d->block_waits = true;
    d->poll_ns = 10000;
    if (const char* v = std::getenv("SURGE_INGEST_WAIT")) {
      d->block_waits = std::strcmp(v, "spin") != 0;
      if (std::strcmp(v, "poll") != 0) d->poll_ns = 0;
    }
    if (d->poll_ns > 0)
      if (const char* u = std::getenv("SURGE_INGEST_POLL_US")) d->poll_ns = std::atoll(u) > 0 ? std::atoll(u) * 1000 : d->poll_ns;
    if (d->block_waits) DCHK(d, hipEventCreateWithFlags(&d->sleeper, hipEventDisableTiming | hipEventBlockingSync));
    DCHK(d, d->key_off.reserve(8, false, d->stream));
    DCHK(d, hipMemset(d->key_off.p, 0, 8));
    if (tmpl) {
      d->h_tmpl = *tmpl;
      // the distinct field names, each once, and per type which of them it reads
      static EvjDevice ev;  // (a few KB of names: off the stack; create is not a hot path)
      static std::mutex ev_mu;
      std::lock_guard<std::mutex> lk(ev_mu);
      std::memset(&ev, 0, sizeof(ev));
      ev.n_types = tmpl->n_types;
      auto intern = [&](const char* name) -> uint8_t {
        if (!name[0]) return 0xff;
        for (uint32_t j = 1; j < ev.n_names; ++j)
          if (std::strncmp(ev.names[j], name, SURGE_EVJ_NAME) == 0) return (uint8_t)j;
        std::memcpy(ev.names[ev.n_names], name, SURGE_EVJ_NAME);
        ev.name_len[ev.n_names] = (uint8_t)strnlen(name, SURGE_EVJ_NAME);
        return (uint8_t)ev.n_names++;
      };
      std::memcpy(ev.names[0], tmpl->discriminator, SURGE_EVJ_NAME);
      ev.name_len[0] = (uint8_t)strnlen(tmpl->discriminator, SURGE_EVJ_NAME);
      ev.n_names = 1;
      for (uint32_t i = 0; i < tmpl->n_types; ++i) {
        const surge_event_json_type& ty = tmpl->types[i];
        std::memcpy(ev.type_name[i], ty.name, SURGE_EVJ_NAME);
        ev.type_name_len[i] = (uint8_t)strnlen(ty.name, SURGE_EVJ_NAME);
        ev.seq_name[i] = intern(ty.seq_field);
        ev.arg_name[i] = intern(ty.arg_field);
        ev.event_type[i] = ty.event_type;
        ev.arg_kind[i] = ty.arg_kind;
      }
      if (ev.n_names - 1 > (uint32_t)kEvjTrack)
        return dfail(d, E_UNSUPPORTED, "the event template names more than 8 distinct sequence / argument fields (decode this topic with surge_ingest_drain_json)");
      DCHK(d, d->d_tmpl.reserve(sizeof(ev), false, d->stream));
      DCHK(d, hipMemcpy(d->d_tmpl.p, &ev, sizeof(ev), hipMemcpyHostToDevice));
      DCHK(d, d->d_ptab.reserve(sizeof(surge::F64ParseTable), false, d->stream));
      DCHK(d, hipMemcpy(d->d_ptab.p, surge::f64_parse_table_host(), sizeof(surge::F64ParseTable), hipMemcpyHostToDevice));
    }
    return OK;
  };
  rc = init();
  (void)hipSetDevice(prev);
  if (rc != OK) {
    surge_device_decoder_destroy(d);
    return rc;
  }
  *out = d;
  return OK;
}

int32_t surge_device_decoder_create(int32_t device_id, void* hip_stream, const surge_event_json_template* tmpl, surge_device_decoder** out) {
  return decoder_create(device_id, hip_stream, tmpl, false, out);
}

int32_t surge_device_decoder_create_states(int32_t device_id, void* hip_stream, surge_device_decoder** out) {
  return decoder_create(device_id, hip_stream, nullptr, true, out);
}

int32_t surge_device_decoder_destroy(surge_device_decoder* d) {
  if (!d) return OK;
#ifdef SURGE_EXPERIMENTS
  std::fprintf(stderr, "[surge experiments] decoder: %lld pushes, %lld batches chained by the one-lane walk after the parallel recognition declined\n", (long long)d->pushes,
               (long long)d->chain_fallbacks);
#endif
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(d->device);
  (void)hipStreamSynchronize(d->stream);
  for (int i = 0; i < d->n_push_streams; ++i) {
    (void)hipStreamSynchronize(d->push_streams[i]);
    (void)hipStreamDestroy(d->push_streams[i]);
  }
  for (PushSlot& s : d->slots) {
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.released) (void)hipEventDestroy(s.released);
    Buf* sb[] = {&s.lz4_blocks, &s.lz4_sizes, &s.lz4_nseq, &s.lz4_seq, &s.lz4_cls, &s.d_bytes, &s.d_sections, &s.rec_a, &s.rec_b, &s.rec_c, &s.meta, &s.ev_tmp,
                 &s.f64_list, &s.d_err, &s.crc_spans};
    for (Buf* b : sb) b->release();
    if (s.pinned) (void)hipHostFree(s.pinned);
  }
  Buf* bufs[] = {&d->d_tmpl, &d->d_ptab, &d->first, &d->first_scan, &d->keep, &d->keep_pos, &d->temp, &d->t_slots,
                 &d->arena, &d->key_off, &d->key_hash, &d->r_agg, &d->r_ev, &d->r_off, &d->vlen, &d->vscan, &d->val_src,
                 &d->long_runs, &d->st_status, &d->r_val, &d->r_val_off, &d->st_spans};
  for (Buf* b : bufs) b->release();
  for (auto& col : d->str_cols)
    for (int k = 0; k < 2; ++k) { col.utf8[k].release(); col.off[k].release(); }
  if (d->ready) (void)hipEventDestroy(d->ready);
  if (d->consumed) (void)hipEventDestroy(d->consumed);
  if (d->sleeper) (void)hipEventDestroy(d->sleeper);
  (void)hipSetDevice(prev);
  delete d;
  return OK;
}

}  // extern "C" (reopened below)

namespace {

// the envelope the decoder's template names (h_tmpl: validated at create), as JsonCtx carries it
int16_t envelope_of(const surge_device_decoder* d) { return d->json ? (int16_t)d->h_tmpl.envelope : (int16_t)0; }

const char* why_bad(uint32_t status) {
  static const char* why[] = {"", "", "has a null key or value (not an event)", "is malformed (a length runs past its record or batch)",
                              "is not the JSON object the event template describes", "names an event type the template does not know",
                              "lacks a field the template names, or the field is not the number it should be", "is not a 16-byte fixed event", "",
                              "collides with another key on its 64-bit hash",
                              "has an empty, non-null value under a key (a state record carries a value or the null of a tombstone)",
                              "is not the protobuf Event envelope the event template names ([aggregateId] [payload] and nothing else)",
                              "names another aggregateId in its envelope than the aggregate id of its key"};
  return status < 13 ? why[status] : "is bad";
}

struct DeviceScope {  // the calling thread's device, restored on the way out
  int prev = 0;
  explicit DeviceScope(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
  ~DeviceScope() { (void)hipSetDevice(prev); }
};

// the slot a new push's stage 1 goes into (nullptr with the error set: every slot holds an unfinished push)
PushSlot* claim_slot(surge_device_decoder* d, int32_t* rc) {
  if (d->poisoned) {
    *rc = dfail(d, SURGE_E_STATE, "an earlier push failed on the device half way: destroy this decoder and create a new one");
    return nullptr;
  }
  PushSlot* s = nullptr;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->n_pending < kSlots) s = &d->slots[(d->head + d->n_pending) % kSlots];  // (a finish on the other thread moves head and n_pending together: the same slot)
    if (s) s->stream = d->push_streams[d->push_seq++ % (uint64_t)d->n_push_active];
  }
  if (!s) *rc = dfail(d, SURGE_E_STATE, "every push slot holds an unfinished push: call surge_device_decoder_push_finish first");
  return s;
}

// the slot's last push was finished without waiting for the device (push_finish_async): its buffers are free once the
// decoder's stream has passed the end of that stage 2
int32_t await_release(surge_device_decoder* d, PushSlot& s) {
  if (!s.released_valid) return OK;
  DCHK(d, hipStreamWaitEvent(s.stream, s.released, 0));
  s.released_valid = false;
  return OK;
}

int32_t slot_scratch(surge_device_decoder* d, PushSlot& s, int64_t n_rec) {
  const size_t R = (size_t)n_rec;
  DCHK(d, s.meta.reserve(R * sizeof(RecMeta), false, s.stream));
  if (!d->states) DCHK(d, s.ev_tmp.reserve(R * 16, false, s.stream));
  if (!d->states) DCHK(d, s.f64_list.reserve(R * 4, false, s.stream));
  static const ErrorCell kZero{~0ull, 0u, 0u, ~0u, ~0u};  // (the source of an asynchronous copy: it must outlive the call)
  DCHK(d, hipMemcpyAsync(s.d_err.p, &kZero, sizeof(kZero), hipMemcpyHostToDevice, s.stream));
  return OK;
}

int32_t slot_pinned(surge_device_decoder* d, PushSlot& s, size_t bytes) {
  if (bytes <= s.pinned_cap) return OK;
  if (s.pinned) (void)hipHostFree(s.pinned);
  s.pinned = nullptr;
  s.pinned_cap = 0;
  bytes += bytes / 4 + 65536;  // (room to spare: the next fetch's tables are a few per cent larger or smaller)
  DCHK(d, hipHostMalloc(&s.pinned, bytes, hipHostMallocDefault));
  s.pinned_cap = bytes;
  return OK;
}

// SURGE_DBG_DECODE=<lz4 mode><section mode> (two digits; timing experiments only — see Lz4Work::dbg / JsonCtx::dbg; a
// lz4 mode needs a section mode, since the sections' bytes are then not the topic's)
int32_t dbg_decode() {
#ifdef SURGE_EXPERIMENTS  // this hook makes the decoder deliver records that are NOT the topic's: experiment builds of the library only
  static const int32_t v = [] {
    const char* e = std::getenv("SURGE_DBG_DECODE");
    const int32_t x = e ? std::atoi(e) : 0;
    return (x >= 10 && x % 10 == 0) ? x + 1 : x;
  }();
  return v;
#else
  return 0;
#endif
}

// SURGE_DBG_TIMING: the host time every step of stage 1 took, to stderr
struct Laps {
  const bool on = std::getenv("SURGE_DBG_TIMING") != nullptr;
  double mark = on ? now_us() : 0.0;
  static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void lap(const char* what) {
    const double t = on ? now_us() : 0.0;
    if (on) std::fprintf(stderr, "[surge dbg] stage1 %-14s %8.1f us\n", what, t - mark);
    mark = t;
  }
};

// Where a wire push's bytes go on the device: the span of each part's arena the push needs, one after the other (16-byte
// aligned), then the sections the host decompressed (`extra`), then — from area_base on — the frames the device decompresses.
struct WireLayout {
  struct Part {
    int64_t lo, len, dev;  // the span [lo, lo + len) of the caller's arena goes to `dev` of the slot's bytes
    bool in_place;         // ... straight out of the arena: it is page-locked (surge_ingest_use_pinned_arena)
  };
  std::vector<Part> parts;
  std::vector<uint8_t> extra;
  int64_t total_sections = 0, n_rec = 0, n_raw = 0;
  int32_t max_recs = 0;  // of one batch of this push (section_kernel's workgroup size)
  int64_t area_base() const { return (n_raw + (int64_t)extra.size() + 15) & ~15ll; }
};

struct SlotNeeds {  // what a slot's buffers have to hold for a push
  size_t bytes, sections, crc_spans, pinned;
  int64_t n_rec;
  Lz4ScratchBytes lz4;
};

size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

// step 1: the parts' spans and the push's section table (s.h_secs)
int32_t layout_sections(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const surge_batch_section* const* sections, const int64_t* n_sections, WireLayout& L) {
  try {
    s.h_secs.resize((size_t)L.total_sections);
    L.parts.resize((size_t)n_parts);
  } catch (const std::bad_alloc&) {
    return dfail(d, E_NOMEM, "out of host memory");
  }
  int64_t at = 0;
  for (int32_t p = 0; p < n_parts; ++p) {
    int64_t lo = INT64_MAX, hi = 0;
    for (int64_t i = 0; i < n_sections[p]; ++i) {
      const surge_batch_section& in = sections[p][i];
      if (in.byte_off < 0 || in.byte_len < 0 || in.n_records < 0) return dfail(d, E_INVALID, "negative section field");
      const int64_t crc_prefix = (in.codec & SURGE_SECTION_CRC_PENDING) ? 8 : (in.codec & SURGE_SECTION_CRC_WIRE) ? 44 : 0;
      if (crc_prefix && (in.byte_off < crc_prefix || in.byte_len >= (1ll << 31) - 64)) return dfail(d, E_INVALID, "a CRC-pending section without the bytes in front of it");
      lo = in.byte_off - crc_prefix < lo ? in.byte_off - crc_prefix : lo;
      hi = in.byte_off + in.byte_len > hi ? in.byte_off + in.byte_len : hi;
    }
    if (n_sections[p] == 0) lo = hi = 0;
    L.parts[(size_t)p] = WireLayout::Part{lo, hi - lo, L.n_raw, false};
    for (int64_t i = 0; i < n_sections[p]; ++i, ++at) {
      const surge_batch_section& in = sections[p][i];
      s.h_secs[(size_t)at] = Section{L.n_raw + (in.byte_off - lo), in.byte_len, in.base_offset, in.n_records, 0, L.n_rec};
      L.n_rec += in.n_records;
      L.max_recs = in.n_records > L.max_recs ? in.n_records : L.max_recs;
    }
    L.n_raw = (L.n_raw + (hi - lo) + 15) & ~15ll;
  }
  return OK;
}

// step 2: one walk over the sections' first bytes on the host — the CRC spans the device finishes (s.h_crc) and the LZ4
// frames' blocks (s.lz4: ingest_lz4.hip reads the frames)
int32_t plan_frames(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                    const int64_t* n_sections, WireLayout& L) {
  try {
    s.lz4.clear();
    s.h_crc.clear();
    int64_t at = 0;
    for (int32_t p = 0; p < n_parts; ++p) {
      for (int64_t i = 0; i < n_sections[p]; ++i, ++at) {
        const surge_batch_section& in = sections[p][i];
        // (the frame headers were written by the framing threads, on other cores: one cache miss per batch — 1.2 ms per
        // 7000-batch push — unless they are asked for ahead of time)
        // ... the lines this walk reads of a section: its first bytes (and, framed in place, the crc field 44 bytes in front of
        // them), and its last words (where lz4_plan_section's walk over a frame ends)
        if (i + 16 < n_sections[p]) {
          const surge_batch_section& nx = sections[p][i + 16];
          __builtin_prefetch(bytes[p] + nx.byte_off - ((nx.codec & SURGE_SECTION_CRC_WIRE) ? 44 : 0));
          __builtin_prefetch(bytes[p] + nx.byte_off + 16);
          if (nx.byte_len > 64) __builtin_prefetch(bytes[p] + nx.byte_off + nx.byte_len - 8);
        }
        Section& sec = s.h_secs[(size_t)at];
        if (in.codec & SURGE_SECTION_CRC_PENDING) {  // {crc, register after the header bytes}, written by the framer in front of the section
          uint32_t pre[2];
          std::memcpy(pre, bytes[p] + in.byte_off - 8, 8);
          s.h_crc.push_back(CrcSpan{sec.byte_off, (int32_t)in.byte_len, (int32_t)at, pre[0], pre[1]});
        } else if (in.codec & SURGE_SECTION_CRC_WIRE) {  // the batch as received: its crc field (big-endian), then the 40 header bytes it covers, then the section
          const uint8_t* c = bytes[p] + in.byte_off - 44;
          const uint32_t expect = ((uint32_t)c[0] << 24) | ((uint32_t)c[1] << 16) | ((uint32_t)c[2] << 8) | c[3];
          s.h_crc.push_back(CrcSpan{sec.byte_off - 40, (int32_t)in.byte_len + 40, (int32_t)at, expect, ~0u});
        }
        if ((in.codec & 0xff) != 3 || in.n_records == 0) continue;
        const size_t ex = L.extra.size();
        int64_t area_off = 0;
        switch (lz4_plan_section(s.lz4, bytes[p] + in.byte_off, in.byte_len, sec.byte_off, (int32_t)at, &area_off, L.extra)) {
          case LZ4_ON_DEVICE:  // byte_off: resolved below, once the raw spans' final size is known; byte_len: set by the kernel that decodes the frame's last block
            sec.byte_off = -1 - area_off;
            sec.byte_len = 0;
            break;
          case LZ4_ON_HOST:
            sec.byte_off = L.n_raw + (int64_t)ex;
            sec.byte_len = (int64_t)(L.extra.size() - ex);
            break;
          case LZ4_TOO_LARGE: return dfail(d, SURGE_E_CORRUPT, "LZ4 batch expands beyond 2 GiB");
          case LZ4_BAD_FRAME: return dfail(d, SURGE_E_CORRUPT, "bad LZ4 frame in the section at base offset " + std::to_string(in.base_offset));
        }
      }
    }
  } catch (const std::bad_alloc&) {
    return dfail(d, E_NOMEM, "out of host memory");
  }
  if (s.lz4.blocks.size() >= (1ull << 31)) return dfail(d, E_UNSUPPORTED, "more than 2^31 LZ4 blocks in one push: push fewer sections at a time");
  for (Section& sc : s.h_secs)
    if (sc.byte_off < 0) sc.byte_off = L.area_base() + (-1 - sc.byte_off);
  return OK;
}

// step 3: what the push needs of a slot.  A part goes straight out of the caller's arena when that is page-locked, else
// through the slot's own pinned staging (one extra host copy); the section, block and CRC tables travel through the staging
// too: a copy from pageable memory waits for the stream (1.4 ms of host time per push went there)
SlotNeeds slot_needs(const PushSlot& s, const uint8_t* const* bytes, WireLayout& L) {
  SlotNeeds n;
  n.bytes = (size_t)(L.area_base() + s.lz4.area) + 64;
  n.sections = sizeof(Section) * s.h_secs.size();
  n.crc_spans = sizeof(CrcSpan) * s.h_crc.size();
  n.n_rec = L.n_rec;
  n.lz4 = lz4_scratch_bytes(s.lz4);
  n.pinned = pad16(L.extra.size()) + n.sections + n.lz4.blocks + pad16(n.crc_spans) + 64;
  for (size_t p = 0; p < L.parts.size(); ++p) {
    WireLayout::Part& part = L.parts[p];
    if (part.len == 0) continue;
    hipPointerAttribute_t attr;
    part.in_place = hipPointerGetAttributes(&attr, bytes[p] + part.lo) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // a pageable pointer makes hipPointerGetAttributes fail: not an error of this call
    if (!part.in_place) n.pinned += pad16((size_t)part.len);
  }
  return n;
}

int32_t size_slot(surge_device_decoder* d, PushSlot& t, const SlotNeeds& n) {
  const size_t per_event = d->states ? 0 : (size_t)n.n_rec;  // (a state decoder decodes no value)
  const std::pair<Buf*, size_t> device[] = {{&t.d_bytes, n.bytes}, {&t.d_sections, n.sections}, {&t.meta, (size_t)n.n_rec * sizeof(RecMeta)}, {&t.ev_tmp, per_event * 16},
                                            {&t.f64_list, per_event * 4}, {&t.crc_spans, n.crc_spans}, {&t.lz4_blocks, n.lz4.blocks}, {&t.lz4_sizes, n.lz4.state},
                                            {&t.lz4_nseq, n.lz4.n_seq}, {&t.lz4_seq, n.lz4.seq}, {&t.lz4_cls, n.lz4.cls}};
  for (const auto& b : device) DCHK(d, b.first->reserve(b.second, false, t.stream));
  return slot_pinned(d, t, n.pinned);
}

// The FIRST wire push of a decoder sizes every slot like its own: the fetches of a recovery are alike, and a slot that sizes
// its buffers when its turn comes does so in the middle of the pipeline (an allocation per buffer, a hipFree — a device-wide
// wait — for every one that grows, and milliseconds to page-lock its staging).
void warm_idle_slots(surge_device_decoder* d, PushSlot& s, const SlotNeeds& n) {
  if (d->slots_sized) return;
  d->slots_sized = true;
  // (only while nothing else is in flight — the decoder's first push as a rule: no other slot is then being read by a push or by
  // the thread that finishes pushes; a slot whose last push was finished without a wait is left alone too)
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->n_pending != 0) return;
  }
  for (PushSlot& t : d->slots)
    if (&t != &s && !t.busy && !t.released_valid && size_slot(d, t, n) != OK) (void)hipGetLastError();  // (best effort: a slot that could not be sized now reports it when its turn comes)
}

// step 4: everything the kernels read, to the device on the slot's stream
int32_t stage_and_copy(surge_device_decoder* d, PushSlot& s, const uint8_t* const* bytes, const WireLayout& L) {
  hipStream_t st = s.stream;
  size_t staged = 0;
  auto stage = [&](const void* src, size_t len) -> const uint8_t* {
    uint8_t* at = (uint8_t*)s.pinned + staged;
    std::memcpy(at, src, len);
    staged += pad16(len);
    return at;
  };
  for (size_t p = 0; p < L.parts.size(); ++p) {
    const WireLayout::Part& part = L.parts[p];
    if (part.len == 0) continue;
    const uint8_t* src = bytes[p] + part.lo;
    if (!part.in_place) src = stage(src, (size_t)part.len);
    DCHK(d, hipMemcpyAsync((uint8_t*)s.d_bytes.p + part.dev, src, (size_t)part.len, hipMemcpyHostToDevice, st));
  }
  if (!L.extra.empty()) DCHK(d, hipMemcpyAsync((uint8_t*)s.d_bytes.p + L.n_raw, stage(L.extra.data(), L.extra.size()), L.extra.size(), hipMemcpyHostToDevice, st));
  const size_t sec_bytes = sizeof(Section) * s.h_secs.size(), crc_bytes = sizeof(CrcSpan) * s.h_crc.size(), blk_bytes = sizeof(Lz4Block) * s.lz4.blocks.size();
  DCHK(d, hipMemcpyAsync(s.d_sections.p, stage(s.h_secs.data(), sec_bytes), sec_bytes, hipMemcpyHostToDevice, st));
  if (crc_bytes) DCHK(d, hipMemcpyAsync(s.crc_spans.p, stage(s.h_crc.data(), crc_bytes), crc_bytes, hipMemcpyHostToDevice, st));
  if (blk_bytes) DCHK(d, hipMemcpyAsync(s.lz4_blocks.p, stage(s.lz4.blocks.data(), blk_bytes), blk_bytes, hipMemcpyHostToDevice, st));
  return OK;
}

// Stage 1 of a wire push: the parts' records sections to the device, LZ4 blocks decoded, every record chained, parsed and
// its value decoded.  Nothing here reads or writes the key table.
int32_t stage1_wire(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                    const int64_t* n_sections) {
  Laps laps;
  const uint64_t seed = d->seed.load();
  WireLayout L;
  for (int32_t p = 0; p < n_parts; ++p) {
    if (n_sections[p] < 0 || (n_sections[p] > 0 && (!bytes[p] || !sections[p]))) return dfail(d, E_INVALID, "bad argument");
    L.total_sections += n_sections[p];
  }
  s.n_rec = 0;
  s.wire = true;
  if (L.total_sections == 0) return OK;
  if (L.total_sections >= (1ll << 31)) return dfail(d, E_UNSUPPORTED, "more than 2^31 batches in one push");
  int32_t rc = layout_sections(d, s, n_parts, sections, n_sections, L);
  if (rc != OK || L.n_rec == 0) return rc;
  if (L.n_rec >= (1ll << 32) - 1) return dfail(d, E_UNSUPPORTED, "more than 2^32 - 2 records in one push: push fewer sections at a time");
  rc = plan_frames(d, s, n_parts, bytes, sections, n_sections, L);
  if (rc != OK) return rc;
  laps.lap("walk sections");
  const SlotNeeds needs = slot_needs(s, bytes, L);
  warm_idle_slots(d, s, needs);
  rc = size_slot(d, s, needs);
  if (rc == OK) rc = slot_scratch(d, s, L.n_rec);
  if (rc == OK) laps.lap("reserve");
  if (rc == OK) rc = stage_and_copy(d, s, bytes, L);
  if (rc != OK) return rc;
  hipStream_t st = s.stream;
  const uint8_t* dby = (const uint8_t*)s.d_bytes.p;
  Section* dsec = (Section*)s.d_sections.p;
  ErrorCell* derr = (ErrorCell*)s.d_err.p;
  // the batches' CRC-32C, finished where their bytes now are (the host ran it over the 40 header bytes only)
  if (!s.h_crc.empty()) DCHK(d, launch_crc(dby, (const CrcSpan*)s.crc_spans.p, (int32_t)s.h_crc.size(), derr, st));
  laps.lap("copies");
  Lz4Work w{dbg_decode() / 10, (int32_t*)s.lz4_sizes.p, (int32_t*)s.lz4_nseq.p, (uint2*)s.lz4_seq.p, (int32_t*)s.lz4_cls.p, nullptr};
  DCHK(d, launch_lz4(s.lz4, dby, (uint8_t*)s.d_bytes.p + L.area_base(), (const Lz4Block*)s.lz4_blocks.p, w, dsec, derr, st));
  laps.lap("lz4 launches");
  JsonCtx jc{d->json ? (const EvjDevice*)d->d_tmpl.p : nullptr, (const surge::F64ParseTable*)d->d_ptab.p, dbg_decode() % 10, (int16_t)(d->states ? 1 : 0), envelope_of(d)};
  DCHK(d, launch_sections(dby, dsec, L.total_sections, L.max_recs, seed, jc, (RecMeta*)s.meta.p, (uint4*)s.ev_tmp.p, (uint32_t*)s.f64_list.p, derr, st));
  laps.lap("section launches");
  s.n_rec = L.n_rec;
  s.seed = seed;
  return OK;
}

// Stage 1 of a push of records that are already framed
int32_t stage1_records(surge_device_decoder* d, PushSlot& s, const uint8_t* keys, const int64_t* key_off, const uint8_t* values, const int64_t* value_off,
                       const int64_t* offsets, int64_t n) {
  s.n_rec = 0;
  s.wire = false;
  const uint64_t seed = d->seed.load();
  if (n == 0) return OK;
  if (n >= (1ll << 32) - 1) return dfail(d, E_UNSUPPORTED, "more than 2^32 - 2 records in one push");
  const int64_t kb = key_off[n] - key_off[0], vb = value_off[n] - value_off[0];
  if (kb < 0 || vb < 0 || (kb > 0 && !keys) || (vb > 0 && !values)) return dfail(d, E_INVALID, "bad key / value spans");
  for (int64_t i = 0; i < n; ++i)  // (the kernels index the staged bytes with these: no launch on offsets that run backwards)
    if (key_off[i + 1] < key_off[i] || value_off[i + 1] < value_off[i]) return dfail(d, E_INVALID, "key_off / value_off must not decrease (record " + std::to_string(i) + ")");
  hipStream_t st = s.stream;
  const size_t n_bytes = (size_t)(kb + vb), off_bytes = (size_t)(n + 1) * 8;
  const size_t stage = n_bytes + 2 * off_bytes + (offsets ? (size_t)n * 8 : 0) + 64;
  DCHK(d, s.d_bytes.reserve(n_bytes + 16, false, st));
  DCHK(d, s.rec_a.reserve(off_bytes, false, st));  // the device copies of key_off / value_off / offsets
  DCHK(d, s.rec_b.reserve(off_bytes, false, st));
  DCHK(d, s.rec_c.reserve((size_t)n * 8 + 8, false, st));
  {
    int32_t rc = slot_scratch(d, s, n);
    if (rc == OK) rc = slot_pinned(d, s, stage);
    if (rc != OK) return rc;
  }
  // pinned staging: [keys][values][key_off (rebased)][value_off (rebased)][offsets]
  uint8_t* pin = (uint8_t*)s.pinned;
  if (kb) std::memcpy(pin, keys + key_off[0], (size_t)kb);
  if (vb) std::memcpy(pin + kb, values + value_off[0], (size_t)vb);
  int64_t* p_ko = (int64_t*)(pin + ((n_bytes + 7) & ~(size_t)7));
  int64_t* p_vo = p_ko + (n + 1);
  int64_t* p_of = p_vo + (n + 1);
  for (int64_t i = 0; i <= n; ++i) { p_ko[i] = key_off[i] - key_off[0]; p_vo[i] = value_off[i] - value_off[0]; }
  if (offsets) std::memcpy(p_of, offsets, (size_t)n * 8);
  if (n_bytes) DCHK(d, hipMemcpyAsync(s.d_bytes.p, pin, n_bytes, hipMemcpyHostToDevice, st));
  DCHK(d, hipMemcpyAsync(s.rec_a.p, p_ko, off_bytes, hipMemcpyHostToDevice, st));
  DCHK(d, hipMemcpyAsync(s.rec_b.p, p_vo, off_bytes, hipMemcpyHostToDevice, st));
  if (offsets) DCHK(d, hipMemcpyAsync(s.rec_c.p, p_of, (size_t)n * 8, hipMemcpyHostToDevice, st));
  DCHK(d, launch_records((const uint8_t*)s.d_bytes.p, (const int64_t*)s.rec_a.p, (const int64_t*)s.rec_b.p, offsets ? (const int64_t*)s.rec_c.p : nullptr, kb, n, seed,
                         JsonCtx{d->json ? (const EvjDevice*)d->d_tmpl.p : nullptr, (const surge::F64ParseTable*)d->d_ptab.p, 0, (int16_t)(d->states ? 1 : 0), envelope_of(d)}, (RecMeta*)s.meta.p,
                         (uint4*)s.ev_tmp.p, (uint32_t*)s.f64_list.p, (ErrorCell*)s.d_err.p, st));
  s.n_rec = n;
  s.seed = seed;
  return OK;
}

// a consumer that folds on another stream than the decoder's adds a stream: stage 1 then rotates over one fewer (surge_device_decoder_create)
void fold_stream_seen(surge_device_decoder* d, hipStream_t fold_stream) {
  if (d->push_streams_pinned || fold_stream == d->stream) return;
  std::lock_guard<std::mutex> lk(d->mu);
  if (d->n_push_active == d->n_push_streams && d->n_push_active > 2) d->n_push_active = d->n_push_streams - 1;
}

// the consumer thread's wait for `st`: naps between event queries (surge_device_decoder_create; SURGE_INGEST_WAIT=block: asleep on
// the blocking event, =spin: hipStreamSynchronize)
hipError_t wait_stream(surge_device_decoder* d, hipStream_t st) {
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

// Stage 2: everything behind the per-record metadata and decoded values — interning, compaction, append — on the
// decoder's stream.  Two synchronisations: one in the middle (what the push discovered: errors, new keys, their bytes,
// delivered records — everything the allocations behind it need), one at the end.  Nothing is committed before the
// first: a push that fails takes the keys it probed out of the table again (rollback_kernel), so a failed push leaves
// the decoder exactly as it was.  wait = false leaves the second synchronisation out: the results are complete in the
// order of the decoder's stream (surge_device_decoder_push_finish_async).
int32_t stage2(surge_device_decoder* d, PushSlot& s, bool wait) {
  const int64_t n_rec = s.n_rec;
  if (n_rec == 0) return OK;
  hipStream_t st = d->stream;
  const size_t R = (size_t)n_rec;
  const uint8_t* dby = (const uint8_t*)s.d_bytes.p;
  ErrorCell* derr = (ErrorCell*)s.d_err.p;
  RecMeta* dmeta = (RecMeta*)s.meta.p;
  auto poison = [&](int32_t rc) { d->poisoned = true; return rc; };
#define PCHK(call)                                                                                                      \
  do {                                                                                                                  \
    hipError_t e_ = (call);                                                                                             \
    if (e_ != hipSuccess) return poison(dfail(d, e_ == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_))); \
  } while (0)
  // scratch (nothing of the push is in the table yet: an allocation failure here needs no rollback)
  DCHK(d, d->first.reserve((R + 1) * 8, false, st));
  DCHK(d, d->first_scan.reserve((R + 1) * 8, false, st));
  DCHK(d, d->keep.reserve((R + 1) * 4, false, st));
  DCHK(d, d->keep_pos.reserve((R + 1) * 4, false, st));
  {
    size_t temp_bytes = 0;
    DCHK(d, intern_temp_bytes(n_rec, &temp_bytes, st));
    DCHK(d, d->temp.reserve(temp_bytes, false, st));
    if (d->states) {
      DCHK(d, d->vlen.reserve((R + 1) * 8, false, st));
      DCHK(d, d->vscan.reserve((R + 1) * 8, false, st));
    }
    const int32_t rc = ensure_table(d, n_rec);
    if (rc != OK) return rc;
  }
  const InternScratch scratch{(unsigned long long*)d->first.p, (unsigned long long*)d->first_scan.p, (uint32_t*)d->keep.p, (uint32_t*)d->keep_pos.p, d->temp.p, d->temp.cap};
  PCHK(hipStreamWaitEvent(st, s.done, 0));
  if (s.seed != d->seed) launch_rekey_records(dmeta, n_rec, dby, d->seed, st);  // the table was re-seeded after this push's stage 1 hashed its keys
  ErrorCell ec;
  unsigned long long first_total = 0, val_total = 0;
  uint32_t kept = 0;
  StateScratch values{(unsigned long long*)d->vlen.p, (unsigned long long*)d->vscan.p, nullptr, nullptr};
  for (int attempt = 0;; ++attempt) {
    PCHK(launch_intern_probe(dmeta, n_rec, dby, keys_of(d), scratch, derr, st));
    if (d->states) {  // the delivered records' value lengths, scanned: where each value goes, and how many bytes the push adds
      PCHK(launch_value_scan(dmeta, n_rec, scratch, values, st));
      PCHK(hipMemcpyAsync(&val_total, values.vscan + R, 8, hipMemcpyDeviceToHost, st));
    }
    PCHK(hipMemcpyAsync(&ec, derr, sizeof(ec), hipMemcpyDeviceToHost, st));
    PCHK(hipMemcpyAsync(&first_total, (unsigned long long*)d->first_scan.p + R, 8, hipMemcpyDeviceToHost, st));
    PCHK(hipMemcpyAsync(&kept, (uint32_t*)d->keep_pos.p + R, 4, hipMemcpyDeviceToHost, st));
    PCHK(wait_stream(d, st));
    if (ec.lz4_bad == ~0u && ec.crc_bad == ~0u && ec.first_bad != ~0ull && (uint32_t)(ec.first_bad & 0xff) == RS_COLLISION && attempt < 3) {
      // Two different keys share a 64-bit hash (about 3 in a million pushes at 10^7 keys): the table gets another hash
      // function — every known key re-hashed from its bytes in the arena, the push's records from theirs — and the push
      // goes through again.  Nothing of it was committed.
      d->seed = (d->seed & ~(1ull << 63)) + 1;
      ++d->reseeds;
      launch_intern_reseed(dmeta, n_rec, dby, keys_of(d), d->seed, st);
      s.h_err = ErrorCell{~0ull, 0u, ec.n_f64_host, ~0u, ~0u};
      PCHK(hipMemcpyAsync(derr, &s.h_err, sizeof(s.h_err), hipMemcpyHostToDevice, st));
      continue;
    }
    break;
  }
  d->counters[0] += n_rec;
  auto fail = [&](int32_t code, const std::string& why) -> int32_t {  // nothing of this push is delivered and no key it discovered stays interned
    launch_intern_rollback(dmeta, n_rec, keys_of(d).t, st);
    PCHK(hipStreamSynchronize(st));
    return dfail(d, code, why);
  };
  auto base_offset_of = [&](uint32_t section) { return std::to_string(section < s.h_secs.size() ? s.h_secs[section].base_offset : -1); };
  if (ec.crc_bad != ~0u) return fail(SURGE_E_CORRUPT, "record batch CRC-32C mismatch (verified on the device) in the batch at base offset " + base_offset_of(ec.crc_bad));
  if (ec.lz4_bad != ~0u)
    return fail(SURGE_E_CORRUPT, "bad LZ4 frame in the batch at base offset " + base_offset_of(ec.lz4_bad) + " (malformed sequence, or a block that is not 64 KiB where it must be)");
  if (ec.first_bad != ~0ull) {
    const int64_t rec = (int64_t)(ec.first_bad >> 8);
    const uint32_t status = (uint32_t)(ec.first_bad & 0xff);
    RecMeta m;
    PCHK(hipMemcpy(&m, dmeta + rec, sizeof(m), hipMemcpyDeviceToHost));
    if (status == RS_MALFORMED && s.wire) {
      // the record stage gives up on such a record before it keeps its offset: read it here, from the section's bytes as the
      // device has them (an LZ4 section exists decompressed there only) — the length varints up to the record, then its head
      size_t si = 0;
      while (si + 1 < s.h_secs.size() && s.h_secs[si + 1].rec_first <= rec) ++si;
      Section sec;
      std::vector<uint8_t> sb;
      if (si < s.h_secs.size() && hipMemcpy(&sec, (const Section*)s.d_sections.p + si, sizeof(sec), hipMemcpyDeviceToHost) == hipSuccess && sec.byte_len > 0 &&
          sec.byte_len < (1ll << 31)) {
        try { sb.resize((size_t)sec.byte_len); } catch (const std::bad_alloc&) { sb.clear(); }
        if (!sb.empty() && hipMemcpy(sb.data(), dby + sec.byte_off, sb.size(), hipMemcpyDeviceToHost) == hipSuccess) {
          size_t pos = 0;
          auto varlong = [&](int64_t* v) -> bool {
            uint64_t u = 0;
            for (int shift = 0; shift <= 63; shift += 7) {
              if (pos >= sb.size()) return false;
              const uint8_t b = sb[pos++];
              u |= (uint64_t)(b & 0x7f) << shift;
              if (!(b & 0x80)) { *v = (int64_t)(u >> 1) ^ -(int64_t)(u & 1); return true; }
            }
            return false;
          };
          int64_t len = 0, ts = 0, delta = 0;
          bool ok = true;
          for (int64_t k = sec.rec_first; ok && k < rec; ++k) {
            ok = varlong(&len) && len >= 0 && (uint64_t)len <= sb.size() - pos;
            if (ok) pos += (size_t)len;
          }
          if (ok && varlong(&len) && pos < sb.size() && (++pos, varlong(&ts)) && varlong(&delta)) m.offset = sec.base_offset + delta;
        }
      }
      (void)hipGetLastError();
    }
    return fail(status == RS_COLLISION ? E_UNSUPPORTED : SURGE_E_CORRUPT, "record " + std::to_string(rec) + " of the push (offset " + std::to_string(m.offset) + ") " +
                                                                             why_bad(status) + (status == RS_COLLISION ? " under four hash functions in a row" : ""));
  }
  const int64_t n_new = (int64_t)(first_total >> 40), new_bytes = (int64_t)(first_total & ((1ull << 40) - 1));
  {
    // everything that can fail for want of memory, before the first commit
    hipError_t e = hipSuccess;
    if (n_new > 0) {
      e = d->key_off.reserve((size_t)(d->n_keys + n_new + 1) * 8, true, st);
      if (e == hipSuccess) e = d->key_hash.reserve((size_t)(d->n_keys + n_new) * 8, true, st);
      if (e == hipSuccess) e = d->arena.reserve((size_t)(d->arena_bytes + new_bytes) + 16, true, st);
    }
    if (e == hipSuccess) e = d->r_agg.reserve((size_t)(d->n_records + kept) * 8 + 16, true, st);
    if (e == hipSuccess && !d->states) e = d->r_ev.reserve((size_t)(d->n_records + kept) * 16 + 16, true, st);
    if (d->states) {  // (the values buffer ends at least 64 bytes behind its last value)
      const size_t n_runs = ((size_t)kept + kGatherRecs - 1) / kGatherRecs;
      if (e == hipSuccess) e = d->r_val_off.reserve((size_t)(d->n_records + kept + 1) * 8 + 16, true, st);
      if (e == hipSuccess) e = d->r_val.reserve((size_t)(d->val_bytes + (int64_t)val_total) + 64, true, st);
      if (e == hipSuccess) e = d->val_src.reserve((size_t)kept * 8 + 16, false, st);
      if (e == hipSuccess) e = d->long_runs.reserve((n_runs + 1) * 4, false, st);
    }
    if (e == hipSuccess) e = d->r_off.reserve((size_t)(d->n_records + kept) * 8 + 16, true, st);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string("growing the key table / result arrays: ") + hipGetErrorString(e));
  }
  if (d->consumed_valid) {  // an asynchronous consumer of the last results (surge_replay_append_decoded_async) reads the arrays finalize_kernel writes
    PCHK(hipStreamWaitEvent(st, d->consumed, 0));
    d->consumed_valid = false;
  }
  launch_intern_commit(dmeta, n_rec, dby, keys_of(d), scratch, n_new, (const uint4*)s.ev_tmp.p, d->n_records, (int64_t*)d->r_agg.p, d->states ? nullptr : (uint4*)d->r_ev.p,
                       (int64_t*)d->r_off.p, st);
  PCHK(hipGetLastError());
  if (d->states) {  // the values leave the slot's bytes (its next push writes those again) for the result's own buffer
    values.val_src = (int64_t*)d->val_src.p;
    values.long_runs = (uint32_t*)d->long_runs.p;
    PCHK(launch_value_gather(dmeta, n_rec, dby, scratch, values, kept, d->n_records, d->val_bytes, (int64_t*)d->r_val_off.p, (uint8_t*)d->r_val.p, st));
    d->val_bytes += (int64_t)val_total;
  }
  d->n_keys += n_new;
  d->arena_bytes += new_bytes;
  if (ec.n_f64_host > 0) {
    PCHK(hipStreamSynchronize(st));  // the results have to be in place before the payloads are patched
    // Doubles the fast parser could not decide (more than 19 digits, or one of Eisel-Lemire's rare ambiguous products):
    // the host parses exactly those values with the library's host decoder and patches the payload in place
    std::vector<uint32_t> list(ec.n_f64_host);
    PCHK(hipMemcpy(list.data(), s.f64_list.p, (size_t)ec.n_f64_host * 4, hipMemcpyDeviceToHost));
    for (uint32_t i : list) {
      RecMeta m;
      uint32_t pos = 0;
      PCHK(hipMemcpy(&m, dmeta + i, sizeof(m), hipMemcpyDeviceToHost));
      PCHK(hipMemcpy(&pos, (uint32_t*)d->keep_pos.p + i, 4, hipMemcpyDeviceToHost));
      uint8_t ev[16];
      std::vector<uint8_t> value((size_t)m.val_len + 1);
      PCHK(hipMemcpy(value.data(), dby + m.val_off, (size_t)m.val_len, hipMemcpyDeviceToHost));  // (an LZ4 section exists decompressed on the device only)
      if (surge_event_json_decode(&d->h_tmpl, value.data(), m.val_len, ev) != 0)  // (the whole value and the template with its envelope; the device compared the id, accepted the number's spelling and its length: cannot happen)
        return poison(dfail(d, SURGE_E_CORRUPT, "record at offset " + std::to_string(m.offset) + ": " + surge_event_json_last_error()));
      PCHK(hipMemcpy((uint8_t*)d->r_ev.p + (size_t)(d->n_records + pos) * 16, ev, 16, hipMemcpyHostToDevice));
    }
    d->counters[3] += ec.n_f64_host;
  }
  d->chain_fallbacks += ec.reserved;
  d->n_records += kept;
  d->counters[1] += kept;
  d->counters[2] += n_rec - kept;
  ++d->pushes;
  if (wait) {
    PCHK(wait_stream(d, st));
  } else {  // the slot's buffers are read until here: its next stage 1 waits for this point of the stream
    PCHK(hipEventRecord(s.released, st));
    s.released_valid = true;
  }
  return OK;
#undef PCHK
}

// stage 1 is enqueued: the slot joins the queue
int32_t commit_slot(surge_device_decoder* d, PushSlot& s) {
  DCHK(d, hipEventRecord(s.done, s.stream));
  s.busy = true;
  std::lock_guard<std::mutex> lk(d->mu);
  ++d->n_pending;
  return OK;
}

int32_t finish_oldest(surge_device_decoder* d, bool wait) {
  PushSlot* sp;
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->n_pending == 0) sp = nullptr;
    else sp = &d->slots[d->head];
  }
  if (!sp) return dfail(d, SURGE_E_STATE, "push_finish without a pending push_async");
  PushSlot& s = *sp;
  const int32_t rc = stage2(d, s, wait);
  if (rc != OK) {
    // the slot's buffers are still being written by its own stream if stage 2 never waited for it, and read by
    // whatever stage 2 launched before it gave up
    (void)hipStreamSynchronize(s.stream);
    (void)hipStreamSynchronize(d->stream);
    s.released_valid = false;
  }
  s.busy = false;
  std::lock_guard<std::mutex> lk(d->mu);
  d->head = (d->head + 1) % kSlots;
  --d->n_pending;
  return rc;
}

// the resident state grows for the keys the decoder has interned
int32_t grow_for_keys(surge_replay_handle* h, surge_device_decoder* d) {
  void* d_states = nullptr;
  int64_t n_agg = 0;
  int32_t rc = surge_replay_device_state(h, &d_states, &n_agg);
  if (rc == OK && d->n_keys > n_agg) rc = surge_replay_grow(h, d->n_keys);
  return rc == OK ? OK : dfail(d, rc, surge_replay_last_error(h));
}

// The hand-over of the result arrays without a host wait on either side: the handle's stream waits (event) for the decoder's
// stream to have written the arrays, the group-by and the fold (fold = false: the copies into the handle's staged log) are
// enqueued behind that, and the next push_finish's stage 2 waits (event) for their last read before it writes the arrays
// again.  The host thread only ever waits in the middle of stage 2 (what the push discovered), so interning of fetch i + 1
// overlaps the fold of fetch i on the device.
int32_t hand_over_async(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out, bool fold) {
  if (!h || !d) return dfail(d, E_INVALID, "NULL argument");
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder holds state values, not events: hand them over with surge_device_decoder_load_states");
  if (n_events_out) *n_events_out = d->n_records;
  if (n_keys_out) *n_keys_out = d->n_keys;
  int32_t rc = fold ? grow_for_keys(h, d) : OK;
  if (rc != OK) return rc;
  if (d->n_records > 0) {
    void* hs = nullptr;
    rc = surge_replay_get_stream(h, &hs);
    if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
    DeviceScope scope(d->device);
    fold_stream_seen(d, (hipStream_t)hs);
    DCHK(d, hipEventRecord(d->ready, d->stream));
    DCHK(d, hipStreamWaitEvent((hipStream_t)hs, d->ready, 0));
    rc = fold ? surge_replay_append_events_device(h, (const int64_t*)d->r_agg.p, d->r_ev.p, d->n_records)
              : surge_replay_stage_events_device(h, (const int64_t*)d->r_agg.p, d->r_ev.p, d->n_records);
    // (recorded also when the call failed half way: whatever it enqueued reads the arrays)
    const hipError_t e = hipEventRecord(d->consumed, (hipStream_t)hs);
    d->consumed_valid = e == hipSuccess;
    if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
    if (e != hipSuccess) {
      (void)surge_replay_synchronize(h);
      return dfail(d, E_DEVICE, std::string("hipEventRecord: ") + hipGetErrorString(e));
    }
  }
  d->n_records = 0;
  return OK;
}

}  // namespace

extern "C" {

int32_t surge_device_decoder_push_parts_async(surge_device_decoder* d, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                                              const int64_t* n_sections) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (n_parts < 0 || (n_parts > 0 && (!bytes || !sections || !n_sections))) return dfail(d, E_INVALID, "bad argument");
  int32_t rc = OK;
  PushSlot* s = claim_slot(d, &rc);
  if (!s) return rc;
  DeviceScope scope(d->device);
  rc = await_release(d, *s);
  if (rc != OK) return rc;
  rc = stage1_wire(d, *s, n_parts, bytes, sections, n_sections);
  if (rc != OK) {
    (void)hipStreamSynchronize(s->stream);  // whatever was enqueued before the failure reads host memory of this call
    return rc;
  }
  return commit_slot(d, *s);
}

int32_t surge_device_decoder_push_async(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections) {
  return surge_device_decoder_push_parts_async(d, 1, &bytes, &sections, &n_sections);
}

int32_t surge_device_decoder_push_finish(surge_device_decoder* d) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  DeviceScope scope(d->device);
  return finish_oldest(d, true);
}

int32_t surge_device_decoder_push_finish_async(surge_device_decoder* d) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  DeviceScope scope(d->device);
  return finish_oldest(d, false);
}

int32_t surge_device_decoder_pending(const surge_device_decoder* d) {
  if (!d) return 0;
  std::lock_guard<std::mutex> lk(const_cast<surge_device_decoder*>(d)->mu);
  return d->n_pending;
}

int32_t surge_device_decoder_reserve(surge_device_decoder* d, int64_t n_keys, int64_t key_bytes) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (n_keys < 0 || key_bytes < 0) return dfail(d, E_INVALID, "negative capacity");
  if (d->n_pending != 0) return dfail(d, SURGE_E_STATE, "asynchronous pushes are pending");
  DeviceScope scope(d->device);
  hipStream_t st = d->stream;
  const int64_t extra = n_keys > d->n_keys ? n_keys - d->n_keys : 0;
  {
    const int32_t rc = ensure_table(d, extra);
    if (rc != OK) return rc;
  }
  DCHK(d, d->key_off.reserve((size_t)(n_keys + 1) * 8, true, st));
  DCHK(d, d->key_hash.reserve((size_t)n_keys * 8, true, st));
  DCHK(d, d->arena.reserve((size_t)key_bytes + 16, true, st));
  DCHK(d, hipStreamSynchronize(st));
  return OK;
}

int32_t surge_device_decoder_push(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (n_sections < 0 || (n_sections > 0 && (!bytes || !sections))) return dfail(d, E_INVALID, "bad argument");
  if (d->n_pending != 0) return dfail(d, SURGE_E_STATE, "asynchronous pushes are pending: finish them first (results are appended in push order)");
  if (n_sections == 0) return OK;
  const int32_t rc = surge_device_decoder_push_async(d, bytes, sections, n_sections);
  return rc != OK ? rc : surge_device_decoder_push_finish(d);
}

int32_t surge_device_decoder_push_records(surge_device_decoder* d, const uint8_t* keys, const int64_t* key_off, const uint8_t* values,
                                          const int64_t* value_off, const int64_t* offsets, int64_t n) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (n < 0 || (n > 0 && (!key_off || !value_off))) return dfail(d, E_INVALID, "bad argument");
  if (d->n_pending != 0) return dfail(d, SURGE_E_STATE, "asynchronous pushes are pending: finish them first (results are appended in push order)");
  if (n == 0) return OK;
  int32_t rc = OK;
  PushSlot* s = claim_slot(d, &rc);
  if (!s) return rc;
  DeviceScope scope(d->device);
  rc = await_release(d, *s);
  if (rc != OK) return rc;
  rc = stage1_records(d, *s, keys, key_off, values, value_off, offsets, n);
  if (rc != OK) {
    (void)hipStreamSynchronize(s->stream);
    return rc;
  }
  rc = commit_slot(d, *s);
  return rc != OK ? rc : finish_oldest(d, true);
}

int32_t surge_device_decoder_result(surge_device_decoder* d, int64_t* n_records, const int64_t** d_agg_idx, const void** d_events16,
                                    const int64_t** d_offsets, int64_t* n_keys) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder has no events: see surge_device_decoder_state_result");
  if (n_records) *n_records = d->n_records;
  if (d_agg_idx) *d_agg_idx = (const int64_t*)d->r_agg.p;
  if (d_events16) *d_events16 = d->r_ev.p;
  if (d_offsets) *d_offsets = (const int64_t*)d->r_off.p;
  if (n_keys) *n_keys = d->n_keys;
  return OK;
}

int32_t surge_device_decoder_state_result(surge_device_decoder* d, int64_t* n_records, const int64_t** d_agg_idx, const uint8_t** d_values,
                                          const int64_t** d_value_off, const int64_t** d_offsets, int64_t* n_keys) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): see surge_device_decoder_result");
  if (n_records) *n_records = d->n_records;
  if (d_agg_idx) *d_agg_idx = (const int64_t*)d->r_agg.p;
  if (d_values) *d_values = (const uint8_t*)d->r_val.p;
  if (d_value_off) *d_value_off = (const int64_t*)d->r_val_off.p;
  if (d_offsets) *d_offsets = (const int64_t*)d->r_off.p;
  if (n_keys) *n_keys = d->n_keys;
  return OK;
}

}  // extern "C"

// state values -> resident state: what a KTable restore of the state topic does with the records it is handed
// (SurgeStateStoreConsumer.scala:69), behind one call.  envelope: the values are protobuf State messages around the
// template's text (surge_device_decoder_load_protobuf_states)
static int32_t load_states(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl, int64_t counts_out[4], bool envelope) {
  if (!h || !d || !counts_out) return dfail(d, E_INVALID, "NULL argument");
  counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder hands over with surge_replay_append_decoded");
  int32_t rc = grow_for_keys(h, d);
  if (rc != OK) return rc;
  if (d->n_records == 0) return OK;
  void* hs = nullptr;
  rc = surge_replay_get_stream(h, &hs);
  if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
  void* d_states = nullptr;
  int64_t n_agg = 0;
  rc = surge_replay_device_state(h, &d_states, &n_agg);
  if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
  DeviceScope scope(d->device);
  DCHK(d, d->st_status.reserve((size_t)d->n_records, false, d->stream));
  if (d->keep_strings) DCHK(d, d->st_spans.reserve((size_t)d->n_records * (2 * SURGE_JSON_STRING_COLUMNS) * 8, false, d->stream));
  // the arrays are written on the decoder's stream and read on the handle's
  DCHK(d, hipEventRecord(d->ready, d->stream));
  DCHK(d, hipStreamWaitEvent((hipStream_t)hs, d->ready, 0));
  // (rows [0, n_keys): every aggregate index of the result is below the decoder's key count, and its key table has that many ids)
  rc = (envelope ? surge_replay_decode_protobuf_states : surge_replay_decode_json_states)(h, tmpl, (const uint8_t*)d->r_val.p, (const int64_t*)d->r_val_off.p, d->n_records, (const uint8_t*)d->arena.p,
                                       (const int64_t*)d->key_off.p, (const int64_t*)d->r_agg.p, d->n_keys, d_states, (uint8_t*)d->st_status.p,
                                       d->keep_strings ? (int64_t*)d->st_spans.p : nullptr, counts_out);
  if (rc != OK && rc != SURGE_E_CORRUPT) return dfail(d, rc, surge_replay_last_error(h));  // nothing was loaded: the records stay
  ++d->state_loads;
  std::string refused;
  if (rc == SURGE_E_CORRUPT) {  // everything else is loaded; name the first refused record by its TOPIC offset
    refused = surge_replay_last_error(h);
    std::vector<uint8_t> status((size_t)d->n_records);
    if (hipMemcpy(status.data(), d->st_status.p, status.size(), hipMemcpyDeviceToHost) == hipSuccess) {
      for (int64_t r = 0; r < d->n_records; ++r) {
        if (status[(size_t)r] == SURGE_STATE_DECODE_OK || status[(size_t)r] == SURGE_STATE_DECODE_SKIPPED) continue;
        int64_t offset = -1;
        if (hipMemcpy(&offset, (const int64_t*)d->r_off.p + r, 8, hipMemcpyDeviceToHost) == hipSuccess)
          refused = std::to_string(counts_out[2]) + " state value(s) were refused (their rows are untouched), the first at topic offset " + std::to_string(offset) +
                    " (record " + std::to_string(r) + " of this load) with status " + std::to_string((int)status[(size_t)r]) + " (SURGE_STATE_DECODE_*); everything else was loaded";
        break;
      }
    }
    (void)hipGetLastError();
  }
  if (d->keep_strings) {  // (a refused winner keeps its earlier string, as it keeps its row: everything else is merged)
    bool named[SURGE_JSON_STRING_COLUMNS] = {};
    for (uint32_t i = 0; i < tmpl->n_parts; ++i)
      if (tmpl->part[i].kind == SURGE_JP_STR && tmpl->part[i].field_offset < SURGE_JSON_STRING_COLUMNS) named[tmpl->part[i].field_offset] = true;
    for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
      if (!named[c]) continue;
      auto& col = d->str_cols[c];
      const int cur = col.cur, nxt = cur < 0 ? 0 : 1 - cur;
      // an unescaped string is never longer than its span, and the spans lie inside the load's values: the merge always fits
      const int64_t cap = col.bytes + d->val_bytes + 16;
      DCHK(d, col.off[nxt].reserve((size_t)(d->n_keys + 1) * 8, false, d->stream));
      DCHK(d, col.utf8[nxt].reserve((size_t)cap, false, d->stream));
      int64_t total = 0;
      const int32_t mrc = surge_replay_merge_state_strings(h, c, (const uint8_t*)d->r_val.p, (const int64_t*)d->r_val_off.p, d->n_records, (const int64_t*)d->r_agg.p,
                                                           (const uint8_t*)d->st_status.p, (const int64_t*)d->st_spans.p,
                                                           cur < 0 ? nullptr : (const uint8_t*)col.utf8[cur].p, cur < 0 ? nullptr : (const int64_t*)col.off[cur].p,
                                                           cur < 0 ? 0 : col.n, d->n_keys, (uint8_t*)col.utf8[nxt].p, cap, (int64_t*)col.off[nxt].p, &total);
      if (mrc != OK) return dfail(d, mrc, std::string("keeping string column ") + std::to_string(c) + ": " + surge_replay_last_error(h));
      col.cur = nxt;
      col.n = d->n_keys;
      col.bytes = total;
    }
  }
  d->n_records = 0;  // (cleared whether or not a winner was refused: the call returns when the rows are written)
  d->val_bytes = 0;
  return rc == OK ? OK : dfail(d, rc, refused);
}

extern "C" {

int32_t surge_device_decoder_load_states(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl, int64_t counts_out[4]) {
  return load_states(d, h, tmpl, counts_out, false);
}

int32_t surge_device_decoder_load_protobuf_states(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* payload_tmpl,
                                                  int64_t counts_out[4]) {
  return load_states(d, h, payload_tmpl, counts_out, true);
}

int32_t surge_device_decoder_keep_strings(surge_device_decoder* d, int32_t on) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder holds no state values");
  if (d->state_loads != 0) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_strings comes before the first surge_device_decoder_load_states");
  d->keep_strings = on != 0;
  return OK;
}

int32_t surge_device_decoder_state_strings(surge_device_decoder* d, int32_t column, const uint8_t** d_utf8, const int64_t** d_off, int64_t* n_agg) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder holds no state values");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return dfail(d, E_INVALID, "string column out of range");
  const auto& col = d->str_cols[column];
  if (d_utf8) *d_utf8 = col.cur < 0 ? nullptr : (const uint8_t*)col.utf8[col.cur].p;
  if (d_off) *d_off = col.cur < 0 ? nullptr : (const int64_t*)col.off[col.cur].p;
  if (n_agg) *n_agg = col.cur < 0 ? 0 : col.n;
  return OK;
}

// result -> resident state: the composition a host would otherwise spell out (grow for the new keys, device group-by +
// fold, clear), behind one call so a JVM needs a single JNI crossing per poll
int32_t surge_replay_append_decoded(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out) {
  if (!h || !d) return dfail(d, E_INVALID, "NULL argument");
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder holds state values, not events: hand them over with surge_device_decoder_load_states");
  if (n_events_out) *n_events_out = d->n_records;
  if (n_keys_out) *n_keys_out = d->n_keys;
  int32_t rc = grow_for_keys(h, d);
  if (rc != OK) return rc;
  if (d->n_records > 0) {
    // the decoder's arrays are written on its stream and read on the handle's: make the hand-over explicit
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(d->device);
    const hipError_t e = wait_stream(d, d->stream);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return dfail(d, E_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    rc = surge_replay_append_events_device(h, (const int64_t*)d->r_agg.p, d->r_ev.p, d->n_records);
    if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
    if (d->block_waits) {  // (sleep until the fold is through, then let surge_replay_synchronize report what it has to)
      void* hs = nullptr;
      if (surge_replay_get_stream(h, &hs) == OK) {
        (void)hipSetDevice(d->device);
        (void)wait_stream(d, (hipStream_t)hs);
        (void)hipSetDevice(prev);
      }
    }
    rc = surge_replay_synchronize(h);  // the arrays are reused by the next push
    if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
  }
  d->n_records = 0;
  return OK;
}

int32_t surge_replay_append_decoded_async(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out) {
  return hand_over_async(h, d, n_events_out, n_keys_out, true);
}

int32_t surge_replay_stage_decoded(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out) {
  return hand_over_async(h, d, n_events_out, n_keys_out, false);
}

int32_t surge_device_decoder_clear(surge_device_decoder* d) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  d->n_records = 0;
  d->val_bytes = 0;
  return OK;
}

int32_t surge_device_decoder_keys(surge_device_decoder* d, uint8_t* utf8_out, int64_t utf8_capacity, int64_t* key_off_out, int64_t* n_keys_out,
                                  int64_t* utf8_bytes_out) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (n_keys_out) *n_keys_out = d->n_keys;
  if (utf8_bytes_out) *utf8_bytes_out = d->arena_bytes;
  if (!utf8_out && !key_off_out) return OK;  // size query
  if (utf8_capacity < d->arena_bytes) return dfail(d, E_INVALID, "utf8_out is too small (see *utf8_bytes_out)");
  int prev = 0;
  (void)hipGetDevice(&prev);
  struct Restore { int dev; ~Restore() { (void)hipSetDevice(dev); } } restore{prev};
  DCHK(d, hipSetDevice(d->device));
  DCHK(d, hipStreamSynchronize(d->stream));
  if (utf8_out && d->arena_bytes > 0) DCHK(d, hipMemcpy(utf8_out, d->arena.p, (size_t)d->arena_bytes, hipMemcpyDeviceToHost));
  if (key_off_out) DCHK(d, hipMemcpy(key_off_out, d->key_off.p, (size_t)(d->n_keys + 1) * 8, hipMemcpyDeviceToHost));
  return OK;
}

int32_t surge_device_decoder_key_table(surge_device_decoder* d, const uint8_t** d_utf8, const int64_t** d_key_off) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (d_utf8) *d_utf8 = (const uint8_t*)d->arena.p;
  if (d_key_off) *d_key_off = (const int64_t*)d->key_off.p;
  return OK;
}

int32_t surge_device_decoder_counters(const surge_device_decoder* d, int64_t out[4]) {
  if (!d || !out) return E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = d->counters[i];
  return OK;
}

int32_t surge_device_decoder_stats(const surge_device_decoder* d, int64_t out[8]) {
  if (!d || !out) return E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = d->counters[i];
  out[4] = d->reseeds;
  out[5] = (int64_t)d->t_cap;
  out[6] = d->pushes;
  out[7] = (int64_t)(d->seed & ~(1ull << 63));
  return OK;
}

}  // extern "C"
