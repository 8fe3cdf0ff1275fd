// ingest_decoder.hip — SURVEY §8f N1 on the device: the records sections of Kafka record batches (message format v2,
// uncompressed or already decompressed by the host framer) -> (aggregate index, 16-byte event, offset) arrays and a key
// table, all resident in HBM, ready for surge_replay_append_events_device / a CSR build.  This unit is the host object
// (surge_device_decoder, ingest_decoder_internal.h): its lifecycle and options, the slot queue, the push exports, reserve,
// the results, clear, the switch from states to events, the counters and the pinned-memory helpers.  What a push does is
// ingest_stage1.hip and ingest_stage2.hip, what reads the key table between pushes ingest_reads.hip, the kept string columns
// ingest_columns.hip, the hand-overs to a replay handle ingest_handover.hip; the kernels and what launches them are the stage
// units ingest_crc / ingest_lz4 / ingest_records / ingest_intern / ingest_order / ingest_strings .hip (ingest_device.h).
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
// Between pushes the key table answers reads, by id and in key order (ingest_reads.hip).
#include <cstdio>
#include <cstdlib>

#include "ingest_decoder_internal.h"

using namespace surge::ingest;
using namespace surge::ingest::host;

namespace {

// ---- lifecycle ---------------------------------------------------------------------------------------------------------------
struct DecoderOptions {  // what the environment says about a decoder, read once at create
  int push_streams = 3;
  bool push_streams_pinned = false, normal_priority = false, block_waits = true, weak_hash = false;
  int64_t poll_ns = 10000;
};

DecoderOptions read_options() {
  DecoderOptions o;
  if (const char* v = std::getenv("SURGE_INGEST_PUSH_STREAMS")) {  // experiments: 5 = a stream per slot (round 4)
    o.push_streams = std::atoi(v);
    o.push_streams_pinned = true;
  }
  o.push_streams = o.push_streams < 1 ? 1 : (o.push_streams > kSlots ? kSlots : o.push_streams);
  if (const char* v = std::getenv("SURGE_INGEST_PUSH_PRIORITY")) o.normal_priority = std::strcmp(v, "normal") == 0;
  // A consumer thread that waits for the device a few times per fetch spins a core away in hipStreamSynchronize (0.4 - 1.2 ms of
  // CPU per 10^6-record fetch, and — on a host whose CPUs the framing threads need — 5 - 15 % of the bytes -> states rate:
  // profiles/r06_e2e_host_budget.jsonl).  The runtime's blocking wait (hipEventBlockingSync) still spins for its first few
  // hundred microseconds — most of a wait here — before it sleeps on the interrupt.  So the waits NAP: the event is queried
  // between nanosleeps of SURGE_INGEST_POLL_US (10) microseconds — the consumer thread's CPU 1.28 -> 0.81 ms per fetch at the
  // same rate (profiles/r06_e2e_wait_modes.txt).  SURGE_INGEST_WAIT=block sleeps on the blocking event, =spin keeps
  // hipStreamSynchronize.
  if (const char* v = std::getenv("SURGE_INGEST_WAIT")) {
    o.block_waits = std::strcmp(v, "spin") != 0;
    if (std::strcmp(v, "poll") != 0) o.poll_ns = 0;
  }
  if (o.poll_ns > 0)
    if (const char* u = std::getenv("SURGE_INGEST_POLL_US")) o.poll_ns = std::atoll(u) > 0 ? std::atoll(u) * 1000 : o.poll_ns;
  if (const char* v = std::getenv("SURGE_INGEST_DEBUG_WEAK_HASH")) o.weak_hash = v[0] == '1';
  return o;
}

// Stage 1 rotates over THREE streams — with the decoder's own stream that makes four, the hardware queues the runtime
// maps streams onto (GPU_MAX_HW_QUEUES).  A fifth stream shares a queue with another one, and a queue runs in order:
// with the fold on a stream of its own every third push's interning sat behind a later push's whole stage 1 (2 ms
// instead of 0.4: profiles/r06_e2e_consumer_waits_trace.txt).  So the hand-over calls (surge_replay_append_decoded_async,
// surge_replay_stage_decoded) take one stream out of the rotation when the handle folds on another stream than the
// decoder's.  Measured, fold on the decoder's stream: 3 streams 9.1 - 9.2e8, 2 streams 8.6 - 8.7e8 events/s
// (profiles/r06_e2e_push_streams.txt); fold on its own stream: 3 streams 6.9 - 7.3e8, 2 streams 8.3 - 8.7e8.  A fourth
// (low-priority) push stream: 6.8 - 7.0e8 with the 2.5 ms stalls back (profiles/r06_e2e_push_priority.txt).
int32_t create_streams_and_events(surge_device_decoder* d, const DecoderOptions& o) {
  d->push_streams_pinned = o.push_streams_pinned;
  for (int i = 0; i < o.push_streams; ++i) {
    // ... and at LOW priority: the runtime keeps a pool of hardware queues per priority, so the stage-1 streams cannot land on
    // the queue of the decoder's own stream or of the fold's whatever other streams the process has created (in bench.py's
    // default line, behind the legs that ran before it, one of three normal-priority push streams did: 7.4 instead of 9.1e8);
    // and stage 1 is the bulk work — interning and fold, the dependent chain, should win a tie (SURGE_INGEST_PUSH_PRIORITY=normal)
    int least = 0, greatest = 0;
    if (!o.normal_priority && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
      DCHK(d, hipStreamCreateWithPriority(&d->push_streams[i], hipStreamNonBlocking, least));
    else
      DCHK(d, hipStreamCreateWithFlags(&d->push_streams[i], hipStreamNonBlocking));
    d->n_push_streams = d->n_push_active = i + 1;
  }
  for (PushSlot& s : d->slots) {
    DCHK(d, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    DCHK(d, hipEventCreateWithFlags(&s.released, hipEventDisableTiming));
    DCHK(d, s.d_err.reserve(sizeof(ErrorCell), false, d->stream));
  }
  DCHK(d, hipEventCreateWithFlags(&d->ready, hipEventDisableTiming));
  DCHK(d, hipEventCreateWithFlags(&d->consumed, hipEventDisableTiming));
  return OK;
}

// the event template as the kernels use it (EvjDevice: the distinct field names, each once, and per type which of them it
// reads), to the device with the number parser's table
int32_t upload_template(surge_device_decoder* d, const surge_event_json_template* tmpl) {
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
  d->h_tmpl = *tmpl;  // (behind every refusal: a template that is not taken leaves the decoder as it was)
  DCHK(d, d->d_tmpl.reserve(sizeof(ev), false, d->stream));
  DCHK(d, hipMemcpy(d->d_tmpl.p, &ev, sizeof(ev), hipMemcpyHostToDevice));
  DCHK(d, d->d_ptab.reserve(sizeof(surge::F64ParseTable), false, d->stream));
  DCHK(d, hipMemcpy(d->d_ptab.p, surge::f64_parse_table_host(), sizeof(surge::F64ParseTable), hipMemcpyHostToDevice));
  return OK;
}

// on the decoder's device: streams, events, wait mode, template
int32_t decoder_init(surge_device_decoder* d, const DecoderOptions& o, const surge_event_json_template* tmpl) {
  const int32_t rc = create_streams_and_events(d, o);
  if (rc != OK) return rc;
  d->block_waits = o.block_waits;
  d->poll_ns = o.poll_ns;
  if (d->block_waits) DCHK(d, hipEventCreateWithFlags(&d->sleeper, hipEventDisableTiming | hipEventBlockingSync));
  DCHK(d, d->key_off.reserve(8, false, d->stream));
  DCHK(d, hipMemset(d->key_off.p, 0, 8));
  return tmpl ? upload_template(d, tmpl) : OK;
}

int32_t decoder_create(int32_t device_id, void* hip_stream, const surge_event_json_template* tmpl, bool states, surge_device_decoder** out) {
  if (!out) return dfail(nullptr, E_INVALID, "out is NULL");
  *out = nullptr;
  if (tmpl && surge_event_json_validate(tmpl) != 0) return dfail(nullptr, E_INVALID, std::string("event template: ") + surge_event_json_last_error());
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return dfail(nullptr, E_DEVICE, "no usable HIP device (the device decoder has no CPU fallback: use surge_ingest_drain_*)");
  if (device_id < 0 || device_id >= n_dev) return dfail(nullptr, E_INVALID, "device_id out of range");
  surge_device_decoder* d = new (std::nothrow) surge_device_decoder();
  if (!d) return dfail(nullptr, E_NOMEM, "out of host memory");
  const DecoderOptions o = read_options();
  d->device = device_id;
  d->stream = (hipStream_t)hip_stream;
  d->json = tmpl != nullptr;
  d->states = states;
  if (o.weak_hash) d->seed = 1ull << 63;  // test hook: the table's first hash function keeps 8 bits, so keys collide and the re-seed runs
  int32_t rc;
  {
    DeviceScope scope(device_id);
    rc = decoder_init(d, o, tmpl);
  }
  if (rc != OK) {
    surge_device_decoder_destroy(d);
    return rc;
  }
  *out = d;
  return OK;
}

// ---- the slot queue ------------------------------------------------------------------------------------------------------------
// the slot a new push's stage 1 goes into (nullptr with the error set: every slot holds an unfinished push)
PushSlot* claim_slot(surge_device_decoder* d, int32_t* rc) {
  if (d->poisoned) {
    *rc = refuse_poisoned(d);
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

// stage 1 is enqueued: the slot joins the queue
int32_t commit_slot(surge_device_decoder* d, PushSlot& s) {
  DCHK(d, hipEventRecord(s.done, s.stream));
  s.busy = true;
  std::lock_guard<std::mutex> lk(d->mu);
  ++d->n_pending;
  return OK;
}

// One push, up to where it waits in the queue: a slot, free of its last push, takes `stage1` (either kind: ingest_stage1.hip)
// and joins the queue.  A push that fails occupies no slot.  The caller has made the decoder's device current.
template <typename Stage1>
int32_t enqueue_push(surge_device_decoder* d, Stage1 stage1) {
  int32_t rc = OK;
  PushSlot* s = claim_slot(d, &rc);
  if (!s) return rc;
  rc = await_release(d, *s);
  if (rc != OK) return rc;
  rc = stage1(*s);
  if (rc != OK) {
    (void)hipStreamSynchronize(s->stream);  // whatever was enqueued before the failure reads host memory of this call
    return rc;
  }
  return commit_slot(d, *s);
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

void* pinned_alloc(size_t n) {
  void* p = nullptr;
  return hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void pinned_release(void* p) { (void)hipHostFree(p); }

}  // namespace

extern "C" {

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
  DeviceScope scope(d->device);
  (void)hipStreamSynchronize(d->stream);
  for (int i = 0; i < d->n_push_streams; ++i) {
    (void)hipStreamSynchronize(d->push_streams[i]);
    (void)hipStreamDestroy(d->push_streams[i]);
  }
  for (PushSlot& s : d->slots) {
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.released) (void)hipEventDestroy(s.released);
  }
  if (d->ready) (void)hipEventDestroy(d->ready);
  if (d->consumed) (void)hipEventDestroy(d->consumed);
  if (d->sleeper) (void)hipEventDestroy(d->sleeper);
  delete d;  // every buffer, device and page-locked, is freed by its owner here: while the decoder's device is still current
  return OK;
}

int32_t surge_device_decoder_push_parts_floored_async(surge_device_decoder* d, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                                                      const int64_t* n_sections, int64_t n_floors, const surge_section_floor* floors) {
  if (!d) return refuse_null_decoder();
  if (n_parts < 0 || (n_parts > 0 && (!bytes || !sections || !n_sections)) || n_floors < 0 || (n_floors > 0 && !floors)) return dfail(d, E_INVALID, "bad argument");
  DeviceScope scope(d->device);
  return enqueue_push(d, [&](PushSlot& s) { return stage1_wire(d, s, n_parts, bytes, sections, n_sections, n_floors, floors); });
}

int32_t surge_device_decoder_push_parts_async(surge_device_decoder* d, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                                              const int64_t* n_sections) {
  return surge_device_decoder_push_parts_floored_async(d, n_parts, bytes, sections, n_sections, 0, nullptr);
}

int32_t surge_device_decoder_push_async(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections) {
  return surge_device_decoder_push_parts_async(d, 1, &bytes, &sections, &n_sections);
}

int32_t surge_device_decoder_push_finish(surge_device_decoder* d) {
  if (!d) return refuse_null_decoder();
  DeviceScope scope(d->device);
  return finish_oldest(d, true);
}

int32_t surge_device_decoder_push_finish_async(surge_device_decoder* d) {
  if (!d) return refuse_null_decoder();
  DeviceScope scope(d->device);
  return finish_oldest(d, false);
}

int32_t surge_device_decoder_pending(const surge_device_decoder* d) {
  if (!d) return 0;
  std::lock_guard<std::mutex> lk(const_cast<surge_device_decoder*>(d)->mu);
  return d->n_pending;
}

int32_t surge_device_decoder_reserve(surge_device_decoder* d, int64_t n_keys, int64_t key_bytes) {
  if (!d) return refuse_null_decoder();
  if (n_keys < 0 || key_bytes < 0) return dfail(d, E_INVALID, "negative capacity");
  if (d->n_pending != 0) return refuse_pending(d);
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

int32_t surge_device_decoder_push_floored(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections, int64_t n_floors,
                                          const surge_section_floor* floors) {
  if (!d) return refuse_null_decoder();
  if (n_sections < 0 || (n_sections > 0 && (!bytes || !sections))) return dfail(d, E_INVALID, "bad argument");
  if (d->n_pending != 0) return refuse_pending(d, kPushOrder);
  if (n_sections == 0) return OK;
  const int32_t rc = surge_device_decoder_push_parts_floored_async(d, 1, &bytes, &sections, &n_sections, n_floors, floors);
  return rc != OK ? rc : surge_device_decoder_push_finish(d);
}

int32_t surge_device_decoder_push(surge_device_decoder* d, const uint8_t* bytes, const surge_batch_section* sections, int64_t n_sections) {
  return surge_device_decoder_push_floored(d, bytes, sections, n_sections, 0, nullptr);
}

// A state decoder that has loaded its topic goes on as the events decoder of the same aggregates: the key table stays where it
// is — its ids are the resident state's rows — and only what names the mode changes.
int32_t surge_device_decoder_continue_as_events(surge_device_decoder* d, const surge_event_json_template* tmpl) {
  if (!d) return refuse_null_decoder();
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder is one already, and the switch is one-way");
  if (d->n_pending != 0) return refuse_pending(d, kFinishAndLoad);
  if (d->n_records != 0) return dfail(d, SURGE_E_STATE, "delivered state records are waiting: load them (surge_device_decoder_load_states) or clear them first");
  if (d->poisoned) return refuse_poisoned(d);
  if (tmpl && surge_event_json_validate(tmpl) != 0) return dfail(d, E_INVALID, std::string("event template: ") + surge_event_json_last_error());
  DeviceScope scope(d->device);
  DCHK(d, hipStreamSynchronize(d->stream));  // (the last load read the value buffers on the handle's stream behind an event of this one; it has returned)
  if (tmpl) {
    const int32_t rc = upload_template(d, tmpl);  // (the decoder is a state decoder still if this fails)
    if (rc != OK) return rc;
  }
  for (surge_device_decoder::Buf* b : {&d->r_val, &d->r_val_off, &d->vlen, &d->vscan, &d->val_src, &d->long_runs, &d->st_status, &d->st_spans}) b->release();
  d->val_bytes = 0;
  d->json = tmpl != nullptr;
  d->states = false;
  d->continued = true;
  d->events_from_push = d->push_seq;
  return OK;
}

// Stage 1 of a push of framed records on the next free slot.  stage1_records copies the caller's arrays into the slot's
// page-locked staging before it returns, so — unlike a wire push — nothing of the caller's is read behind this call.
int32_t surge_device_decoder_push_records_async(surge_device_decoder* d, const uint8_t* keys, const int64_t* key_off, const uint8_t* values,
                                                const int64_t* value_off, const int64_t* offsets, int64_t n) {
  if (!d) return refuse_null_decoder();
  if (n < 0 || (n > 0 && (!key_off || !value_off))) return dfail(d, E_INVALID, "bad argument");
  if (n == 0) return OK;  // (no slot: there is nothing to finish)
  DeviceScope scope(d->device);
  return enqueue_push(d, [&](PushSlot& s) { return stage1_records(d, s, keys, key_off, values, value_off, offsets, n); });
}

int32_t surge_device_decoder_push_records(surge_device_decoder* d, const uint8_t* keys, const int64_t* key_off, const uint8_t* values,
                                          const int64_t* value_off, const int64_t* offsets, int64_t n) {
  if (!d) return refuse_null_decoder();
  if (n < 0 || (n > 0 && (!key_off || !value_off))) return dfail(d, E_INVALID, "bad argument");
  if (d->n_pending != 0) return refuse_pending(d, kPushOrder);
  if (n == 0) return OK;
  const int32_t rc = surge_device_decoder_push_records_async(d, keys, key_off, values, value_off, offsets, n);
  return rc != OK ? rc : surge_device_decoder_push_finish(d);
}

int32_t surge_device_decoder_result(surge_device_decoder* d, int64_t* n_records, const int64_t** d_agg_idx, const void** d_events16,
                                    const int64_t** d_offsets, int64_t* n_keys) {
  if (!d) return refuse_null_decoder();
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
  if (!d) return refuse_null_decoder();
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): see surge_device_decoder_result");
  if (n_records) *n_records = d->n_records;
  if (d_agg_idx) *d_agg_idx = (const int64_t*)d->r_agg.p;
  if (d_values) *d_values = (const uint8_t*)d->r_val.p;
  if (d_value_off) *d_value_off = (const int64_t*)d->r_val_off.p;
  if (d_offsets) *d_offsets = (const int64_t*)d->r_off.p;
  if (n_keys) *n_keys = d->n_keys;
  return OK;
}

int32_t surge_device_decoder_clear(surge_device_decoder* d) {
  if (!d) return refuse_null_decoder();
  d->n_records = 0;
  d->val_bytes = 0;
  d->strings.ev.drop_pending();  // (ingest_columns.hip: what was kept and not merged goes with the records)
  return OK;
}

int32_t surge_device_decoder_counters(const surge_device_decoder* d, int64_t out[4]) {
  if (!d || !out) return E_INVALID;
  for (int i = 0; i < 4; ++i) out[i] = d->counters[i];
  return OK;
}

int32_t surge_device_decoder_below_floor(const surge_device_decoder* d, int64_t* n_out) {
  if (!d || !n_out) return E_INVALID;
  *n_out = d->below_floor;
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

int32_t surge_device_decoder_route_stats(const surge_device_decoder* d, int64_t out[2]) {
  if (!d || !out) return E_INVALID;
  out[0] = d->snappy_device_chunks;
  out[1] = d->snappy_host_sections;
  return OK;
}

}  // extern "C"
