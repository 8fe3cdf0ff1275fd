// ingest_handover.hip — the device decoder's hand-overs to a replay handle (ingest_decoder_internal.h): an events decoder's
// result arrays into the handle's fold or its staged log (surge_replay_append_decoded[_async], surge_replay_stage_decoded), a
// state decoder's values into the handle's resident state (surge_device_decoder_load_states, with the kept string columns).
#include <cstdlib>

#include "event_strings_parse.h"
#include "ingest_decoder_internal.h"

using namespace surge::ingest;
using namespace surge::ingest::host;

namespace {

// the resident state grows for the keys the decoder has interned
int32_t grow_for_keys(surge_replay_handle* h, surge_device_decoder* d) {
  void* d_states = nullptr;
  int64_t n_agg = 0;
  int32_t rc = surge_replay_device_state(h, &d_states, &n_agg);
  if (rc == OK && d->n_keys > n_agg) rc = surge_replay_grow(h, d->n_keys);
  return rc == OK ? OK : dfail(d, rc, surge_replay_last_error(h));
}

// what every hand-over of events begins with: the arguments, the decoder's mode, the counts the caller asked for, room for the new keys
int32_t begin_events_hand_over(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out, bool grow) {
  if (!h || !d) return dfail(d, E_INVALID, "NULL argument");
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder holds state values, not events: hand them over with surge_device_decoder_load_states");
  if (n_events_out) *n_events_out = d->n_records;
  if (n_keys_out) *n_keys_out = d->n_keys;
  return grow ? grow_for_keys(h, d) : OK;
}

int32_t handle_stream(surge_replay_handle* h, surge_device_decoder* d, void** hs) {
  const int32_t rc = surge_replay_get_stream(h, hs);
  return rc == OK ? OK : dfail(d, rc, surge_replay_last_error(h));
}

// the arrays are written on the decoder's stream and read on the handle's: that one waits (event) for this one
int32_t ready_for(surge_device_decoder* d, void* hs) {
  DCHK(d, hipEventRecord(d->ready, d->stream));
  DCHK(d, hipStreamWaitEvent((hipStream_t)hs, d->ready, 0));
  return OK;
}

// a consumer that folds on another stream than the decoder's adds a stream: stage 1 then rotates over one fewer (create_streams_and_events, ingest_decoder.hip)
void fold_stream_seen(surge_device_decoder* d, hipStream_t fold_stream) {
  if (d->push_streams_pinned || fold_stream == d->stream) return;
  std::lock_guard<std::mutex> lk(d->mu);
  if (d->n_push_active == d->n_push_streams && d->n_push_active > 2) d->n_push_active = d->n_push_streams - 1;
}

// The hand-over of the result arrays without a host wait on either side: the handle's stream waits (event) for the decoder's
// stream to have written the arrays, the group-by and the fold (fold = false: the copies into the handle's staged log) are
// enqueued behind that, and the next push_finish's stage 2 waits (event) for their last read before it writes the arrays
// again.  The host thread only ever waits in the middle of stage 2 (what the push discovered), so interning of fetch i + 1
// overlaps the fold of fetch i on the device.
int32_t hand_over_async(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out, bool fold) {
  int32_t rc = begin_events_hand_over(h, d, n_events_out, n_keys_out, fold);
  if (rc != OK) return rc;
  if (d->n_records > 0) {
    void* hs = nullptr;
    rc = handle_stream(h, d, &hs);
    if (rc != OK) return rc;
    DeviceScope scope(d->device);
    fold_stream_seen(d, (hipStream_t)hs);
    rc = ready_for(d, hs);
    if (rc != OK) return rc;
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

// the first record of a load that the decode refused, by its TOPIC offset (`fallback`: the handle's own words)
std::string name_refused(surge_device_decoder* d, const int64_t counts_out[4], std::string fallback) {
  std::vector<uint8_t> status((size_t)d->n_records);
  if (hipMemcpy(status.data(), d->st_status.p, status.size(), hipMemcpyDeviceToHost) == hipSuccess) {
    for (int64_t r = 0; r < d->n_records; ++r) {
      if (status[(size_t)r] == SURGE_STATE_DECODE_OK || status[(size_t)r] == SURGE_STATE_DECODE_SKIPPED) continue;
      int64_t offset = -1;
      if (hipMemcpy(&offset, (const int64_t*)d->r_off.p + r, 8, hipMemcpyDeviceToHost) == hipSuccess)
        fallback = std::to_string(counts_out[2]) + " state value(s) were refused (their rows are untouched), the first at topic offset " + std::to_string(offset) +
                   " (record " + std::to_string(r) + " of this load) with status " + std::to_string((int)status[(size_t)r]) + " (SURGE_STATE_DECODE_*); everything else was loaded";
      break;
    }
  }
  (void)hipGetLastError();
  return fallback;
}

// surge_device_decoder_keep_strings: the STR columns the template names, merged with what earlier loads kept (a refused
// winner keeps its earlier string, as it keeps its row: everything else is merged)
int32_t merge_kept_strings(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl) {
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
  return OK;
}

// state values -> resident state: what a KTable restore of the state topic does with the records it is handed
// (SurgeStateStoreConsumer.scala:69), behind one call.  envelope: the values are protobuf State messages around the
// template's text (surge_device_decoder_load_protobuf_states)
int32_t load_states(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl, int64_t counts_out[4], bool envelope) {
  if (!h || !d || !counts_out) return dfail(d, E_INVALID, "NULL argument");
  counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder hands over with surge_replay_append_decoded");
  int32_t rc = grow_for_keys(h, d);
  if (rc != OK) return rc;
  if (d->n_records == 0) return OK;
  void* hs = nullptr;
  rc = handle_stream(h, d, &hs);
  if (rc != OK) return rc;
  void* d_states = nullptr;
  int64_t n_agg = 0;
  rc = surge_replay_device_state(h, &d_states, &n_agg);
  if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
  DeviceScope scope(d->device);
  DCHK(d, d->st_status.reserve((size_t)d->n_records, false, d->stream));
  if (d->keep_strings) DCHK(d, d->st_spans.reserve((size_t)d->n_records * (2 * SURGE_JSON_STRING_COLUMNS) * 8, false, d->stream));
  rc = ready_for(d, hs);
  if (rc != OK) return rc;
  // (rows [0, n_keys): every aggregate index of the result is below the decoder's key count, and its key table has that many ids)
  rc = (envelope ? surge_replay_decode_protobuf_states : surge_replay_decode_json_states)(h, tmpl, (const uint8_t*)d->r_val.p, (const int64_t*)d->r_val_off.p, d->n_records, (const uint8_t*)d->arena.p,
                                       (const int64_t*)d->key_off.p, (const int64_t*)d->r_agg.p, d->n_keys, d_states, (uint8_t*)d->st_status.p,
                                       d->keep_strings ? (int64_t*)d->st_spans.p : nullptr, counts_out);
  if (rc != OK && rc != SURGE_E_CORRUPT) return dfail(d, rc, surge_replay_last_error(h));  // nothing was loaded: the records stay
  ++d->state_loads;
  std::string refused;
  if (rc == SURGE_E_CORRUPT) refused = name_refused(d, counts_out, surge_replay_last_error(h));  // everything else is loaded
  if (d->keep_strings) {
    const int32_t mrc = merge_kept_strings(d, h, tmpl);
    if (mrc != OK) return mrc;
  }
  d->n_records = 0;  // (cleared whether or not a winner was refused: the call returns when the rows are written)
  d->val_bytes = 0;
  return rc == OK ? OK : dfail(d, rc, refused);
}

}  // namespace

namespace {

// would the next merge write column c: a column the rule names or a state decoder kept, with records pending or ids interned since
bool column_merges(const surge_device_decoder* d, int c) {
  const auto& col = d->str_cols[c];
  if (!d->ev_named[c] && col.cur < 0) return false;
  return !(d->ev_pend_n == 0 && col.cur >= 0 && col.n == d->n_keys);
}

// the buffers the next merge of column c writes — the other one of the column's two — sized for it: n_keys + 1 offsets, and the
// bytes of the column so far plus those of the pending values (an unescaped string is never longer than its span, and the spans
// lie inside the pending values: the merge always fits)
int32_t reserve_next_column(surge_device_decoder* d, int c, int* nxt_out) {
  auto& col = d->str_cols[c];
  const int nxt = col.cur < 0 ? 0 : 1 - col.cur;
  DCHK(d, col.off[nxt].reserve((size_t)(d->n_keys + 1) * 8, false, d->stream));
  DCHK(d, col.utf8[nxt].reserve((size_t)(col.bytes + d->ev_pend_bytes + 16), false, d->stream));
  *nxt_out = nxt;
  return OK;
}

}  // namespace

// surge_device_decoder_keep_event_strings: what the pushes since the last merge selected goes into the columns — per named
// column one merge over the pending records with that column's statuses, the decoder's own previous column and n_agg = its key
// count — and what is pending is dropped.  A column that holds fewer aggregates than the key table (ids interned since) is
// brought up to it as well: the new ones are empty.  Columns a state decoder kept before it continued are merged into, not replaced.
int32_t surge::ingest::host::merge_event_strings(surge_device_decoder* d) {
  DeviceScope scope(d->device);
  hipStream_t st = d->stream;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
    auto& col = d->str_cols[c];
    if (!column_merges(d, c)) continue;
    const int cur = col.cur;
    int nxt = 0;
    const int32_t rrc = reserve_next_column(d, c, &nxt);
    if (rrc != OK) return rrc;
    DCHK(d, d->es_win.reserve((size_t)(d->n_keys + 1) * 8, false, st));
    DCHK(d, d->es_bad.reserve(8, false, st));
    DCHK(d, d->es_merge_totals.reserve((size_t)((d->n_keys + 1023) / 1024 + 1) * 8, false, st));
    const StringsColumn sc{cur < 0 ? nullptr : (const uint8_t*)col.utf8[cur].p, cur < 0 ? nullptr : (const int64_t*)col.off[cur].p, cur < 0 ? 0 : col.n,
                           (uint8_t*)col.utf8[nxt].p, (int64_t*)col.off[nxt].p};
    int64_t total = 0;
    DCHK(d, strings_merge_column(strings_pending_of(d), c, d->n_keys, sc, (unsigned long long*)d->es_win.p, (unsigned long long*)d->es_bad.p,
                                 (int64_t*)d->es_merge_totals.p, &total, st));
    col.cur = nxt;
    col.n = d->n_keys;
    col.bytes = total;
  }
  if (d->ev_pend_n > 0) ++d->ev_merges;
  d->ev_pend_n = 0;
  d->ev_pend_bytes = 0;
  return OK;
}

extern "C" {

int32_t surge_device_decoder_keep_event_strings(surge_device_decoder* d, const surge_event_strings* strings) {
  if (!d) return dfail(nullptr, E_INVALID, "decoder is NULL");
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder reads no events: arm it behind surge_device_decoder_continue_as_events");
  if (!d->json) return dfail(d, SURGE_E_STATE, "a decoder of 16-byte fixed events has no event template: its values carry no strings");
  if (d->ev_strings) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings was called before");
  if (d->push_seq != d->events_from_push) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings comes before the decoder's first push of events");
  if (surge_event_strings_validate(&d->h_tmpl, strings) != 0) return dfail(d, E_INVALID, surge_event_json_last_error());
  surge::EvsRule rule;
  (void)surge::evs_compile(&d->h_tmpl, strings, &rule);
  EvsTypes types{};
  bool named[SURGE_JSON_STRING_COLUMNS] = {};
  for (uint32_t e = 0; e < rule.n_entries; ++e) {
    const uint32_t type = rule.event_type[rule.entry_type[e]];
    bool known = false;
    for (uint32_t k = 0; k < types.n; ++k) known = known || types.type[k] == type;
    if (!known) types.type[types.n++] = type;
    named[rule.entry_column[e]] = true;
  }
  DeviceScope scope(d->device);
  DCHK(d, d->d_evs_rule.reserve(sizeof(rule), false, d->stream));
  DCHK(d, hipMemcpy(d->d_evs_rule.p, &rule, sizeof(rule), hipMemcpyHostToDevice));
  if (const char* v = std::getenv("SURGE_INGEST_EVENT_STRINGS_PENDING"))
    if (std::atoll(v) >= 0) d->ev_pend_bound = std::atoll(v);
  d->ev_types = types;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) d->ev_named[c] = named[c];
  d->ev_strings = true;
  return OK;
}

int32_t surge_device_decoder_event_strings_pending(surge_device_decoder* d, int64_t out[4], const uint8_t** d_values, const int64_t** d_value_off, const int64_t** d_rows) {
  if (!d || !out) return dfail(d, E_INVALID, "NULL argument");
  if (!d->ev_strings) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings has not armed this decoder");
  out[0] = d->ev_pend_n;
  out[1] = d->ev_pend_bytes;
  out[2] = (int64_t)d->ev_pend_val.cap;
  out[3] = d->ev_merges;
  if (d_values) *d_values = (const uint8_t*)d->ev_pend_val.p;
  if (d_value_off) *d_value_off = (const int64_t*)d->ev_pend_off.p;
  if (d_rows) *d_rows = (const int64_t*)d->ev_pend_rows.p;
  return OK;
}

int32_t surge_device_decoder_event_strings_next_column(surge_device_decoder* d, int32_t column, int64_t out[3], uint8_t** d_utf8, int64_t** d_off) {
  if (!d || !out) return dfail(d, E_INVALID, "NULL argument");
  if (!d->ev_strings) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings has not armed this decoder");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return dfail(d, E_INVALID, "string column out of range");
  out[0] = out[1] = 0;
  out[2] = d->n_keys;
  if (d_utf8) *d_utf8 = nullptr;
  if (d_off) *d_off = nullptr;
  if (!column_merges(d, column)) return OK;
  DeviceScope scope(d->device);
  int nxt = 0;
  const int32_t rc = reserve_next_column(d, column, &nxt);
  if (rc != OK) return rc;
  const auto& col = d->str_cols[column];
  out[0] = (int64_t)col.utf8[nxt].cap;
  out[1] = (int64_t)col.off[nxt].cap;
  if (d_utf8) *d_utf8 = (uint8_t*)col.utf8[nxt].p;
  if (d_off) *d_off = (int64_t*)col.off[nxt].p;
  return OK;
}

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
  if (!d->states && !d->continued && !d->ev_strings)
    return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder holds no state values");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return dfail(d, E_INVALID, "string column out of range");
  if (d->ev_strings) {  // the columns are asked for: what the pushes since the last merge kept goes into them
    const int32_t rc = merge_event_strings(d);
    if (rc != OK) return rc;
  }
  const auto& col = d->str_cols[column];
  if (d_utf8) *d_utf8 = col.cur < 0 ? nullptr : (const uint8_t*)col.utf8[col.cur].p;
  if (d_off) *d_off = col.cur < 0 ? nullptr : (const int64_t*)col.off[col.cur].p;
  if (n_agg) *n_agg = col.cur < 0 ? 0 : col.n;
  return OK;
}

// result -> resident state: the composition a host would otherwise spell out (grow for the new keys, device group-by +
// fold, clear), behind one call so a JVM needs a single JNI crossing per poll
int32_t surge_replay_append_decoded(surge_replay_handle* h, surge_device_decoder* d, int64_t* n_events_out, int64_t* n_keys_out) {
  int32_t rc = begin_events_hand_over(h, d, n_events_out, n_keys_out, true);
  if (rc != OK) return rc;
  if (d->n_records > 0) {
    // the decoder's arrays are written on its stream and read on the handle's: make the hand-over explicit
    hipError_t e;
    {
      DeviceScope scope(d->device);
      e = wait_stream(d, d->stream);
    }
    if (e != hipSuccess) return dfail(d, E_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    rc = surge_replay_append_events_device(h, (const int64_t*)d->r_agg.p, d->r_ev.p, d->n_records);
    if (rc != OK) return dfail(d, rc, surge_replay_last_error(h));
    if (d->block_waits) {  // (sleep until the fold is through, then let surge_replay_synchronize report what it has to)
      void* hs = nullptr;
      if (surge_replay_get_stream(h, &hs) == OK) {
        DeviceScope scope(d->device);
        (void)wait_stream(d, (hipStream_t)hs);
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

}  // extern "C"
