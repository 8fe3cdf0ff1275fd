// ingest_handover.hip — the device decoder's hand-overs to a replay handle (ingest_decoder_internal.h): an events decoder's
// result arrays into the handle's fold or its staged log (surge_replay_append_decoded[_async], surge_replay_stage_decoded), a
// state decoder's values into the handle's resident state (surge_device_decoder_load_states; the strings a load keeps are
// merged into their columns by ingest_columns.hip).
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
    const int32_t mrc = merge_state_strings(d, h, tmpl);  // (ingest_columns.hip)
    if (mrc != OK) return mrc;
  }
  d->n_records = 0;  // (cleared whether or not a winner was refused: the call returns when the rows are written)
  d->val_bytes = 0;
  return rc == OK ? OK : dfail(d, rc, refused);
}

}  // namespace

extern "C" {

int32_t surge_device_decoder_load_states(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl, int64_t counts_out[4]) {
  return load_states(d, h, tmpl, counts_out, false);
}

int32_t surge_device_decoder_load_protobuf_states(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* payload_tmpl,
                                                  int64_t counts_out[4]) {
  return load_states(d, h, payload_tmpl, counts_out, true);
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
