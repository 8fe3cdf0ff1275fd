// ingest_columns.hip — the host side of the device decoder's kept string columns (ingest_decoder_internal.h, StringsState):
// a state decoder's (surge_device_decoder_keep_strings: every load merges the STR columns its template names,
// merge_state_strings) and an events decoder's (surge_device_decoder_keep_event_strings: arming the rule, and
// merge_event_strings over what stage 2 left pending; the kernels are ingest_strings.hip's), read through
// surge_device_decoder_state_strings.  Both merges write a column by StrColumn's one rule: the other buffer, sized for the
// merge, then the flip.
#include <cstdlib>

#include "event_strings_parse.h"
#include "ingest_decoder_internal.h"

using namespace surge::ingest;
using namespace surge::ingest::host;

namespace {

// would the next merge write column c: a column the rule names or a state decoder kept, with records pending or ids interned since
bool column_merges(const surge_device_decoder* d, int c) {
  const StrColumn& col = d->strings.col[c];
  const EventStringsState& ev = d->strings.ev;
  if (!ev.named[c] && col.cur < 0) return false;
  return !(ev.pend.n == 0 && col.cur >= 0 && col.n == d->n_keys);
}

}  // namespace

// surge_device_decoder_keep_strings: the STR columns the template names, merged with what earlier loads kept (a refused
// winner keeps its earlier string, as it keeps its row: everything else is merged).  What comes in are the load's values.
int32_t surge::ingest::host::merge_state_strings(surge_device_decoder* d, surge_replay_handle* h, const surge_json_template* tmpl) {
  bool named[SURGE_JSON_STRING_COLUMNS] = {};
  for (uint32_t i = 0; i < tmpl->n_parts; ++i)
    if (tmpl->part[i].kind == SURGE_JP_STR && tmpl->part[i].field_offset < SURGE_JSON_STRING_COLUMNS) named[tmpl->part[i].field_offset] = true;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
    if (!named[c]) continue;
    StrColumn& col = d->strings.col[c];
    const int nxt = col.next();
    DCHK(d, col.reserve_next(d->n_keys, d->val_bytes, d->stream));
    int64_t total = 0;
    const int32_t mrc = surge_replay_merge_state_strings(h, c, (const uint8_t*)d->r_val.p, (const int64_t*)d->r_val_off.p, d->n_records, (const int64_t*)d->r_agg.p,
                                                         (const uint8_t*)d->st_status.p, (const int64_t*)d->st_spans.p, col.cur_utf8(), col.cur_off(), col.cur_n(), d->n_keys,
                                                         (uint8_t*)col.utf8[nxt].p, col.next_capacity(d->val_bytes), (int64_t*)col.off[nxt].p, &total);
    if (mrc != OK) return dfail(d, mrc, std::string("keeping string column ") + std::to_string(c) + ": " + surge_replay_last_error(h));
    col.flip(d->n_keys, total);
  }
  return OK;
}

// surge_device_decoder_keep_event_strings: what the pushes since the last merge selected goes into the columns — per named
// column one merge over the pending records with that column's statuses, the decoder's own previous column and n_agg = its key
// count — and what is pending is dropped.  A column that holds fewer aggregates than the key table (ids interned since) is
// brought up to it as well: the new ones are empty.  Columns a state decoder kept before it continued are merged into, not
// replaced.  What comes in are the pending values.
int32_t surge::ingest::host::merge_event_strings(surge_device_decoder* d) {
  DeviceScope scope(d->device);
  hipStream_t st = d->stream;
  EventStringsState& ev = d->strings.ev;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
    if (!column_merges(d, c)) continue;
    StrColumn& col = d->strings.col[c];
    const int nxt = col.next();
    DCHK(d, col.reserve_next(d->n_keys, ev.pend.bytes, st));
    DCHK(d, ev.merge.win.reserve((size_t)(d->n_keys + 1) * 8, false, st));
    DCHK(d, ev.merge.bad.reserve(8, false, st));
    DCHK(d, ev.merge.totals.reserve((size_t)((d->n_keys + 1023) / 1024 + 1) * 8, false, st));
    const StringsColumn sc{col.cur_utf8(), col.cur_off(), col.cur_n(), (uint8_t*)col.utf8[nxt].p, (int64_t*)col.off[nxt].p};
    int64_t total = 0;
    DCHK(d, strings_merge_column(ev.pending(), c, d->n_keys, sc, (unsigned long long*)ev.merge.win.p, (unsigned long long*)ev.merge.bad.p, (int64_t*)ev.merge.totals.p,
                                 &total, st));
    col.flip(d->n_keys, total);
  }
  if (ev.pend.n > 0) ++ev.merge.count;
  ev.drop_pending();
  return OK;
}

extern "C" {

int32_t surge_device_decoder_keep_event_strings(surge_device_decoder* d, const surge_event_strings* strings) {
  if (!d) return refuse_null_decoder();
  EventStringsState& ev = d->strings.ev;
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder reads no events: arm it behind surge_device_decoder_continue_as_events");
  if (!d->json) return dfail(d, SURGE_E_STATE, "a decoder of 16-byte fixed events has no event template: its values carry no strings");
  if (ev.armed) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings was called before");
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
  DCHK(d, ev.rule.reserve(sizeof(rule), false, d->stream));
  DCHK(d, hipMemcpy(ev.rule.p, &rule, sizeof(rule), hipMemcpyHostToDevice));
  if (const char* v = std::getenv("SURGE_INGEST_EVENT_STRINGS_PENDING"))
    if (std::atoll(v) >= 0) ev.pend.bound = std::atoll(v);
  ev.types = types;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) ev.named[c] = named[c];
  ev.armed = true;
  return OK;
}

int32_t surge_device_decoder_event_strings_pending(surge_device_decoder* d, int64_t out[4], const uint8_t** d_values, const int64_t** d_value_off, const int64_t** d_rows) {
  if (!d || !out) return dfail(d, E_INVALID, "NULL argument");
  const EventStringsState& ev = d->strings.ev;
  if (!ev.armed) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings has not armed this decoder");
  out[0] = ev.pend.n;
  out[1] = ev.pend.bytes;
  out[2] = (int64_t)ev.pend.val.cap;
  out[3] = ev.merge.count;
  if (d_values) *d_values = (const uint8_t*)ev.pend.val.p;
  if (d_value_off) *d_value_off = (const int64_t*)ev.pend.off.p;
  if (d_rows) *d_rows = (const int64_t*)ev.pend.rows.p;
  return OK;
}

int32_t surge_device_decoder_event_strings_next_column(surge_device_decoder* d, int32_t column, int64_t out[3], uint8_t** d_utf8, int64_t** d_off) {
  if (!d || !out) return dfail(d, E_INVALID, "NULL argument");
  if (!d->strings.ev.armed) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_event_strings has not armed this decoder");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return dfail(d, E_INVALID, "string column out of range");
  out[0] = out[1] = 0;
  out[2] = d->n_keys;
  if (d_utf8) *d_utf8 = nullptr;
  if (d_off) *d_off = nullptr;
  if (!column_merges(d, column)) return OK;
  DeviceScope scope(d->device);
  StrColumn& col = d->strings.col[column];
  const int nxt = col.next();
  DCHK(d, col.reserve_next(d->n_keys, d->strings.ev.pend.bytes, d->stream));
  out[0] = (int64_t)col.utf8[nxt].cap;
  out[1] = (int64_t)col.off[nxt].cap;
  if (d_utf8) *d_utf8 = (uint8_t*)col.utf8[nxt].p;
  if (d_off) *d_off = (int64_t*)col.off[nxt].p;
  return OK;
}

int32_t surge_device_decoder_keep_strings(surge_device_decoder* d, int32_t on) {
  if (!d) return refuse_null_decoder();
  if (!d->states) return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder holds no state values");
  if (d->state_loads != 0) return dfail(d, SURGE_E_STATE, "surge_device_decoder_keep_strings comes before the first surge_device_decoder_load_states");
  d->keep_strings = on != 0;
  return OK;
}

int32_t surge_device_decoder_state_strings(surge_device_decoder* d, int32_t column, const uint8_t** d_utf8, const int64_t** d_off, int64_t* n_agg) {
  if (!d) return refuse_null_decoder();
  if (!d->states && !d->continued && !d->strings.ev.armed)
    return dfail(d, SURGE_E_STATE, "not a state decoder (surge_device_decoder_create_states): an events decoder holds no state values");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return dfail(d, E_INVALID, "string column out of range");
  if (d->strings.ev.armed) {  // the columns are asked for: what the pushes since the last merge kept goes into them
    const int32_t rc = merge_event_strings(d);
    if (rc != OK) return rc;
  }
  const StrColumn& col = d->strings.col[column];
  if (d_utf8) *d_utf8 = col.cur_utf8();
  if (d_off) *d_off = col.cur_off();
  if (n_agg) *n_agg = col.cur_n();
  return OK;
}

}  // extern "C"
