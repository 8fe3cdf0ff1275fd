// state_decode_host.cpp — surge_decode_json_state / surge_decode_protobuf_state and their _lenient pair: one serialized state
// value (bare, or in the multilanguage module's protobuf State envelope) -> the fixed 64-byte state on the host, with
// the parser the device kernel runs (state_parse.h); surge_unescape_json_string: a STR span -> its string, likewise.  Plain C++ (no HIP): point reads of a state-topic record, the
// device decoder's re-parse of a Double it cannot decide, and the reference the device kernel is held to in the tests.
#include <cstring>

#include "state_parse.h"

static int32_t decode_state(const surge_json_template* tmpl, const uint8_t* value, int64_t len, const uint8_t* key, int64_t key_len,
                            void* state64_out, int64_t* str_span_out, bool envelope, bool lenient = false) {
  if (!state64_out || len < 0 || (!value && len > 0) || (!key && key_len > 0)) return SURGE_E_INVALID;
  if (surge::state_template_problem(tmpl)) return SURGE_E_INVALID;
  alignas(16) uint8_t row[64];
  int64_t span[2 * SURGE_JSON_STRING_COLUMNS] = {0};
  if (key_len < 0) key_len = -1;
  int rc;
  if (lenient) {
    surge::StateFieldTable tab;
    uint32_t bad_part = 0;
    if (surge::state_field_table(tmpl, &tab, &bad_part)) return SURGE_E_UNSUPPORTED;
    rc = envelope ? surge::state_parse_protobuf_state_lenient<true>(*tmpl, tab, value, len, key, key_len, surge::f64_parse_table_host(), row, span)
                  : surge::state_parse_json_lenient<true>(*tmpl, tab, value, len, key, key_len, surge::f64_parse_table_host(), row, span);
  } else {
    rc = envelope ? surge::state_parse_protobuf_state<true>(*tmpl, value, len, key, key_len, surge::f64_parse_table_host(), row, span)
                  : surge::state_parse_json<true>(*tmpl, value, len, key, key_len, surge::f64_parse_table_host(), row, span);
  }
  if (rc != SURGE_STATE_DECODE_OK) return rc;
  std::memcpy(state64_out, row, 64);
  if (str_span_out) std::memcpy(str_span_out, span, sizeof(span));
  return SURGE_STATE_DECODE_OK;
}

extern "C" int32_t surge_decode_json_state(const surge_json_template* tmpl, const uint8_t* value, int64_t len, const uint8_t* key,
                                           int64_t key_len, void* state64_out, int64_t* str_span_out) {
  return decode_state(tmpl, value, len, key, key_len, state64_out, str_span_out, false);
}

extern "C" int32_t surge_decode_protobuf_state(const surge_json_template* payload_tmpl, const uint8_t* value, int64_t len, const uint8_t* key,
                                               int64_t key_len, void* state64_out, int64_t* str_span_out) {
  return decode_state(payload_tmpl, value, len, key, key_len, state64_out, str_span_out, true);
}

extern "C" int32_t surge_decode_json_state_lenient(const surge_json_template* tmpl, const uint8_t* value, int64_t len, const uint8_t* key,
                                                   int64_t key_len, void* state64_out, int64_t* str_span_out) {
  return decode_state(tmpl, value, len, key, key_len, state64_out, str_span_out, false, true);
}

extern "C" int32_t surge_decode_protobuf_state_lenient(const surge_json_template* payload_tmpl, const uint8_t* value, int64_t len, const uint8_t* key,
                                                       int64_t key_len, void* state64_out, int64_t* str_span_out) {
  return decode_state(payload_tmpl, value, len, key, key_len, state64_out, str_span_out, true, true);
}

extern "C" int64_t surge_unescape_json_string(const uint8_t* raw, int64_t raw_len, uint8_t* out, int64_t capacity) {
  if (raw_len < 0 || (!raw && raw_len > 0)) return -(int64_t)SURGE_STATE_DECODE_STRING;
  int64_t n = 0;
  const int rc = surge::sp_unescape(raw, raw_len, nullptr, 0, &n);  // the length first: nothing is written unless all of it fits
  if (rc != SURGE_STATE_DECODE_OK) return -(int64_t)rc;
  if (out && capacity >= n) (void)surge::sp_unescape(raw, raw_len, out, n, &n);
  return n;
}
