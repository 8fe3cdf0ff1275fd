// event_strings_parse.h — the string fields of one event value (include/surge_ingest.h, "the STRING fields of events"): one
// text for the host export (surge_event_json_string_spans, event_decode.cpp) and the device pass (ingest_strings.hip),
// the way state_parse.h is one text for the state decoders.
//
// The walk is event_decode.cpp's scan of the top-level object, restated without its field array: optional white space, '{',
// fields `"name" : value` separated by ',', '}', optional white space, nothing else.  A name or a string runs to the next
// quote that no backslash stands in front of; a number is -?[0-9.eE+-]* with a digit; anything else is skipped with its
// nesting.  The first 24 fields whose NAME holds no backslash are the fields; everything else is walked and not looked at.
// Two passes over them: the class — the LAST field named like the discriminator, a string without a backslash that is a type's
// name, first type first (no discriminator: type 0) — then, for every entry of that class, the FIRST string-valued field of
// the entry's name, whose bytes between the quotes must pass sp_unescape.  Nothing at or beyond v + len is read; nothing but
// span[0 .. 8) and status[0 .. 4) is written.
#pragma once
#include <stdint.h>

#include "../../include/surge_ingest.h"
#include "state_parse.h"

namespace surge {

constexpr int kEvsFields = 24;  // event_decode.cpp's kMaxFields

// template + strings as the walk reads them (plain data: the device gets a copy)
struct EvsRule {
  uint32_t n_types, n_entries, envelope, disc_len;
  char disc[SURGE_EVJ_NAME];
  char type_name[SURGE_EVJ_MAX_TYPES][SURGE_EVJ_NAME];
  uint8_t type_name_len[SURGE_EVJ_MAX_TYPES];
  uint32_t event_type[SURGE_EVJ_MAX_TYPES];
  uint8_t entry_type[SURGE_EVS_MAX], entry_column[SURGE_EVS_MAX], entry_field_len[SURGE_EVS_MAX];
  char entry_field[SURGE_EVS_MAX][SURGE_EVJ_NAME];
};

SURGE_HD bool evs_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// a string whose opening quote is v[*i]: the span between the quotes, whether a backslash stands in it
SURGE_HD bool evs_string(const uint8_t* v, int64_t len, int64_t* i, int64_t* off, int64_t* n, bool* escaped) {
  int64_t p = *i;
  if (p >= len || v[p] != '"') return false;
  ++p;
  *off = p;
  *escaped = false;
  while (p < len && v[p] != '"') {
    if (v[p] == '\\') {
      *escaped = true;
      ++p;
      if (p >= len) return false;
    }
    ++p;
  }
  if (p >= len) return false;
  *n = p - *off;
  *i = p + 1;
  return true;
}

SURGE_HD bool evs_number(const uint8_t* v, int64_t len, int64_t* i) {
  int64_t p = *i;
  if (p < len && (v[p] == '-' || v[p] == '+')) ++p;
  bool digits = false;
  while (p < len && ((v[p] >= '0' && v[p] <= '9') || v[p] == '.' || v[p] == 'e' || v[p] == 'E' || v[p] == '+' || v[p] == '-')) {
    digits = digits || (v[p] >= '0' && v[p] <= '9');
    ++p;
  }
  *i = p;
  return digits;
}

// one value of any other kind (containers by depth, strings honoured)
SURGE_HD bool evs_skip(const uint8_t* v, int64_t len, int64_t* i) {
  int64_t p = *i, o = 0, n = 0;
  bool e = false;
  if (p >= len) return false;
  if (v[p] == '{' || v[p] == '[') {
    int depth = 0;
    while (p < len) {
      if (v[p] == '"') {
        if (!evs_string(v, len, &p, &o, &n, &e)) return false;
        continue;
      }
      if (v[p] == '{' || v[p] == '[') ++depth;
      if (v[p] == '}' || v[p] == ']') {
        --depth;
        if (depth == 0) { *i = p + 1; return true; }
      }
      ++p;
    }
    return false;
  }
  if (v[p] == 't' || v[p] == 'f' || v[p] == 'n') {
    while (p < len && v[p] >= 'a' && v[p] <= 'z') ++p;
    *i = p;
    return true;
  }
  const bool ok = evs_number(v, len, &p);
  *i = p;
  return ok;
}

SURGE_HD bool evs_name_is(const char* want, uint32_t want_len, const uint8_t* got, int64_t got_len) {
  if ((int64_t)want_len != got_len) return false;
  for (uint32_t b = 0; b < want_len; ++b)
    if ((uint8_t)want[b] != got[b]) return false;
  return true;
}

// The walk over the object v[0 .. len).  CLASS: *cls = the type the discriminator selects (-1: none such); else: span / status
// of the entries of class *cls.  false: not the object the event decoder reads.
template <bool CLASS>
SURGE_HD bool evs_walk(const EvsRule& t, const uint8_t* v, int64_t len, int* cls, int64_t* span, uint8_t* status) {
  int64_t i = 0;
  while (i < len && evs_ws(v[i])) ++i;
  if (i >= len || v[i] != '{') return false;
  ++i;
  int nf = 0;
  bool disc_seen = false, disc_string = false;
  int64_t disc_off = 0, disc_n = 0;
  while (i < len && evs_ws(v[i])) ++i;
  if (i < len && v[i] == '}') {
    ++i;
  } else {
    for (;;) {
      while (i < len && evs_ws(v[i])) ++i;
      int64_t name_off = 0, name_n = 0, str_off = 0, str_n = 0;
      bool name_esc = false, str_esc = false, is_str = false;
      if (!evs_string(v, len, &i, &name_off, &name_n, &name_esc)) return false;
      while (i < len && evs_ws(v[i])) ++i;
      if (i >= len || v[i] != ':') return false;
      ++i;
      while (i < len && evs_ws(v[i])) ++i;
      if (i >= len) return false;
      if (v[i] == '"') {
        if (!evs_string(v, len, &i, &str_off, &str_n, &str_esc)) return false;
        is_str = true;
      } else if (v[i] == '-' || (v[i] >= '0' && v[i] <= '9')) {
        if (!evs_number(v, len, &i)) return false;
      } else if (!evs_skip(v, len, &i)) {
        return false;
      }
      if (!name_esc && nf < kEvsFields) {
        ++nf;
        if (CLASS) {
          if (evs_name_is(t.disc, t.disc_len, v + name_off, name_n)) {  // the last one decides, whatever its kind
            disc_seen = true;
            disc_string = is_str && !str_esc;
            disc_off = str_off;
            disc_n = str_n;
          }
        } else if (is_str) {
          for (uint32_t e = 0; e < t.n_entries; ++e) {
            const uint32_t c = t.entry_column[e];
            if ((int)t.entry_type[e] != *cls || status[c] != SURGE_EVENT_STRING_MISSING) continue;
            if (!evs_name_is(t.entry_field[e], t.entry_field_len[e], v + name_off, name_n)) continue;
            int64_t unescaped = 0;
            span[2 * c] = str_off;
            span[2 * c + 1] = str_n;
            status[c] = (uint8_t)sp_unescape(v + str_off, str_n, nullptr, 0, &unescaped);
          }
        }
      }
      while (i < len && evs_ws(v[i])) ++i;
      if (i < len && v[i] == ',') { ++i; continue; }
      if (i < len && v[i] == '}') { ++i; break; }
      return false;
    }
  }
  while (i < len && evs_ws(v[i])) ++i;
  if (i != len) return false;
  if (CLASS) {
    *cls = -1;
    if (t.disc_len == 0) {
      *cls = 0;
    } else if (disc_seen && disc_string) {
      for (uint32_t k = 0; k < t.n_types && *cls < 0; ++k)
        if (evs_name_is(t.type_name[k], t.type_name_len[k], v + disc_off, disc_n)) *cls = (int)k;
    }
  }
  return true;
}

// One record value by the rule.  span: 2 x SURGE_JSON_STRING_COLUMNS {offset into v, length}; status: one byte per column.
// Returns SURGE_EVENT_STRING_OK, or the first refusal in column order (every column _RECORD for a value that is no event).
SURGE_HD int evs_string_spans(const EvsRule& t, const uint8_t* v, int64_t len, int64_t* span, uint8_t* status) {
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
    span[2 * c] = span[2 * c + 1] = 0;
    status[c] = SURGE_EVENT_STRING_RECORD;
  }
  int64_t pay_off = 0, pay_len = len;
  if (t.envelope == SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT) {
    int64_t id_off = 0, id_len = 0;
    if (sp_envelope_spans(v, len, &id_off, &id_len, &pay_off, &pay_len) != SURGE_STATE_DECODE_OK) return SURGE_EVENT_STRING_RECORD;
  }
  int cls = -1;
  if (!evs_walk<true>(t, v + pay_off, pay_len, &cls, span, status) || cls < 0) return SURGE_EVENT_STRING_RECORD;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) status[c] = SURGE_EVENT_STRING_ABSENT;
  bool any = false;
  for (uint32_t e = 0; e < t.n_entries; ++e)
    if ((int)t.entry_type[e] == cls) {
      status[t.entry_column[e]] = SURGE_EVENT_STRING_MISSING;
      any = true;
    }
  if (!any) return SURGE_EVENT_STRING_OK;
  (void)evs_walk<false>(t, v + pay_off, pay_len, &cls, span, status);  // (the same text walked once more: it cannot fail now)
  int first = SURGE_EVENT_STRING_OK;
  for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {
    if (status[c] == SURGE_EVENT_STRING_OK) span[2 * c] += pay_off;
    else if (status[c] != SURGE_EVENT_STRING_ABSENT && first == SURGE_EVENT_STRING_OK) first = status[c];
  }
  return first;
}

// template + strings -> the rule (host).  nullptr = usable, `out` (nullable) filled; else what surge_event_strings_validate
// refuses.  The template has passed surge_event_json_validate.
inline const char* evs_compile(const surge_event_json_template* tmpl, const surge_event_strings* s, EvsRule* out) {
  if (!tmpl || !s) return "NULL argument";
  if (s->n < 1 || s->n > SURGE_EVS_MAX) return "strings.n out of range";
  EvsRule r{};
  r.n_types = tmpl->n_types;
  r.n_entries = s->n;
  r.envelope = tmpl->envelope;
  for (r.disc_len = 0; r.disc_len < SURGE_EVJ_NAME && tmpl->discriminator[r.disc_len]; ++r.disc_len) r.disc[r.disc_len] = tmpl->discriminator[r.disc_len];
  for (uint32_t k = 0; k < tmpl->n_types; ++k) {
    uint32_t n = 0;
    for (; n < SURGE_EVJ_NAME && tmpl->types[k].name[n]; ++n) r.type_name[k][n] = tmpl->types[k].name[n];
    r.type_name_len[k] = (uint8_t)n;
    r.event_type[k] = tmpl->types[k].event_type;
  }
  for (uint32_t e = 0; e < s->n; ++e) {
    const surge_event_string_field& f = s->entry[e];
    uint32_t tn = 0, fn = 0;
    while (tn < SURGE_EVJ_NAME && f.type_name[tn]) ++tn;
    while (fn < SURGE_EVJ_NAME && f.field[fn]) ++fn;
    if (tn == SURGE_EVJ_NAME || fn == SURGE_EVJ_NAME) return "a name is not NUL-terminated";
    if (fn == 0) return "an empty field name";
    if (f.column >= SURGE_JSON_STRING_COLUMNS) return "a string column out of range";
    int type = -1;
    for (uint32_t k = 0; k < tmpl->n_types && type < 0; ++k)
      if (evs_name_is(r.type_name[k], r.type_name_len[k], (const uint8_t*)f.type_name, tn)) type = (int)k;
    if (type < 0) return "a type name the event template does not have";
    for (uint32_t q = 0; q < e; ++q)
      if (r.entry_type[q] == type && r.entry_column[q] == f.column) return "the same (type, column) named twice";
    r.entry_type[e] = (uint8_t)type;
    r.entry_column[e] = (uint8_t)f.column;
    r.entry_field_len[e] = (uint8_t)fn;
    for (uint32_t b = 0; b < fn; ++b) r.entry_field[e][b] = f.field[b];
  }
  if (out) *out = r;
  return nullptr;
}

}  // namespace surge
