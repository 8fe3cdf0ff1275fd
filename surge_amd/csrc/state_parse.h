// state_parse.h — one serialized state value (the text the state encoders write, include/surge_replay.h) -> the fixed
// 64-byte state, on the host and on the device (same code): the inverse of json_encode_kernel (state_kernels.hip).
//
// What is parsed: compact play-json, `Json.toJson(state).toString()` over a `Json.format` case-class format
// (TestBoundedContext.scala:127-129, BankAccountSurgeModel.scala:26-28) — the fields in case-class order with nothing
// between the tokens, exactly the text a surge_json_template describes.  The parser walks the template's parts in order;
// anything else is refused with a status that names the part kind that did not match, never guessed at:
//   LITERAL            the bytes must match
//   KEY                a JSON string; with a key given, its unescaped bytes must be the aggregate's id
//   STR                a JSON string; validated, its still-escaped span (offset, length between the quotes) reported —
//                      sp_unescape turns such a span into the string (state_strings.hip keeps them as side columns)
//   I32 / U32 / I64    -?[0-9]+ and nothing of a decimal after it (the event decoder's integer rule, event_decode.cpp),
//                      inside the field's range — a value outside it is reported, never wrapped
//   F64                f64_parse_json_number (f64_parse.h): correctly rounded, or AMBIGUOUS for the caller to settle
// Strings: every byte below 0x20 must be escaped (Jackson writes them as \u00XX and refuses them raw); the escapes are
// \" \\ \/ \b \f \n \r \t and \uXXXX for a code point outside the surrogate range, unescaped to UTF-8.  Bytes from 0x80
// on are taken as they are (the id is compared byte for byte).
// The parser never reads at or beyond value + len, and writes nothing but row[0 .. 64) and span[0 .. 8).
// A value the multilanguage module wrote holds that text inside a protobuf State message: state_parse_protobuf_state (at
// the end of this file) reads the envelope and hands the payload to the same parser.
#pragma once
#include <stdint.h>

#include "../../include/surge_replay.h"
#include "f64_parse.h"

#if !defined(__HIP_DEVICE_COMPILE__)
extern "C" int32_t surge_parse_f64_json(const uint8_t* text, int64_t len, uint64_t* bits_out);  // f64_text.cpp: Eisel-Lemire, strtod where that cannot decide
#endif

namespace surge {

// the template's own consistency (what the encoders check before they launch); 0 = usable, else a message
inline const char* state_template_problem(const surge_json_template* t) {
  if (!t) return "template is NULL";
  if (t->n_parts == 0 || t->n_parts > SURGE_JSON_MAX_PARTS) return "template.n_parts out of range";
  for (uint32_t i = 0; i < t->n_parts; ++i) {
    const auto& pt = t->part[i];
    if (pt.kind > SURGE_JP_STR) return "unknown template part kind";
    if (pt.kind == SURGE_JP_LITERAL && (pt.lit_off > 256 || pt.lit_len > 256 - pt.lit_off)) return "literal out of range";
    if (pt.kind == SURGE_JP_STR) {
      if (pt.field_offset >= SURGE_JSON_STRING_COLUMNS) return "SURGE_JP_STR names a string column out of range";
    } else if (pt.kind >= SURGE_JP_I32) {
      const uint32_t width = (pt.kind == SURGE_JP_I64 || pt.kind == SURGE_JP_F64) ? 8u : 4u;
      if (pt.field_offset > 64u - width || pt.field_offset % width) return "field outside the 64-byte state or misaligned";
      if (pt.field_offset < 40u && pt.field_offset + width > 36u) return "field overlaps the flags word";
    }
  }
  return nullptr;
}

SURGE_HD int sp_hex(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

// One character of a JSON string's body, the one place that knows the accepted escapes: `c` is the byte just read at
// v[*i - 1] (not a closing quote); an escape's remaining bytes are read from v[*i ..] and never at or beyond v + len.
// *cp = the code point (a byte from 0x80 on stands for itself), *n_out = how many UTF-8 bytes it unescapes to (1 .. 3).
SURGE_HD int sp_string_unit(const uint8_t* v, int64_t len, int64_t* i, uint32_t c, uint32_t* cp, uint32_t* n_out) {
  *n_out = 1;
  *cp = c;
  if (c < 0x20u) return SURGE_STATE_DECODE_STRING;  // a control character is always escaped
  if (c != '\\') return SURGE_STATE_DECODE_OK;
  if (*i >= len) return SURGE_STATE_DECODE_STRING;
  const uint8_t e = v[(*i)++];
  switch (e) {
    case '"': *cp = '"'; break;
    case '\\': *cp = '\\'; break;
    case '/': *cp = '/'; break;
    case 'b': *cp = '\b'; break;
    case 'f': *cp = '\f'; break;
    case 'n': *cp = '\n'; break;
    case 'r': *cp = '\r'; break;
    case 't': *cp = '\t'; break;
    case 'u': {
      if (len - *i < 4) return SURGE_STATE_DECODE_STRING;  // the text ends inside the escape
      uint32_t u = 0;
      for (int d = 0; d < 4; ++d) {
        const int h = sp_hex(v[*i + d]);
        if (h < 0) return SURGE_STATE_DECODE_ESCAPE;
        u = (u << 4) | (uint32_t)h;
      }
      *i += 4;
      if (u >= 0xD800u && u <= 0xDFFFu) return SURGE_STATE_DECODE_SURROGATE;
      *cp = u;
      *n_out = u < 0x80u ? 1u : u < 0x800u ? 2u : 3u;
      break;
    }
    default: return SURGE_STATE_DECODE_ESCAPE;
  }
  return SURGE_STATE_DECODE_OK;
}

// byte b of the n_out UTF-8 bytes of code point c (sp_string_unit's pair)
SURGE_HD uint32_t sp_utf8_byte(uint32_t c, uint32_t n_out, uint32_t b) {
  if (n_out == 1) return c;
  if (n_out == 2) return b == 0 ? (0xC0u | (c >> 6)) : (0x80u | (c & 0x3Fu));
  return b == 0 ? (0xE0u | (c >> 12)) : b == 1 ? (0x80u | ((c >> 6) & 0x3Fu)) : (0x80u | (c & 0x3Fu));
}

// A JSON string whose opening quote is v[*pos].  key_len >= 0: the unescaped bytes must equal key[0 .. key_len).
// *pos ends behind the closing quote; the raw span between the quotes goes to *raw_off / *raw_len.
SURGE_HD int sp_string(const uint8_t* v, int64_t len, int64_t* pos, const uint8_t* key, int64_t key_len, int64_t* raw_off,
                       int64_t* raw_len) {
  int64_t i = *pos;
  if (i >= len || v[i] != '"') return SURGE_STATE_DECODE_STRING;
  ++i;
  *raw_off = i;
  int64_t k = 0;       // unescaped bytes so far
  bool same = true;    // ... and they equal the key's
  while (true) {
    if (i >= len) return SURGE_STATE_DECODE_STRING;  // unterminated
    uint32_t c = v[i++];
    if (c == '"') break;
    uint32_t n_out = 1;
    const int rc = sp_string_unit(v, len, &i, c, &c, &n_out);
    if (rc != SURGE_STATE_DECODE_OK) return rc;
    if (key_len >= 0) {
      // the code point as UTF-8, byte by byte against the key
      for (uint32_t b = 0; b < n_out; ++b) {
        same = same && k < key_len && key[k] == (uint8_t)sp_utf8_byte(c, n_out, b);
        ++k;
      }
    }
  }
  *raw_len = i - 1 - *raw_off;
  *pos = i;
  if (key_len >= 0 && !(same && k == key_len)) return SURGE_STATE_DECODE_KEY_MISMATCH;
  return SURGE_STATE_DECODE_OK;
}

// The raw span of a JSON string (the bytes between the quotes, as sp_string reports them) -> its unescaped UTF-8.
// *n_out = the unescaped length; with `out`, bytes [0, min(length, capacity)) are written — never one beyond capacity.
// The rules are sp_string's (sp_string_unit); a bare quote cannot lie inside a span and is refused as STRING.  Reads
// raw[0 .. raw_len) only.
SURGE_HD int sp_unescape(const uint8_t* raw, int64_t raw_len, uint8_t* out, int64_t capacity, int64_t* n_out) {
  int64_t i = 0, k = 0;
  *n_out = 0;
  while (i < raw_len) {
    uint32_t c = raw[i++];
    if (c == '"') return SURGE_STATE_DECODE_STRING;
    uint32_t n = 1;
    const int rc = sp_string_unit(raw, raw_len, &i, c, &c, &n);
    if (rc != SURGE_STATE_DECODE_OK) return rc;
    for (uint32_t b = 0; b < n; ++b) {
      if (out && k < capacity) out[k] = (uint8_t)sp_utf8_byte(c, n, b);
      ++k;
    }
  }
  *n_out = k;
  return SURGE_STATE_DECODE_OK;
}

// -?[0-9]+ not followed by a fraction, an exponent or a sign -> magnitude and sign; `over`: beyond 64 bits
SURGE_HD int sp_integer(const uint8_t* v, int64_t len, int64_t* pos, bool* neg, uint64_t* mag, bool* over) {
  int64_t i = *pos;
  *neg = false;
  if (i < len && v[i] == '-') { *neg = true; ++i; }
  uint64_t m = 0;
  bool any = false, ov = false;
  while (i < len && v[i] >= '0' && v[i] <= '9') {
    const uint64_t d = (uint64_t)(v[i] - '0');
    if (m > (0xFFFFFFFFFFFFFFFFull - d) / 10ull) ov = true; else m = m * 10ull + d;
    any = true;
    ++i;
  }
  if (!any) return SURGE_STATE_DECODE_INT;
  if (i < len && (v[i] == '.' || v[i] == 'e' || v[i] == 'E' || v[i] == '+' || v[i] == '-')) return SURGE_STATE_DECODE_INT;
  *mag = m;
  *over = ov;
  *pos = i;
  return SURGE_STATE_DECODE_OK;
}

// One value -> row[0 .. 64) (16-byte aligned; complete only when the result is OK) and, for STR parts, span[2 c] /
// span[2 c + 1] = offset / length of column c's still-escaped bytes (span nullable).  key_len < 0: the id is not compared.
// RESOLVE (host only): a Double the fast algorithm cannot decide is settled by surge_parse_f64_json's strtod path; without
// it the value is reported as SURGE_STATE_DECODE_AMBIGUOUS.
template <bool RESOLVE>
SURGE_HD int state_parse_json(const surge_json_template& t, const uint8_t* v, int64_t len, const uint8_t* key, int64_t key_len,
                              const F64ParseTable* tb, uint8_t* row, int64_t* span) {
  uint64_t* row8 = (uint64_t*)row;
  for (int q = 0; q < 8; ++q) row8[q] = 0;
  int64_t i = 0;
  for (uint32_t p = 0; p < t.n_parts; ++p) {
    const uint32_t kind = t.part[p].kind, off = t.part[p].field_offset;
    if (kind == SURGE_JP_LITERAL) {
      const uint32_t lo = t.part[p].lit_off, ll = t.part[p].lit_len;
      if (len - i < (int64_t)ll) return SURGE_STATE_DECODE_LITERAL;
      for (uint32_t b = 0; b < ll; ++b)
        if (v[i + b] != t.literals[lo + b]) return SURGE_STATE_DECODE_LITERAL;
      i += ll;
    } else if (kind == SURGE_JP_KEY || kind == SURGE_JP_STR) {
      int64_t ro = 0, rl = 0;
      const int rc = sp_string(v, len, &i, key, kind == SURGE_JP_KEY ? key_len : -1, &ro, &rl);
      if (rc != SURGE_STATE_DECODE_OK) return rc;
      if (kind == SURGE_JP_STR && span && off < SURGE_JSON_STRING_COLUMNS) { span[2 * off] = ro; span[2 * off + 1] = rl; }
    } else if (kind == SURGE_JP_F64) {
      int64_t e = i;
      while (e < len && e - i < 400 && ((v[e] >= '0' && v[e] <= '9') || v[e] == '-' || v[e] == '+' || v[e] == '.' || v[e] == 'e' || v[e] == 'E')) ++e;
      if (e - i >= 400) return SURGE_STATE_DECODE_NUMBER;
      uint64_t bits = 0;
      const int rc = f64_parse_json_number(v + i, (int)(e - i), tb, &bits);
      if (rc == F64_PARSE_MALFORMED) return SURGE_STATE_DECODE_NUMBER;
      if (rc == F64_PARSE_AMBIGUOUS) {
#if !defined(__HIP_DEVICE_COMPILE__)
        if (RESOLVE) {
          if (surge_parse_f64_json(v + i, e - i, &bits) < 0) return SURGE_STATE_DECODE_NUMBER;
        } else
#endif
          return SURGE_STATE_DECODE_AMBIGUOUS;
      }
      *(uint64_t*)(row + off) = bits;
      i = e;
    } else {
      bool neg = false, over = false;
      uint64_t mag = 0;
      const int rc = sp_integer(v, len, &i, &neg, &mag, &over);
      if (rc != SURGE_STATE_DECODE_OK) return rc;
      if (kind == SURGE_JP_I32) {
        if (over || mag > (neg ? 0x80000000ull : 0x7FFFFFFFull)) return SURGE_STATE_DECODE_RANGE;
        *(uint32_t*)(row + off) = neg ? (uint32_t)0 - (uint32_t)mag : (uint32_t)mag;
      } else if (kind == SURGE_JP_U32) {
        if (over || mag > (neg ? 0ull : 0xFFFFFFFFull)) return SURGE_STATE_DECODE_RANGE;
        *(uint32_t*)(row + off) = (uint32_t)mag;
      } else {
        if (over || mag > (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull)) return SURGE_STATE_DECODE_RANGE;
        *(uint64_t*)(row + off) = neg ? (uint64_t)0 - mag : mag;
      }
    }
  }
  if (i != len) return SURGE_STATE_DECODE_TRAILING;
  *(uint32_t*)(row + 36) = SURGE_STATE_PRESENT;
  return SURGE_STATE_DECODE_OK;
}

// ---- the multilanguage module's envelope around such a text ------------------------------------------------------------
//   message State { string aggregateId = 1; bytes payload = 2; }   (multilanguage-protocol.proto:7-10)
// as the state encoders write it with envelope == 1 (state_kernels.hip) and GenericSurgeCommandBusinessLogic stores it
// (pbState.toByteArray, GenericSurgeCommandBusinessLogic.scala:36-39; read back with State.parseFrom, :25-27).
// Accepted: optionally field 1 (tag 0x0A, a length varint, that many id bytes), then optionally field 2 (tag 0x12, a
// length varint, that many payload bytes), and nothing else: the value ends exactly behind the last accepted field.
// proto3 omits an empty field; scalapb writes field 1 before field 2 and only that order is read, as only case-class order
// is read of the JSON.  Any other tag, a repeated field, field 2 before field 1, a length beyond the value's end, bytes
// behind field 2 and a value that ends inside a tag or a varint are SURGE_STATE_DECODE_ENVELOPE.

// A length varint at v[*pos]: 1 - 5 bytes, value <= 2^31 - 1; an over-long (non-minimal) spelling is accepted, as the
// protobuf runtime accepts it.  Never reads at or beyond v + len.
// (P: the kind of pointer the bytes are read through — const uint8_t* on the host and in the state decoder; the event kernels
// of ingest_records.hip also read a staged section through an LDS pointer.  One text for all of them.)
template <typename P>
SURGE_HD int sp_length_varint(P v, int64_t len, int64_t* pos, int64_t* value) {
  uint64_t x = 0;
  int64_t i = *pos;
  for (int b = 0; b < 5; ++b) {
    if (i >= len) return SURGE_STATE_DECODE_ENVELOPE;  // the value ends inside the varint
    const uint32_t c = v[i++];
    x |= (uint64_t)(c & 0x7Fu) << (7 * b);
    if (!(c & 0x80u)) {
      if (x > 0x7FFFFFFFull) return SURGE_STATE_DECODE_ENVELOPE;
      *value = (int64_t)x;
      *pos = i;
      return SURGE_STATE_DECODE_OK;
    }
  }
  return SURGE_STATE_DECODE_ENVELOPE;  // the 5th byte still continues
}

// The envelope's grammar alone: where field 1 lies (*id_off / *id_len; absent = the empty id) and where the payload lies
// (*pay_off / *pay_len; an absent field 2 is the empty payload at the value's end).  The same message shape holds the
// events topic's values: Event { string aggregateId = 1; bytes payload = 2; } (multilanguage-protocol.proto:17-20).
template <typename P>
SURGE_HD int sp_envelope_spans(P v, int64_t len, int64_t* id_off, int64_t* id_len, int64_t* pay_off, int64_t* pay_len) {
  int64_t i = 0, n = 0;
  *id_off = 0;
  *id_len = 0;
  if (i < len && v[i] == 0x0Au) {
    ++i;
    const int rc = sp_length_varint(v, len, &i, &n);
    if (rc != SURGE_STATE_DECODE_OK) return rc;
    if (n > len - i) return SURGE_STATE_DECODE_ENVELOPE;
    *id_off = i;
    *id_len = n;
    i += n;
  }
  *pay_off = i;
  *pay_len = 0;
  if (i < len && v[i] == 0x12u) {
    ++i;
    const int rc = sp_length_varint(v, len, &i, &n);
    if (rc != SURGE_STATE_DECODE_OK) return rc;
    if (n > len - i) return SURGE_STATE_DECODE_ENVELOPE;
    *pay_off = i;
    *pay_len = n;
    i += n;
  }
  if (i != len) return SURGE_STATE_DECODE_ENVELOPE;  // another tag, a repeated field, field 1 behind field 2, stray bytes
  return SURGE_STATE_DECODE_OK;
}

// The envelope with its id: sp_envelope_spans, then, with key_len >= 0, the raw bytes of field 1 against the id byte for
// byte (no unescaping: the encoder writes the raw UTF-8 id; an absent field 1 is the empty id).  Grammar errors come
// before the comparison.  (PK: the key's pointer kind.)
template <typename P, typename PK>
SURGE_HD int sp_envelope(P v, int64_t len, PK key, int64_t key_len, int64_t* pay_off, int64_t* pay_len) {
  int64_t id_off = 0, id_len = 0;
  const int rc = sp_envelope_spans(v, len, &id_off, &id_len, pay_off, pay_len);
  if (rc != SURGE_STATE_DECODE_OK) return rc;
  if (key_len >= 0) {
    if (id_len != key_len) return SURGE_STATE_DECODE_KEY_MISMATCH;
    for (int64_t b = 0; b < id_len; ++b)
      if (v[id_off + b] != key[b]) return SURGE_STATE_DECODE_KEY_MISMATCH;
  }
  return SURGE_STATE_DECODE_OK;
}

// One enveloped value: sp_envelope, then the payload through state_parse_json with the payload template exactly as a bare
// value (a KEY part inside the payload is still compared; the payload's statuses are reported as they are: an absent or
// empty payload is what the template makes of no text).  The STR spans are relative to v, not to the payload, so that what
// reads them (sp_unescape over the record's value) needs to know nothing of the envelope.
template <bool RESOLVE>
SURGE_HD int state_parse_protobuf_state(const surge_json_template& t, const uint8_t* v, int64_t len, const uint8_t* key, int64_t key_len,
                                        const F64ParseTable* tb, uint8_t* row, int64_t* span) {
  int64_t pay_off = 0, pay_len = 0;
  int rc = sp_envelope(v, len, key, key_len, &pay_off, &pay_len);
  if (rc != SURGE_STATE_DECODE_OK) return rc;
  rc = state_parse_json<RESOLVE>(t, v + pay_off, pay_len, key, key_len, tb, row, span);
  if (rc != SURGE_STATE_DECODE_OK || !span) return rc;
  for (uint32_t c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {  // (once per column, however many parts name it)
    bool named = false;
    for (uint32_t p = 0; p < t.n_parts; ++p) named = named || (t.part[p].kind == SURGE_JP_STR && t.part[p].field_offset == c);
    if (named) span[2 * c] += pay_off;
  }
  return SURGE_STATE_DECODE_OK;
}

}  // namespace surge
