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

// ---- the lenient reading mode: what `Json.parse(bytes).asOpt[State]` takes ------------------------------------------------
// Every readState of the reference parses the bytes into a JSON tree and reads the case class out of it by name
// (TestBoundedContext.scala:156, scaladsl/TestBoundedContext.scala:131-132, BankAccountSurgeModel.scala:23, and the
// multilanguage side on pbState.payload): that reader takes the members in any order, insignificant whitespace, and members
// the case class does not know (a field a later release added, or an SDK application's own JSON library).  The strict parser
// above stays the default; this one reads the same template through a table of its fields:
//   - optional whitespace (0x20 \t \n \r) around every token, in front of the object and behind it; the top level must be an
//     object, else SYNTAX; bytes other than whitespace behind its closing brace are TRAILING;
//   - a member name is a JSON string by sp_string's rules ("count" names count) and is compared unescaped;
//   - a member the table knows is parsed by the routine the strict parser uses for its kind and reports that routine's
//     status (`null` is therefore INT / NUMBER / STRING by kind; KEY is compared with the id when a key is given);
//   - a name that occurs more than once: every occurrence is parsed and a refused one refuses the value, the last one gives
//     the field and the STR span.  play-json's map and Python's json.loads both keep the last and never look at the earlier
//     ones: refusing a bad earlier occurrence is narrower than either;
//   - a member the table does not know is skipped and validated as JSON (strings: no raw byte below 0x20, the escapes
//     \" \\ \/ \b \f \n \r \t and \u + four hex digits — surrogates pass, nothing is unescaped; numbers
//     -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?; true / false / null; arrays and objects to a nesting depth of 32 below
//     the top-level object, kept in a 32-bit stack of kinds: no recursion, nothing indexed per lane); deeper nesting and
//     anything malformed are SYNTAX;
//   - when the object closes, a field of the table that never occurred is MISSING (Json.format gives None there).
// Unchanged: the integer rule is -?[0-9]+ (play-json would also take 1.0 or 1e2 for an Int); POISONED and the sign of -0.0
// are not restored; bytes from 0x80 on are not checked as UTF-8.  The two promises hold as above: nothing at or beyond
// value + len is read, nothing but row[0 .. 64) and span[0 .. 8) is written.

constexpr uint32_t kStateMaxFields = (SURGE_JSON_MAX_PARTS - 1) / 2;  // LITERAL value LITERAL value ... LITERAL

// The template as the lenient parser reads it: per field its name (a span of template.literals), its part kind and the
// part's field_offset.  Built on the host once per call (state_field_table), passed to the kernel by value.
struct StateFieldTable {
  uint32_t n_fields;
  struct { uint32_t name_off, name_len, kind, field_offset; } field[kStateMaxFields];
};

// 0 = `t` (already consistent: state_template_problem) has the shape the lenient parser can read and *tab describes it: the
// parts alternate LITERAL, value, ..., LITERAL; the first literal is {"<name>": each inner one ,"<name>": the last one } ;
// a name has at least one byte, no backslash and no quote; no two names are equal.  Else a message, and *bad_part = the part
// that did not fit.
inline const char* state_field_table(const surge_json_template* t, StateFieldTable* tab, uint32_t* bad_part) {
  *tab = StateFieldTable{};
  *bad_part = 0;
  if (t->n_parts < 3 || t->n_parts % 2 == 0) {
    *bad_part = t->n_parts ? t->n_parts - 1 : 0;
    return "the parts do not alternate LITERAL, value, ..., LITERAL";
  }
  for (uint32_t p = 0; p < t->n_parts; ++p) {
    *bad_part = p;
    const auto& pt = t->part[p];
    if ((p % 2 == 0) != (pt.kind == SURGE_JP_LITERAL)) return "the parts do not alternate LITERAL, value, ..., LITERAL";
    if (pt.kind != SURGE_JP_LITERAL) continue;
    const uint8_t* s = t->literals + pt.lit_off;
    if (p == t->n_parts - 1) {
      if (pt.lit_len != 1 || s[0] != '}') return "the last literal is not }";
      continue;
    }
    // {"<name>":  or  ,"<name>":
    if (pt.lit_len < 5 || s[0] != (p == 0 ? '{' : ',') || s[1] != '"' || s[pt.lit_len - 2] != '"' || s[pt.lit_len - 1] != ':')
      return p == 0 ? "the first literal is not {\"<name>\":" : "an inner literal is not ,\"<name>\":";
    const uint32_t no = pt.lit_off + 2, nl = pt.lit_len - 4;
    for (uint32_t b = 0; b < nl; ++b)
      if (t->literals[no + b] == '"' || t->literals[no + b] == '\\') return "a field name holds a quote or a backslash";
    for (uint32_t f = 0; f < tab->n_fields; ++f) {
      bool same = tab->field[f].name_len == nl;
      for (uint32_t b = 0; same && b < nl; ++b) same = t->literals[tab->field[f].name_off + b] == t->literals[no + b];
      if (same) return "two fields have the same name";
    }
    auto& fd = tab->field[tab->n_fields++];
    fd.name_off = no;
    fd.name_len = nl;
    fd.kind = t->part[p + 1].kind;
    fd.field_offset = t->part[p + 1].field_offset;
  }
  *bad_part = 0;
  return nullptr;
}

SURGE_HD int64_t sp_skip_ws(const uint8_t* v, int64_t len, int64_t i) {
  while (i < len && (v[i] == ' ' || v[i] == '\t' || v[i] == '\n' || v[i] == '\r')) ++i;
  return i;
}

// A JSON string that is only validated (the opening quote is v[*pos]): SYNTAX for whatever is not one.
SURGE_HD int sp_skip_string(const uint8_t* v, int64_t len, int64_t* pos) {
  int64_t i = *pos;
  if (i >= len || v[i] != '"') return SURGE_STATE_DECODE_SYNTAX;
  ++i;
  while (true) {
    if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
    const uint32_t c = v[i++];
    if (c == '"') break;
    if (c < 0x20u) return SURGE_STATE_DECODE_SYNTAX;
    if (c != '\\') continue;
    if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
    const uint32_t e = v[i++];
    if (e == 'u') {
      if (len - i < 4) return SURGE_STATE_DECODE_SYNTAX;
      for (int d = 0; d < 4; ++d)
        if (sp_hex(v[i + d]) < 0) return SURGE_STATE_DECODE_SYNTAX;
      i += 4;
    } else if (!(e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't')) {
      return SURGE_STATE_DECODE_SYNTAX;
    }
  }
  *pos = i;
  return SURGE_STATE_DECODE_OK;
}

// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? at v[*pos]; what follows it is the caller's to judge
SURGE_HD int sp_skip_number(const uint8_t* v, int64_t len, int64_t* pos) {
  int64_t i = *pos;
  if (i < len && v[i] == '-') ++i;
  if (i >= len || v[i] < '0' || v[i] > '9') return SURGE_STATE_DECODE_SYNTAX;
  if (v[i] == '0') ++i;
  else while (i < len && v[i] >= '0' && v[i] <= '9') ++i;
  if (i < len && v[i] == '.') {
    ++i;
    if (i >= len || v[i] < '0' || v[i] > '9') return SURGE_STATE_DECODE_SYNTAX;
    while (i < len && v[i] >= '0' && v[i] <= '9') ++i;
  }
  if (i < len && (v[i] == 'e' || v[i] == 'E')) {
    ++i;
    if (i < len && (v[i] == '+' || v[i] == '-')) ++i;
    if (i >= len || v[i] < '0' || v[i] > '9') return SURGE_STATE_DECODE_SYNTAX;
    while (i < len && v[i] >= '0' && v[i] <= '9') ++i;
  }
  *pos = i;
  return SURGE_STATE_DECODE_OK;
}

// the word w[0 .. n) at v[*pos]
SURGE_HD int sp_skip_word(const uint8_t* v, int64_t len, int64_t* pos, uint32_t w, int n) {  // w: the word's bytes, first byte lowest
  if (len - *pos < n) return SURGE_STATE_DECODE_SYNTAX;
  for (int b = 0; b < n; ++b)
    if (v[*pos + b] != ((w >> (8 * b)) & 0xFFu)) return SURGE_STATE_DECODE_SYNTAX;
  *pos += n;
  return SURGE_STATE_DECODE_OK;
}

// Any JSON value at v[*pos] (whitespace in front of it allowed), validated and passed over; *pos ends behind it.  Containers
// are walked with a stack of kinds in one 32-bit word (bit 0 = the innermost: 1 object, 0 array) to a depth of 32.
SURGE_HD int sp_skip_value(const uint8_t* v, int64_t len, int64_t* pos) {
  uint32_t stack = 0, depth = 0;
  int64_t i = *pos;
  while (true) {
    // a value is expected
    i = sp_skip_ws(v, len, i);
    if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
    const uint32_t c = v[i];
    int rc = SURGE_STATE_DECODE_OK;
    bool opened = false;
    if (c == '{' || c == '[') {
      if (depth == 32u) return SURGE_STATE_DECODE_SYNTAX;
      const bool obj = c == '{';
      stack = (stack << 1) | (obj ? 1u : 0u);
      ++depth;
      i = sp_skip_ws(v, len, i + 1);
      if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
      if (v[i] == (obj ? '}' : ']')) {  // empty: closed at once
        ++i;
        stack >>= 1;
        --depth;
      } else {
        opened = true;
        if (obj) {  // the first member's name and colon; its value is the next round's
          rc = sp_skip_string(v, len, &i);
          if (rc != SURGE_STATE_DECODE_OK) return rc;
          i = sp_skip_ws(v, len, i);
          if (i >= len || v[i] != ':') return SURGE_STATE_DECODE_SYNTAX;
          ++i;
        }
      }
    } else if (c == '"') {
      rc = sp_skip_string(v, len, &i);
    } else if (c == '-' || (c >= '0' && c <= '9')) {
      rc = sp_skip_number(v, len, &i);
    } else if (c == 't') {
      rc = sp_skip_word(v, len, &i, 0x65757274u, 4);
    } else if (c == 'f') {
      ++i;
      rc = sp_skip_word(v, len, &i, 0x65736C61u, 4);
    } else if (c == 'n') {
      rc = sp_skip_word(v, len, &i, 0x6C6C756Eu, 4);
    } else {
      return SURGE_STATE_DECODE_SYNTAX;
    }
    if (rc != SURGE_STATE_DECODE_OK) return rc;
    if (opened) continue;
    // a value is complete: close what it completes, or go on to the next element
    while (true) {
      if (depth == 0u) {
        *pos = i;
        return SURGE_STATE_DECODE_OK;
      }
      i = sp_skip_ws(v, len, i);
      if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
      const bool obj = (stack & 1u) != 0u;
      const uint32_t d = v[i++];
      if (d == (obj ? '}' : ']')) {
        stack >>= 1;
        --depth;
        continue;
      }
      if (d != ',') return SURGE_STATE_DECODE_SYNTAX;
      if (obj) {
        i = sp_skip_ws(v, len, i);
        rc = sp_skip_string(v, len, &i);
        if (rc != SURGE_STATE_DECODE_OK) return rc;
        i = sp_skip_ws(v, len, i);
        if (i >= len || v[i] != ':') return SURGE_STATE_DECODE_SYNTAX;
        ++i;
      }
      break;
    }
  }
}

// A member name (the opening quote is v[*pos]) by sp_string's rules, compared unescaped with every name of the table at
// once: *field = the field it names, or -1.  The candidates are a bit mask; the table is read with indices that are the
// same for every lane, the literals with the lane's own.
SURGE_HD int sp_member_name(const surge_json_template& t, const StateFieldTable& tab, const uint8_t* v, int64_t len, int64_t* pos, int* field) {
  int64_t i = *pos;
  if (i >= len || v[i] != '"') return SURGE_STATE_DECODE_SYNTAX;
  ++i;
  uint32_t alive = (1u << tab.n_fields) - 1u;
  uint32_t k = 0;  // unescaped bytes so far
  while (true) {
    if (i >= len) return SURGE_STATE_DECODE_STRING;
    uint32_t c = v[i++];
    if (c == '"') break;
    uint32_t n_out = 1;
    const int rc = sp_string_unit(v, len, &i, c, &c, &n_out);
    if (rc != SURGE_STATE_DECODE_OK) return rc;
    for (uint32_t b = 0; b < n_out; ++b) {
      const uint32_t byte = sp_utf8_byte(c, n_out, b);
      for (uint32_t f = 0; f < tab.n_fields; ++f)
        if (((alive >> f) & 1u) && !(k < tab.field[f].name_len && t.literals[(tab.field[f].name_off + k) & 255u] == byte)) alive &= ~(1u << f);
      ++k;
    }
  }
  *field = -1;
  for (uint32_t f = 0; f < tab.n_fields; ++f)
    if (((alive >> f) & 1u) && tab.field[f].name_len == k) *field = (int)f;
  *pos = i;
  return SURGE_STATE_DECODE_OK;
}

// state_parse_json's arguments and the field table of `t` (state_field_table); the same results, for the wider grammar above.
template <bool RESOLVE>
SURGE_HD int state_parse_json_lenient(const surge_json_template& t, const StateFieldTable& tab, const uint8_t* v, int64_t len, const uint8_t* key,
                                      int64_t key_len, const F64ParseTable* tb, uint8_t* row, int64_t* span) {
  uint64_t* row8 = (uint64_t*)row;
  for (int q = 0; q < 8; ++q) row8[q] = 0;
  int64_t i = sp_skip_ws(v, len, 0);
  if (i >= len || v[i] != '{') return SURGE_STATE_DECODE_SYNTAX;
  i = sp_skip_ws(v, len, i + 1);
  if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
  uint32_t seen = 0;
  if (v[i] == '}') {
    ++i;
  } else {
    while (true) {
      int field = -1;
      int rc = sp_member_name(t, tab, v, len, &i, &field);
      if (rc != SURGE_STATE_DECODE_OK) return rc;
      i = sp_skip_ws(v, len, i);
      if (i >= len || v[i] != ':') return SURGE_STATE_DECODE_SYNTAX;
      i = sp_skip_ws(v, len, i + 1);
      if (field < 0) {
        rc = sp_skip_value(v, len, &i);
        if (rc != SURGE_STATE_DECODE_OK) return rc;
      } else {
        uint32_t kind = 0, off = 0;
        for (uint32_t f = 0; f < tab.n_fields; ++f)  // (read with f, the same for every lane)
          if ((int)f == field) { kind = tab.field[f].kind; off = tab.field[f].field_offset; }
        seen |= 1u << field;
        // (the three branches below restate state_parse_json's: sharing one routine between the two parsers changes the strict
        // kernels' instruction streams, and those stay what they were)
        if (kind == SURGE_JP_KEY || kind == SURGE_JP_STR) {
          int64_t ro = 0, rl = 0;
          rc = sp_string(v, len, &i, key, kind == SURGE_JP_KEY ? key_len : -1, &ro, &rl);
          if (rc != SURGE_STATE_DECODE_OK) return rc;
          if (kind == SURGE_JP_STR && span && off < SURGE_JSON_STRING_COLUMNS) { span[2 * off] = ro; span[2 * off + 1] = rl; }
        } else if (kind == SURGE_JP_F64) {
          int64_t e = i;
          while (e < len && e - i < 400 && ((v[e] >= '0' && v[e] <= '9') || v[e] == '-' || v[e] == '+' || v[e] == '.' || v[e] == 'e' || v[e] == 'E')) ++e;
          if (e - i >= 400) return SURGE_STATE_DECODE_NUMBER;
          uint64_t bits = 0;
          rc = f64_parse_json_number(v + i, (int)(e - i), tb, &bits);
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
          rc = sp_integer(v, len, &i, &neg, &mag, &over);
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
      i = sp_skip_ws(v, len, i);
      if (i >= len) return SURGE_STATE_DECODE_SYNTAX;
      const uint32_t d = v[i++];
      if (d == '}') break;
      if (d != ',') return SURGE_STATE_DECODE_SYNTAX;
      i = sp_skip_ws(v, len, i);
    }
  }
  i = sp_skip_ws(v, len, i);
  if (i != len) return SURGE_STATE_DECODE_TRAILING;
  if (seen != (1u << tab.n_fields) - 1u) return SURGE_STATE_DECODE_MISSING;
  *(uint32_t*)(row + 36) = SURGE_STATE_PRESENT;
  return SURGE_STATE_DECODE_OK;
}

// sp_envelope unchanged in front of the lenient parser; the spans relative to v, as state_parse_protobuf_state reports them
template <bool RESOLVE>
SURGE_HD int state_parse_protobuf_state_lenient(const surge_json_template& t, const StateFieldTable& tab, const uint8_t* v, int64_t len,
                                                const uint8_t* key, int64_t key_len, const F64ParseTable* tb, uint8_t* row, int64_t* span) {
  int64_t pay_off = 0, pay_len = 0;
  int rc = sp_envelope(v, len, key, key_len, &pay_off, &pay_len);
  if (rc != SURGE_STATE_DECODE_OK) return rc;
  rc = state_parse_json_lenient<RESOLVE>(t, tab, v + pay_off, pay_len, key, key_len, tb, row, span);
  if (rc != SURGE_STATE_DECODE_OK || !span) return rc;
  for (uint32_t c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c) {  // (once per column, however many fields name it)
    bool named = false;
    for (uint32_t f = 0; f < tab.n_fields; ++f) named = named || (tab.field[f].kind == SURGE_JP_STR && tab.field[f].field_offset == c);
    if (named) span[2 * c] += pay_off;
  }
  return SURGE_STATE_DECODE_OK;
}

}  // namespace surge
