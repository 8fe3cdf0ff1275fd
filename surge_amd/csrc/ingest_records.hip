// ingest_records.hip — the device decoder's record stage: the varint-framed records of every batch found (chain), parsed
// (key span, value span, offset; 64-bit hash of the key up to ':') and their values decoded (16-byte events as they are, or
// the reference's play-json text through the event template, surge_amd/csrc/event_decode.cpp's rules).  In state mode
// (JsonCtx::states, the state topic) the id is the whole key, a null value is a delivered tombstone and no value is decoded: the
// value spans stay in RecMeta for stage 2's gather.  Enveloped events (JsonCtx::envelope: a multilanguage application's events
// topic) carry the JSON text inside the protobuf message Event{aggregateId, payload}: the envelope is read with state_parse.h's
// reader, its id compared with the record's aggregate id, the payload decoded as a bare value.  Nothing here reads or writes
// the key table.
#include <cstdio>
#include <cstdlib>

#include "ingest_device.h"
#include "state_parse.h"

namespace surge {
namespace ingest {
namespace {

// ---- records: chain, parse, decode (round 4: one workgroup per batch, out of LDS) -----------------------------------------
// Round 3 ran three kernels over the decompressed bytes in global memory — chain (one thread per batch walking its
// records' length varints), parse (one thread per record), resolve (one thread per record walking the JSON text byte by
// byte) — every step a dependent single-byte load: 1.45 ms per 1 M records, almost all of it waiting (SQ_WAIT_ANY 3/4 of
// the wave cycles; the LDS staging resolve_kernel had never fired on lz4 topics: a block's 256 records came from two
// batches whose decompressed bytes lie 64 KiB apart).  Now one workgroup owns one batch: it copies the batch's records
// section into LDS with 16-byte loads, one thread walks the length varints there (the only sequential step, now at LDS
// latency), then every thread parses its record and decodes its value from LDS.  A section that does not fit the LDS of
// its launch is read in place (same code, global pointers).

// 0x80 in every byte of x that equals c (exact in the lowest matching byte and below it — all a first-match search needs)
__device__ __forceinline__ uint32_t bytes_eq(uint32_t x, uint32_t c) {
  const uint32_t v = x ^ (c * 0x01010101u);
  return (v - 0x01010101u) & ~v & 0x80808080u;
}

template <typename P>
struct ReaderT {
  P p;
  P end;
  bool ok;
  __device__ int64_t varlong() {
    // one and two bytes without the loop: a record's length, its key / value lengths and its offset delta almost always
    // (the counters put most of section_kernel's scalar instructions into the exec-mask bookkeeping of these loops)
    if (end - p >= 2) {
      const uint32_t w2 = load4(p);
      const uint32_t b0 = w2 & 0xffu, b1 = (w2 >> 8) & 0xffu;
      if (!(b0 & 0x80u)) { ++p; return (int64_t)(b0 >> 1) ^ -(int64_t)(b0 & 1u); }
      if (!(b1 & 0x80u)) {
        p += 2;
        const uint32_t w = (b0 & 0x7fu) | (b1 << 7);
        return (int64_t)(w >> 1) ^ -(int64_t)(w & 1u);
      }
    }
    uint64_t v = 0;
    int shift = 0;
    while (true) {
      if (p >= end || shift > 63) { ok = false; return 0; }
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7f) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }
};

// ---- event values ------------------------------------------------------------------------------------------------------
template <typename P>
struct JsonScanT {
  P p;
  P end;
  __device__ void ws() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p; }
  __device__ bool string(P* s, int* len, bool* escaped) {
    if (p >= end || *p != '"') return false;
    ++p;
    *s = p;
    *escaped = false;
    for (;;) {
      // four bytes at a time to the next quote or backslash
      while (end - p >= 4) {
        const uint32_t x = load4(p);
        const uint32_t m = bytes_eq(x, '"') | bytes_eq(x, '\\');
        if (m) { p += (__builtin_ctz(m) >> 3); break; }
        p += 4;
      }
      if (p >= end) return false;
      const uint8_t c = *p;
      if (c == '"') break;
      if (c == '\\') {
        *escaped = true;
        ++p;
        if (p >= end) return false;
      }
      ++p;
    }
    *len = (int)(p - *s);
    ++p;
    return true;
  }
  __device__ bool number(P* s, int* len) {
    *s = p;
    if (p < end && (*p == '-' || *p == '+')) ++p;
    bool digits = false;
    while (p < end && ((*p >= '0' && *p <= '9') || *p == '.' || *p == 'e' || *p == 'E' || *p == '+' || *p == '-')) {
      digits = digits || (*p >= '0' && *p <= '9');
      ++p;
    }
    *len = (int)(p - *s);
    return digits;
  }
  __device__ bool skip_value() {
    ws();
    if (p >= end) return false;
    P s; int l; bool e;
    if (*p == '"') return string(&s, &l, &e);
    if (*p == '{' || *p == '[') {
      int depth = 0;
      while (p < end) {
        if (*p == '"') {
          if (!string(&s, &l, &e)) return false;
          continue;
        }
        if (*p == '{' || *p == '[') ++depth;
        if (*p == '}' || *p == ']') {
          --depth;
          if (depth == 0) { ++p; return true; }
        }
        ++p;
      }
      return false;
    }
    if (*p == 't' || *p == 'f' || *p == 'n') {
      while (p < end && *p >= 'a' && *p <= 'z') ++p;
      return true;
    }
    return number(&s, &l);
  }
};

// (`want` is one of EvjDevice's name arrays: 8-byte aligned, zero-padded to 64 bytes)
template <typename P>
__device__ __forceinline__ bool name_is(const char* want, int want_len, P got, int got_len) {
  if (want_len != got_len) return false;
  const uint32_t* w4 = (const uint32_t*)want;
  for (int i = 0; i < want_len; i += 4) {
    const int left = want_len - i;
    const uint32_t keep = left >= 4 ? 0xffffffffu : ((1u << (8 * left)) - 1u);
    if (((w4[i >> 2] ^ load4(got + i)) & keep) != 0u) return false;
  }
  return true;
}

template <typename P>
struct FoundT {
  P s;
  int len;
  bool present, is_num, is_str, escaped;
};


template <typename P>
__device__ int parse_i32(P s, int len, int32_t* out) {  // 0 ok, else not an Int
  if (len <= 0 || len > 11) return 1;
  int i = 0;
  bool neg = false;
  if (s[0] == '-') { neg = true; i = 1; }
  if (i >= len) return 1;
  int64_t v = 0;
  for (; i < len; ++i) {
    if (s[i] < '0' || s[i] > '9') return 1;
    v = v * 10 + (s[i] - '0');
  }
  if (neg) v = -v;
  if (v < -2147483648ll || v > 2147483647ll) return 1;
  *out = (int32_t)v;
  return 0;
}

// the rules of surge_event_json_decode (event_decode.cpp), on the device, in one pass over the object: the discriminator
// is the LAST field of its name among the first 24 fields with unescaped names, a sequence / argument field the FIRST
// numeric field of its name among them
template <typename P>
__device__ uint32_t decode_json_event(const EvjDevice* __restrict__ t, const surge::F64ParseTable* ptab, P v, int len, uint4* out) {
  JsonScanT<P> sc{v, v + len};
  FoundT<P> disc;
  disc.present = false; disc.is_num = disc.is_str = disc.escaped = false; disc.len = 0; disc.s = v;
  P num_s[kEvjTrack];
  int num_len[kEvjTrack];
#pragma unroll
  for (int j = 0; j < kEvjTrack; ++j) { num_s[j] = v; num_len[j] = -1; }
  const int n_names = (int)t->n_names;
  sc.ws();
  if (sc.p >= sc.end || *sc.p != '{') return RS_JSON;
  ++sc.p;
  sc.ws();
  if (sc.p < sc.end && *sc.p == '}') {
    ++sc.p;
  } else {
    int n_fields = 0;
    for (;;) {
      sc.ws();
      P key; int key_len; bool esc = false;
      if (!sc.string(&key, &key_len, &esc)) return RS_JSON;
      sc.ws();
      if (sc.p >= sc.end || *sc.p != ':') return RS_JSON;
      ++sc.p;
      sc.ws();
      if (sc.p >= sc.end) return RS_JSON;
      FoundT<P> cur;
      cur.s = sc.p; cur.len = 0; cur.present = true; cur.is_num = cur.is_str = cur.escaped = false;
      if (*sc.p == '"') {
        if (!sc.string(&cur.s, &cur.len, &cur.escaped)) return RS_JSON;
        cur.is_str = true;
      } else if (*sc.p == '-' || (*sc.p >= '0' && *sc.p <= '9')) {
        if (!sc.number(&cur.s, &cur.len)) return RS_JSON;
        cur.is_num = true;
      } else if (!sc.skip_value()) {
        return RS_JSON;
      }
      if (!esc && n_fields < 24) {  // the host decoder remembers 24 fields and ignores names with escapes
        ++n_fields;
        if (t->name_len[0] && name_is(t->names[0], t->name_len[0], key, key_len)) disc = cur;
        if (cur.is_num) {
#pragma unroll
          for (int j = 0; j < kEvjTrack; ++j)
            if (j + 1 < n_names && num_len[j] < 0 && name_is(t->names[j + 1], t->name_len[j + 1], key, key_len)) { num_s[j] = cur.s; num_len[j] = cur.len; }
        }
      }
      sc.ws();
      if (sc.p < sc.end && *sc.p == ',') { ++sc.p; continue; }
      if (sc.p < sc.end && *sc.p == '}') { ++sc.p; break; }
      return RS_JSON;
    }
  }
  sc.ws();
  if (sc.p != sc.end) return RS_JSON;
  int ty = -1;
  if (t->name_len[0] == 0) {
    ty = 0;
  } else {
    if (!disc.present || !disc.is_str) return RS_FIELD;
    for (uint32_t i = 0; i < t->n_types && ty < 0; ++i)
      if (!disc.escaped && name_is(t->type_name[i], t->type_name_len[i], disc.s, disc.len)) ty = (int)i;
    if (ty < 0) return RS_TYPE;
  }
  auto pick = [&](int name_idx, P* s, int* l) {  // the tracked field of that name (name_idx >= 1)
    *l = -1;
#pragma unroll
    for (int j = 0; j < kEvjTrack; ++j)
      if (j + 1 == name_idx) { *s = num_s[j]; *l = num_len[j]; }
  };
  int32_t seq = 0;
  if (t->seq_name[ty] != 0xff) {
    P s = v; int l;
    pick(t->seq_name[ty], &s, &l);
    if (l < 0 || parse_i32(s, l, &seq) != 0) return RS_FIELD;
  }
  uint64_t raw = 0;
  uint32_t status = RS_OK;
  if (t->arg_kind[ty] != SURGE_EVJ_ARG_NONE) {
    P s = v; int l;
    pick(t->arg_name[ty], &s, &l);
    if (l < 0) return RS_FIELD;
    if (t->arg_kind[ty] == SURGE_EVJ_ARG_I32) {
      int32_t a = 0;
      if (parse_i32(s, l, &a) != 0) return RS_FIELD;
      raw = (uint64_t)(uint32_t)a;
    } else {
      if (l >= 400) return RS_FIELD;  // surge_parse_f64_json refuses a number of 400 bytes or more before it parses: the host is the rule
      const int rc = surge::f64_parse_json_number((const uint8_t*)s, l, ptab, &raw);  // (a flat pointer: the parser is shared with the host)
      if (rc == surge::F64_PARSE_MALFORMED) return RS_FIELD;
      if (rc == surge::F64_PARSE_AMBIGUOUS) status = RS_F64_HOST;  // type and seq are final; the host fills in the payload
    }
  }
  *out = make_uint4(t->event_type[ty], (uint32_t)seq, (uint32_t)raw, (uint32_t)(raw >> 32));
  return status;
}

// (Tried in round 4 and dropped: the same grammar as a table-driven automaton — one loop over the bytes in lockstep, next
// state looked up by (state, byte) in LDS, field names recognised by length + hash and verified afterwards, this walk as
// the fallback.  It traded the walk's scalar exec-mask bookkeeping for twice the vector instructions: section_kernel
// alone 0.70 -> 0.77 ms per 1 M records.  The counters say where this kernel's scalar work really is: chaining and
// parsing the varint-framed records, not the JSON.)

// a record value -> event16 + status
template <typename P>
__device__ __forceinline__ uint32_t decode_value(const JsonCtx& jc, P vp, int val_len, uint4* e) {
  if (jc.tmpl) return decode_json_event(jc.tmpl, jc.ptab, vp, val_len, e);
  if (val_len != 16) return RS_SIZE;
  uint32_t w[4];
  for (int q = 0; q < 4; ++q) w[q] = (uint32_t)vp[4 * q] | ((uint32_t)vp[4 * q + 1] << 8) | ((uint32_t)vp[4 * q + 2] << 16) | ((uint32_t)vp[4 * q + 3] << 24);
  *e = make_uint4(w[0], w[1], w[2], w[3]);
  return RS_OK;
}

// An enveloped record value (JsonCtx::envelope == SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT) -> event16 + status: the grammar first
// (sp_envelope_spans, state_parse.h: the text the host and the state kernel compile), then field 1 against the record's aggregate
// id [key, key + key_len) — the key already cut at its ':' — then the payload through decode_json_event as a bare value (an absent
// or empty payload is RS_JSON: no object).  The reader is byte-wise and bounded by the value's length: a value that ends inside
// a varint or a field never reads its neighbour.  The ids are compared four bytes at a time (load4 reads up to 7 bytes past its
// pointer, masked here: the staged bytes end 16 bytes behind their last byte) — byte by byte, two dependent loads and a branch
// per byte of a 13-byte id were most of what the envelope cost.
template <typename P, typename PK>
__device__ __forceinline__ uint32_t decode_enveloped_value(const JsonCtx& jc, P vp, int val_len, PK key, int key_len, uint4* e) {
  int64_t id_off = 0, id_len = 0, pay_off = 0, pay_len = 0;
  if (surge::sp_envelope_spans(vp, (int64_t)val_len, &id_off, &id_len, &pay_off, &pay_len) != SURGE_STATE_DECODE_OK) return RS_ENVELOPE;
  if (id_len != (int64_t)key_len) return RS_KEY_MISMATCH;
  const P id = vp + id_off;
  for (int b = 0; b < key_len; b += 4) {
    const int left = key_len - b;
    const uint32_t keep = left >= 4 ? 0xffffffffu : ((1u << (8 * left)) - 1u);
    if (((load4(id + b) ^ load4(key + b)) & keep) != 0u) return RS_KEY_MISMATCH;
  }
  return decode_json_event(jc.tmpl, jc.ptab, vp + pay_off, (int)pay_len, e);
}

// One record body [body, end) of a section that starts at `base` (absolute offset sec_off in the staged bytes); `valid` =
// this lane has a record.  kEnvelope: the values are enveloped events (an instantiation of its own, see section_kernel).
// kFloor: the section straddles its partition's start offset (surge_ingest_set_start_offset): a well-formed record whose offset
// lies below `floor` is RS_BELOW — what the host drain passes over: no key hashed, no value looked at (so none refused, none handed
// back for its Double), not kept by stage 2; counted in ErrorCell::n_below.  A record that is malformed is malformed on either side
// of the floor, as it is to the host framer, which parses every record of a batch it takes.
template <bool kEnvelope, bool kFloor, typename P>
__device__ __forceinline__ void decode_record(P base, int64_t sec_off, int64_t base_offset, int64_t floor, bool valid, int32_t body, int32_t end, int64_t gi, uint64_t seed,
                                              const JsonCtx& jc, RecMeta* __restrict__ meta, uint4* __restrict__ ev_tmp,
                                              uint32_t* __restrict__ f64_host_list, ErrorCell* err) {
  RecMeta m;
  m.key_off = m.val_off = m.offset = 0; m.hash = 0; m.key_len = m.val_len = 0; m.slot = 0; m.status = RS_MALFORMED;
  uint4 e = make_uint4(0, 0, 0, 0);
  bool has_value = false;
  P val = base;
  P id = base;  // (kEnvelope) the aggregate id: the key up to ':'
  int vlen32 = 0;
  if (valid && body >= 0) {
    ReaderT<P> q{base + body, base + end, true};
    if (q.p < q.end) ++q.p; else q.ok = false;  // attributes
    (void)q.varlong();                            // timestampDelta
    const int64_t offset_delta = q.varlong();
    const int64_t klen = q.varlong();
    P key = q.p;
    if (q.ok && klen > 0) { if (q.end - q.p >= klen) q.p += klen; else q.ok = false; }
    const int64_t vlen = q.ok ? q.varlong() : 0;
    val = q.p;
    if (q.ok && vlen > 0) { if (q.end - q.p >= vlen) q.p += vlen; else q.ok = false; }
    // (headers follow; the chain already knows where the record ends)
    if (q.ok && klen >= -1 && vlen >= -1 && klen < (1ll << 31) && vlen < (1ll << 31)) {
      m.offset = base_offset + offset_delta;
      if (kFloor && m.offset < floor) {  // (kFloor is a constant: without it the test and its branch are not compiled at all)
        m.status = RS_BELOW;
      } else if (klen == 0 && vlen == 0) {
        m.status = RS_SKIP;  // KafkaProducerActorImpl.scala:322-329
      } else if (klen < 0 || vlen < 0) {
        m.status = RS_NULL;
      } else {
        int n = 0;
        uint64_t hk = hash_key_begin(seed);
        for (bool colon = false; n < (int)klen && !colon;) {  // PartitionStringUpToColon (KafkaPartitioner.scala:38-42), hashed on the way
          uint32_t w4 = load4(key + n);
          const int take = (int)klen - n < 4 ? (int)klen - n : 4;
          for (int b = 0; b < take; ++b, w4 >>= 8) {
            const uint32_t c = w4 & 0xffu;
            if (c == (uint32_t)':') { colon = true; break; }
            hk = (hk ^ c) * 0x100000001B3ull;
            ++n;
          }
        }
        m.key_off = sec_off + (key - base);
        m.key_len = n;
        m.val_off = sec_off + (val - base);
        m.val_len = (int32_t)vlen;
        m.hash = hash_key_end(hk, n, seed);
        if constexpr (kEnvelope) id = key;
        has_value = true;
        vlen32 = (int32_t)vlen;
      }
    }
  }
  if (has_value) {
    uint32_t st;
    if constexpr (kEnvelope) st = decode_enveloped_value(jc, val, vlen32, id, (int)m.key_len, &e);
    else st = decode_value(jc, val, vlen32, &e);
    if (st == RS_F64_HOST) {
      f64_host_list[atomicAdd(&err->n_f64_host, 1u)] = (uint32_t)gi;
      st = RS_OK;
    }
    m.status = st;
  }
  if (!valid) return;
  if (kFloor && m.status == RS_BELOW) atomicAdd(&err->n_below, 1u);  // (at most one section per partition ever carries a floor)
  else if (m.status >= RS_NULL) report(err, gi, m.status);
  meta[gi] = m;
  ev_tmp[gi] = e;
}

// The same record in STATE mode (JsonCtx::states: the compacted state topic).  The id is the WHOLE key — the state topic's key is the
// id itself, "a:b" and "a" are two ids; a null value is a tombstone and is delivered, with no bytes; a null key, and an empty
// non-null value under a key (writeState never writes one, the loader would read it as a tombstone), are refused; the flush record
// is skipped as above; headers are skipped (the chain knows where the record ends); no value is decoded — its span stays in
// RecMeta for stage 2's gather.  A function of its own behind a uniform branch: the events path keeps its instructions and registers.
template <typename P>
__device__ __forceinline__ void decode_state_record(P base, int64_t sec_off, int64_t base_offset, bool valid, int32_t body, int32_t end, int64_t gi, uint64_t seed,
                                                    RecMeta* __restrict__ meta, ErrorCell* err) {
  if (!valid) return;
  RecMeta m;
  m.key_off = m.val_off = m.offset = 0; m.hash = 0; m.key_len = m.val_len = 0; m.slot = 0; m.status = RS_MALFORMED;
  if (body >= 0) {
    ReaderT<P> q{base + body, base + end, true};
    if (q.p < q.end) ++q.p; else q.ok = false;  // attributes
    (void)q.varlong();                            // timestampDelta
    const int64_t offset_delta = q.varlong();
    const int64_t klen = q.varlong();
    P key = q.p;
    if (q.ok && klen > 0) { if (q.end - q.p >= klen) q.p += klen; else q.ok = false; }
    const int64_t vlen = q.ok ? q.varlong() : 0;
    P val = q.p;
    if (q.ok && vlen > 0) { if (q.end - q.p >= vlen) q.p += vlen; else q.ok = false; }
    if (q.ok && klen >= -1 && vlen >= -1 && klen < (1ll << 31) && vlen < (1ll << 31)) {
      m.offset = base_offset + offset_delta;
      if (klen == 0 && vlen == 0) {
        m.status = RS_SKIP;  // KafkaProducerActorImpl.scala:322-329: the producer flushes on the state topic
      } else if (klen < 0) {
        m.status = RS_NULL;
      } else if (vlen == 0) {
        m.status = RS_EMPTY_VALUE;
      } else {
        uint64_t hk = hash_key_begin(seed);
        for (int n = 0; n < (int)klen; n += 4) {
          uint32_t w4 = load4(key + n);
          const int take = (int)klen - n < 4 ? (int)klen - n : 4;
          for (int b = 0; b < take; ++b, w4 >>= 8) hk = (hk ^ (w4 & 0xffu)) * 0x100000001B3ull;
        }
        m.key_off = sec_off + (key - base);
        m.key_len = (int32_t)klen;
        m.val_off = sec_off + (val - base);
        m.val_len = vlen < 0 ? 0 : (int32_t)vlen;
        m.hash = hash_key_end(hk, (int)klen, seed);
        m.status = RS_OK;
      }
    }
  }
  if (m.status >= RS_NULL) report(err, gi, m.status);
  meta[gi] = m;
}

// Workgroup sizes of section_kernel.  The decode walks are latency-bound: what counts is how many batches a CU has in
// flight, and a workgroup's lanes beyond its batch's records only take registers away from other batches.  A 16 KiB batch of
// the reference's publisher holds ~140 play-json events: 192 lanes decode it in one round where 256 idled 45 % of theirs — and
// at 90 VGPRs a CU held 5 workgroups of four waves; three-wave workgroups at <= 80 VGPRs make it the 8 the LDS allows.  A
// push picks the smallest size that takes its largest batch's records in one round (64 for small publisher flushes).
constexpr int kSecRecs = 256;  // records chained per round (LDS: two int32 per record)

// the length varints of up to kSecRecs records from relative position *pos on; false = unreadable from record `bad` on
// (This walk is the one sequential step of a batch — one lane works, 255 wait: per record ONE load (the four bytes at the
// record's start hold its whole length varint unless the record is 256 KiB or longer) and a dozen 32-bit instructions.  The
// first version went through ReaderT's general varlong: two byte loads, 64-bit pointer arithmetic and a loop the compiler
// could not drop — 0.19 of section_kernel's 0.55 ms per 10^6 records, measured with the decode switched off.)
// (forced inline: the compiler inlined it into every instantiation of section_kernel while there were eight; left to its cost
// model with twelve it calls it, and pos / bad then live in scratch memory)
template <typename P>
__device__ __forceinline__ bool chain_records(P base, int32_t len, int32_t* pos, int32_t cnt, int32_t* rec_body, int32_t* rec_end, int32_t* bad) {
  int32_t at = *pos;
  for (int32_t i = 0; i < cnt; ++i) {
    const int32_t room = len - at;
    const uint32_t w = room > 0 ? load4(base + at) : 0x80808080u;
    uint32_t v;
    int32_t n;
    if (!(w & 0x80u)) { v = w & 0x7fu; n = 1; }
    else if (!(w & 0x8000u)) { v = (w & 0x7fu) | ((w >> 1) & 0x3f80u); n = 2; }
    else if (!(w & 0x800000u)) { v = (w & 0x7fu) | ((w >> 1) & 0x3f80u) | ((w >> 2) & 0x1fc000u); n = 3; }
    else {  // four bytes or more (or nothing left): the general reader decides
      ReaderT<P> r{base + at, base + len, true};
      const int64_t l = r.varlong();
      const int32_t body = (int32_t)(r.p - base);
      if (!r.ok || l < 0 || r.end - r.p < l) { *bad = i; return false; }
      rec_body[i] = body;
      rec_end[i] = body + (int32_t)l;
      at = body + (int32_t)l;
      continue;
    }
    const int32_t l = (int32_t)(v >> 1) ^ -(int32_t)(v & 1u);
    const int32_t body = at + n;
    if (n > room || l < 0 || l > len - body) { *bad = i; return false; }
    rec_body[i] = body;
    rec_end[i] = body + l;
    at = body + l;
  }
  *pos = at;
  return true;
}

// The same walk by the batch's first WAVE, every lane on its own 1/64th of the section (the walk above is
// the one sequential step of a batch — half of section_kernel's time alone, profiles/r06_section_chain_ab.txt).  A record's
// start cannot be computed without the records before it, but it can be RECOGNISED and the recognition verified:
//   * find: lane k looks in its chunk [k C, (k + 1) C) for the first position that reads as a record start — a length
//     varint of one to three bytes, the attributes byte 0 behind it (kafka-clients writes 0; zero bytes are found four at a
//     time), the record ending inside the section, and the same again at the position where it ends (lane 0: position 0);
//   * walk: from there the lane follows the lengths to the first start at or behind its chunk's end, counting its records;
//   * link: the find is a guess, the walk is exact GIVEN a true start — so if every lane's find is the position the nearest
//     lane in front of it walked to (lane 0's is 0, which is a start by definition), every lane stood on the true chain, by
//     induction; the last walk has to end at the section's end and the counts have to add up to the batch's record count.
//   * write: an exclusive prefix sum of the counts gives each lane its records' indices; it walks its chunk once more and
//     writes their bounds.
// Anything else — a find that does not link (binary values full of zero bytes can fake a start), a four-byte varint, a length
// that leaves the section, a count that differs — makes the function return false with nothing used: the one-lane walk then
// does what it always did, and reports what it always reported.  Called by the 64 lanes of a workgroup's first wave.
__device__ bool chain_records_parallel(lds_ptr_t base, int32_t len, int32_t cnt, int32_t* rec_body, int32_t* rec_end, int32_t* link) {
  const int lane = (int)(threadIdx.x & 63u);
  int32_t C = (((len + 63) >> 6) + 3) & ~3;  // a chunk: a multiple of four bytes ...
  C += (C & 4) ? 0 : 4;                      // ... and an odd number of dwords: lane l's w-th word then lies in bank (l C / 4 + w) % 64, a different one
                                             // for every lane (a 16 KiB section's 256-byte chunks put all 64 lanes on ONE bank: 64-way conflicts, measured 2 x slower)
  if (C > 284) return false;                       // (the find keeps a chunk's zero bytes in 288 bits: sections up to 17.75 KiB, a 16 KiB batch with room to spare)
  const int32_t lo = lane * C, hi = lo + C < len ? lo + C : len;
  // one step of the walk at p (< len): false = not a record start this walk follows
  auto step = [&](int32_t p, int32_t& body, int32_t& end) -> bool {
    const uint32_t w = load4(base + p);
    uint32_t v;
    int32_t n;
    if (!(w & 0x80u)) { v = w & 0x7fu; n = 1; }
    else if (!(w & 0x8000u)) { v = (w & 0x7fu) | ((w >> 1) & 0x3f80u); n = 2; }
    else if (!(w & 0x800000u)) { v = (w & 0x7fu) | ((w >> 1) & 0x3f80u) | ((w >> 2) & 0x1fc000u); n = 3; }
    else return false;
    if (v & 1u) return false;  // (zig-zag: a negative length)
    body = p + n;
    end = body + (int32_t)(v >> 1);
    return end <= len;  // (n bytes of varint fit as well: end >= body)
  };
  // find, part one (the same instructions in every lane: a wave pays for the union of its lanes' paths): the zero bytes of
  // positions [lo, lo + 288) — a record that starts in my chunk has its attributes byte there — as nine 32-bit masks
  uint32_t zm[9];
#pragma unroll
  for (int g = 0; g < 9; ++g) {
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int32_t q = lo + 32 * g + 4 * k;
      const uint32_t w = q < len ? load4(base + q) : 0xffffffffu;
      const uint32_t z = ~(((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w | 0x7f7f7f7fu);  // 0x80 exactly where a byte is zero
      m |= (((z >> 7) * 0x10204080u) >> 28) << (4 * k);                             // ... as four bits
    }
    const int32_t left = len - lo - 32 * g;  // positions of this mask inside the section
    zm[g] = left >= 32 ? m : left <= 0 ? 0u : m & ((1u << left) - 1u);
  }
  // find, part two: my zero bytes in ascending order, for each the starts one to three bytes in front of it, longest varint
  // first (= ascending position); a start has to read as a record — varint, attributes 0, at least the six one-byte fields,
  // inside the section — and so has the position where it ends.  At most 32 candidates: binary values are left to the one-lane walk
  int32_t s = -1;
  if (lane == 0) {
    s = len > 0 ? 0 : -1;
  } else {
    int g = 0, tests = 0;
    uint32_t cur = zm[0];
    while (s < 0 && tests < 32) {
      while (cur == 0u && g < 8) {
        ++g;
        cur = g == 1 ? zm[1] : g == 2 ? zm[2] : g == 3 ? zm[3] : g == 4 ? zm[4] : g == 5 ? zm[5] : g == 6 ? zm[6] : g == 7 ? zm[7] : zm[8];
      }
      if (cur == 0u) break;
      const int32_t at = lo + 32 * g + __builtin_ctz(cur);
      cur &= cur - 1u;
      if (at <= lo) continue;
      const uint32_t f = load4(base + at - 3);  // (at >= 5: lane >= 1, C >= 4)
      const uint32_t b3 = f & 0xffu, b2 = (f >> 8) & 0xffu, b1 = (f >> 16) & 0xffu;
      if (b1 & 0x80u) continue;
      for (int n = (b2 & 0x80u) ? ((b3 & 0x80u) ? 3 : 2) : 1; n >= 1 && s < 0; --n) {
        const int32_t p = at - n;
        if (p < lo || p >= hi) continue;
        ++tests;
        const uint32_t v = n == 1 ? b1 : n == 2 ? ((b2 & 0x7fu) | (b1 << 7)) : ((b3 & 0x7fu) | ((b2 & 0x7fu) << 7) | (b1 << 14));
        const int32_t l = (int32_t)(v >> 1), end = at + l;
        if ((v & 1u) || l < 6 || end > len) continue;
        if (end < len) {  // the record behind it
          const uint32_t w2 = load4(base + end);
          const int n2 = !(w2 & 0x80u) ? 1 : !(w2 & 0x8000u) ? 2 : !(w2 & 0x800000u) ? 3 : 0;
          if (n2 == 0) continue;
          const uint32_t v2 = n2 == 1 ? (w2 & 0x7fu) : n2 == 2 ? ((w2 & 0x7fu) | ((w2 >> 1) & 0x3f80u)) : ((w2 & 0x7fu) | ((w2 >> 1) & 0x3f80u) | ((w2 >> 2) & 0x1fc000u));
          const uint32_t attr2 = n2 == 3 ? (w2 >> 24) : (w2 >> (8 * n2)) & 0xffu;
          if ((v2 & 1u) || (v2 >> 1) < 6u || attr2 != 0u || end + n2 + (int32_t)(v2 >> 1) > len) continue;
        }
        s = p;
      }
    }
  }
  // walk my chunk: count
  int32_t c = 0, e = s;
  bool ok = true;
  if (s >= 0) {
    int32_t p = s;
    while (p < lo + C && p < len) {
      int32_t body, end;
      if (!step(p, body, end)) { ok = false; break; }
      ++c;
      p = end;
    }
    e = p;
  }
  link[lane] = e;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const unsigned long long have = __ballot(s >= 0);
  if (s >= 0 && lane > 0) {
    const unsigned long long front = have & ((1ull << lane) - 1ull);
    ok = ok && front != 0ull && link[63 - __builtin_clzll(front)] == s;
  }
  const int last = 63 - __builtin_clzll(have | 1ull);
  if (lane == last) ok = ok && e == len;
  // the counts: inclusive scan over the lanes
  int32_t incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  const int32_t total = __shfl(incl, 63, 64);
  if (__ballot(!ok) != 0ull || total != cnt || (have & 1ull) == 0ull) return false;
  // write
  if (s >= 0) {
    int32_t idx = incl - c, p = s;
    while (p < lo + C && p < len) {
      int32_t body, end;
      (void)step(p, body, end);
      rec_body[idx] = body;
      rec_end[idx] = end;
      ++idx;
      p = end;
    }
  }
  return true;
}

// A workgroup takes its section when lo_excl < byte_len and (byte_len <= cap or take_rest); byte_len <= cap is staged.
// kStates: the state-mode instantiation.  The mode travels in JsonCtx::states and is the same for every record of a launch, so the
// branch is taken where it is cheapest, at the launch: as a branch INSIDE the one kernel it cost the events path its register
// budget (80 VGPRs hold the kernel only because ~170 scalar registers already live in spare vector lanes; a second record path
// pushed those into scratch memory).
// kEnvelope: the same again for enveloped event values (JsonCtx::envelope, launch-uniform too): the envelope reader in front of
// the JSON walk is an instantiation of its own, and the two above keep their instructions and registers.
// kFloor: and once more for a push that carries a floor (decode_record; events mode only — the state topic is read from its
// beginning): floors[] holds one int64 per section, INT64_MIN where there is none.  Every other push launches the instantiations
// without it, which never read the argument.
template <int kSecThreads, bool kStates, bool kEnvelope, bool kFloor>
__global__ void __launch_bounds__(kSecThreads) __attribute__((amdgpu_waves_per_eu(kSecThreads == 256 ? 5 : 6)))  // (four waves at 80 VGPRs spill)
section_kernel(const uint8_t* __restrict__ bytes, const Section* __restrict__ sections, int64_t n_sections, int64_t lo_excl, int64_t cap, int32_t take_rest,
               uint64_t seed, JsonCtx jc, RecMeta* __restrict__ meta, uint4* __restrict__ ev_tmp, uint32_t* __restrict__ f64_host_list, ErrorCell* err,
               const int64_t* __restrict__ floors) {
  static_assert(!(kFloor && kStates), "the state topic has no floor");
  extern __shared__ __attribute__((aligned(16))) uint8_t sec_smem[];
  __shared__ int32_t s_pos, s_bad;
  __shared__ int32_t s_link[64];
  const Section sec = sections[blockIdx.x];
  if (sec.n_records <= 0) return;
  const int64_t len = sec.byte_len;
  if (!(len > lo_excl && (len <= cap || take_rest))) return;
  const bool staged = len <= cap && len < (1ll << 31);
#ifdef SURGE_EXPERIMENTS
#define SURGE_TICK(k) do { if (jc.ticks && threadIdx.x == 0) jc.ticks[4ull * blockIdx.x + (k)] = wall_clock64(); } while (0)
#else
#define SURGE_TICK(k) do { } while (0)
#endif
  SURGE_TICK(0);
  int32_t* const rec_body = (int32_t*)(sec_smem + ((cap + 47) & ~15ll));
  int32_t* const rec_end = rec_body + kSecRecs;
  const int64_t a0 = sec.byte_off & ~15ll;
  const int32_t skew = (int32_t)(sec.byte_off - a0);
  const int n16 = staged ? (int)((skew + len + 15) >> 4) : 0;
  if (staged) {  // (the staged bytes buffer ends 16 bytes after its last byte)
    for (int c = threadIdx.x; c < n16; c += kSecThreads) ((uint4*)sec_smem)[c] = *(const uint4*)(bytes + a0 + 16ll * c);
  }
  if (threadIdx.x == 0) { s_pos = 0; s_bad = -1; }
  __syncthreads();
  SURGE_TICK(1);
  if (jc.dbg) {  // timing experiments: every record of the batch is "skipped"
    RecMeta m;
    m.key_off = m.val_off = m.offset = 0; m.hash = 0; m.key_len = m.val_len = 0; m.slot = 0; m.status = RS_SKIP;
    for (int32_t i = threadIdx.x; i < sec.n_records; i += kSecThreads) { meta[sec.rec_first + i] = m; if constexpr (!kStates) ev_tmp[sec.rec_first + i] = make_uint4(0, 0, 0, 0); }
    if (jc.dbg == 1) return;
  }
  if (len >= (1ll << 31)) {  // a section of 2 GiB: nothing writes one (a batch's length is an int32)
    for (int32_t i0 = 0; i0 < sec.n_records; i0 += kSecThreads) {
      if constexpr (kStates) decode_state_record(bytes, 0, 0, i0 + (int32_t)threadIdx.x < sec.n_records, -1, -1, sec.rec_first + i0 + threadIdx.x, seed, meta, err);
      else decode_record<kEnvelope, kFloor>(bytes, 0, 0, 0, i0 + (int32_t)threadIdx.x < sec.n_records, -1, -1, sec.rec_first + i0 + threadIdx.x, seed, jc, meta, ev_tmp, f64_host_list, err);
    }
    return;
  }
  const lds_ptr_t lbase = (lds_ptr_t)sec_smem + skew;
  const uint8_t* gbase = bytes + sec.byte_off;
  int64_t floor = 0;
  if constexpr (kFloor) floor = floors[blockIdx.x];
  for (int32_t r0 = 0; r0 < sec.n_records; r0 += kSecRecs) {
    const int32_t cnt = sec.n_records - r0 < kSecRecs ? sec.n_records - r0 : kSecRecs;
    int32_t chained = 0;
    if (staged && sec.n_records <= kSecRecs && threadIdx.x < 64u) {  // (the first wave, all of it; a batch of one round)
      if (chain_records_parallel(lbase, (int32_t)len, cnt, rec_body, rec_end, s_link)) chained = cnt;
      else if (threadIdx.x == 0) atomicAdd(&err->reserved, 1u);
    }
    if (threadIdx.x == 0) {
      if (s_bad < 0) {
        if (chained < cnt) {  // not chained by the wave, or left by it at a record it does not read: the one-lane walk from there
          int32_t pos = s_pos, bad = 0;
          const bool ok = staged ? chain_records(lbase, (int32_t)len, &pos, cnt - chained, rec_body + chained, rec_end + chained, &bad)
                                 : chain_records(gbase, (int32_t)len, &pos, cnt - chained, rec_body + chained, rec_end + chained, &bad);
          s_pos = pos;
          if (!ok) {
            // everything from here to the end of the batch is unreadable: the rest is marked, the first is reported
            bad += chained;
            s_bad = r0 + bad;
            for (int32_t k = bad; k < cnt; ++k) rec_body[k] = -1;
            report(err, sec.rec_first + r0 + bad, RS_MALFORMED);
          }
        }
      } else {
        for (int32_t k = 0; k < cnt; ++k) rec_body[k] = -1;
      }
    }
    __syncthreads();
    SURGE_TICK(2);
    for (int32_t i0 = 0; i0 < (jc.dbg ? 0 : cnt); i0 += kSecThreads) {
      const int32_t i = i0 + (int32_t)threadIdx.x;
      const bool valid = i < cnt;
      const int32_t body = valid ? rec_body[i] : -1, end = body >= 0 ? rec_end[i] : -1;
      if constexpr (kStates) {
        if (staged) decode_state_record(lbase, sec.byte_off, sec.base_offset, valid, body, end, sec.rec_first + r0 + i, seed, meta, err);
        else decode_state_record(gbase, sec.byte_off, sec.base_offset, valid, body, end, sec.rec_first + r0 + i, seed, meta, err);
      } else if (staged) {
        decode_record<kEnvelope, kFloor>(lbase, sec.byte_off, sec.base_offset, floor, valid, body, end, sec.rec_first + r0 + i, seed, jc, meta, ev_tmp, f64_host_list, err);
      } else {
        decode_record<kEnvelope, kFloor>(gbase, sec.byte_off, sec.base_offset, floor, valid, body, end, sec.rec_first + r0 + i, seed, jc, meta, ev_tmp, f64_host_list, err);
      }
    }
    __syncthreads();
    SURGE_TICK(3);
  }
}

// records that arrive already framed (a JVM's ConsumerRecords: key bytes, value bytes, offset per record): the bytes buffer
// holds the keys first, the values from `val_base` on.  kEnvelope: enveloped event values — chosen at the launch like
// section_kernel's (as a branch inside the one kernel the envelope reader cost the bare path two vector registers)
template <bool kEnvelope>
__global__ void __launch_bounds__(256) records_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ key_off, const int64_t* __restrict__ val_off,
                                                      const int64_t* __restrict__ offsets, int64_t val_base, int64_t n_rec, uint64_t seed, JsonCtx jc,
                                                      RecMeta* __restrict__ meta, uint4* __restrict__ ev_tmp, uint32_t* __restrict__ f64_host_list, ErrorCell* err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n_rec;
  RecMeta m;
  m.key_off = m.val_off = m.offset = 0; m.hash = 0; m.key_len = m.val_len = 0; m.slot = 0; m.status = RS_MALFORMED;
  uint4 e = make_uint4(0, 0, 0, 0);
  bool has_value = false;
  if (valid) {
    const int64_t k0 = key_off[i], k1 = key_off[i + 1], v0 = val_off[i], v1 = val_off[i + 1];
    m.key_off = k0; m.val_off = val_base + v0; m.offset = offsets ? offsets[i] : i;
    if (k1 < k0 || v1 < v0 || k1 - k0 >= (1ll << 31) || v1 - v0 >= (1ll << 31)) {
      m.status = RS_MALFORMED;
    } else if (k1 == k0 && v1 == v0) {
      m.status = RS_SKIP;  // the producer's flush record
    } else {
      const uint8_t* key = bytes + k0;
      int n = 0;
      if (jc.states) n = (int)(k1 - k0);  // the id is the whole key; an empty value is the tombstone
      else while (n < (int)(k1 - k0) && key[n] != (uint8_t)':') ++n;
      m.key_len = n;
      m.val_len = (int32_t)(v1 - v0);
      m.hash = hash_key(key, n, seed);
      has_value = !jc.states;
      if (jc.states) m.status = RS_OK;
    }
  }
  if (!valid) return;
  if (has_value) {
    uint32_t st;
    if constexpr (kEnvelope) st = decode_enveloped_value(jc, bytes + m.val_off, m.val_len, bytes + m.key_off, m.key_len, &e);
    else st = decode_value(jc, bytes + m.val_off, m.val_len, &e);
    if (st == RS_F64_HOST) {
      f64_host_list[atomicAdd(&err->n_f64_host, 1u)] = (uint32_t)i;
      st = RS_OK;
    }
    m.status = st;
  }
  if (m.status >= RS_NULL) report(err, i, m.status);
  meta[i] = m;
  if (!jc.states) ev_tmp[i] = e;
}

}  // namespace

// chain + parse + decode, one workgroup per batch: sections up to 16.25 KiB (the reference producer closes a batch at 16 KiB)
// out of 18.3 KiB of LDS (8 workgroups per CU), the rest out of 66 KiB or, beyond 64 KiB, in place
// (round 5: a third, 8 KiB class in front — a publisher that flushes every 64 events writes 7 KiB batches, and 10.4 KiB of LDS
// instead of 18.3 lets a CU hold 15 of them; the workgroup is as wide as the push's largest batch needs)
// floors: one int64 per section for a push that carries a floor (nullptr: none — the instantiations without kFloor)
hipError_t launch_sections(const uint8_t* bytes, const Section* sections, int64_t n_sections, int32_t max_recs, uint64_t seed, JsonCtx jc, RecMeta* meta,
                           uint4* ev_tmp, uint32_t* f64_host_list, ErrorCell* err, const int64_t* floors, hipStream_t st) {
  if (floors && jc.states) return hipErrorInvalidValue;  // (stage 1 refuses it by name)
  const int64_t caps[3] = {8320, 16640, 65536};
  const int n_caps = 3;
#ifdef SURGE_EXPERIMENTS
  static unsigned long long* tick_buf = nullptr;
  static const bool want_ticks = std::getenv("SURGE_SECTION_TICKS") != nullptr;
  if (want_ticks && !tick_buf) (void)hipMalloc(&tick_buf, 4ull * 8 * 65536);
#endif
  for (int c = 0; c < n_caps; ++c) {
#ifdef SURGE_EXPERIMENTS
    if (want_ticks && n_sections <= 65536 && c == 1) {
      (void)hipMemsetAsync(tick_buf, 0, 4ull * 8 * 65536, st);
      jc.ticks = tick_buf;
    } else {
      jc.ticks = nullptr;
    }
#endif
    const size_t lds = (size_t)((caps[c] + 47) & ~15ll) + 2 * (size_t)kSecRecs * 4;
    const int64_t lo_excl = c == 0 ? -1 : caps[c - 1];
    const int32_t rest = c == n_caps - 1 ? 1 : 0;
#define SURGE_SECTION_LAUNCH(T, S, E, F)                                                                                                             \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(section_kernel<T, S, E, F>), dim3((unsigned)n_sections), dim3(T), lds, st, bytes, sections, n_sections, lo_excl, caps[c], rest, seed, jc, meta, \
                     ev_tmp, f64_host_list, err, floors)
#define SURGE_SECTION_WIDTH(S, E, F)                     \
  do {                                                   \
    if (max_recs <= 64) SURGE_SECTION_LAUNCH(64, S, E, F);        \
    else if (max_recs <= 128) SURGE_SECTION_LAUNCH(128, S, E, F); \
    else if (max_recs <= 192) SURGE_SECTION_LAUNCH(192, S, E, F); \
    else SURGE_SECTION_LAUNCH(256, S, E, F);                      \
  } while (0)
    const bool enveloped = jc.envelope && jc.tmpl;  // enveloped event values: an instantiation of their own
    if (jc.states) SURGE_SECTION_WIDTH(true, false, false);
    else if (floors && enveloped) SURGE_SECTION_WIDTH(false, true, true);  // a push that carries a floor: likewise
    else if (floors) SURGE_SECTION_WIDTH(false, false, true);
    else if (enveloped) SURGE_SECTION_WIDTH(false, true, false);
    else SURGE_SECTION_WIDTH(false, false, false);
#undef SURGE_SECTION_WIDTH
#undef SURGE_SECTION_LAUNCH
#ifdef SURGE_EXPERIMENTS
    if (jc.ticks) {  // (blocks: experiment runs only)
      (void)hipStreamSynchronize(st);
      std::vector<unsigned long long> t(4ull * (size_t)n_sections);
      (void)hipMemcpy(t.data(), tick_buf, t.size() * 8, hipMemcpyDeviceToHost);
      double sum[3] = {0, 0, 0};
      unsigned long long first = ~0ull, last = 0;
      size_t n = 0;
      for (size_t b = 0; b < (size_t)n_sections; ++b) {
        const unsigned long long* q = &t[4 * b];
        if (!q[0] || !q[3]) continue;
        ++n;
        for (int k = 0; k < 3; ++k) sum[k] += (double)(q[k + 1] - q[k]);
        first = q[0] < first ? q[0] : first;
        last = q[3] > last ? q[3] : last;
      }
      if (n) std::fprintf(stderr, "[surge experiments] section launch (class 2): %zu workgroups with work, mean us: staging %.2f, chain %.2f, decode %.2f; first start to last end %.1f us\n", n,
                          sum[0] / n / 100.0, sum[1] / n / 100.0, sum[2] / n / 100.0, (double)(last - first) / 100.0);
    }
#endif
  }
  return hipGetLastError();
}

hipError_t launch_records(const uint8_t* bytes, const int64_t* key_off, const int64_t* val_off, const int64_t* offsets, int64_t val_base, int64_t n_rec,
                          uint64_t seed, JsonCtx jc, RecMeta* meta, uint4* ev_tmp, uint32_t* f64_host_list, ErrorCell* err, hipStream_t st) {
  const auto kernel = (jc.envelope && jc.tmpl && !jc.states) ? records_kernel<true> : records_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, bytes, key_off, val_off, offsets, val_base, n_rec, seed, jc, meta,
                     ev_tmp, f64_host_list, err);
  return hipGetLastError();
}

}  // namespace ingest
}  // namespace surge
