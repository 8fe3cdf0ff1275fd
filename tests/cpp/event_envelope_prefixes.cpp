// event_envelope_prefixes.cpp — surge_event_json_decode_keyed (surge_amd/csrc/event_decode.cpp + state_parse.h) under
// -fsanitize=address,undefined: with an enveloped template the envelope reader and the event parser behind it must never read
// at or beyond value + len, nor the key beyond key + key_len.  Every case is copied into a malloc of EXACTLY len bytes (so one
// byte too far is a heap-buffer-overflow report): every proper prefix of valid enveloped values, the values with a byte
// appended, and seeded random mutations of them (the tag, varint and JSON bytes the parsers branch on, written, inserted and
// cut anywhere).  Built and run stand-alone by tests/test_event_envelope.py; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "surge_ingest.h"

namespace {

surge_event_json_template make_template(const char* discriminator, const char* type_name, const char* seq, const char* arg, uint32_t arg_kind, uint32_t envelope) {
  surge_event_json_template t;
  std::memset(&t, 0, sizeof(t));
  t.n_types = 1;
  t.envelope = envelope;
  std::strcpy(t.discriminator, discriminator);
  std::strcpy(t.types[0].name, type_name);
  t.types[0].event_type = 5;
  t.types[0].arg_kind = arg_kind;
  std::strcpy(t.types[0].seq_field, seq);
  std::strcpy(t.types[0].arg_field, arg);
  return t;
}

std::string varint(uint64_t v) {
  std::string out;
  while (v >= 0x80) { out.push_back((char)((v & 0x7F) | 0x80)); v >>= 7; }
  out.push_back((char)v);
  return out;
}

// Event{aggregateId, payload} as proto3 writes it: an empty field is left out
std::string envelope(const std::string& id, const std::string& payload) {
  std::string out;
  if (!id.empty()) out += "\x0a" + varint(id.size()) + id;
  if (!payload.empty()) out += "\x12" + varint(payload.size()) + payload;
  return out;
}

int64_t g_cases = 0, g_ok = 0;

int32_t decode_exact(const surge_event_json_template& t, const std::string& text, const std::string* key, uint8_t* event16 = nullptr) {
  uint8_t* v = (uint8_t*)std::malloc(text.size() ? text.size() : 1);  // (a zero-length case reads nothing at all)
  std::memcpy(v, text.data(), text.size());
  uint8_t* k = nullptr;
  if (key) {
    k = (uint8_t*)std::malloc(key->size() ? key->size() : 1);
    std::memcpy(k, key->data(), key->size());
  }
  uint8_t ev[16];
  const int32_t rc = surge_event_json_decode_keyed(&t, k, key ? (int64_t)key->size() : -1, v, (int64_t)text.size(), ev);
  if (rc == 0 && event16) std::memcpy(event16, ev, 16);
  std::free(v);
  std::free(k);
  ++g_cases;
  g_ok += rc == 0;
  return rc;
}

uint32_t g_rng = 20250611u;
uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
  return g_rng;
}

}  // namespace

int main() {
  const surge_event_json_template sdk = make_template("", "", "", "amount", SURGE_EVJ_ARG_I32, SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT);
  const surge_event_json_template sdk_bare = make_template("", "", "", "amount", SURGE_EVJ_ARG_I32, SURGE_EVJ_ENVELOPE_NONE);
  const surge_event_json_template f64 = make_template("", "", "", "x", SURGE_EVJ_ARG_F64, SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT);
  const surge_event_json_template f64_bare = make_template("", "", "", "x", SURGE_EVJ_ARG_F64, SURGE_EVJ_ENVELOPE_NONE);
  const surge_event_json_template inc = make_template("_type", "countIncremented", "sequenceNumber", "incrementBy", SURGE_EVJ_ARG_I32, SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT);
  const surge_event_json_template inc_bare = make_template("_type", "countIncremented", "sequenceNumber", "incrementBy", SURGE_EVJ_ARG_I32, SURGE_EVJ_ENVELOPE_NONE);
  struct Case { const surge_event_json_template *t, *bare; std::string key, payload; };
  const std::string id200(200, 'k');
  const std::vector<Case> valid = {
      {&sdk, &sdk_bare, "0c3f1d9e-7a55-4a5c-9d5e-00000000002a", "{\"amount\":-2147483648}"},
      {&sdk, &sdk_bare, "", "{\"amount\":7}"},
      {&sdk, &sdk_bare, id200, "{\"amount\":2147483647}"},
      {&sdk, &sdk_bare, "agg-\xc3\xa9\n\\", " { \"x\" : [1, {\"amount\": 3}], \"amount\" : 5 , \"s\":\"}\\\"\" } "},
      {&sdk, &sdk_bare, "p", "{\"amount\":1,\"pad\":\"" + std::string(150, 'p') + "\"}"},
      {&f64, &f64_bare, "a-1", "{\"x\":-1.25E+3}"},
      {&f64, &f64_bare, "k", "{\"x\":0.1000000000000000055511151231257827021181583404541015625}"},
      {&inc, &inc_bare, "c1", "{\"aggregateId\":\"c1\",\"incrementBy\":3,\"sequenceNumber\":4,\"_type\":\"countIncremented\"}"},
  };
  int failures = 0;
  for (const Case& c : valid) {
    const std::string text = envelope(c.key, c.payload);
    uint8_t got[16], got_nokey[16], want[16];
    if (decode_exact(*c.t, text, &c.key, got) != 0 || decode_exact(*c.t, text, nullptr, got_nokey) != 0 || decode_exact(*c.bare, c.payload, nullptr, want) != 0 ||
        std::memcmp(got, want, 16) != 0 || std::memcmp(got_nokey, want, 16) != 0) {
      std::printf("FAIL valid value refused or decoded differently from its bare payload: %s\n", c.payload.c_str());
      ++failures;
    }
    const std::string longer = c.key + "x", colon = c.key + ":1";
    if (decode_exact(*c.t, text, &longer) != SURGE_E_CORRUPT || decode_exact(*c.t, text, &colon) != SURGE_E_CORRUPT) { std::printf("FAIL another key accepted\n"); ++failures; }
    if (decode_exact(*c.bare, text, &c.key) == 0) { std::printf("FAIL the bare template read an enveloped value\n"); ++failures; }
    for (size_t cut = 0; cut < text.size(); ++cut)
      for (const std::string* k : {&c.key, (const std::string*)nullptr})
        if (decode_exact(*c.t, text.substr(0, cut), k) == 0) { std::printf("FAIL prefix %zu accepted: %s\n", cut, c.payload.c_str()); ++failures; }
    for (const char extra : {'}', '\0', '\x0a', '\x12', 'x'})
      if (decode_exact(*c.t, text + extra, &c.key) != SURGE_E_CORRUPT) { std::printf("FAIL a byte behind field 2 accepted: %s\n", c.payload.c_str()); ++failures; }
    // mutations: the bytes the two parsers branch on, anywhere (half of them in the envelope's own bytes); cuts after them
    const char alphabet[] = "\x0a\x12\x1a\x08\x10\x01\x7f\x80\x81\x85\xff\"\\u/bfnrt0123456789aAfF-+.eE{}:, ";
    const size_t head = text.size() - c.payload.size();
    for (int it = 0; it < 4000; ++it) {
      std::string m = text;
      const int edits = 1 + (int)(rnd() % 3);
      for (int e = 0; e < edits; ++e) {
        const size_t at = (rnd() & 1) ? rnd() % m.size() : rnd() % (head < m.size() ? head + 1 : m.size());
        switch (rnd() % 4) {
          case 0: m[at] = alphabet[rnd() % (sizeof(alphabet) - 1)]; break;
          case 1: m.insert(at, 1, alphabet[rnd() % (sizeof(alphabet) - 1)]); break;
          case 2: m.erase(at, 1 + rnd() % 3); break;
          default: m[at] = (char)(rnd() & 0xff); break;
        }
        if (m.empty()) m = "\x0a";
      }
      if (rnd() % 3 == 0) m.resize(rnd() % (m.size() + 1));
      (void)decode_exact(*c.t, m, (rnd() & 1) ? &c.key : nullptr);
    }
  }
  // hand-spelled lengths: over-long varints are read, a 5th byte that continues and a length beyond 2^31 - 1 are not
  const std::string pay = "{\"amount\":1}", f2 = "\x12" + varint(pay.size()) + pay, hello = "hello";
  if (decode_exact(sdk, std::string("\x0a\x85\x00", 3) + "hello" + f2, &hello) != 0) { std::printf("FAIL 2-byte varint for 5\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\x85\x80\x80\x80\x00", 6) + "hello" + f2, &hello) != 0) { std::printf("FAIL 5-byte varint for 5\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\x85\x80\x80\x80\x80\x00", 7) + "hello" + f2, &hello) != SURGE_E_CORRUPT) { std::printf("FAIL 6-byte varint\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\x80\x80\x80\x80\x08", 6) + "hello" + f2, &hello) != SURGE_E_CORRUPT) { std::printf("FAIL length 2^31\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\xff\xff\xff\xff\x07", 6) + "hello" + f2, &hello) != SURGE_E_CORRUPT) { std::printf("FAIL length 2^31 - 1 beyond the end\n"); ++failures; }
  surge_event_json_template unknown = sdk;
  unknown.envelope = 2;
  if (surge_event_json_validate(&unknown) == 0 || decode_exact(unknown, pay, nullptr) == 0) { std::printf("FAIL unknown envelope value accepted\n"); ++failures; }
  std::printf("%s event_envelope_prefixes: %lld cases, %lld decoded, %d failures\n", failures ? "FAIL" : "PASS", (long long)g_cases, (long long)g_ok, failures);
  return failures ? 1 : 0;
}
