// state_envelope_prefixes.cpp — surge_decode_protobuf_state (surge_amd/csrc/state_decode_host.cpp + state_parse.h) under
// -fsanitize=address,undefined: the envelope grammar and the payload parser behind it must never read at or beyond
// value + len.  Every case is copied into a malloc of EXACTLY len bytes (so one byte too far is a heap-buffer-overflow
// report): every proper prefix of valid enveloped SDK-sample, Counter and BankAccount values, the values with a byte appended,
// and seeded random mutations of them (the tag, varint and JSON bytes the parser branches on, written, inserted and cut
// anywhere).  Built and run stand-alone by tests/test_state_envelope.py; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "surge_replay.h"

namespace {

surge_json_template make_template(const std::vector<std::pair<int, std::string>>& parts) {  // kind, literal text / field offset as text
  surge_json_template t;
  std::memset(&t, 0, sizeof(t));
  uint32_t pool = 0;
  for (const auto& p : parts) {
    auto& pt = t.part[t.n_parts++];
    pt.kind = (uint32_t)p.first;
    if (p.first == (int)SURGE_JP_LITERAL) {
      pt.lit_off = pool;
      pt.lit_len = (uint32_t)p.second.size();
      std::memcpy(t.literals + pool, p.second.data(), p.second.size());
      pool += pt.lit_len;
    } else if (p.first != (int)SURGE_JP_KEY) {
      pt.field_offset = (uint32_t)std::atoi(p.second.c_str());
    }
  }
  return t;
}

std::string varint(uint64_t v) {
  std::string out;
  while (v >= 0x80) { out.push_back((char)((v & 0x7F) | 0x80)); v >>= 7; }
  out.push_back((char)v);
  return out;
}

// State{aggregateId, payload} as proto3 writes it: an empty field is left out
std::string envelope(const std::string& id, const std::string& payload) {
  std::string out;
  if (!id.empty()) out += "\x0a" + varint(id.size()) + id;
  if (!payload.empty()) out += "\x12" + varint(payload.size()) + payload;
  return out;
}

int64_t g_cases = 0, g_ok = 0;

int32_t decode_exact(const surge_json_template& t, const std::string& text, const std::string* key, int64_t* span_out = nullptr) {
  uint8_t* v = (uint8_t*)std::malloc(text.size() ? text.size() : 1);  // (a zero-length case reads nothing at all)
  std::memcpy(v, text.data(), text.size());
  uint8_t* k = nullptr;
  if (key) {
    k = (uint8_t*)std::malloc(key->size() ? key->size() : 1);
    std::memcpy(k, key->data(), key->size());
  }
  uint8_t state[64];
  int64_t span[2 * SURGE_JSON_STRING_COLUMNS];
  const int32_t rc = surge_decode_protobuf_state(&t, v, (int64_t)text.size(), k, key ? (int64_t)key->size() : -1, state, span);
  if (rc == 0 && span_out) std::memcpy(span_out, span, sizeof(span));
  std::free(v);
  std::free(k);
  ++g_cases;
  g_ok += rc == 0;
  return rc;
}

uint32_t g_rng = 20240607u;
uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
  return g_rng;
}

}  // namespace

int main() {
  const surge_json_template sdk = make_template({{SURGE_JP_LITERAL, "{\"balance\":"}, {SURGE_JP_I32, "0"}, {SURGE_JP_LITERAL, "}"}});
  const surge_json_template counter = make_template({{SURGE_JP_LITERAL, "{\"aggregateId\":"}, {SURGE_JP_KEY, ""}, {SURGE_JP_LITERAL, ",\"count\":"},
                                                     {SURGE_JP_I32, "0"}, {SURGE_JP_LITERAL, ",\"version\":"}, {SURGE_JP_I32, "4"}, {SURGE_JP_LITERAL, "}"}});
  const surge_json_template bank = make_template({{SURGE_JP_LITERAL, "{\"accountNumber\":"}, {SURGE_JP_KEY, ""}, {SURGE_JP_LITERAL, ",\"accountOwner\":"},
                                                  {SURGE_JP_STR, "0"}, {SURGE_JP_LITERAL, ",\"securityCode\":"}, {SURGE_JP_STR, "1"},
                                                  {SURGE_JP_LITERAL, ",\"balance\":"}, {SURGE_JP_F64, "16"}, {SURGE_JP_LITERAL, "}"}});
  struct Case { const surge_json_template* t; std::string key, payload; };
  const std::string id200(200, 'k');
  const std::vector<Case> valid = {
      {&sdk, "0c3f1d9e-7a55-4a5c-9d5e-00000000002a", "{\"balance\":-2147483648}"},
      {&sdk, "", "{\"balance\":7}"},
      {&sdk, id200, "{\"balance\":2147483647}"},
      {&counter, "agg-\xc3\xa9\n\\", "{\"aggregateId\":\"agg-\\u00e9\\n\\\\\",\"count\":-2147483648,\"version\":2147483647}"},
      {&bank, "a-1", "{\"accountNumber\":\"a-1\",\"accountOwner\":\"J \\\"q\\\" \\/ \\u20ac\",\"securityCode\":\"\",\"balance\":-1.25E+3}"},
      {&bank, "k", "{\"accountNumber\":\"k\",\"accountOwner\":\"" + std::string(150, 'o') +
                       "\",\"securityCode\":\"0001\",\"balance\":0.1000000000000000055511151231257827021181583404541015625}"},
  };
  int failures = 0;
  for (const Case& c : valid) {
    const std::string text = envelope(c.key, c.payload);
    int64_t span[2 * SURGE_JSON_STRING_COLUMNS] = {0};
    if (decode_exact(*c.t, text, &c.key, span) != 0 || decode_exact(*c.t, text, nullptr) != 0) { std::printf("FAIL valid value refused: %s\n", c.payload.c_str()); ++failures; }
    if (c.t == &bank) {  // the spans are relative to the value: the bytes before each are the opening quote
      for (int col = 0; col < 2; ++col)
        if (span[2 * col] < 1 || span[2 * col] + span[2 * col + 1] >= (int64_t)text.size() || text[(size_t)span[2 * col] - 1] != '"' ||
            text[(size_t)(span[2 * col] + span[2 * col + 1])] != '"') { std::printf("FAIL span of column %d\n", col); ++failures; }
    }
    for (size_t cut = 0; cut < text.size(); ++cut)
      for (const std::string* k : {&c.key, (const std::string*)nullptr})
        if (decode_exact(*c.t, text.substr(0, cut), k) == 0) { std::printf("FAIL prefix %zu accepted: %s\n", cut, c.payload.c_str()); ++failures; }
    for (const char extra : {' ', '}', '\0', '\x0a', '\x12'})
      if (decode_exact(*c.t, text + extra, &c.key) != SURGE_STATE_DECODE_ENVELOPE) { std::printf("FAIL no ENVELOPE: %s\n", c.payload.c_str()); ++failures; }
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
  const std::string pay = "{\"balance\":1}", f2 = "\x12" + varint(pay.size()) + pay, hello = "hello";
  if (decode_exact(sdk, std::string("\x0a\x85\x00", 3) + "hello" + f2, &hello) != 0) { std::printf("FAIL 2-byte varint for 5\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\x85\x80\x80\x80\x00", 6) + "hello" + f2, &hello) != 0) { std::printf("FAIL 5-byte varint for 5\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\x85\x80\x80\x80\x80\x00", 7) + "hello" + f2, &hello) != SURGE_STATE_DECODE_ENVELOPE) { std::printf("FAIL 6-byte varint\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\x80\x80\x80\x80\x08", 6) + "hello" + f2, &hello) != SURGE_STATE_DECODE_ENVELOPE) { std::printf("FAIL length 2^31\n"); ++failures; }
  if (decode_exact(sdk, std::string("\x0a\xff\xff\xff\xff\x07", 6) + "hello" + f2, &hello) != SURGE_STATE_DECODE_ENVELOPE) { std::printf("FAIL length 2^31 - 1 beyond the end\n"); ++failures; }
  std::printf("%s state_envelope_prefixes: %lld cases, %lld decoded, %d failures\n", failures ? "FAIL" : "PASS", (long long)g_cases, (long long)g_ok, failures);
  return failures ? 1 : 0;
}
