// state_lenient_prefixes.cpp — surge_decode_json_state_lenient / surge_decode_protobuf_state_lenient
// (surge_amd/csrc/state_decode_host.cpp + state_parse.h) under -fsanitize=address,undefined: the lenient parser must never
// read at or beyond value + len.  Every case is copied into a malloc of EXACTLY len bytes (so one byte too far is a
// heap-buffer-overflow report): every proper prefix of reordered, spaced texts with unknown members of every JSON type — bare
// and inside the protobuf State envelope —, the texts with a byte appended, and seeded one- to three-byte mutations of them.
// Built and run stand-alone by tests/test_state_lenient.py; never loaded into Python.
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

int64_t g_cases = 0, g_ok = 0;

int32_t decode_exact(const surge_json_template& t, const std::string& text, const std::string* key, bool envelope) {
  uint8_t* v = (uint8_t*)std::malloc(text.size() ? text.size() : 1);  // (a zero-length case reads nothing at all)
  std::memcpy(v, text.data(), text.size());
  uint8_t* k = nullptr;
  if (key) {
    k = (uint8_t*)std::malloc(key->size() ? key->size() : 1);
    std::memcpy(k, key->data(), key->size());
  }
  uint8_t state[64];
  int64_t span[2 * SURGE_JSON_STRING_COLUMNS];
  const int32_t rc = (envelope ? surge_decode_protobuf_state_lenient : surge_decode_json_state_lenient)(&t, v, (int64_t)text.size(), k,
                                                                                                        key ? (int64_t)key->size() : -1, state, span);
  if (rc == 0) {  // the spans lie inside the value
    for (int c = 0; c < SURGE_JSON_STRING_COLUMNS; ++c)
      if (span[2 * c] < 0 || span[2 * c + 1] < 0 || span[2 * c] + span[2 * c + 1] > (int64_t)text.size()) { std::printf("FAIL span outside the value: %s\n", text.c_str()); std::exit(1); }
  }
  std::free(v);
  std::free(k);
  ++g_cases;
  g_ok += rc == 0;
  return rc;
}

std::string varint(size_t n) {
  std::string s;
  while (n >= 0x80) { s.push_back((char)(0x80 | (n & 0x7F))); n >>= 7; }
  s.push_back((char)n);
  return s;
}

std::string wrap(const std::string& key, const std::string& payload) {  // State{aggregateId, payload}; proto3 omits an empty field
  std::string s;
  if (!key.empty()) s += "\x0a" + varint(key.size()) + key;
  if (!payload.empty()) s += "\x12" + varint(payload.size()) + payload;
  return s;
}

uint32_t g_rng = 24680u;
uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
  return g_rng;
}

std::string nested(int depth, bool objects) {
  std::string s = "1";
  for (int d = 0; d < depth; ++d) s = objects ? "{\"a\":" + s + "}" : "[" + s + "]";
  return s;
}

}  // namespace

int main() {
  const surge_json_template counter = make_template({{SURGE_JP_LITERAL, "{\"aggregateId\":"}, {SURGE_JP_KEY, ""}, {SURGE_JP_LITERAL, ",\"count\":"},
                                                     {SURGE_JP_I32, "0"}, {SURGE_JP_LITERAL, ",\"version\":"}, {SURGE_JP_I32, "4"}, {SURGE_JP_LITERAL, "}"}});
  const surge_json_template bank = make_template({{SURGE_JP_LITERAL, "{\"accountNumber\":"}, {SURGE_JP_KEY, ""}, {SURGE_JP_LITERAL, ",\"accountOwner\":"},
                                                  {SURGE_JP_STR, "0"}, {SURGE_JP_LITERAL, ",\"securityCode\":"}, {SURGE_JP_STR, "1"},
                                                  {SURGE_JP_LITERAL, ",\"balance\":"}, {SURGE_JP_F64, "16"}, {SURGE_JP_LITERAL, "}"}});
  const surge_json_template sdk = make_template({{SURGE_JP_LITERAL, "{\"balance\":"}, {SURGE_JP_I32, "0"}, {SURGE_JP_LITERAL, "}"}});
  struct Case { const surge_json_template* t; std::string text, key; };
  const std::vector<Case> valid = {  // (each ends with its closing brace: every proper prefix is refused)
      {&counter, "{\"aggregateId\":\"agg-\\u00e9\\n\\\\\",\"count\":-2147483648,\"version\":2147483647}", "agg-\xc3\xa9\n\\"},
      {&counter, " {\t\"version\" : 7 ,\r\n\"x\":[1,{\"a\":\"b\\\"}\"},[],{}],\"\\u0063ount\":0,\"aggregateId\":\"\",\"n\":null,\"t\":true,\"f\":false,\"e\":-0.5e+10}", ""},
      {&counter, "{\"count\":1,\"count\":2,\"coun\":\"\\uD83D\\uDE00\",\"counter\":{\"count\":[]},\"\":0,\"version\":3,\"aggregateId\":\"k\",\"aggregateId\":\"k\"}", "k"},
      {&counter, "{\"deep\":" + nested(32, false) + ",\"deeper\":" + nested(32, true) + ",\"aggregateId\":\"k\",\"count\":1,\"version\":2}", "k"},
      {&bank, "{\"balance\":-1.25E+3,\"securityCode\":\"\",\"later\":{\"since\":[2]},\"accountOwner\":\"J \\\"q\\\" \\/ \\u20ac\",\"accountNumber\":\"a-1\"}", "a-1"},
      {&bank, "{ \"accountOwner\" : \"first\" , \"accountNumber\":\"k\",\"accountOwner\":\"o\\\\\",\"securityCode\":\"0001\",\"balance\":0.1000000000000000055511151231257827021181583404541015625 }", "k"},
      {&bank, "{\"accountNumber\":\"k\",\"balance\":4.9E-324,\"accountOwner\":\"o\",\"securityCode\":\"0001\"}", "k"},
      {&sdk, "{\"owner\":\"x\",\"balance\":-12}", "k1"},
  };
  int failures = 0;
  for (const Case& c : valid) {
    for (const bool envelope : {false, true}) {
      const std::string text = envelope ? wrap(c.key, c.text) : c.text;
      if (decode_exact(*c.t, text, &c.key, envelope) != 0 || decode_exact(*c.t, text, nullptr, envelope) != 0) { std::printf("FAIL valid text refused: %s\n", c.text.c_str()); ++failures; }
      for (size_t cut = 0; cut < text.size(); ++cut)
        for (const std::string* k : {&c.key, (const std::string*)nullptr})
          if (decode_exact(*c.t, text.substr(0, cut), k, envelope) == 0) { std::printf("FAIL prefix %zu accepted: %s\n", cut, c.text.c_str()); ++failures; }
      if (!envelope) {
        for (const char extra : {' ', '\t', '\n', '\r'})
          if (decode_exact(*c.t, c.text + extra, &c.key, false) != 0) { std::printf("FAIL whitespace behind the object refused: %s\n", c.text.c_str()); ++failures; }
        for (const char extra : {'}', '\0', '1', ','})
          if (decode_exact(*c.t, c.text + extra, &c.key, false) != SURGE_STATE_DECODE_TRAILING) { std::printf("FAIL no TRAILING: %s\n", c.text.c_str()); ++failures; }
      }
      // mutations: the bytes the parser branches on, anywhere; cuts after them
      const char alphabet[] = "\"\\u/bfnrt0123456789aAfF-+.eE{}[]:, \t\n\x01\x1f\x7f\xc3\xff";
      for (int it = 0; it < 3000; ++it) {
        std::string m = text;
        const int edits = 1 + (int)(rnd() % 3);
        for (int e = 0; e < edits; ++e) {
          const size_t at = rnd() % m.size();
          switch (rnd() % 4) {
            case 0: m[at] = alphabet[rnd() % (sizeof(alphabet) - 1)]; break;
            case 1: m.insert(at, 1, alphabet[rnd() % (sizeof(alphabet) - 1)]); break;
            case 2: m.erase(at, 1 + rnd() % 3); break;
            default: m[at] = (char)(rnd() & 0xff); break;
          }
          if (m.empty()) m = "{";
        }
        if (rnd() % 3 == 0) m.resize(rnd() % (m.size() + 1));
        (void)decode_exact(*c.t, m, (rnd() & 1) ? &c.key : nullptr, envelope);
      }
    }
  }
  // nesting one deeper than the stack holds, and a template the mode cannot read
  if (decode_exact(counter, "{\"deep\":" + nested(33, false) + ",\"aggregateId\":\"k\",\"count\":1,\"version\":2}", nullptr, false) != SURGE_STATE_DECODE_SYNTAX) { std::printf("FAIL depth 33 arrays\n"); ++failures; }
  if (decode_exact(counter, "{\"deep\":" + nested(33, true) + ",\"aggregateId\":\"k\",\"count\":1,\"version\":2}", nullptr, false) != SURGE_STATE_DECODE_SYNTAX) { std::printf("FAIL depth 33 objects\n"); ++failures; }
  const surge_json_template flat = make_template({{SURGE_JP_LITERAL, "balance="}, {SURGE_JP_I32, "0"}, {SURGE_JP_LITERAL, "\n"}});
  if (decode_exact(flat, "balance=1\n", nullptr, false) != SURGE_E_UNSUPPORTED) { std::printf("FAIL a template of another shape was not refused\n"); ++failures; }
  std::printf("%s state_lenient_prefixes: %lld cases, %lld decoded, %d failures\n", failures ? "FAIL" : "PASS", (long long)g_cases, (long long)g_ok, failures);
  return failures ? 1 : 0;
}
