// state_parse_prefixes.cpp — surge_decode_json_state (surge_amd/csrc/state_decode_host.cpp + state_parse.h) under
// -fsanitize=address,undefined: the parser must never read at or beyond value + len.  Every case is copied into a malloc of
// EXACTLY len bytes (so one byte too far is a heap-buffer-overflow report): every proper prefix of valid Counter and
// BankAccount texts, the texts with a byte appended, and seeded random mutations of them (byte flips, cuts, splices of the
// bytes the parser branches on).  Built and run stand-alone by tests/test_state_decode.py; never loaded into Python.
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

int32_t decode_exact(const surge_json_template& t, const std::string& text, const std::string* key) {
  uint8_t* v = (uint8_t*)std::malloc(text.size() ? text.size() : 1);  // (a zero-length case reads nothing at all)
  std::memcpy(v, text.data(), text.size());
  uint8_t* k = nullptr;
  if (key) {
    k = (uint8_t*)std::malloc(key->size() ? key->size() : 1);
    std::memcpy(k, key->data(), key->size());
  }
  uint8_t state[64];
  int64_t span[2 * SURGE_JSON_STRING_COLUMNS];
  const int32_t rc = surge_decode_json_state(&t, v, (int64_t)text.size(), k, key ? (int64_t)key->size() : -1, state, span);
  std::free(v);
  std::free(k);
  ++g_cases;
  g_ok += rc == 0;
  return rc;
}

uint32_t g_rng = 12345u;
uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
  return g_rng;
}

}  // namespace

int main() {
  const surge_json_template counter = make_template({{SURGE_JP_LITERAL, "{\"aggregateId\":"}, {SURGE_JP_KEY, ""}, {SURGE_JP_LITERAL, ",\"count\":"},
                                                     {SURGE_JP_I32, "0"}, {SURGE_JP_LITERAL, ",\"version\":"}, {SURGE_JP_I32, "4"}, {SURGE_JP_LITERAL, "}"}});
  const surge_json_template bank = make_template({{SURGE_JP_LITERAL, "{\"accountNumber\":"}, {SURGE_JP_KEY, ""}, {SURGE_JP_LITERAL, ",\"accountOwner\":"},
                                                  {SURGE_JP_STR, "0"}, {SURGE_JP_LITERAL, ",\"securityCode\":"}, {SURGE_JP_STR, "1"},
                                                  {SURGE_JP_LITERAL, ",\"balance\":"}, {SURGE_JP_F64, "16"}, {SURGE_JP_LITERAL, "}"}});
  struct Case { const surge_json_template* t; std::string text, key; };
  const std::vector<Case> valid = {
      {&counter, "{\"aggregateId\":\"agg-\\u00e9\\n\\\\\",\"count\":-2147483648,\"version\":2147483647}", "agg-\xc3\xa9\n\\"},
      {&counter, "{\"aggregateId\":\"\",\"count\":0,\"version\":7}", ""},
      {&bank, "{\"accountNumber\":\"a-1\",\"accountOwner\":\"J \\\"q\\\" \\/ \\u20ac\",\"securityCode\":\"\",\"balance\":-1.25E+3}", "a-1"},
      {&bank, "{\"accountNumber\":\"k\",\"accountOwner\":\"o\",\"securityCode\":\"0001\",\"balance\":0.1000000000000000055511151231257827021181583404541015625}", "k"},
      {&bank, "{\"accountNumber\":\"k\",\"accountOwner\":\"o\",\"securityCode\":\"0001\",\"balance\":4.9E-324}", "k"},
  };
  int failures = 0;
  for (const Case& c : valid) {
    if (decode_exact(*c.t, c.text, &c.key) != 0 || decode_exact(*c.t, c.text, nullptr) != 0) { std::printf("FAIL valid text refused: %s\n", c.text.c_str()); ++failures; }
    for (size_t cut = 0; cut < c.text.size(); ++cut)
      for (const std::string* k : {&c.key, (const std::string*)nullptr})
        if (decode_exact(*c.t, c.text.substr(0, cut), k) == 0) { std::printf("FAIL prefix %zu accepted: %s\n", cut, c.text.c_str()); ++failures; }
    for (const char extra : {' ', '}', '\0', '1'})
      if (decode_exact(*c.t, c.text + extra, &c.key) != SURGE_STATE_DECODE_TRAILING) { std::printf("FAIL no TRAILING: %s\n", c.text.c_str()); ++failures; }
    // mutations: the bytes the parser branches on, anywhere; cuts after them
    const char alphabet[] = "\"\\u/bfnrt0123456789aAfF-+.eE{}:, \x01\x7f\xc3\xff";
    for (int it = 0; it < 4000; ++it) {
      std::string m = c.text;
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
      (void)decode_exact(*c.t, m, (rnd() & 1) ? &c.key : nullptr);
    }
  }
  std::printf("%s state_parse_prefixes: %lld cases, %lld decoded, %d failures\n", failures ? "FAIL" : "PASS", (long long)g_cases, (long long)g_ok, failures);
  return failures ? 1 : 0;
}
