// state_unescape_prefixes.cpp — surge_unescape_json_string (surge_amd/csrc/state_decode_host.cpp + state_parse.h: the routine
// the device kernels of state_strings.hip run) under -fsanitize=address,undefined: it must never read at or beyond
// raw + raw_len and never write beyond the length it reports.  Every case is copied into a malloc of EXACTLY raw_len bytes
// and unescaped into a malloc of EXACTLY the reported length (and, once more, of one byte less: nothing may be written
// then): every prefix of valid spans, and seeded random mutations of them over the bytes the routine branches on.
// Built and run stand-alone by tests/test_state_strings.py; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "surge_replay.h"

namespace {

int64_t g_cases = 0, g_ok = 0;
int g_failures = 0;

int64_t unescape_exact(const std::string& raw, std::string* out) {
  uint8_t* v = (uint8_t*)std::malloc(raw.size() ? raw.size() : 1);
  std::memcpy(v, raw.data(), raw.size());
  ++g_cases;
  const int64_t n = surge_unescape_json_string(v, (int64_t)raw.size(), nullptr, 0);
  if (n >= 0) {
    ++g_ok;
    uint8_t* o = (uint8_t*)std::malloc(n ? (size_t)n : 1);
    if (surge_unescape_json_string(v, (int64_t)raw.size(), o, n) != n) { std::printf("FAIL length changed with an output buffer\n"); ++g_failures; }
    if (out) out->assign((const char*)o, (size_t)n);
    std::free(o);
    if (n > 0) {  // one byte short: the length again, and not a byte written
      uint8_t* s = (uint8_t*)std::malloc((size_t)n - 1 ? (size_t)n - 1 : 1);
      std::memset(s, 0xA5, (size_t)n - 1 ? (size_t)n - 1 : 1);
      if (surge_unescape_json_string(v, (int64_t)raw.size(), s, n - 1) != n) { std::printf("FAIL length changed with a short buffer\n"); ++g_failures; }
      for (int64_t i = 0; i + 1 < n; ++i)
        if (s[i] != 0xA5) { std::printf("FAIL a short buffer was written\n"); ++g_failures; break; }
      std::free(s);
    }
  }
  std::free(v);
  return n;
}

uint32_t g_rng = 2463534242u;
uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5;
  return g_rng;
}

}  // namespace

int main() {
  struct Case { std::string raw, want; };
  const std::vector<Case> valid = {
      {"", ""},
      {"plain ascii", "plain ascii"},
      {"\\\"\\\\\\/\\b\\f\\n\\r\\t", "\"\\/\b\f\n\r\t"},
      {"\\u007f\\u0080\\u07ff\\u0800\\uffff\\uD7FF\\uE000", "\x7f\xc2\x80\xdf\xbf\xe0\xa0\x80\xef\xbf\xbf\xed\x9f\xbf\xee\x80\x80"},
      {"J \\\"q\\\" \\/ \\u20ac \xc3\xa9 \xe2\x82\xac \xf0\x9f\x98\x80", "J \"q\" / \xe2\x82\xac \xc3\xa9 \xe2\x82\xac \xf0\x9f\x98\x80"},
      {"\\u0041", "A"},
      {"end\\\\", "end\\"},
  };
  for (const Case& c : valid) {
    std::string got;
    if (unescape_exact(c.raw, &got) != (int64_t)c.want.size() || got != c.want) { std::printf("FAIL valid span: %s\n", c.raw.c_str()); ++g_failures; }
    for (size_t cut = 0; cut < c.raw.size(); ++cut) (void)unescape_exact(c.raw.substr(0, cut), nullptr);  // (a prefix may or may not be a span)
    const char alphabet[] = "\"\\u/bfnrt0123456789aAfFdD8 \x01\x1f\x7f\xc3\xff";
    for (int it = 0; it < 3000; ++it) {
      std::string m = c.raw.empty() ? std::string("\\u00e9x") : c.raw;
      const int edits = 1 + (int)(rnd() % 3);
      for (int e = 0; e < edits; ++e) {
        const size_t at = rnd() % m.size();
        switch (rnd() % 4) {
          case 0: m[at] = alphabet[rnd() % (sizeof(alphabet) - 1)]; break;
          case 1: m.insert(at, 1, alphabet[rnd() % (sizeof(alphabet) - 1)]); break;
          case 2: m.erase(at, 1 + rnd() % 3); break;
          default: m[at] = (char)(rnd() & 0xff); break;
        }
        if (m.empty()) m = "\\";
      }
      if (rnd() % 3 == 0) m.resize(rnd() % (m.size() + 1));
      (void)unescape_exact(m, nullptr);
    }
  }
  // the named refusals
  const struct { const char* raw; size_t len; int status; } bad[] = {
      {"a\x01", 2, SURGE_STATE_DECODE_STRING}, {"\\q", 2, SURGE_STATE_DECODE_ESCAPE}, {"\\ud800", 6, SURGE_STATE_DECODE_SURROGATE},
      {"ab\\", 3, SURGE_STATE_DECODE_STRING}, {"\\u12", 4, SURGE_STATE_DECODE_STRING}, {"\\u12g4", 6, SURGE_STATE_DECODE_ESCAPE}, {"a\"b", 3, SURGE_STATE_DECODE_STRING}};
  for (const auto& b : bad)
    if (unescape_exact(std::string(b.raw, b.len), nullptr) != -(int64_t)b.status) { std::printf("FAIL status of %s\n", b.raw); ++g_failures; }
  std::printf("%s state_unescape_prefixes: %lld cases, %lld unescaped, %d failures\n", g_failures ? "FAIL" : "PASS", (long long)g_cases, (long long)g_ok, g_failures);
  return g_failures ? 1 : 0;
}
