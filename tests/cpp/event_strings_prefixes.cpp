// event_strings_prefixes.cpp — surge_event_json_string_spans (surge_amd/csrc/event_decode.cpp + event_strings_parse.h: the rule
// the device pass of ingest_strings.hip runs) under -fsanitize=address,undefined: it must never read at or beyond value + len.
// The corpus comes from tests/event_strings_cases.py through a file (argv[1]): records of {u8 rule, u8 whole, u32 length,
// 4 x u8 expected status (0xFF: not known), the value}.  Every value is copied into a malloc of EXACTLY its length; a `whole`
// value must give its expected statuses, and then every prefix of it is walked too; the others (seeded mutations) are walked as
// they are.  A span reported OK must lie between two quotes inside the value.  Built and run stand-alone by
// tests/test_event_strings.py; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "surge_ingest.h"

namespace {

int64_t g_walks = 0, g_ok = 0;
int g_failures = 0;

struct Rule {
  surge_event_json_template tmpl;
  surge_event_strings strings;
};

void set(char* dst, const char* s) { std::strncpy(dst, s, SURGE_EVJ_NAME - 1); }

void add_type(surge_event_json_template& t, const char* name, uint32_t type, const char* arg, uint32_t kind) {
  surge_event_json_type& e = t.types[t.n_types++];
  set(e.name, name);
  e.event_type = type;
  e.arg_kind = kind;
  set(e.arg_field, arg);
}

void add_string(surge_event_strings& s, const char* type, const char* field, uint32_t column) {
  surge_event_string_field& f = s.entry[s.n++];
  set(f.type_name, type);
  set(f.field, field);
  f.column = column;
}

// tests/event_strings_cases.py's RULES, in the order of their sorted names: bank, bank_env, short, two
std::vector<Rule> rules() {
  std::vector<Rule> r(4);
  for (Rule& x : r) std::memset(&x, 0, sizeof(x));
  const char* created = "docs.command.BankAccountCreated";
  for (int k = 0; k < 2; ++k) {
    set(r[k].tmpl.discriminator, "_type");
    add_type(r[k].tmpl, created, 0, "balance", SURGE_EVJ_ARG_F64);
    add_type(r[k].tmpl, "docs.command.BankAccountUpdated", 1, "newBalance", SURGE_EVJ_ARG_F64);
    add_string(r[k].strings, created, "accountOwner", 0);
    add_string(r[k].strings, created, "securityCode", 1);
  }
  r[1].tmpl.envelope = SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT;
  add_type(r[2].tmpl, "", 0, "", SURGE_EVJ_ARG_NONE);
  add_string(r[2].strings, "", "o", 3);
  set(r[3].tmpl.discriminator, "k");
  add_type(r[3].tmpl, "a", 0, "n", SURGE_EVJ_ARG_I32);
  add_type(r[3].tmpl, "b", 1, "n", SURGE_EVJ_ARG_I32);
  add_type(r[3].tmpl, "c", 2, "", SURGE_EVJ_ARG_NONE);
  add_string(r[3].strings, "a", "owner", 0);
  add_string(r[3].strings, "b", "label", 0);
  add_string(r[3].strings, "b", "tag", 2);
  return r;
}

// one walk over exactly `len` bytes; expect: 4 statuses or nullptr
void walk(const Rule& rule, const uint8_t* bytes, size_t len, const uint8_t* expect, const char* what) {
  uint8_t* v = (uint8_t*)std::malloc(len ? len : 1);
  std::memcpy(v, bytes, len);
  int64_t spans[8];
  uint8_t status[4];
  ++g_walks;
  const int32_t rc = surge_event_json_string_spans(&rule.tmpl, &rule.strings, v, (int64_t)len, spans, status);
  if (rc != 0 && rc != -7) { std::printf("FAIL %s: status %d\n", what, rc); ++g_failures; }
  bool refused = false;
  for (int c = 0; c < 4; ++c) {
    if (status[c] == SURGE_EVENT_STRING_OK) {
      ++g_ok;
      const int64_t off = spans[2 * c], n = spans[2 * c + 1];
      if (off < 1 || n < 0 || off + n >= (int64_t)len || v[off - 1] != '"' || v[off + n] != '"') { std::printf("FAIL %s: a span outside its quotes\n", what); ++g_failures; }
    } else if (status[c] != SURGE_EVENT_STRING_ABSENT) {
      refused = true;
    }
    if (expect && expect[c] != status[c]) { std::printf("FAIL %s: column %d status %d, expected %d\n", what, c, status[c], expect[c]); ++g_failures; }
  }
  if (refused != (rc == -7)) { std::printf("FAIL %s: the return value and the statuses disagree\n", what); ++g_failures; }
  std::free(v);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("FAIL usage: event_strings_prefixes <corpus>\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("FAIL cannot open the corpus\n"); return 2; }
  const std::vector<Rule> rs = rules();
  for (const Rule& r : rs)
    if (surge_event_strings_validate(&r.tmpl, &r.strings) != 0) { std::printf("FAIL a rule does not validate: %s\n", surge_event_json_last_error()); return 1; }
  int64_t n_cases = 0;
  uint8_t head[10];
  std::vector<uint8_t> value;
  while (std::fread(head, 1, sizeof(head), f) == sizeof(head)) {
    uint32_t len = 0;
    std::memcpy(&len, head + 2, 4);
    value.resize(len);
    if (len && std::fread(value.data(), 1, len, f) != len) { std::printf("FAIL the corpus is cut\n"); return 2; }
    if (head[0] >= rs.size()) { std::printf("FAIL unknown rule\n"); return 2; }
    const Rule& r = rs[head[0]];
    ++n_cases;
    walk(r, value.data(), len, head[1] ? head + 6 : nullptr, "value");
    if (head[1]) {
      for (size_t cut = 0; cut < len; ++cut) walk(r, value.data(), cut, nullptr, "prefix");
    }
  }
  std::fclose(f);
  std::printf("%s event_strings_prefixes: %lld cases, %lld walks, %lld spans, %d failures\n", g_failures || n_cases < 100 ? "FAIL" : "PASS", (long long)n_cases,
              (long long)g_walks, (long long)g_ok, g_failures);
  return g_failures || n_cases < 100 ? 1 : 0;
}
