// snappy_prefixes.cpp — the snappy reader (surge_amd/csrc/snappy_block.h through snappy_frame.cpp's exports) under
// -fsanitize=address,undefined: it must never read at or beyond src + len and never write beyond the capacity given.
// The corpus comes from tests/snappy_cases.py through a file (argv[1]): records of {u8 whole, u8 expected status (0xFF: not
// known), u32 length, u32 expected output length, the section}.  Every section is copied into a malloc of EXACTLY its length
// and decoded into a malloc of exactly the capacity tried: the expected output length (a `whole` one must then give its
// expected status and size), that length less one (never more than that is written: the decoder must say "no space" or
// refuse) and zero.  Every prefix of a `whole` section is walked too; the others (seeded mutations) are walked as they are.
// Built and run stand-alone by tests/test_snappy_host.py; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "surge_ingest.h"

namespace {

int64_t g_walks = 0, g_decoded = 0;
int g_failures = 0;

void fail(const char* what, const char* why, long long a, long long b) {
  std::printf("FAIL %s: %s (%lld, %lld)\n", what, why, a, b);
  ++g_failures;
}

// one decode of exactly `len` bytes into exactly `cap` bytes
int64_t decode(const uint8_t* bytes, size_t len, int64_t cap, int32_t* status, const char* what) {
  uint8_t* src = (uint8_t*)std::malloc(len ? len : 1);
  std::memcpy(src, bytes, len);
  uint8_t* dst = (uint8_t*)std::malloc(cap ? (size_t)cap : 1);
  ++g_walks;
  const int64_t got = surge_snappy_frame_decompress(src, (int64_t)len, dst, cap, status);
  if (got >= 0) {
    ++g_decoded;
    if (got > cap) fail(what, "more output than the capacity", got, cap);
    if (*status != 0) fail(what, "a size with a refusal's status", got, *status);
  } else if (got != -6 && got != SURGE_E_CORRUPT) {
    fail(what, "an unknown return value", got, *status);
  } else if ((got == -6) != (*status == 1)) {
    fail(what, "the return value and the status disagree", got, *status);
  }
  if (!surge_snappy_status_name(*status) || !surge_snappy_status_name(*status)[0]) fail(what, "a status without a name", *status, 0);
  std::free(dst);
  std::free(src);
  return got;
}

void walk(const uint8_t* bytes, size_t len, int64_t out_len, int expect, const char* what) {
  int32_t status = -1;
  // what the preambles promise (nothing decoded): never more than the caller should have to allocate for this input
  int32_t bs = -1;
  uint8_t* src = (uint8_t*)std::malloc(len ? len : 1);
  std::memcpy(src, bytes, len);
  const int64_t bound = surge_snappy_frame_bound(src, (int64_t)len, &bs);
  std::free(src);
  const int64_t got = decode(bytes, len, out_len, &status, what);
  if (got >= 0 && bound != got) fail(what, "the bound is not the decoded size", bound, got);
  if (expect != 0xFF) {
    if (status != expect) fail(what, "status", status, expect);
    if (expect == 0 && got != out_len) fail(what, "decoded size", got, out_len);
  }
  if (out_len > 0) {
    int32_t s1 = -1;
    const int64_t short_got = decode(bytes, len, out_len - 1, &s1, what);
    if (expect == 0 && short_got != -6) fail(what, "a capacity one byte short must be refused as no space", short_got, s1);
  }
  int32_t s0 = -1;
  (void)decode(bytes, len, 0, &s0, what);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("FAIL usage: snappy_prefixes <corpus>\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("FAIL cannot open the corpus\n"); return 2; }
  int64_t n_cases = 0;
  uint8_t head[10];
  std::vector<uint8_t> section;
  while (std::fread(head, 1, sizeof(head), f) == sizeof(head)) {
    uint32_t len = 0, out_len = 0;
    std::memcpy(&len, head + 2, 4);
    std::memcpy(&out_len, head + 6, 4);
    section.resize(len);
    if (len && std::fread(section.data(), 1, len, f) != len) { std::printf("FAIL the corpus is cut\n"); return 2; }
    ++n_cases;
    walk(section.data(), len, out_len, head[1], "section");
    if (head[0]) {
      // every prefix; the first 2048 and the last 64 at every capacity, the ones between (inside the long literals of the
      // 64 KiB cases) at the full capacity only
      for (size_t cut = 0; cut < len; ++cut) {
        if (cut < 2048 || len - cut < 64) {
          walk(section.data(), cut, out_len, 0xFF, "prefix");
        } else {
          int32_t s = -1;
          (void)decode(section.data(), cut, out_len, &s, "prefix");
        }
      }
    }
  }
  std::fclose(f);
  const bool bad = g_failures || n_cases < 60;
  std::printf("%s snappy_prefixes: %lld cases, %lld walks, %lld decoded, %d failures\n", bad ? "FAIL" : "PASS", (long long)n_cases, (long long)g_walks,
              (long long)g_decoded, g_failures);
  return bad ? 1 : 0;
}
