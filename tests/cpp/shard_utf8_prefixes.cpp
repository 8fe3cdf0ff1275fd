// shard_utf8_prefixes.cpp — the UTF-8 shard map (surge_amd/csrc/shard_utf8.h through shard_utf8.cpp's export) under
// -fsanitize=address,undefined: for an id of len bytes it must never read at or beyond utf8 + len.
// The corpus comes from tests/shard_utf8_cases.py through a file (argv[1]): records of {u32 length, i32 the partition of the
// whole id among 7, i32 the same with the cut at ':', the id}.  Every prefix of every id (the id itself included) is copied
// into a malloc of EXACTLY its length and hashed from there, whole and cut; the id itself must give what the file says.  Then
// the ids are laid back to back in one allocation of exactly their total length and hashed in one call: every id must give
// what it gave alone — a sequence its own end cuts is not completed by its neighbour's bytes.
// Built and run stand-alone by tests/test_shard_utf8.py; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "surge_replay.h"

namespace {

constexpr int32_t kPartitions = 7;
int64_t g_calls = 0;
int g_failures = 0;

void fail(const char* what, long long id, long long a, long long b) {
  std::printf("FAIL id %lld: %s (%lld, %lld)\n", id, what, a, b);
  ++g_failures;
}

// one id of exactly `len` bytes, alone: its partition or -1
int32_t hash_one(const uint8_t* bytes, size_t len, int cut, long long id) {
  uint8_t* src = (uint8_t*)std::malloc(len ? len : 1);
  if (len) std::memcpy(src, bytes, len);
  const int64_t off[2] = {0, (int64_t)len};
  int32_t part = -99;
  int64_t first_bad = -99;
  ++g_calls;
  const int32_t rc = surge_replay_partition_hash_utf8(len ? src : nullptr, off, 1, kPartitions, cut, &part, &first_bad);
  std::free(src);
  if (rc == SURGE_OK) {
    if (part < 0 || part >= kPartitions || first_bad != -1) fail("OK without a partition", id, part, first_bad);
  } else if (rc == SURGE_E_CORRUPT) {
    if (part != -1 || first_bad != 0) fail("CORRUPT without -1", id, part, first_bad);
  } else {
    fail("an unknown status", id, rc, 0);
  }
  return part;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("FAIL usage: shard_utf8_prefixes <corpus>\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("FAIL cannot open the corpus\n"); return 2; }
  std::vector<std::vector<uint8_t>> ids;
  std::vector<int32_t> alone[2];
  uint8_t head[12];
  while (std::fread(head, 1, sizeof(head), f) == sizeof(head)) {
    uint32_t len = 0;
    int32_t want[2] = {0, 0};
    std::memcpy(&len, head, 4);
    std::memcpy(&want[0], head + 4, 4);
    std::memcpy(&want[1], head + 8, 4);
    std::vector<uint8_t> id(len);
    if (len && std::fread(id.data(), 1, len, f) != len) { std::printf("FAIL the corpus is cut\n"); return 2; }
    const long long n = (long long)ids.size();
    for (int cut = 0; cut < 2; ++cut) {
      for (size_t p = 0; p < len; ++p) (void)hash_one(id.data(), p, cut, n);
      const int32_t got = hash_one(id.data(), len, cut, n);
      if (got != want[cut]) fail(cut ? "the cut id's partition" : "the whole id's partition", n, got, want[cut]);
      alone[cut].push_back(got);
    }
    ids.push_back(std::move(id));
  }
  std::fclose(f);
  // back to back, no byte of slack
  size_t total = 0;
  for (const auto& id : ids) total += id.size();
  uint8_t* arena = (uint8_t*)std::malloc(total ? total : 1);
  std::vector<int64_t> off(ids.size() + 1, 0);
  for (size_t i = 0; i < ids.size(); ++i) {
    if (!ids[i].empty()) std::memcpy(arena + off[i], ids[i].data(), ids[i].size());
    off[i + 1] = off[i] + (int64_t)ids[i].size();
  }
  for (int cut = 0; cut < 2; ++cut) {
    std::vector<int32_t> part(ids.size(), -99);
    int64_t first_bad = -99, want_first = -1;
    ++g_calls;
    const int32_t rc = surge_replay_partition_hash_utf8(arena, off.data(), (int64_t)ids.size(), kPartitions, cut, part.data(), &first_bad);
    for (size_t i = 0; i < ids.size(); ++i) {
      if (part[i] != alone[cut][i]) fail("differs among its neighbours", (long long)i, part[i], alone[cut][i]);
      if (alone[cut][i] < 0 && want_first < 0) want_first = (int64_t)i;
    }
    if (first_bad != want_first || rc != (want_first < 0 ? SURGE_OK : SURGE_E_CORRUPT)) fail("status of the whole table", -1, rc, first_bad);
  }
  std::free(arena);
  const bool bad = g_failures || ids.size() < 100;
  std::printf("%s shard_utf8_prefixes: %lld ids, %lld calls, %d failures\n", bad ? "FAIL" : "PASS", (long long)ids.size(), (long long)g_calls, g_failures);
  return bad ? 1 : 0;
}
