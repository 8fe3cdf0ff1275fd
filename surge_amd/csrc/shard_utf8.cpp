// shard_utf8.cpp — the host form of the shard map over UTF-8 ids (surge_replay_partition_hash_utf8): shard_utf8.h, id by id.
// Host only, no device and no handle: any C++17 compiler builds it (tests/cpp/shard_utf8_prefixes.cpp does, under sanitizers).
#include "shard_utf8.h"

#include "../../include/surge_replay.h"

extern "C" int32_t surge_replay_partition_hash_utf8(const uint8_t* utf8, const int64_t* str_off, int64_t n, int32_t n_partitions,
                                                    int32_t up_to_colon, int32_t* part_out, int64_t* first_bad_out) {
  if (n < 0 || n_partitions <= 0) return SURGE_E_INVALID;
  if (n == 0) {
    if (first_bad_out) *first_bad_out = -1;
    return SURGE_OK;
  }
  if (!str_off || !part_out) return SURGE_E_INVALID;
  for (int64_t i = 0; i < n; ++i)  // before anything is written
    if (str_off[i + 1] < str_off[i]) return SURGE_E_INVALID;
  if (!utf8 && str_off[n] != str_off[0]) return SURGE_E_INVALID;
  int64_t first_bad = -1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = str_off[i], len = str_off[i + 1] - b;
    const uint8_t* s = len ? utf8 + b : nullptr;  // (an empty id has no address to form)
    const int32_t part = up_to_colon ? surge::shard_partition_utf8<true>(s, len, n_partitions)
                                     : surge::shard_partition_utf8<false>(s, len, n_partitions);
    part_out[i] = part;
    if (part < 0 && first_bad < 0) first_bad = i;
  }
  if (first_bad_out) *first_bad_out = first_bad;
  return first_bad < 0 ? SURGE_OK : SURGE_E_CORRUPT;
}
