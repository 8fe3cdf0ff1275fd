// snappy_frame.cpp — the C exports over snappy_block.h (include/surge_ingest.h, next to surge_lz4_frame_*): reading only.
// Everything the format needs is inline in the header — the host framer decompresses through it without this unit — so this
// file only gives tests and other bindings a way in.
#include "snappy_block.h"

#include "../../include/surge_ingest.h"

namespace {

using namespace surge::snappy;

int64_t answer(Status s, int64_t n, int32_t* status_out) {
  if (status_out) *status_out = (int32_t)s;
  return s == SN_OK ? n : s == SN_NO_SPACE ? -6 : (int64_t)SURGE_E_CORRUPT;
}

bool bad_args(const uint8_t* src, int64_t n, const uint8_t* dst, int64_t cap) { return !src || n < 0 || cap < 0 || (!dst && cap > 0); }

}  // namespace

extern "C" {

int64_t surge_snappy_uncompressed_length(const uint8_t* src, int64_t n, int32_t* status_out) {
  if (!src || n < 0) return -1;
  uint32_t want = 0;
  int32_t pre = 0;
  const Status s = read_preamble(src, n, &want, &pre);
  return answer(s, (int64_t)want, status_out);
}

int64_t surge_snappy_uncompress(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* status_out) {
  if (bad_args(src, n, dst, cap)) return -1;
  int64_t got = 0;
  const Status s = uncompress_block(src, n, dst, cap, &got);
  return answer(s, got, status_out);
}

int64_t surge_snappy_frame_bound(const uint8_t* src, int64_t n, int32_t* status_out) {
  if (!src || n < 0) return -1;
  int64_t total = 0;
  const Status s = frame_bound(src, n, &total);
  return answer(s, total, status_out);
}

int64_t surge_snappy_frame_decompress(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* status_out) {
  if (bad_args(src, n, dst, cap)) return -1;
  int64_t got = 0;
  const Status s = frame_decompress(src, n, dst, cap, &got);
  return answer(s, got, status_out);
}

const char* surge_snappy_status_name(int32_t status) { return status_name(status); }

}  // extern "C"
