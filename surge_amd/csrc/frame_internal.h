// frame_internal.h — what the host units of the device framer share (device_framer.hip: the handle's lifecycle, the C exports,
// the steps of a publish, the host CRC pass; frame_lz4.hip: the LZ4 step): the handle and its device memory, what flows
// between the steps of one publish, error reporting, the device guard and the one scan path with its scratch rule.  Host only
// and internal, like ingest_decoder_internal.h: not part of the C ABI (that is include/surge_snapshot.h).  The kernels and
// their launchers know none of this (frame_device.h).
#pragma once

#include <new>
#include <string>
#include <vector>

#include "../../include/surge_replay.h"  // SURGE_SNAP_*
#include "../../include/surge_snapshot.h"
#include "frame_device.h"

namespace surge {
namespace frame {
namespace host __attribute__((visibility("hidden"))) {

constexpr int32_t OK = 0, E_INVALID = -1, E_DEVICE = -3, E_NOMEM = -4, E_RANGE = -6;

// Device memory, owned: freed with the buffer, which must happen while its device is current and nothing on the stream uses
// it any more (surge_device_framer_destroy).  Grows to max(2 * cap, bytes) and keeps nothing of what it held: every buffer
// here is written whole by the publish that sizes it.  (A regrowth is a hipFree, which waits for the whole device.)
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    const size_t want = cap * 2 > bytes ? cap * 2 : bytes;
    void* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, want);
    if (e != hipSuccess) return e;
    if (p) (void)hipFree(p);
    p = fresh;
    cap = want;
    return hipSuccess;
  }
};

template <class T>
struct Dev : Buf {  // ... of elements of one type
  T* ptr() const { return (T*)p; }
  hipError_t room(size_t count) { return reserve(count * sizeof(T)); }
};

struct Pinned {  // the page-locked bytes a publish is copied into: a quarter more than asked for, nothing kept
  uint8_t* p = nullptr;
  size_t cap = 0;
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 4;
    void* hp = nullptr;
    const hipError_t e = hipHostMalloc(&hp, want, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    p = (uint8_t*)hp;
    cap = want;
    return hipSuccess;
  }
};

// One publish: the inputs as the caller gave them, and the counts and device pointers its steps hand on.  What a step reads
// and writes of it stands at the step (device_framer.hip).
struct Publish {
  int64_t n = 0;
  const uint8_t* kind = nullptr;
  const int32_t* partition = nullptr;
  const uint8_t* keys_utf8 = nullptr;
  const int64_t* key_off = nullptr;
  const uint8_t* values = nullptr;
  const int64_t* val_off = nullptr;
  int64_t timestamp_ms = 0;
  int64_t n_sel = 0;                                 // select: the changed aggregates = the records
  const uint32_t* order = nullptr;                   // plan: order[j] = the record at position j of the partition order
  int64_t *c1 = nullptr, *c2 = nullptr, *c3 = nullptr;  // plan: the three scanned sizes, n_sel + 1 each
  int64_t n_batches = 0;                             // cut
  int64_t uncompressed_bytes = 0;                    // cut: of the batches in the uncompressed layout
  int64_t n_bytes = 0;                               // cut: of the output; the LZ4 step replaces it
  uint8_t* d_final = nullptr;                        // write: the output on the device; the LZ4 step replaces it
};

}  // namespace host
}  // namespace frame
}  // namespace surge

struct surge_device_framer {
  template <class T>
  using Dev = surge::frame::host::Dev<T>;
  int device = 0;
  hipStream_t stream = nullptr;
  int32_t n_part = 0, max_records = 10000;
  int64_t max_bytes = 1 << 20;
  int32_t codec = SURGE_SNAPSHOT_CODEC_NONE;
  std::string err;
  // what a publish commits (commit, device_framer.hip)
  int64_t uncompressed_bytes = 0;  // of the last publish's batches
  std::vector<int64_t> next_offset, part_byte_off;
  // copy out and host CRCs (declared ahead of the device buffers: they are freed first, the page-locked bytes after them)
  surge::frame::host::Pinned pinned;
  std::vector<surge::frame::Batch> h_batches;
  // select
  Dev<int64_t> sel, n_sel;
  Dev<uint32_t> bad;
  // plan
  Dev<uint32_t> keys_a, keys_b, vals_a, vals_b, base;
  Dev<int64_t> c, pstart;
  // cut
  Dev<int64_t> nb, pbytes, d_next;
  Dev<surge::frame::Batch> batches;
  // write
  Dev<uint8_t> out;
  // the scratch of select, sort and every scan (scan_in_place)
  surge::frame::host::Buf temp;
  // LZ4 mode only (frame_lz4.hip)
  Dev<int64_t> lz_nblk, lz_bsz, lz_bbytes;
  Dev<surge::frame::LzBlock> lz_blocks;
  Dev<uint8_t> lz_tmp, lz_out;
};

namespace surge {
namespace frame {
namespace host __attribute__((visibility("hidden"))) {

inline thread_local std::string g_frame_err;

inline int32_t ffail(surge_device_framer* f, int32_t code, const std::string& m) {
  if (f) f->err = m;
  g_frame_err = m;
  return code;
}

#define FCHK(f, call)                                                                                                       \
  do {                                                                                                                      \
    const hipError_t e_ = (call);                                                                                           \
    if (e_ != hipSuccess) return ffail(f, e_ == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct Guard {  // the calling thread's device, restored on the way out
  int prev = -1;
  explicit Guard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
  ~Guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Exclusive scan of `count` int64 in place on the framer's stream: all eight scans of a publish.  It owns the scratch rule:
// the scratch may only be regrown after the stream has drained, because work queued earlier (a scan, the sort) may still use it.
inline int32_t scan_in_place(surge_device_framer* f, int64_t* v, size_t count) {
  size_t need = 0;
  FCHK(f, scan_exclusive(nullptr, need, v, count, f->stream));
  if (need > f->temp.cap) {
    FCHK(f, hipStreamSynchronize(f->stream));
    FCHK(f, f->temp.reserve(need));
  }
  FCHK(f, scan_exclusive(f->temp.p, need, v, count, f->stream));
  return OK;
}

// ---- frame_lz4.hip ----------------------------------------------------------------------------------------------------
int32_t compress_and_pack(surge_device_framer* f, Publish& pub);

}  // namespace host
}  // namespace frame
}  // namespace surge
