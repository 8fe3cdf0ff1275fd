// frame_device.h — what the kernels of the device framer and what launches them share: the batch table, the
// layout constants and one launcher per step.  Internal, like ingest_device.h: not part of the C ABI (that is
// include/surge_snapshot.h).  The units: frame_records.hip (the uncompressed framing and the select / sort / scan steps),
// frame_lz4.hip (the LZ4 mode), device_framer.hip (the host object: surge_device_framer_*, which shares frame_internal.h with
// frame_lz4.hip).  The launchers know plain pointers, counts and a stream and nothing of the handle; they enqueue and none of
// them waits for the device.
//
// What the framer replaces: snapshot_writer.cpp's append loop on the host.  A publish of config C5 (0.95 M changed aggregates of
// 10 M, 85 MB of record batches every 30 micro-batches) spent 40 of its 52 ms there — one host thread per partition
// pushing varints and bytes into vectors — while the states, their JSON text and their keys were already in HBM.  Here
// the GPU writes the records where they go and only what the host is better at stays on the host: the CRC-32C of each
// finished batch (the crc32 instruction: 11 GB/s per thread) over the bytes after they arrived in page-locked memory.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace surge {
namespace frame {

constexpr int kHeader = 61;
constexpr int64_t kD1 = 64, kD2 = 8192, kD3 = 1 << 20;  // offsetDelta below these takes 1 / 2 / 3 bytes

struct Batch {          // device + host
  int64_t out_off;      // first byte of the batch (its header) in the output
  int64_t first;        // index of its first record in partition-sorted order
  int64_t base_offset;  // Kafka offset of its first record
  int32_t count;
  int32_t partition;
  int64_t records_bytes;
};

// ---- LZ4 mode -------------------------------------------------------------------------------------------------------
constexpr int32_t kLzBlock = 65536;     // input bytes per block: the device decoder places block k at k * 64 KiB
constexpr int kLzFrameHeader = 7;       // magic, FLG, BD, HC
constexpr int32_t kLzSmall = 4096;      // blocks up to this size are compressed with the small hash table
constexpr int kLzHashLogSmall = 11, kLzHashLog = 13;  // 4 KiB / 16 KiB of LDS per wave

struct LzBlock {
  int64_t src_off;  // first byte of the block in the uncompressed buffer (and of its slot in the scratch buffer)
  int32_t n;        // input bytes: 65536 for all but a frame's last block
  int32_t batch;
};

inline unsigned grid(int64_t n) { return (unsigned)((n + 255) / 256); }  // blocks of 256 threads, one thread per element

// ---- frame_records.hip ------------------------------------------------------------------------------------------------
// The three library steps, as rocPRIM words them: temp == nullptr asks for the scratch they need (temp_bytes), anything else runs.
// the indices of the aggregates with kind != 0, in index order, and how many there are
hipError_t select_changed(void* temp, size_t& temp_bytes, const uint8_t* kind, int64_t* sel, int64_t* n_sel, int64_t n, hipStream_t st);
// stable sort of (partition, record) pairs by the low `bits` bits of the partition
hipError_t sort_by_partition(void* temp, size_t& temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                             int64_t n_sel, unsigned bits, hipStream_t st);
// exclusive scan of count int64 in place
hipError_t scan_exclusive(void* temp, size_t& temp_bytes, int64_t* v, size_t count, hipStream_t st);

void launch_frame_size(const int64_t* sel, int64_t n_sel, const uint8_t* kind, const int32_t* part, int32_t n_part, const int64_t* key_off,
                       const int64_t* val_off, bool have_keys, bool have_values, uint32_t* keys, uint32_t* vals, uint32_t* base, uint32_t* bad,
                       hipStream_t st);
void launch_frame_sizes3(const uint32_t* order, const uint32_t* base, int64_t n_sel, int64_t* c1, int64_t* c2, int64_t* c3, hipStream_t st);
void launch_frame_pstart(const uint32_t* sorted_part, int64_t n_sel, int32_t n_part, int64_t* pstart, hipStream_t st);
// emit == false: nb[p] / pbytes[p] only; emit == true: the batches, at the scanned nb[p] / pbytes[p]
void launch_frame_batches(const int64_t* pstart, int32_t n_part, const int64_t* c1, const int64_t* c2, const int64_t* c3, int32_t max_records,
                          int64_t max_bytes, const int64_t* next_offset, bool emit, int64_t* nb, int64_t* pbytes, Batch* batches, hipStream_t st);
void launch_frame_write(const Batch* batches, int64_t n_batches, const uint32_t* order, const int64_t* sel, int64_t n_sel, const uint8_t* kind,
                        const uint32_t* base, const int64_t* c1, const int64_t* c2, const int64_t* c3, const uint8_t* keys_utf8, const int64_t* key_off,
                        const uint8_t* values, const int64_t* val_off, uint8_t* out, hipStream_t st);
void launch_frame_header(const Batch* batches, int64_t n_batches, int64_t timestamp_ms, int32_t codec, uint8_t* out, hipStream_t st);

}  // namespace frame
}  // namespace surge
