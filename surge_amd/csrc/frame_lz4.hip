// frame_lz4.hip — the LZ4 mode of the device framer: its seven kernels and the one step that runs them (compress_and_pack).
//
// LZ4 mode (surge_device_framer_set_compression): what the reference's producer writes (compression.type = lz4).  The
// batch cuts, offsets and counts are those of the uncompressed framing — they are decided on the uncompressed sizes, as
// the host writer decides them —; the records section of every batch then becomes ONE LZ4 frame as kafka-clients writes
// it (magic, FLG 0x60, BD 0x40, HC 0x82, independent blocks of 64 KiB of input, EndMark; no checksums), attributes = 3,
// and the CRC covers the compressed batch.  After the write kernel has put the records into the uncompressed buffer:
//     block table (batch, block) -> frame_lz4_block_kernel, ONE WAVE PER BLOCK, into a scratch slot per block ->
//     scan of the block sizes -> every batch's frame size and final place -> frame_lz4_pack_kernel moves size words and
//     block bytes (from the scratch slot, or from the uncompressed buffer for a block that did not shrink: stored) ->
//     header kernel -> device -> host copy of the COMPRESSED bytes -> host CRCs.
// The output is not the host compressor's byte for byte (a wave looks at 64 positions at once and sees the hash table
// differently); it decodes to the same records and is about as small (tests/test_frame_lz4_gpu.py).
// Device memory at the peak of an LZ4 publish of U uncompressed batch bytes: the uncompressed buffer (U), the scratch
// slots (U: a slot is as long as its block, a block that would not shrink is abandoned before it outgrows it) and the
// final buffer (at most U + 11 bytes per batch + 4 per block) — about 3 U, beside the tables of the uncompressed mode.
#include "frame_internal.h"

namespace surge {
namespace frame {
namespace {

__global__ void frame_lz4_count_kernel(const Batch* __restrict__ batches, int64_t n_batches, int64_t* __restrict__ nblk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_batches) return;
  nblk[i] = i == n_batches ? 0 : (batches[i].records_bytes + kLzBlock - 1) / kLzBlock;
}

// one thread per block: find its batch in blk_first (the exclusive scan of the counts; every batch has a block, so it
// rises strictly), its place in it, write its entry
__global__ void frame_lz4_blocks_kernel(const Batch* __restrict__ batches, int64_t n_batches, const int64_t* __restrict__ blk_first, int64_t n_blocks,
                                        LzBlock* __restrict__ blocks) {
  const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= n_blocks) return;
  int64_t lo = 0, hi = n_batches;  // last batch whose first block is <= blk
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (blk_first[mid] <= blk) lo = mid; else hi = mid;
  }
  const Batch b = batches[lo];
  const int64_t k = blk - blk_first[lo];
  const int64_t rest = b.records_bytes - k * kLzBlock;
  LzBlock e;
  e.src_off = b.out_off + kHeader + k * kLzBlock;
  e.n = (int32_t)(rest < kLzBlock ? rest : kLzBlock);
  e.batch = (int32_t)lo;
  blocks[blk] = e;
}

__device__ inline uint32_t load32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// bytes of the 255-continued length that follows a saturated token nibble
__device__ inline int32_t lz4_len_bytes(int32_t len) { return len >= 15 ? (len - 15) / 255 + 1 : 0; }

__device__ inline void lz4_put_len(uint8_t* dst, int32_t len, int lane) {  // the whole wave; len >= 15
  const int32_t v = len - 15, nb = v / 255 + 1;
  for (int32_t i = lane; i < nb; i += 64) dst[i] = i < nb - 1 ? (uint8_t)255 : (uint8_t)(v % 255);
}

// One wave compresses one block (LZ4 block format) into the block's scratch slot; bsz[blk] = 4 + its compressed size, or
// 4 + n when it is to be stored.  Launched once per size class (n_lo < n <= n_hi) with a hash table to match, so that
// the many small batches of a many-partition publish do not each hold the LDS a 64 KiB block wants.
//
// The wave looks at the 64 positions ip .. ip + 63: every lane hashes its 4 bytes, reads its candidate from the table and
// tests it; the lowest matching lane f wins, the wave extends its match 64 bytes per step, emits the sequence together
// and goes on behind the match; with no match in the window it moves on by 64.  Two rules that a lane-for-lane
// simulation of this scheme showed to matter:
//   * only the lanes up to and including f insert their position into the table (all of them when nothing matched).
//     Were all 64 to insert before the decision, the positions behind a short match would overwrite the very entries
//     the next window needs, and then point at themselves: the ratio on Counter state records fell from 2.54 to 1.23;
//   * a candidate must lie strictly BEFORE the lane's position.  The table starts as all zeros (position 0 is a valid
//     candidate for every later position: what counts is that the bytes are equal) and a 16-bit entry has no value to
//     spare for "empty", so a lane at position 0 meets itself; one compare keeps the offset in 1 .. 65535.
// A third rule is for what the window scheme cannot see: all 64 lanes read their candidates before any of them inserts, so
// a repeat that begins inside a window of new content is found one window late -- and in the block's LAST window
// (ip + 64 > n - 12) not at all.  There, when the table gave no hit, every lane takes the nearest earlier lane of the
// window with the same 4 bytes as its candidate: one shuffle per active lane of that window, in every block whose last
// window has no table hit -- every incompressible block, and every small block without a repeat, of which a
// many-partition publish has many (200 000 blocks of 35 to 75 random bytes: 232 us for the launch, 73 us without the
// search, in a publish of 25 ms).  Without it no block below 76 bytes could shrink unless it repeated its own first
// bytes, and a batch of one small record of zeros was stored.
// The table holds 16-bit positions (a block is at most 64 KiB), the block's bytes are read from global memory (the write
// kernel has just put them there) — 16 KiB of LDS per wave leaves room for ten waves per CU.
// Writes: a sequence is emitted only if the output stays BELOW n bytes with it; otherwise the block is given up as
// stored (the output only grows, so it would have ended up stored anyway).  So whatever the input, nothing is written
// beyond the n bytes of the block's own slot, and table indices are hash values of HASH_LOG bits.
template <int HASH_LOG>
__global__ __launch_bounds__(64) void frame_lz4_block_kernel(const LzBlock* __restrict__ blocks, int64_t n_blocks, int32_t n_lo, int32_t n_hi,
                                                             const uint8_t* __restrict__ src_base, uint8_t* __restrict__ tmp_base,
                                                             int64_t* __restrict__ bsz) {
  __shared__ uint16_t table[1 << HASH_LOG];
  const int64_t blk = blockIdx.x;
  if (blk >= n_blocks) return;
  const LzBlock B = blocks[blk];
  const int32_t n = B.n;
  if (n <= n_lo || n > n_hi) return;
  const int lane = threadIdx.x;
  const uint8_t* __restrict__ src = src_base + B.src_off;
  uint8_t* __restrict__ dst = tmp_base + B.src_off;
  for (int i = lane; i < (1 << HASH_LOG); i += 64) table[i] = 0;
  __syncthreads();
  const int32_t mflimit = n - 12;    // no match starts after this position ...
  const int32_t matchlimit = n - 5;  // ... and none reaches this one: the last 5 bytes are literals
  int32_t ip = 0, anchor = 0, op = 0;
  while (ip <= mflimit) {  // (a block below 13 bytes is one literal run, longer than its input: stored)
    const int32_t pos = ip + lane;
    const bool active = pos <= mflimit;
    const uint32_t v = active ? load32(src + pos) : 0u;
    const uint32_t h = (v * 2654435761u) >> (32 - HASH_LOG);
    int32_t cand = active ? (int32_t)table[h] : 0;
    bool hit = active && cand < pos && load32(src + cand) == v;
    uint64_t hits = __ballot(hit);
    if (!hits && ip + 64 > mflimit) {  // the block's last window: nearest earlier lane with the same 4 bytes
      const int live = mflimit - ip + 1;  // its active lanes, 1 .. 64: the same for the whole wave
      for (int d = 1; d < live; ++d) {
        const uint32_t w = __shfl_up(v, d);
        if (!hit && active && lane >= d && w == v) {
          hit = true;
          cand = pos - d;
        }
      }
      hits = __ballot(hit);
    }
    const int f = hits ? __ffsll((long long)hits) - 1 : 63;
    if (active && lane <= f) table[h] = (uint16_t)pos;
    __syncthreads();  // one wave: orders this window's inserts before the next window's reads
    if (!hits) {
      ip += 64;
      continue;
    }
    const int32_t mpos = ip + f;
    const int32_t off = mpos - __shfl(cand, f);
    int32_t len = 4;
    for (;;) {
      const int32_t q = mpos + len + lane;
      const bool same = q < matchlimit && src[q] == src[q - off];
      const uint64_t diff = __ballot(!same);
      if (diff) {
        len += __ffsll((long long)diff) - 1;
        break;
      }
      len += 64;
    }
    const int32_t lit = mpos - anchor, ml = len - 4;
    const int32_t lit_lb = lz4_len_bytes(lit), ml_lb = lz4_len_bytes(ml);
    const int32_t need = 1 + lit_lb + lit + 2 + ml_lb;
    if (op + need >= n) {
      if (lane == 0) bsz[blk] = 4 + (int64_t)n;
      return;
    }
    uint8_t* o = dst + op;
    if (lane == 0) o[0] = (uint8_t)((lit >= 15 ? 15 : lit) << 4 | (ml >= 15 ? 15 : ml));
    if (lit >= 15) lz4_put_len(o + 1, lit, lane);
    o += 1 + lit_lb;
    for (int32_t i = lane; i < lit; i += 64) o[i] = src[anchor + i];
    o += lit;
    if (lane == 0) {
      o[0] = (uint8_t)off;
      o[1] = (uint8_t)(off >> 8);
    }
    if (ml >= 15) lz4_put_len(o + 2, ml, lane);
    op += need;
    ip = mpos + len;
    anchor = ip;
  }
  const int32_t lit = n - anchor;  // the last sequence is literals only
  const int32_t lit_lb = lz4_len_bytes(lit);
  const int32_t need = 1 + lit_lb + lit;
  if (op + need >= n) {
    if (lane == 0) bsz[blk] = 4 + (int64_t)n;
    return;
  }
  uint8_t* o = dst + op;
  if (lane == 0) o[0] = (uint8_t)((lit >= 15 ? 15 : lit) << 4);
  if (lit >= 15) lz4_put_len(o + 1, lit, lane);
  o += 1 + lit_lb;
  for (int32_t i = lane; i < lit; i += 64) o[i] = src[anchor + i];
  if (lane == 0) bsz[blk] = 4 + (int64_t)(op + need);
}

// per batch (and one entry beyond): bytes of the compressed batch, from the scanned block sizes (bscan[b] = bytes of
// the size words and blocks before block b)
__global__ void frame_lz4_batch_size_kernel(int64_t n_batches, const int64_t* __restrict__ blk_first, const int64_t* __restrict__ bscan,
                                            int64_t* __restrict__ bbytes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_batches) return;
  bbytes[i] = i == n_batches ? 0 : kHeader + kLzFrameHeader + (bscan[blk_first[i + 1]] - bscan[blk_first[i]]) + 4;
}

// the partitions' spans in the compressed output: nb[p] = first batch of partition p, new_off = scanned batch bytes
__global__ void frame_lz4_spans_kernel(int32_t n_part, const int64_t* __restrict__ nb, const int64_t* __restrict__ new_off, int64_t* __restrict__ pspan) {
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n_part) return;
  pspan[p] = new_off[nb[p]];
}

// One workgroup per block moves it to its final place: size word + bytes; the batch's first block also writes the frame
// header, its last the EndMark.  Reads blocks[].src_off (the uncompressed layout), so it runs before the batches are
// re-addressed.
__global__ __launch_bounds__(256) void frame_lz4_pack_kernel(const LzBlock* __restrict__ blocks, const int64_t* __restrict__ blk_first,
                                                             const int64_t* __restrict__ bscan, const int64_t* __restrict__ new_off,
                                                             const uint8_t* __restrict__ src_base, const uint8_t* __restrict__ tmp_base,
                                                             uint8_t* __restrict__ out) {
  const int64_t blk = blockIdx.x;
  const LzBlock B = blocks[blk];
  const int64_t first = blk_first[B.batch], last = blk_first[B.batch + 1] - 1;
  const int64_t csize = bscan[blk + 1] - bscan[blk] - 4;
  const bool stored = csize >= B.n;
  uint8_t* frame = out + new_off[B.batch] + kHeader;
  uint8_t* o = frame + kLzFrameHeader + (bscan[blk] - bscan[first]);
  const int t = threadIdx.x;
  if (t < 4) {
    const uint32_t word = stored ? ((uint32_t)B.n | 0x80000000u) : (uint32_t)csize;
    o[t] = (uint8_t)(word >> (8 * t));
  }
  if (blk == first && t >= 32 && t < 32 + kLzFrameHeader) {
    const uint8_t head[kLzFrameHeader] = {0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82};  // HC = (XXH32(FLG BD) >> 8) & 0xff
    frame[t - 32] = head[t - 32];
  }
  if (blk == last && t >= 64 && t < 68) o[4 + csize + (t - 64)] = 0;  // EndMark
  const uint8_t* s = (stored ? src_base : tmp_base) + B.src_off;
  o += 4;
  for (int64_t i = (int64_t)t * 8; i < csize; i += 256 * 8) {
    if (i + 8 <= csize) {
      uint64_t v;
      __builtin_memcpy(&v, s + i, 8);
      __builtin_memcpy(o + i, &v, 8);
    } else {
      for (int64_t k = i; k < csize; ++k) o[k] = s[k];
    }
  }
}

// the batches in the compressed layout: what the header kernel, the copy and the host CRCs work from
__global__ void frame_lz4_readdress_kernel(Batch* __restrict__ batches, int64_t n_batches, const int64_t* __restrict__ new_off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_batches) return;
  batches[i].out_off = new_off[i];
  batches[i].records_bytes = new_off[i + 1] - new_off[i] - kHeader;
}

}  // namespace

namespace host {

// Every batch's records section -> one LZ4 frame, the batches packed at their compressed sizes.  In: the uncompressed batches
// (f->batches, their bytes in f->out) and every partition's first batch (f->nb, scanned).  Out: the packed bytes (pub.d_final,
// pub.n_bytes of them), the spans of the compressed output (f->part_byte_off) and the batch table readdressed to it.  Two waits
// for the device: for the block count, and for the spans, whose last entry is the size of the output.
int32_t compress_and_pack(surge_device_framer* f, Publish& pub) {
  hipStream_t st = f->stream;
  const int32_t P = f->n_part;
  const int64_t n_batches = pub.n_batches;
  const uint8_t* plain = f->out.ptr();  // the uncompressed layout, pub.n_bytes long so far
  FCHK(f, f->lz_nblk.room((size_t)n_batches + 1));
  FCHK(f, f->lz_bbytes.room((size_t)n_batches + 1));
  FCHK(f, f->lz_tmp.room((size_t)pub.n_bytes));
  int64_t* blk_first = f->lz_nblk.ptr();
  int64_t* new_off = f->lz_bbytes.ptr();
  hipLaunchKernelGGL(frame_lz4_count_kernel, dim3(grid(n_batches + 1)), dim3(256), 0, st, f->batches.ptr(), n_batches, blk_first);
  if (const int32_t rc = scan_in_place(f, blk_first, (size_t)n_batches + 1)) return rc;
  int64_t n_blocks = 0;
  FCHK(f, hipMemcpyAsync(&n_blocks, blk_first + n_batches, 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  if (n_blocks < n_batches || n_blocks > 0x7fffffffll)  // (every batch has a block; LzBlock.batch and the grids are 32 bits wide)
    return ffail(f, E_RANGE, n_blocks < n_batches ? "the LZ4 block count is inconsistent with the batches" : "more than 2^31 LZ4 blocks in one publish");
  FCHK(f, f->lz_blocks.room((size_t)n_blocks));
  FCHK(f, f->lz_bsz.room((size_t)n_blocks + 1));
  const LzBlock* blocks = f->lz_blocks.ptr();
  int64_t* bscan = f->lz_bsz.ptr();
  hipLaunchKernelGGL(frame_lz4_blocks_kernel, dim3(grid(n_blocks)), dim3(256), 0, st, f->batches.ptr(), n_batches, blk_first, n_blocks, f->lz_blocks.ptr());
  FCHK(f, hipMemsetAsync(bscan + n_blocks, 0, 8, st));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(frame_lz4_block_kernel<kLzHashLogSmall>), dim3((unsigned)n_blocks), dim3(64), 0, st, blocks, n_blocks, 0, kLzSmall,
                     plain, f->lz_tmp.ptr(), bscan);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(frame_lz4_block_kernel<kLzHashLog>), dim3((unsigned)n_blocks), dim3(64), 0, st, blocks, n_blocks, kLzSmall, kLzBlock,
                     plain, f->lz_tmp.ptr(), bscan);
  if (const int32_t rc = scan_in_place(f, bscan, (size_t)n_blocks + 1)) return rc;
  hipLaunchKernelGGL(frame_lz4_batch_size_kernel, dim3(grid(n_batches + 1)), dim3(256), 0, st, n_batches, blk_first, bscan, new_off);
  if (const int32_t rc = scan_in_place(f, new_off, (size_t)n_batches + 1)) return rc;
  // the two per-partition tables of the cut under their second meaning: nb, scanned, is every partition's first batch, and
  // pbytes is free again since the emit pass read it: the spans of the compressed output
  const int64_t* first_batch = f->nb.ptr();
  int64_t* lz_span = f->pbytes.ptr();
  hipLaunchKernelGGL(frame_lz4_spans_kernel, dim3(grid(P + 1)), dim3(256), 0, st, P, first_batch, new_off, lz_span);
  FCHK(f, hipGetLastError());
  FCHK(f, hipMemcpyAsync(f->part_byte_off.data(), lz_span, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  pub.n_bytes = f->part_byte_off[(size_t)P];
  FCHK(f, f->lz_out.room((size_t)pub.n_bytes));
  hipLaunchKernelGGL(frame_lz4_pack_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, blocks, blk_first, bscan, new_off, plain, f->lz_tmp.ptr(),
                     f->lz_out.ptr());
  hipLaunchKernelGGL(frame_lz4_readdress_kernel, dim3(grid(n_batches)), dim3(256), 0, st, f->batches.ptr(), n_batches, new_off);
  pub.d_final = f->lz_out.ptr();
  return OK;
}

}  // namespace host
}  // namespace frame
}  // namespace surge
