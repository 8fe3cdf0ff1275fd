// ingest_lz4.hip — the device decoder's LZ4 stage: everything that knows the LZ4 frame and block formats.  The host half walks
// a frame's header and block size words (lz4_plan_section: nothing per byte), the device half decodes the blocks (launch_lz4).
#include <new>

#include "ingest_device.h"

namespace surge {
namespace ingest {
namespace {

// ---- LZ4 (the reference's producer publishes lz4: reference.conf:112) ------------------------------------------------
// A record batch's records section is ONE LZ4 frame; kafka-clients writes it with independent blocks of at most 64 KiB
// (KafkaLZ4BlockOutputStream's default), so every block but a frame's last decompresses to exactly 64 KiB and block k
// of a frame lands at k x 64 KiB of the frame's output.  The host walks the frame header and the block size words
// (nothing per byte); one WAVE decodes one block: the token / length / offset bytes are wave-uniform (every lane reads
// the same byte: one broadcast load), literal runs and matches are copied by the 64 lanes together, an overlapping
// match (offset < length: the period IS the data) as out[op + i] = out[op - offset + i % offset].  The block is
// assembled in LDS — lanes read what other lanes wrote a sequence ago, which global memory does not promise inside a
// wave — and leaves as whole 16-byte stores.
constexpr int kLz4BlockMax = 65536;
// The compressed stream is read through a 256-byte WINDOW held in registers (lane l: bytes [4l, 4l + 4) from `wbase`):
// control bytes come out of it with v_readlane, short literal runs with one shuffle — no global load on the path from
// one sequence to the next, only a refill every ~250 consumed bytes.  (First version: token, length bytes and offset
// were three dependent global loads per sequence.)
struct Lz4Window {
  const uint8_t* in;
  int32_t n_in, wbase;
  uint32_t win;
  int lane;
  __device__ void refill(int32_t at) {
    wbase = at;
    const int32_t pos = at + 4 * lane;
    uint32_t v = 0;
    if (pos + 4 <= n_in) {
      v = (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16) | ((uint32_t)in[pos + 3] << 24);
    } else {
      for (int k = 0; k < 4; ++k)
        if (pos + k < n_in) v |= (uint32_t)in[pos + k] << (8 * k);
    }
    win = v;
  }
  __device__ uint32_t byte_at(int32_t at) {  // `at` is wave-uniform
    if (at - wbase >= 256 || at < wbase) refill(at);
    const int32_t idx = at - wbase;
    const uint32_t word = __builtin_amdgcn_readlane(win, __builtin_amdgcn_readfirstlane(idx >> 2));
    return (word >> ((idx & 3) * 8)) & 0xffu;
  }
  // one sequence's header at ip: literal length, then (after the literals) offset and match length; false = malformed
  __device__ bool literal_length(int32_t& ip, uint32_t& token, int32_t& lit) {
    token = byte_at(ip++);
    lit = (int32_t)(token >> 4);
    if (lit == 15) {
      uint32_t x;
      do {
        if (ip >= n_in) return false;
        x = byte_at(ip++);
        lit += (int32_t)x;
      } while (x == 255u && lit < (1 << 24));
    }
    return lit <= n_in - ip;
  }
  __device__ bool match(int32_t& ip, uint32_t token, int32_t& offset, int32_t& ml) {
    if (n_in - ip < 2) return false;
    offset = (int32_t)(byte_at(ip) | (byte_at(ip + 1) << 8));
    ip += 2;
    ml = (int32_t)(token & 15u);
    if (ml == 15) {
      uint32_t x;
      do {
        if (ip >= n_in) return false;
        x = byte_at(ip++);
        ml += (int32_t)x;
      } while (x == 255u && ml < (1 << 24));
    }
    ml += 4;
    return offset != 0;
  }
};

// One launch per LDS size class (16 / 32 / 64 KiB per wave), smallest first.  Nothing tells what a block decompresses to
// but decoding it — the reference's producer closes a batch at 16 KiB (kafka.publisher.batch-size = 16384,
// reference.conf:115), so its blocks need a quarter of the 64 KiB a block may take, and four times as many waves fit a CU
// — so a block is TRIED in the smallest class its compressed size does not already rule out, every write bounded by the
// class's LDS; a block that outgrows it is left for the next class (state[b] = -(class + 2)) and decoded again there from
// its start.  (Rounds before: a separate first pass walked every block's sequence headers for its size — 1.3 ms of the
// 5.8 ms a 1 M-record fetch spends on the device; the retry costs a producer of large batches up to a quarter of a
// block, the 16 KiB producer nothing.)   state[b]: >= 0 decoded (its size), -1 malformed, -2 / -3 waiting for class 1 / 2.
__global__ void __launch_bounds__(64) lz4_block_kernel(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ out_base, const Lz4Block* __restrict__ blocks,
                                                       int64_t n_blocks, int32_t* __restrict__ state, int32_t cls, int32_t cap,
                                                       Section* __restrict__ sections, ErrorCell* err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lz4_out[];
  const int lane = threadIdx.x;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    if (cls > 0 && state[b] != -(cls + 1)) continue;
    const Lz4Block blk = blocks[b];
    if (blk.seq_off >= 0) continue;  // decoded in two passes (lz4_parse_kernel / lz4_exec_kernel)
    const uint8_t* in = bytes + blk.src_off;
    const int32_t n_in = blk.src_len & 0x7fffffff;
    int32_t op = 0;
    bool ok = true, grow = false;
    if (!blk.last && cap < kLz4BlockMax) {  // every block of a frame but its last holds exactly 64 KiB
      grow = true;
    } else if (blk.src_len < 0) {  // stored
      if (n_in > cap) {
        grow = true;
      } else {
        for (int i = lane; i < n_in; i += 64) lz4_out[i] = in[i];
        op = n_in;
      }
    } else if (n_in > cap + (cap >> 7) + 64) {  // a compressed block is never much longer than what it holds
      grow = true;
    } else {
      Lz4Window w{in, n_in, 0, 0u, lane};
      w.refill(0);
      int32_t ip = 0;
      while (ip < n_in) {
        uint32_t token;
        int32_t lit, offset, ml;
        if (!w.literal_length(ip, token, lit)) { ok = false; break; }
        if (lit > cap - op) { grow = true; break; }
        if (lit > 0) {
          if (lit <= 64 && ip >= w.wbase && ip + lit - w.wbase <= 256) {  // the whole run is in the window
            const int32_t idx = ip - w.wbase + lane;
            const uint32_t word = (uint32_t)__shfl((int)w.win, (idx >> 2) & 63, 64);
            if (lane < lit) lz4_out[op + lane] = (uint8_t)(word >> ((idx & 3) * 8));
          } else {
            for (int i = lane; i < lit; i += 64) lz4_out[op + i] = in[ip + i];
          }
        }
        ip += lit;
        op += lit;
        if (ip >= n_in) break;  // the last sequence carries literals only
        if (!w.match(ip, token, offset, ml) || offset > op) { ok = false; break; }
        if (ml > cap - op) { grow = true; break; }
        // (LDS operations of one wave execute in order: a read sees every earlier write of any lane of this wave)
        const uint8_t* src = lz4_out + op - offset;
        if (offset >= ml) {
          for (int i = lane; i < ml; i += 64) lz4_out[op + i] = src[i];
        } else {  // the period IS the data
          for (int i = lane; i < ml; i += 64) lz4_out[op + i] = src[i % offset];
        }
        op += ml;
      }
    }
    if (grow && cap >= kLz4BlockMax) { grow = false; ok = false; }   // larger than a block may be
    if (ok && !grow && !blk.last && op != kLz4BlockMax) ok = false;  // every block of a frame but its last is exactly full
    if (grow) {
      if (lane == 0) state[b] = -(cls + 2);
    } else if (!ok) {
      if (lane == 0) {
        state[b] = -1;
        atomicMin(&err->lz4_bad, (unsigned int)blk.section);
        if (blk.last) sections[blk.section].byte_len = 0;
      }
    } else {
      uint8_t* dst = out_base + blk.dst_off;  // 16-byte aligned: dst_off is a multiple of 64 KiB from an aligned base
      const int n16 = op >> 4;
      for (int i = lane; i < n16; i += 64) ((uint4*)dst)[i] = ((const uint4*)lz4_out)[i];
      for (int i = (n16 << 4) + lane; i < op; i += 64) dst[i] = lz4_out[i];
      if (lane == 0) {
        state[b] = op;
        if (blk.last) sections[blk.section].byte_len = (int64_t)blk.index * kLz4BlockMax + op;
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // the copy-out has read the LDS before the next block overwrites it
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- LZ4 in two passes (round 4) ---------------------------------------------------------------------------------------
// What the counters said about the one-pass kernel above (profiles/r04_e2e_r3sources_summary.txt: 1 M records = 7142
// blocks of ~16 KiB, ~1050 sequences each — play-json text compresses into sequences of 1.4 literal and 13.5 match bytes):
// 108 k SCALAR instructions per block — the sequence headers are wave-uniform, so every length / offset / bounds step is
// SALU work that 63 of 64 lanes only wait for — against 20 k VALU and 3 k LDS instructions; 2.4 ms per fetch, bound by the
// one scalar pipe of a CU.  Two things are serial in an LZ4 block — finding where the next sequence starts, and a match
// reading what an earlier match wrote — and neither needs a wave per sequence:
//   pass 1  lz4_parse_kernel   ONE LANE per block (64 blocks per wave) walks its block's sequence headers: a 16-byte
//           unaligned load at the sequence's first byte holds the token, up to 12 literal bytes, the offset and one length
//           byte — the whole header of all but a fraction of a percent of the sequences — so a step is one load and ~50
//           branch-free VALU instructions for 64 blocks at once.  It writes an 8-byte entry per sequence {position,
//           literal length, match length, offset}, stores the literal bytes where they belong in the decompressed area
//           (they come from the compressed stream, never from earlier output), and validates what the one-pass decoder
//           validates, so the block's exact decompressed size — the section's length and the LDS class of pass 2 — is
//           known before a match is copied.
//   pass 2  lz4_exec_kernel    one WAVE per block, in a launch with exactly the LDS its size needs: the block's image
//           (literals in place) is loaded into LDS; per 64 entries the lanes expand their matches into a byte map
//           (map[p] = the position byte p copies from; identity for literals), then the map is applied 64 output bytes at
//           a time, lane per byte: one gather when no byte of the window reads another byte of the same window, else once
//           more per byte that does (a chain inside a window cannot be longer).  ~5 instructions per sequence instead of
//           ~140, and the serial chain is per 64 bytes of output instead of per sequence.  Overlapping matches (offset <
//           length: the period IS the data), matches above 256 bytes and groups that span more than the map holds take
//           the sequence-by-sequence loop.
constexpr int kLz4Map = 2048;  // bytes of output one group's map may span (a power of two; 64 sequences of play-json text span ~1 KB)
__device__ __constant__ int32_t kLz4ClassCap[kLz4Classes] = {8192, 16384, 24576, 32768, 49152, 65536};
static const int32_t kLz4ClassCapHost[kLz4Classes] = {8192, 16384, 24576, 32768, 49152, 65536};


struct __attribute__((packed)) Unaligned16 { uint64_t lo, hi; };

// bits [b, b + 64) of the 128-bit little-endian window hi:lo, b in [0, 128)
__device__ __forceinline__ uint64_t window_bits(uint64_t lo, uint64_t hi, int b) {
  const uint64_t low = (lo >> (b & 63)) | ((hi << 1) << (63 - (b & 63)));
  return b < 64 ? low : hi >> (b & 63);
}

__device__ __forceinline__ int32_t wave_inclusive_sum(int32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// One sequence whose header does not fit the 16-byte window (literal runs above 12 bytes, lengths continued over several
// bytes) or that ends the block: its header byte by byte out of LDS — every lane reads the same bytes, the values are
// wave-uniform — and its literal run copied by the whole wave.  false = malformed.
__device__ bool lz4_slow_sequence(lds_ptr_t in, int32_t n_in, uint8_t* __restrict__ dst, int32_t& ip, int32_t& op, uint2* __restrict__ out, int32_t& ns,
                                  int lane) {
  const uint32_t token = in[ip++];
  int32_t lit = (int32_t)(token >> 4);
  if (lit == 15) {
    uint32_t x;
    do {
      if (ip >= n_in) return false;
      x = in[ip++];
      lit += (int32_t)x;
    } while (x == 255u && lit < (1 << 24));
  }
  if (lit > n_in - ip || lit > kLz4BlockMax - op) return false;  // (n_in < 64 KiB: a length always fits 16 bits)
  for (int32_t j = lane; j < lit; j += 64) dst[op + j] = in[ip + j];
  ip += lit;
  if (ip >= n_in) {  // the last sequence carries literals only
    // An EMPTY last sequence (token 0x00 behind the last match: encoders other than liblz4 write one) gets no entry: it has
    // nothing to copy, and when the block is full its position, 65536, does not fit the entry's 16 bits (it would read as
    // "op 0, one literal" and push the last group's matches out of lz4_exec_kernel's range — ADVICE r4).
    if (lit > 0) {
      if (lane == 0) out[ns] = make_uint2((uint32_t)op | ((uint32_t)lit << 16), 0u);
      ++ns;
    }
    op += lit;
    return true;
  }
  if (n_in - ip < 2) return false;
  const int32_t offset = (int32_t)in[ip] | ((int32_t)in[ip + 1] << 8);
  ip += 2;
  int32_t ml = (int32_t)(token & 15u);
  if (ml == 15) {
    uint32_t x;
    do {
      if (ip >= n_in) return false;
      x = in[ip++];
      ml += (int32_t)x;
    } while (x == 255u && ml < (1 << 24));
  }
  ml += 4;
  const int32_t D = op + lit;
  // offset <= D and offset >= 1 make D >= 1, so a match that fits the block is at most 65535 long
  if (offset == 0 || offset > D || ml > kLz4BlockMax - D) return false;
  if (lane == 0) out[ns] = make_uint2((uint32_t)op | ((uint32_t)lit << 16), (uint32_t)ml | ((uint32_t)offset << 16));
  ++ns;
  op = D + ml;
  return true;
}

// Pass 1, one WAVE per block.  Where a sequence starts is only known once the one before it is decoded — but decoding a
// header is cheap, so every lane decodes the header that WOULD start at its byte of the current 64-byte window of the
// compressed block (staged in LDS), and the wave then follows the chain of real starts through those 64 candidates with
// v_readlane (a play-json block has a sequence every ~5 bytes: a dozen real ones per window).  The real lanes get their
// output positions from a wave prefix sum, write their table entries side by side and store their literal bytes.  (The
// first version gave every block ONE LANE that walked its headers alone: ~150 dependent instructions per sequence on a
// wave that has the SIMD to itself — 0.9 ms per 1 M records however the loads were arranged.)  A wave takes its block
// when lo_excl < staged bytes <= cap (two launches: 8 KiB of LDS, 20 waves per CU, for the batches a 16 KiB producer
// writes; 64 KiB for the rest).
__global__ void __launch_bounds__(64) lz4_parse_kernel(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ out_base, const Lz4Block* __restrict__ blocks,
                                                       int32_t n_blocks, Lz4Work w, Section* __restrict__ sections, ErrorCell* err, int32_t lo_excl, int32_t cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lz4_in[];
  const int lane = threadIdx.x;
  const int32_t b = (int32_t)blockIdx.x;
  const Lz4Block blk = blocks[b];
  if (blk.seq_off < 0) return;  // the one-pass kernel's
  const int32_t n_in = blk.src_len & 0x7fffffff;
  const bool stored = blk.src_len < 0;
  const int32_t skew = (int32_t)(blk.src_off & 15);
  const int32_t need_lds = stored ? 0 : skew + n_in + 48;
  if (!(need_lds > lo_excl && need_lds <= cap)) return;
  uint8_t* __restrict__ dst = out_base + blk.dst_off;
  int32_t op = 0, ns = 0;
  bool ok = true;
  int32_t cls = kLz4Classes;  // stored
  if (stored) {
    op = n_in;
    ok = n_in <= kLz4BlockMax;
  } else {
    {  // the block's bytes, from the 16-byte line its first byte lies in (the staged bytes end 64 bytes after their last byte)
      const uint4* src = (const uint4*)(bytes + blk.src_off - skew);
      const int n16 = (skew + n_in + 47) >> 4;
      for (int i = lane; i < n16; i += 64) ((uint4*)lz4_in)[i] = src[i];
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const lds_ptr_t in = (lds_ptr_t)lz4_in + skew;
    const uint32_t* in32 = (const uint32_t*)lz4_in;
    uint2* __restrict__ out = w.seq + blk.seq_off;
    int32_t base = 0, t0 = 0;
    while (ok && base + t0 < n_in) {
      const int32_t q = base + lane;
      // the 16 bytes from this lane's position on: five aligned dwords, shifted into place
      const uint32_t A = (uint32_t)(skew + q);
      const uint32_t* d = in32 + (A >> 2);
      const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
      const uint32_t shb = A & 3u;
      const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, shb), w1 = __builtin_amdgcn_alignbyte(d2, d1, shb);
      const uint32_t w2 = __builtin_amdgcn_alignbyte(d3, d2, shb), w3 = __builtin_amdgcn_alignbyte(d4, d3, shb);
      const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w2 | ((uint64_t)w3 << 32);
      const uint32_t token = w0 & 0xffu;
      const int32_t lit = (int32_t)(token >> 4), mlc = (int32_t)(token & 15u);
      const int32_t need = 3 + lit + (mlc == 15 ? 1 : 0);
      const uint32_t tail = (uint32_t)window_bits(lo, hi, 8 * (1 + (lit & 15)));  // offset (16 bits), then the length byte
      // (the block's last, literal-only sequence has no room for an offset: not simple)
      const bool simple = q < n_in && lit <= 12 && need <= n_in - q && !(mlc == 15 && ((tail >> 16) & 0xffu) == 255u);
      const int32_t offset = (int32_t)(tail & 0xffffu);
      const int32_t ml = mlc + 4 + (mlc == 15 ? (int32_t)((tail >> 16) & 0xffu) : 0);
      const int32_t nxt = lane + need;
      // the chain of real sequence starts through this window
      const unsigned long long smask = __ballot(simple);
      unsigned long long real = 0ull;
      int32_t t = t0;
      while (t < 64 && ((smask >> t) & 1ull)) {
        real |= 1ull << t;
        t = __builtin_amdgcn_readlane(nxt, t);
      }
      const bool is_real = (real >> lane) & 1ull;
      const int32_t v = is_real ? lit + ml : 0;
      const int32_t incl = wave_inclusive_sum(v, lane);
      const int32_t my_op = op + incl - v, D = my_op + lit;
      const bool bad = is_real && (lit > kLz4BlockMax - my_op || offset == 0 || offset > D || ml > kLz4BlockMax - D);
      if (__any(bad)) { ok = false; break; }
      if (is_real) {
        const int32_t rank = __builtin_popcountll(real & ((1ull << lane) - 1ull));
        out[ns + rank] = make_uint2((uint32_t)my_op | ((uint32_t)lit << 16), (uint32_t)ml | ((uint32_t)offset << 16));
      }
      // the literal bytes, exactly (two sequences of one window may lie closer together than a wide store is long)
      {
        const int32_t my_lit = is_real ? lit : 0;
        const uint64_t lits_lo = (lo >> 8) | (hi << 56), lits_hi = hi >> 8;
        for (int32_t j = 0; __any(j < my_lit); ++j)
          if (j < my_lit) dst[my_op + j] = (uint8_t)((j < 8 ? lits_lo : lits_hi) >> (8 * (j & 7)));
      }
      ns += __builtin_popcountll(real);
      op += __builtin_amdgcn_readlane(incl, 63);
      if (t >= 64) {
        base += 64;
        t0 = t - 64;
      } else {
        int32_t ip = base + t;
        if (ip >= n_in) break;
        // (stores of this wave to one address keep their order: the literal bytes written above are not overtaken)
        if (!lz4_slow_sequence(in, n_in, dst, ip, op, out, ns, lane)) { ok = false; break; }
        base = ip & ~63;
        t0 = ip & 63;
      }
    }
    cls = 0;
    while (cls < kLz4Classes - 1 && op > kLz4ClassCap[cls]) ++cls;
  }
  if (ok && !blk.last && op != kLz4BlockMax) ok = false;  // every block of a frame but its last is exactly full
  if (lane != 0) return;
  w.n_seq[b] = ns;
  if (!ok) {
    w.state[b] = -1;
    atomicMin(&err->lz4_bad, (unsigned int)blk.section);
    if (blk.last) sections[blk.section].byte_len = 0;
    return;
  }
  w.state[b] = op;
  if (blk.last) sections[blk.section].byte_len = (int64_t)blk.index * kLz4BlockMax + op;
  if (op > 0) w.cls_list[(int64_t)cls * n_blocks + atomicAdd(&w.cls_count[cls], 1)] = b;
}

// cls == kLz4Classes: stored blocks (launched without LDS).  LDS: the block's image (the class's capacity), then the byte
// map (kLz4Map 16-bit positions).  A masked-off lane may READ up to 63 bytes past the image — the start of the map, harmless;
// nothing is written past the class's capacity — so the image needs no pad of its own: 16 KiB + 4 KiB = 20 480 bytes is
// exactly an eighth of a CU's 160 KiB (the 64-byte pad of round 4 made it seven waves per CU for the batches the reference's
// 16 KiB producer writes).
// (As first written the map was read per window and the dependency rounds went through a cross-lane read; the batched loop
// below is 1.8 % faster end to end, profiles/r04_e2e_lz4_windows.txt — the kernels' LDS footprint x time bounds the path, not
// this loop's latency alone.)
__global__ void __launch_bounds__(64) lz4_exec_kernel(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ out_base, const Lz4Block* __restrict__ blocks,
                                                      int32_t n_blocks, Lz4Work w, int32_t cls, int32_t cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lz4_out[];
  uint16_t* const map = (uint16_t*)(lz4_out + cap);
  const int lane = threadIdx.x;
  const int32_t count = w.cls_count[cls];
  for (int32_t k = (int32_t)blockIdx.x; k < count; k += (int32_t)gridDim.x) {
    const int32_t b = w.cls_list[(int64_t)cls * n_blocks + k];
    const Lz4Block blk = blocks[b];
    uint8_t* __restrict__ dst = out_base + blk.dst_off;  // 16-byte aligned: dst_off is a multiple of 64 KiB from an aligned base
    const int32_t size = w.state[b];
    if (cls == kLz4Classes) {  // stored: the bytes as they are
      const uint8_t* __restrict__ in = bytes + blk.src_off;
      for (int i = lane; i < size; i += 64) dst[i] = in[i];
      continue;
    }
    // the image with the literals the first pass put in place
    const int n16 = (size + 15) >> 4;
    for (int i = lane; i < n16; i += 64) ((uint4*)lz4_out)[i] = ((const uint4*)dst)[i];
    const int32_t n = w.n_seq[b];
    const uint2* __restrict__ sq = w.seq + blk.seq_off;
    uint2 e_next = lane < n ? sq[lane] : make_uint2(0u, 0u);
    for (int32_t g = 0; g < (w.dbg == 1 ? 0 : n); g += 64) {
      const uint2 e = e_next;
      if (g + 64 < n) e_next = g + 64 + lane < n ? sq[g + 64 + lane] : make_uint2(0u, 0u);  // in flight during this group
      const int32_t cnt = n - g < 64 ? n - g : 64;
      const int32_t op = (int32_t)(e.x & 0xffffu), lit = (int32_t)(e.x >> 16), M = (int32_t)(e.y & 0xffffu), O = (int32_t)(e.y >> 16);
      const int32_t D = op + lit, end = D + M;
      const int32_t g0 = __builtin_amdgcn_readfirstlane(op), g1 = __builtin_amdgcn_readlane(end, cnt - 1);
      const bool mapped = g1 - g0 <= kLz4Map && !__any(lane < cnt && M > 0 && (O < M || M > 256));
      if (mapped) {
        // (LDS operations of one wave execute in order: a read sees every earlier write of any lane of this wave)
        for (int32_t p = g0 + lane; p < g1; p += 64) map[p & (kLz4Map - 1)] = (uint16_t)p;
        const int32_t m_lane = lane < cnt ? M : 0;
        for (int32_t i = 0; __any(i < m_lane); ++i)
          if (i < m_lane) map[(D + i) & (kLz4Map - 1)] = (uint16_t)(D - O + i);
        // Eight windows' map entries are read together (the map does not change while it is applied): one LDS round trip
        // for eight windows instead of one each.  A window is then: gather, write, and per dependency round a ballot, a
        // gather and a write — whether a byte's source is written yet is a bit of the ballot, not a cross-lane read.
        constexpr int kWin = 8;
        if (w.dbg == 2) continue;
        for (int32_t p0 = g0; p0 < g1; p0 += 64 * kWin) {
          int32_t srcs[kWin];
#pragma unroll
          for (int k = 0; k < kWin; ++k) {
            const int32_t pos = p0 + 64 * k + lane;
            srcs[k] = pos < g1 ? (int32_t)map[pos & (kLz4Map - 1)] : pos;
          }
#pragma unroll
          for (int k = 0; k < kWin; ++k) {
            const int32_t p = p0 + 64 * k;
            if (p >= g1) break;  // (wave-uniform)
            const int32_t pos = p + lane;
            const bool act = pos < g1;
            const int32_t src = srcs[k];
            // Bytes that copy from THIS window wait for their source: first everything whose source lies below the window (or
            // is the byte itself: a literal), then, round by round, the bytes whose source was written in the round before —
            // as many rounds as the longest chain inside the window is deep (one or two; the first version ran one round per
            // dependent BYTE: a 13-byte match at offset 20 cost 14 rounds).
            const bool dep = act && src >= p && src != pos;
            bool done = !dep;
            {
              const uint8_t v = lz4_out[src];
              if (act && !dep) lz4_out[pos] = v;
            }
            unsigned long long dm = __ballot(done);
            while (dm != ~0ull) {
              const bool can = !done && ((dm >> ((src - p) & 63)) & 1ull) != 0ull;
              const uint8_t v = lz4_out[src];
              if (can) lz4_out[pos] = v;
              done = done || can;
              dm = __ballot(done);
            }
          }
        }
      } else {
        // sequence by sequence, strictly in order
        for (int32_t s = 0; s < cnt; ++s) {
          const int32_t Ms = __builtin_amdgcn_readlane(M, s);
          if (Ms == 0) continue;  // the block's last sequence
          const int32_t Os = __builtin_amdgcn_readlane(O, s), Ds = __builtin_amdgcn_readlane(D, s);
          const uint8_t* src = lz4_out + Ds - Os;
          if (Os >= Ms || Os >= 64) {  // chunks of 64 bytes never read what the same instruction writes
            for (int32_t i = lane; i < Ms; i += 64) lz4_out[Ds + i] = src[i];
          } else {                     // the period IS the data
            for (int32_t i = lane; i < Ms; i += 64) lz4_out[Ds + i] = src[i % Os];
          }
        }
      }
    }
    const int f16 = size >> 4;
    for (int i = lane; i < f16; i += 64) ((uint4*)dst)[i] = ((const uint4*)lz4_out)[i];
    for (int i = (f16 << 4) + lane; i < size; i += 64) dst[i] = lz4_out[i];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // the copy-out has read the LDS before the next block overwrites it
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

// LZ4 sections (codec 3: the batch's records section is still one LZ4 frame): the host reads the frame header and the
// block size words, the device decodes the blocks.  Frames it cannot take block by block (blocks larger than 64 KiB,
// dependent blocks) are decompressed here, on the host, and travel as plain bytes behind the raw spans.
Lz4Route lz4_plan_section(Lz4Plan& plan, const uint8_t* f, int64_t fl, int64_t src_off, int32_t section, int64_t* area_off, std::vector<uint8_t>& host_out) {
  std::vector<Lz4Block>& blocks = plan.blocks;
  bool device_ok = fl >= 7 && f[0] == 0x04 && f[1] == 0x22 && f[2] == 0x4D && f[3] == 0x18 && (f[4] >> 6) == 1 && (f[4] & 0x20) &&
                   ((f[5] >> 4) & 7) == 4;
  int64_t q = 6;
  if (device_ok) {
    if (f[4] & 0x08) q += 8;  // content size
    if (f[4] & 0x01) q += 4;  // dictionary id
    device_ok = q < fl && f[q] == (uint8_t)(surge_xxh32(f + 4, q - 4, 0) >> 8);
    ++q;
  }
  const size_t first_block = blocks.size();
  const int64_t seq_mark = plan.n_seq;
  int32_t k = 0;
  while (device_ok) {
    if (fl - q < 4) { device_ok = false; break; }
    const uint32_t bs = (uint32_t)f[q] | ((uint32_t)f[q + 1] << 8) | ((uint32_t)f[q + 2] << 16) | ((uint32_t)f[q + 3] << 24);
    q += 4;
    if (bs == 0) break;  // EndMark
    const uint32_t size = bs & 0x7fffffffu;
    if ((int64_t)size > fl - q || size > (1u << 30)) { device_ok = false; break; }
    Lz4Block b;
    b.src_off = src_off + q;
    b.dst_off = plan.area + (int64_t)k * kLz4BlockMax;
    b.src_len = (int32_t)size | (int32_t)(bs & 0x80000000u);
    b.section = section;
    b.last = 0;
    b.index = k++;
    // a sequence with a match takes at least 3 bytes of the block, the closing literal run at least 1
    if (size < (uint32_t)kLz4BlockMax) {
      b.seq_off = plan.n_seq;
      plan.n_seq += (bs & 0x80000000u) ? 0 : (int64_t)size / 3 + 2;
    } else {
      b.seq_off = -1;
    }
    blocks.push_back(b);
    q += size;
    if (f[4] & 0x10) q += 4;  // block checksum (not verified: the batch CRC already covers these bytes)
  }
  if (device_ok && k > 0) {
    blocks.back().last = 1;
    *area_off = plan.area;
    plan.area += (int64_t)k * kLz4BlockMax;
    return LZ4_ON_DEVICE;
  }
  blocks.resize(first_block);
  plan.n_seq = seq_mark;
  int64_t cap = fl * 8 + 1024, got;
  const size_t ex = host_out.size();
  while (true) {
    host_out.resize(ex + (size_t)cap);
    got = surge_lz4_frame_decompress(f, fl, host_out.data() + ex, cap);
    if (got != -6) break;
    cap *= 4;
    if (cap > (1ll << 31)) return LZ4_TOO_LARGE;
  }
  if (got < 0) return LZ4_BAD_FRAME;
  host_out.resize(ex + (size_t)got);
  return LZ4_ON_HOST;
}

Lz4ScratchBytes lz4_scratch_bytes(const Lz4Plan& plan) {
  Lz4ScratchBytes n;
  const size_t nb = plan.blocks.size();
  if (nb == 0) return n;
  n.blocks = nb * sizeof(Lz4Block);
  n.state = nb * 4;
  n.n_seq = nb * 4;
  n.seq = (size_t)(plan.n_seq + 1) * 8;
  n.cls = (size_t)(kLz4Classes + 1) * (nb + 1) * 4;
  return n;
}

hipError_t launch_lz4_exec(const uint8_t* bytes, uint8_t* area, const Lz4Block* d_blocks, int64_t nb, Lz4Work w, hipStream_t st) {
  for (int c = 0; c <= kLz4Classes; ++c) {
    const int32_t cap = c < kLz4Classes ? kLz4ClassCapHost[c] : 0;
    const size_t lds = cap ? (size_t)cap + (size_t)kLz4Map * 2 : 0;
    const int64_t resident = 256ll * (lds ? (int64_t)(160 * 1024 / lds) : 16);  // waves the chip holds at this LDS size
    hipLaunchKernelGGL(lz4_exec_kernel, dim3((unsigned)(nb < resident ? nb : resident)), dim3(64), lds, st, bytes, area, d_blocks, (int32_t)nb, w, c, cap);
  }
  return hipGetLastError();
}

hipError_t launch_lz4(const Lz4Plan& plan, const uint8_t* bytes, uint8_t* area, const Lz4Block* d_blocks, Lz4Work w, Section* sections, ErrorCell* err,
                      hipStream_t st) {
  const int64_t nb = (int64_t)plan.blocks.size();
  if (nb == 0) return hipSuccess;
  // two passes: the sequence headers by one wave per block, then the copies by one wave per block in a launch with
  // the LDS the block's size needs (the first pass knows it)
  w.cls_list = w.cls_count + (kLz4Classes + 1);
  const hipError_t e = hipMemsetAsync(w.cls_count, 0, (kLz4Classes + 1) * 4, st);
  if (e != hipSuccess) return e;
  // LDS of the launches of the first pass.  A block of the 16 KiB producer compresses to 3 - 5.5 KiB: 6.5 KiB of LDS is what
  // 24 waves per CU — all the kernel's 78 VGPRs allow — leave each other (8 KiB: 20 waves); a batch that compresses badly
  // takes the 16 KiB class (9 waves per CU) instead of sharing a CU with one other wave in the 64 KiB one.  (Round 4 had two
  // launches, {8 KiB, 64 KiB}.)
  const int32_t parse_caps[3] = {6656, 16384 + 64, kLz4BlockMax + 64};
  for (int c = 0; c < 3; ++c)
    hipLaunchKernelGGL(lz4_parse_kernel, dim3((unsigned)nb), dim3(64), (size_t)parse_caps[c], st, bytes, area, d_blocks, (int32_t)nb, w, sections, err,
                       c == 0 ? -1 : parse_caps[c - 1], parse_caps[c]);
  (void)launch_lz4_exec(bytes, area, d_blocks, nb, w, st);
  bool any_one_pass = false;  // blocks of exactly 64 KiB (or more) compressed
  for (const Lz4Block& b : plan.blocks) any_one_pass = any_one_pass || b.seq_off < 0;
  if (any_one_pass) {
    const unsigned grid = (unsigned)(nb < 8192 ? nb : 8192);
    const int32_t caps[3] = {16384, 32768, kLz4BlockMax};  // LDS per wave of the three launches
    for (int c = 0; c < 3; ++c)
      hipLaunchKernelGGL(lz4_block_kernel, dim3(grid), dim3(64), (size_t)caps[c], st, bytes, area, d_blocks, nb, w.state, c, caps[c], sections, err);
  }
  // (a frame that does not decode zeroes its section and raises the error cell: the push fails in stage 2's first
  // synchronisation, before anything is committed)
  return hipGetLastError();
}

}  // namespace ingest
}  // namespace surge
