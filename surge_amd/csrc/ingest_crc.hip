// ingest_crc.hip — the device decoder's first stage: a record batch's CRC-32C, finished where its bytes now are.
#include <mutex>

#include "ingest_device.h"

namespace surge {
namespace ingest {
namespace {

// ---- CRC-32C of a batch, finished on the device (SURGE_INGEST_DEVICE_CRC) ----------------------------------------------------
// A record batch's CRC-32C (Castagnoli, reflected; kafka-clients: Crc32C over attributes .. end of the batch) covers 40 header
// bytes and then the records section — the bytes this decoder is handed anyway.  The host framer runs the CRC over the 40
// header bytes only and passes on the register (in-place framing: not even those); one WAVE per section takes it from there,
// 4 KiB at a time (a compressed batch of the reference's publisher is 2 - 5 KB: one or two tiles):
//   * the tile is laid right-aligned into a 4 KiB frame, lane l owns frame bytes [64 l, 64 l + 64) (the lanes in front of a
//     short tile are empty: a zero register is neutral under what follows) and runs the CRC over its piece a dword at a time
//     out of LDS (pieces of 16 dwords, 17 apart: lanes read different banks), four table look-ups per dword (slicing by four:
//     4 x 256 entries in LDS, loaded once per workgroup of four waves);
//   * a CRC register is linear in (register, data): crc(A || B) = shift(crc(A), |B|) ^ crc_0(B), and shifting by a FIXED
//     length is one multiplication mod P by a constant x^(8 |B|): lane l multiplies its register by x^(8 * 64 (63 - l)) — ONE
//     multiplication per lane, all lanes at once — and the tile's register is the XOR over the wave; one more multiplication
//     (by x^(8 * 4096), wave-uniform) chains a tile to the ones before it.  65 constants, computed once on the host.
// History: bit-serial CRC, 16 KiB tiles, 182 us per 10^6-record fetch (profiles/r06_e2e_inplace_kernel_stats.csv); slicing by
// four with 256-byte pieces and a six-level lane tree of multiplications, 122 us alone / 244 us on the wider topic's 66 MB
// (r06_e2e_*_depth1_kernel_stats.csv): 64 dependent look-up rounds and seven serial 32-step multiplications per tile, most
// lanes of a 4 KB section idle.  A mismatch is reported like a bad LZ4 frame: the push fails with SURGE_E_CORRUPT, nothing of
// it is delivered, no key it brought stays interned.
constexpr uint32_t kCrcPoly = 0x82F63B78u;
constexpr int kCrcTile = 4096, kCrcPiece = 64, kCrcWaves = 4;
constexpr int kCrcLdsDwords = 65 * 17;  // 64 pieces + the dword a misaligned tile spills into, every piece padded by one dword

// a * b mod P, reflected representation (bit 31 = x^0): 32 fixed steps (zlib's multmodp stops early on a's last set bit —
// and never on a == 0, which an empty lane's register is)
__host__ __device__ inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0u;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    p ^= b & (uint32_t)-(int32_t)((a >> (31 - i)) & 1u);
    b = (b >> 1) ^ (kCrcPoly & (uint32_t)-(int32_t)(b & 1u));
  }
  return p;
}

// x^(8 n) mod P
static uint32_t crc_x8n(uint64_t n) {
  uint32_t sq = 1u << 30, p = 1u << 31;  // x^1, x^0
  for (uint64_t bits = n * 8; bits; bits >>= 1) {
    if (bits & 1u) p = crc_mulmod(sq, p);
    sq = crc_mulmod(sq, sq);
  }
  return p;
}

// What the kernel reads from device memory: the slicing-by-four tables (T[k][b] = the register after byte b followed by k
// zero bytes), lane l's shift x^(8 * 64 (63 - l)), the tile's shift x^(8 * 4096).
struct CrcTables {
  uint32_t slice[4][256];
  uint32_t lane_shift[64];
  uint32_t tile_shift, pad[3];
};
static const CrcTables& crc_tables() {
  static const CrcTables T = [] {
    CrcTables x{};
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
      x.slice[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int k = 1; k < 4; ++k) x.slice[k][i] = (x.slice[k - 1][i] >> 8) ^ x.slice[0][x.slice[k - 1][i] & 0xffu];
    for (int l = 0; l < 64; ++l) x.lane_shift[l] = crc_x8n((uint64_t)kCrcPiece * (uint64_t)(63 - l));
    x.tile_shift = crc_x8n((uint64_t)kCrcTile);
    return x;
  }();
  return T;
}

__global__ void __launch_bounds__(64 * kCrcWaves) crc_kernel(const uint8_t* __restrict__ bytes, const CrcSpan* __restrict__ spans, int32_t n_spans,
                                                             const CrcTables* __restrict__ tables, ErrorCell* err) {
  __shared__ uint32_t frames[kCrcWaves][kCrcLdsDwords];
  __shared__ uint32_t Ts[4 * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * 256; i += 64 * kCrcWaves) Ts[i] = (&tables->slice[0][0])[i];
  __syncthreads();
  const int32_t span = (int32_t)blockIdx.x * kCrcWaves + wave;
  if (span >= n_spans) return;  // (behind the workgroup's only barrier)
  uint32_t* A = frames[wave];
  const uint32_t lane_k = tables->lane_shift[lane], tile_k = tables->tile_shift;
  const CrcSpan sp = spans[span];
  const uint32_t expect = sp.expect, state = sp.state;
  uint32_t total = state;  // (a section of no bytes: the register as the host left it)
  int64_t done = 0;
  bool first = true;
  while (done < sp.len) {
    int32_t T = (int32_t)((sp.len - done) % kCrcTile);
    if (T == 0) T = kCrcTile;
    // frame byte p of this tile = global byte base + p, valid for p >= v0
    const int32_t v0 = kCrcTile - T;
    const int64_t base = sp.off + done - v0;   // (may lie in front of the staged bytes: only p >= v0 is ever read)
    const int32_t sh = (int32_t)(base & 3);
    const int64_t abase = base - sh;           // the aligned stream A[j] = dword at abase + 4 j, j in [0, 1024]
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k <= kCrcTile / 256; ++k) {
      const int j = lane + 64 * k;
      if (j > kCrcTile / 4) continue;  // (the 1025th dword: lane 0 only)
      const int64_t g = abase + 4ll * j;
      uint32_t w = 0u;
      if (g + 4 > base + v0 && g < base + kCrcTile) {  // overlaps the tile
        if (g >= sp.off - 4 && g + 4 <= sp.off + sp.len + 64) w = *(const uint32_t*)(bytes + g);  // inside what was staged (at least 4 bytes of prefix in front, 64 spare bytes behind)
        else
          for (int b = 0; b < 4; ++b)
            if (g + b >= sp.off && g + b < sp.off + sp.len) w |= (uint32_t)bytes[g + b] << (8 * b);
      }
      A[(j >> 4) * 17 + (j & 15)] = w;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // my 64 bytes: frame [64 lane, 64 lane + 64)
    const int32_t p0 = kCrcPiece * lane, p1 = p0 + kCrcPiece;
    uint32_t r = 0u;
    if (p1 > v0) {
      int32_t p = p0 > v0 ? p0 : v0;
      const bool holds_first = first && p0 <= v0;  // the section's very first byte is mine: the host's register goes in here
      if (holds_first) r = state;
      auto dword_at = [&](int32_t q) -> uint32_t {  // frame dword q (frame bytes [4 q, 4 q + 4))
        const uint32_t lo = A[(q >> 4) * 17 + (q & 15)], hi = A[((q + 1) >> 4) * 17 + ((q + 1) & 15)];
        return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
      };
      // the bytes in front of my first whole dword (a tile that starts inside one)
      while ((p & 3) && p < p1) {
        const uint32_t w = dword_at(p >> 2);
        r ^= (w >> (8 * (p & 3))) & 0xffu;
        r = (r >> 8) ^ Ts[r & 0xffu];
        ++p;
      }
      for (; p + 4 <= p1; p += 4) {
        const uint32_t x = r ^ dword_at(p >> 2);
        r = Ts[768 + (x & 0xffu)] ^ Ts[512 + ((x >> 8) & 0xffu)] ^ Ts[256 + ((x >> 16) & 0xffu)] ^ Ts[x >> 24];
      }
    }
    // every lane shifts its register over the pieces behind it; the tile's register is the XOR of them all
    r = crc_mulmod(r, lane_k);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) r ^= (uint32_t)__shfl_xor((int)r, s, 64);
    total = first ? r : crc_mulmod(total, tile_k) ^ r;
    first = false;
    done += T;
  }
  if (lane == 0 && ~total != expect) atomicMin(&err->crc_bad, (unsigned int)sp.section);
}

}  // namespace

hipError_t launch_crc(const uint8_t* bytes, const CrcSpan* spans, int32_t n_spans, ErrorCell* err, hipStream_t st) {
  // the tables on the calling thread's device: 4.3 KB, made at the first call there and kept for the life of the process
  static std::mutex mu;
  static const CrcTables* per_device[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const CrcTables* tables = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!per_device[dev]) {
      void* p = nullptr;
      if ((e = hipMalloc(&p, sizeof(CrcTables))) != hipSuccess) return e;
      if ((e = hipMemcpy(p, &crc_tables(), sizeof(CrcTables), hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipFree(p);
        return e;
      }
      per_device[dev] = (const CrcTables*)p;
    }
    tables = per_device[dev];
  }
  hipLaunchKernelGGL(crc_kernel, dim3((unsigned)((n_spans + kCrcWaves - 1) / kCrcWaves)), dim3(64 * kCrcWaves), 0, st, bytes, spans, n_spans, tables, err);
  return hipGetLastError();
}

}  // namespace ingest
}  // namespace surge
