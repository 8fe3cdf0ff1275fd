// ingest_snappy.hip — the device decoder's snappy stage: what knows how a snappy stream spells literals and copies
// (snappy_block.h has the grammar, for this file and the host alike).  The host half walks a section's framing — per chunk the
// length word and the preamble varint, nothing per byte (snappy_plan_section) — the device half is a parse pass only
// (snappy_parse_kernel): it writes the entry table and the literal bytes the LZ4 stage's second pass works from, and that pass
// (lz4_exec_kernel, launch_lz4_exec) applies the copies as it applies LZ4 matches: it never knew which format the entries
// came from.
#include <new>

#include "ingest_device.h"
#include "snappy_block.h"

namespace surge {
namespace ingest {
namespace {

constexpr int32_t kSnappyChunkMax = 65536;  // output of a chunk the device takes: what an entry's 16-bit positions and the exec pass's largest LDS class hold
// LDS of the parse launches, smallest first (a wave takes its chunk in the first that holds it).  kafka-clients' chunk is 32 KiB
// of records; as play-json text that is 5 - 8 KiB compressed: 10 KiB of LDS lets 16 such waves share a CU, where one class for
// everything would leave each of them the CU with one other wave.  The largest holds the longest stream 64 KiB can compress
// to (32 + n + n / 6 = 76 490 bytes) with its skew and pad.
constexpr int kSnappyParseClasses = 4;
constexpr int32_t kSnappyParseCap[kSnappyParseClasses] = {10240, 20480, 40960, 81920};
// A lane of a chunk's last window looks at the 12 bytes from its own position on, up to 63 bytes behind the chunk's last: LDS
// the kernel owns (what it finds there is never used — a candidate counts only when its header ends inside the chunk).
constexpr int32_t kSnappyStagePad = 80;
constexpr int32_t kSnappyStageMax = kSnappyParseCap[kSnappyParseClasses - 1] - 15 - kSnappyStagePad;  // compressed bytes of a chunk the device takes
constexpr int32_t kSnappyShortLiteral = 16;  // literals up to here are stored by their own lane, longer ones by the whole wave

__device__ __forceinline__ int32_t wave_inclusive_sum(int32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// One WAVE per chunk, the chunk's bytes (preamble included) staged in LDS by 16-byte loads.  Where an element starts is only
// known once the one before it is decoded — but a snappy element's header length follows from its tag byte alone, so every lane
// decodes the element that WOULD start at its byte of the current 64-byte window, and the wave follows the chain of real starts
// through those 64 candidates with v_readlane (lz4_parse_kernel's answer to the same problem; there a long header needs a slow
// path, here none does).  A wave prefix sum gives the real elements their output positions; real literals store their bytes
// where they belong in the destination (they come from the stream, never from earlier output) — short ones lane by lane, runs
// above kSnappyShortLiteral by the whole wave — and every real copy writes one entry {op | lit << 16, M | O << 16}: op = where
// the literals since the previous copy begin, lit = their count.  Literal-only stretches need no entry: after a copy-free chunk
// nothing is listed for the exec pass.  op, D = op + lit and O stay <= 65 535 because a copy of M >= 1 must end inside 65 536.
// Checked as the host decoder checks (snappy_block.h): headers and literals inside the chunk, offset 0, an offset beyond the
// output so far, output beyond the preamble — and the chunk is good only when the output ends exactly at the preamble.
__global__ void __launch_bounds__(64) snappy_parse_kernel(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ out_base, const Lz4Block* __restrict__ blocks,
                                                          int32_t n_blocks, Lz4Work w, Section* __restrict__ sections, ErrorCell* err, int32_t lo_excl, int32_t cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sn_in[];
  const int lane = threadIdx.x;
  const int32_t b = (int32_t)blockIdx.x;
  const Lz4Block blk = blocks[b];
  const int32_t n_in = blk.src_len;
  const int32_t skew = (int32_t)(blk.src_off & 15);
  const int32_t need_lds = skew + n_in + kSnappyStagePad;
  if (!(need_lds > lo_excl && need_lds <= cap)) return;  // another launch's
  uint8_t* __restrict__ dst = out_base + blk.dst_off;
  {  // the chunk's bytes, from the 16-byte line its first byte lies in
    const uint4* src = (const uint4*)(bytes + blk.src_off - skew);
    const int n16 = (skew + n_in + 15) >> 4;
    for (int i = lane; i < n16; i += 64) ((uint4*)sn_in)[i] = src[i];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const lds_ptr_t in = (lds_ptr_t)sn_in + skew;
  const uint32_t* in32 = (const uint32_t*)sn_in;
  uint2* __restrict__ out = w.seq + blk.seq_off;
  // the preamble (wave-uniform: every lane reads the same bytes)
  uint32_t want_u = 0;
  int32_t ip0 = 0;
  bool ok = false;
  {
    uint32_t v = 0;
    for (int32_t k = 0; k < 5 && k < n_in; ++k) {
      const uint32_t x = in[k];
      if (k == 4 && x > 0x0fu) break;  // more than 2^32 - 1, or a sixth byte
      v |= (x & 0x7fu) << (7 * k);
      if (!(x & 0x80u)) {
        want_u = v;
        ip0 = k + 1;
        ok = true;
        break;
      }
    }
  }
  if (ok && want_u > (uint32_t)kSnappyChunkMax) ok = false;  // (the plan sends such a chunk through the host: not reached by what it planned)
  const int32_t want = (int32_t)want_u;
  int32_t op = 0, ns = 0, prev_end = 0;
  int32_t base = 0, t0 = ip0;
  while (ok && base + t0 < n_in) {
    const int32_t q = base + lane;
    // the 8 bytes from this lane's position on: three aligned dwords, shifted into place
    const uint32_t A = (uint32_t)(skew + q);
    const uint32_t* d = in32 + (A >> 2);
    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
    const uint32_t shb = A & 3u;
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, shb), w1 = __builtin_amdgcn_alignbyte(d2, d1, shb);
    const surge::snappy::Element e = surge::snappy::element(w0 & 0xffu, (w0 >> 8) | (w1 << 24));
    const int32_t hdr = (int32_t)e.header;
    const int32_t n = (int32_t)(e.n1 < 65536u ? e.n1 : 65536u) + 1;  // length (a literal beyond 65 536 never fits the chunk: refused below)
    const bool fits = q < n_in && hdr <= n_in - q && (e.copy || (e.n1 < 65536u && n <= n_in - q - hdr));
    const int32_t nxt = lane + hdr + (e.copy ? 0 : n);
    // the chain of real element starts through this window
    const unsigned long long fmask = __ballot(fits);
    unsigned long long real = 0ull;
    int32_t t = t0;
    while (t < 64 && base + t < n_in) {
      if (!((fmask >> t) & 1ull)) { ok = false; break; }  // a header or a literal that runs past the chunk
      real |= 1ull << t;
      t = __builtin_amdgcn_readlane(nxt, t);
    }
    if (!ok) break;
    const bool is_real = (real >> lane) & 1ull;
    const int32_t v = is_real ? n : 0;
    const int32_t incl = wave_inclusive_sum(v, lane);
    const int32_t my_op = op + incl - v;
    const bool bad = is_real && (v > want - my_op || (e.copy && (e.offset == 0u || e.offset > (uint32_t)my_op)));
    if (__any(bad)) { ok = false; break; }
    // one entry per real copy, side by side
    const bool is_copy = is_real && e.copy;
    const unsigned long long cmask = __ballot(is_copy);
    const unsigned long long below = cmask & ((1ull << lane) - 1ull);
    const int32_t end = my_op + v;
    const int32_t end_below = __shfl(end, below ? 63 - __builtin_clzll(below) : 0, 64);
    if (is_copy) {
      const int32_t from = below ? end_below : prev_end;  // where the previous copy ended: the literals since begin there
      out[ns + __builtin_popcountll(below)] = make_uint2((uint32_t)from | ((uint32_t)(my_op - from) << 16), (uint32_t)v | (e.offset << 16));
    }
    // the literal bytes
    {
      const int32_t my_lit = is_real && !e.copy ? v : 0;
      const int32_t my_src = q + hdr;
      const int32_t mine = my_lit <= kSnappyShortLiteral ? my_lit : 0;
      for (int32_t j = 0; __any(j < mine); ++j)
        if (j < mine) dst[my_op + j] = in[my_src + j];
      unsigned long long longs = __ballot(my_lit > kSnappyShortLiteral);
      while (longs) {
        const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(longs));
        longs &= longs - 1ull;
        const int32_t r_op = __builtin_amdgcn_readlane(my_op, l), r_len = __builtin_amdgcn_readlane(my_lit, l), r_src = __builtin_amdgcn_readlane(my_src, l);
        for (int32_t i = lane; i < r_len; i += 64) dst[r_op + i] = in[r_src + i];
      }
    }
    ns += __builtin_popcountll(cmask);
    if (cmask) prev_end = __builtin_amdgcn_readlane(end, 63 - __builtin_clzll(cmask));
    op += __builtin_amdgcn_readlane(incl, 63);
    const int32_t ip = base + t;  // (t >= 64: the chain left the window — behind a long literal by more than one)
    base = ip & ~63;
    t0 = ip & 63;
  }
  if (ok && op != want) ok = false;  // short of the preamble
  if (lane != 0) return;
  w.n_seq[b] = ns;
  if (!ok) {
    w.state[b] = -1;
    atomicMin(&err->snappy_bad, (unsigned int)blk.section);
    if (blk.last) sections[blk.section].byte_len = 0;
    return;
  }
  w.state[b] = op;
  if (blk.last) sections[blk.section].byte_len = (int64_t)blk.index * 16 + op;
  if (ns > 0) {  // the exec pass's LDS class, by what the image holds: ingest_lz4.hip's kLz4ClassCap = 8, 16, 24, 32, 48, 64 KiB
    static_assert(kLz4Classes == 6, "the class bounds below are the exec pass's six");
    const int32_t cls = (op > 8192) + (op > 16384) + (op > 24576) + (op > 32768) + (op > 49152);
    w.cls_list[(int64_t)cls * n_blocks + atomicAdd(&w.cls_count[cls], 1)] = b;
  }
}

}  // namespace

Lz4Route snappy_plan_section(Lz4Plan& plan, const uint8_t* sec, int64_t len, int64_t src_off, int32_t section, int64_t* area_off, std::vector<uint8_t>& host_out,
                             const char** why) {
  namespace sn = surge::snappy;
  std::vector<Lz4Block>& blocks = plan.blocks;
  const size_t first_block = blocks.size();
  const int64_t seq_mark = plan.n_seq;
  bool device_ok = true;
  int64_t total = 0;
  const sn::Status walked = sn::walk_chunks(sec, len, [&](int64_t at, int64_t clen, uint32_t want) {
    if ((int64_t)want > clen * 32) return sn::SN_OUTPUT_SHORT;  // (never reached by that few bytes: a damaged preamble must not size a buffer)
    // on the device: at most 64 KiB of output, a stream the parse kernel's LDS holds, and a destination on the 16-byte grid —
    // every chunk in front of this one a multiple of 16 long
    if (want > (uint32_t)kSnappyChunkMax || clen > (int64_t)kSnappyStageMax || (total & 15)) device_ok = false;
    if (device_ok) {
      Lz4Block b;
      b.src_off = src_off + at;
      b.dst_off = plan.area + total;
      b.src_len = (int32_t)clen;
      b.section = section;
      b.last = 0;
      b.index = (int32_t)(total >> 4);
      b.seq_off = plan.n_seq;
      plan.n_seq += clen / 2 + 2;  // a copy takes at least 2 bytes of the stream
      blocks.push_back(b);
    }
    total += (int64_t)want;
    return total > (1ll << 31) ? sn::SN_TOO_LARGE : sn::SN_OK;
  });
  if (walked == sn::SN_OK && device_ok && blocks.size() > first_block) {
    blocks.back().last = 1;
    *area_off = plan.area;
    plan.area += (total + 15) & ~15ll;  // (the exec pass loads a chunk's image in 16-byte pieces: up to 15 bytes behind the last chunk's end)
    return LZ4_ON_DEVICE;
  }
  blocks.resize(first_block);
  plan.n_seq = seq_mark;
  sn::Status st = walked;
  if (st == sn::SN_OK) {
    const size_t ex = host_out.size();
    host_out.resize(ex + (size_t)total);
    int64_t got = 0;
    st = sn::frame_decompress(sec, len, host_out.data() + ex, total, &got);
    if (st == sn::SN_OK) return LZ4_ON_HOST;
    host_out.resize(ex);
  }
  *why = sn::status_name(st);
  return st == sn::SN_TOO_LARGE ? LZ4_TOO_LARGE : LZ4_BAD_FRAME;
}

hipError_t launch_snappy(const Lz4Plan& plan, const uint8_t* bytes, uint8_t* area, const Lz4Block* d_blocks, Lz4Work w, Section* sections, ErrorCell* err,
                         hipStream_t st) {
  const int64_t nb = (int64_t)plan.blocks.size();
  if (nb == 0) return hipSuccess;
  w.cls_list = w.cls_count + (kLz4Classes + 1);
  const hipError_t e = hipMemsetAsync(w.cls_count, 0, (kLz4Classes + 1) * 4, st);
  if (e != hipSuccess) return e;
  for (int c = 0; c < kSnappyParseClasses; ++c)
    hipLaunchKernelGGL(snappy_parse_kernel, dim3((unsigned)nb), dim3(64), (size_t)kSnappyParseCap[c], st, bytes, area, d_blocks, (int32_t)nb, w, sections, err,
                       c == 0 ? -1 : kSnappyParseCap[c - 1], kSnappyParseCap[c]);
  // (a chunk that does not decode zeroes its section when it is the last and raises the error cell: the push fails in stage 2's
  // first synchronisation, before anything is committed)
  return launch_lz4_exec(bytes, area, d_blocks, nb, w, st);
}

}  // namespace ingest
}  // namespace surge
