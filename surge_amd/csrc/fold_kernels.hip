// fold_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the aggregate-replay hot path.
//
// What is computed (reference semantics):
//   state[a] = events[seg_off[a] .. seg_off[a+1]).foldLeft(init[a])(handleEvent)
//   — modules/command-engine/scaladsl/src/main/scala/surge/scaladsl/command/CommandModels.scala:26
// with handleEvent restated per event type by a 32-bit descriptor (include/surge_replay.h).
//
// How (MI355X-first; there is no reference counterpart — the reference folds one event per
// actor message on the JVM):
//   * The event log is streamed exactly once, 16 B/lane, perfectly coalesced, by direct
//     global->LDS loads (global_load_lds_dwordx4).  One wave owns one 16 KiB tile at a time
//     (64 lanes x 16 consecutive events); the source lane permutation rotates each lane's
//     16 events inside its own 256 B LDS row so that the later ds_read_b128 of
//     "event j of lane l" is bank-conflict free.
//   * foldLeft is sequential, the GPU is not: each lane folds its 16 consecutive events into a
//     *state transformer* (per field either "relative to the incoming state": a delta for
//     count/sum64/event_count, a clamp for min/max, unchanged for version/balance — or "absolute"),
//     and transformers compose associatively, so a wave-level segmented scan (segment heads =
//     aggregate boundaries) yields every aggregate's final state in strict event order.  Integer
//     adds wrap mod 2^32 / 2^64 exactly like JVM Int/Long, min/max/set are exact, f64 payloads are
//     only moved — the result is bit-identical to the sequential fold under any association.
//   * The only thing a transformer cannot be relative to is PRESENCE (Some/None decides whether a
//     REQUIRE-class event applies and whether MATERIALIZE resets to defaults).  So presence (and the
//     sticky "an event threw" flag) is resolved first: a cheap pre-pass tracks three booleans per
//     lane, four wave ballots turn them into each lane's incoming (present, poisoned) with a couple
//     of bit scans, and the main walk then runs ONE evaluation path per lane with mask arithmetic
//     from a pre-expanded per-type op table (no per-event decode, no divergent branches).
//   * A wave task is a contiguous range of WHOLE segments (~256 KiB of events) chosen by a tiny
//     plan kernel from the CSR offsets, so waves never exchange carries through memory: the
//     running state of a segment that spans tiles is carried in scalar registers.
//   * No MFMA: this is an HBM-bound fold (16 B in per event, 64 B out per aggregate).
#include <cstdlib>
#include <cstring>

#include "fold_flat_device.h"
#include "fold_lane_device.h"

namespace surge {
namespace {

template <int MODE, int LE>
__global__ void __launch_bounds__(kWave) fold_kernel(const FoldParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fold_flat_body<MODE, LE>(p, smem);
}

// ---- K1 "rows": uniform fan-in, one lane per aggregate --------------------------------------------
// When every aggregate has the same number of events L (L % 16 == 0) a wave takes 64 consecutive
// aggregates and walks them in lockstep: tile c holds events [LE c, LE c + LE) of each of its 64 rows
// (64 pieces of LE*16 bytes at a row stride of 16 L bytes; the bare load pattern streams 6.1-6.8 TB/s on MI355X, close to
// the linear stream).  Lane l then owns row l outright, so its running state is CONCRETE from the first
// event on: no presence pre-pass, no transformer scan, no cross-lane traffic at all — the walk is the
// same mask arithmetic as the flat kernel and the 64 B results leave as one contiguous 4 KiB store.
template <int LE, bool CONC>
__global__ void __launch_bounds__(kWave) fold_rows_kernel(const FoldParams p) {
  __shared__ __attribute__((aligned(16))) char lds_ev[Geo<LE>::kTileBytes];
  __shared__ __attribute__((aligned(16))) uint32_t lds_tab[kTableLdsDwords];
  fold_rows_body<LE, CONC>(p, lds_ev, lds_tab);
}

// ---- K2 "sorted rows": arbitrary CSR, one lane per aggregate ----------------------------------------
// Segments are counting-sorted by length at load time (perm, longest first).  Persistent waves pull
// groups of 64 consecutive perm entries from an atomic counter; inside a group the lengths are (almost)
// equal, so the 64 lanes walk their own segments in lockstep exactly like the uniform rows kernel:
// concrete running state, no presence pre-pass, no scan.  A lane whose segment ends early pads with the
// null event.  Row pieces are LE*16 bytes at arbitrary 16 B-aligned addresses.

template <int LE>
__global__ void __launch_bounds__(kWave) fold_sorted_kernel(const FoldParams p) {
  using G = Geo<LE>;
  // one dynamic LDS buffer (separate objects as in fold_rows_kernel made no measurable difference here)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lds_ev = smem;
  int64_t* lds_rs = (int64_t*)(smem + G::kTileBytes);              // 64 row starts (aux area) ...
  uint32_t* lds_len = (uint32_t*)(smem + G::kTileBytes + kWave * 8);  // ... and 64 row lengths
  uint32_t* lds_tab = (uint32_t*)(smem + G::kTileBytes + G::kAuxSorted);
  const int lane = threadIdx.x;
  load_table<LE>(p, lds_tab, lane);
  const uint32_t ev_row = G::ev_row(lane);
  const int64_t n_groups = (p.n_seg + kWave - 1) / kWave;
  const int64_t* perm = p.plan;

  auto grab = [&]() -> int64_t {
    unsigned long long g = 0;
    if (lane == 0) g = atomicAdd(p.counter, 1ull);
    return (int64_t)(((uint64_t)rl((uint32_t)(g >> 32), 0) << 32) | rl((uint32_t)g, 0));
  };
  // A row is tiled from the 128 B line that contains its first event: `start` is rounded down to a multiple
  // of 8 events and the `pad` events in front of the segment (they belong to its predecessor) are treated as
  // null events.  Every LE*16-byte piece is then line-aligned; without this each 512 B piece touched five
  // lines instead of four (FETCH_SIZE was 22 % above the algorithmic bytes).
  struct Meta { int64_t s, start; uint32_t len, pad; };
  auto load_meta = [&](int64_t g) -> Meta {
    Meta m; m.s = -1; m.start = 0; m.len = 0u; m.pad = 0u;
    const int64_t idx = g * kWave + lane;
    if (g < n_groups && idx < p.n_seg) {
      m.s = perm[idx];
      const int64_t st = p.seg_off[m.s];
      m.pad = (uint32_t)(st & 7);
      m.start = st - m.pad;
      m.len = (uint32_t)(p.seg_off[m.s + 1] - st) + m.pad;
    }
    return m;
  };

  int64_t g = grab();
  Meta cur = load_meta(g);
  while (g < n_groups) {
    const int64_t g_next = grab();
    const Meta nxt = load_meta(g_next);  // in flight while this group is walked

    uint32_t maxlen = cur.len, minlen = cur.s >= 0 ? cur.len : 0xffffffffu;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      maxlen = max(maxlen, (uint32_t)__shfl_xor((int)maxlen, d, 64));
      minlen = min(minlen, (uint32_t)__shfl_xor((int)minlen, d, 64));
    }
    const int n_tiles = (int)((maxlen + LE - 1) / LE);

    // the rows each load instruction serves (row RPL*q + lane/LE): starts and lengths live in a small LDS
    // table rather than in 3 registers per load instruction — the register budget buys resident waves
    lds_rs[lane] = cur.start;
    lds_len[lane] = cur.len;
    auto issue = [&](int c) {
      if ((uint32_t)(c + 1) * LE <= minlen) {
#pragma unroll
        for (int q = 0; q < G::kLoads; ++q) {
          const int64_t e = lds_rs[G::kRowsPerLoad * q + lane / LE] + (int64_t)c * LE + G::load_j(lane, q % G::kClasses);
          __builtin_amdgcn_global_load_lds((gptr_t)(p.events + e), (lptr_t)(lds_ev + q * 1024), 16, 0, kLoadAux);
        }
      } else {  // some row ends inside this tile: never read past a row's own events
#pragma unroll
        for (int q = 0; q < G::kLoads; ++q) {
          const int r = G::kRowsPerLoad * q + lane / LE;
          const uint32_t rlen = lds_len[r];
          uint32_t j = (uint32_t)c * LE + G::load_j(lane, q % G::kClasses);
          const uint32_t lastj = rlen ? rlen - 1u : 0u;
          j = j < lastj ? j : lastj;
          __builtin_amdgcn_global_load_lds((gptr_t)(p.events + (lds_rs[r] + j)), (lptr_t)(lds_ev + q * 1024), 16, 0, kLoadAux);
        }
      }
    };

    const int64_t oi = cur.s >= 0 ? (p.out_map ? p.out_map[cur.s] : cur.s) : -1;
    Acc a = (p.init && oi >= 0) ? load_state(p.init, oi) : acc_none();
    uint32_t frozenM = (uint32_t)__builtin_amdgcn_sbfe((int32_t)a.fl, 1, 1);
    uint32_t corr = 0u;
    issue(0);
    for (int c = 0; c < n_tiles; ++c) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      uint4 ev[LE];
#pragma unroll
      for (int j = 0; j < LE; ++j) ev[j] = *(const uint4*)(lds_ev + (ev_row ^ (uint32_t)(j * 16)));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (c + 1 < n_tiles) issue(c + 1);

      uint32_t tyc[LE];
      if (c > 0 && (uint32_t)(c + 1) * LE <= minlen) {
#pragma unroll
        for (int j = 0; j < LE; ++j) tyc[j] = type_off(ev[j].x);
      } else {
        const int32_t rem = (int32_t)cur.len - c * LE;         // my remaining events (may be <= 0)
        const int32_t skip = c == 0 ? (int32_t)cur.pad : 0;   // events in front of my segment
#pragma unroll
        for (int j = 0; j < LE; ++j)
          tyc[j] = (j >= skip && j < rem) ? type_off(ev[j].x) : kNullEntryOffBytes;
      }
      walk_events<LE, false>(a, frozenM, corr, ev, tyc, 0u, lds_tab, p, [](int) {});
    }
    a.sum = (int64_t)((uint64_t)a.sum + corr);
    if (oi >= 0) store_state(p.out, oi, a);

    g = g_next;
    cur = nxt;
  }
  dispenser_leave(p.counter, lane);
}

// ---- K1s "short rows": any CSR of many short aggregates, one lane per aggregate, no LDS transport, no index ---------------
// Rows r .. r + 63 of a wave are consecutive in the log, so what the wave reads is one contiguous stretch of it (every cache
// line it touches is used whole, by neighbouring lanes); every lane loads its own events — four 16-byte loads in flight — and
// walks a concrete state like the rows kernels do.  A wave takes as many steps as its longest row needs: the kernel is for logs
// whose rows are all short (engine.hip: longest <= 64 events, mean < 16), where the tile kernels' 16-event lanes would walk
// mostly padding and the flat kernel pays a presence pass, a scan and a state store per segment HEAD.  Empty rows are rows
// like any other (their state is the prior one, or None): no compaction, no fill pass.
__global__ void __launch_bounds__(256) fold_short_kernel(const FoldParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t lds_tab[kTableLdsDwords];
  {
    const uint32_t* src = &p.table[0][0];
    for (int i = threadIdx.x; i < kTableEntries * kTableWords; i += 256)
      lds_tab[(i / kTableWords == kTableEntries - 1 ? kNullEntryOff : (i / kTableWords) * kTableStride) + (i % kTableWords)] = src[i];
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool mine = r < p.n_seg;
  const int64_t s0 = mine ? p.seg_off[r] : 0, s1 = mine ? p.seg_off[r + 1] : 0;
  Acc a = (mine && p.init) ? load_state(p.init, r) : acc_none();
  uint32_t frozenM = (uint32_t)__builtin_amdgcn_sbfe((int32_t)a.fl, 1, 1), presentM = (uint32_t)__builtin_amdgcn_sbfe((int32_t)a.fl, 0, 1), corr = 0u;
  begin_concrete(a);
  const int64_t last = p.n_events > 0 ? p.n_events - 1 : 0;
  for (int64_t j = s0; __builtin_amdgcn_ballot_w64(j < s1) != 0ull; j += 4) {  // (wave-uniform trip count: the longest row of the wave)
    uint4 ev[4];
    uint32_t tyc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t at = j + k < s1 ? j + k : (j + k <= last ? j + k : last);  // (a load past my row still hits the log: its event is replaced by the null event)
      typedef unsigned int v4u __attribute__((ext_vector_type(4)));
      const v4u w = __builtin_nontemporal_load((const v4u*)&p.events[at]);
      ev[k] = make_uint4(w.x, w.y, w.z, w.w);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tyc[k] = j + k < s1 ? type_off(ev[k].x) : kNullEntryOffBytes;
    // (rows of one or two events are the rule here: a step that no lane of the wave has an event for is not walked)
    if (__builtin_amdgcn_ballot_w64(j + 2 < s1) != 0ull) {
      walk_events_concrete<4>(a, presentM, frozenM, corr, ev, tyc, lds_tab, p);
    } else if (__builtin_amdgcn_ballot_w64(j + 1 < s1) != 0ull) {
      walk_events_concrete<2>(a, presentM, frozenM, corr, ev, tyc, lds_tab, p);
    } else {
      walk_events_concrete<1>(a, presentM, frozenM, corr, ev, tyc, lds_tab, p);
    }
  }
  finish_concrete(a, presentM, frozenM, corr, p);
  if (mine) store_state(p.out, r, a);
}

}  // namespace

bool concrete_walk() {
  static const bool v = [] { const char* e = std::getenv("SURGE_REPLAY_WALK"); return !(e && std::strcmp(e, "transformer") == 0); }();
  return v;
}

hipError_t launch_fold_fixed(const FoldParams& p, int64_t n_tasks, int lane_events, hipStream_t stream) {
  if (n_tasks <= 0) return hipSuccess;
  if (lane_events == 8)
    hipLaunchKernelGGL((fold_kernel<MODE_FIXED, 8>), dim3((unsigned)n_tasks), dim3(kWave), Geo<8>::lds_bytes(Geo<8>::kAuxFlat), stream, p);
  else
    hipLaunchKernelGGL((fold_kernel<MODE_FIXED, 16>), dim3((unsigned)n_tasks), dim3(kWave), Geo<16>::lds_bytes(Geo<16>::kAuxFlat), stream, p);
  return hipGetLastError();
}

hipError_t launch_fold_flat(const FoldParams& p, const V1Kernels* spec, int64_t n_tasks, int lane_events, hipStream_t stream) {
  if (n_tasks <= 0) return hipSuccess;
  if (spec) {  // no op table in LDS: the tile and the head bitmask only
    const unsigned lds = lane_events == 8 ? Geo<8>::kTileBytes + Geo<8>::kAuxFlat : Geo<16>::kTileBytes + Geo<16>::kAuxFlat;
    return launch_module_kernel(lane_events == 8 ? spec->flat8 : spec->flat16, n_tasks, lds, stream, &p, sizeof(p));
  }
  if (lane_events == 8)
    hipLaunchKernelGGL((fold_kernel<MODE_FLAT, 8>), dim3((unsigned)n_tasks), dim3(kWave), Geo<8>::lds_bytes(Geo<8>::kAuxFlat), stream, p);
  else
    hipLaunchKernelGGL((fold_kernel<MODE_FLAT, 16>), dim3((unsigned)n_tasks), dim3(kWave), Geo<16>::lds_bytes(Geo<16>::kAuxFlat), stream, p);
  return hipGetLastError();
}

hipError_t launch_fold_rows(const FoldParams& p, const V1Kernels* spec, int64_t n_tasks, int lane_events, hipStream_t stream) {
  if (n_tasks <= 0) return hipSuccess;
  if (spec && lane_events != 32) return launch_module_kernel(lane_events == 8 ? spec->rows8 : spec->rows16, n_tasks, 0, stream, &p, sizeof(p));
  // LDS is static in the kernel
  if (lane_events == 32) {
    hipLaunchKernelGGL((fold_rows_kernel<32, false>), dim3((unsigned)n_tasks), dim3(kWave), 0, stream, p);
  } else {
    for_lane_walk(lane_events, [&](auto w) {
      hipLaunchKernelGGL((fold_rows_kernel<decltype(w)::LE, decltype(w)::CONC>), dim3((unsigned)n_tasks), dim3(kWave), 0, stream, p);
    });
  }
  return hipGetLastError();
}

hipError_t launch_fold_short(const FoldParams& p, hipStream_t stream) {
  if (p.n_seg <= 0) return hipSuccess;
  hipLaunchKernelGGL(fold_short_kernel, dim3((unsigned)((p.n_seg + 255) / 256)), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_fold_sorted(const FoldParams& p, int64_t n_waves, int lane_events, hipStream_t stream) {
  if (n_waves <= 0) return hipSuccess;
  if (lane_events == 8)
    hipLaunchKernelGGL((fold_sorted_kernel<8>), dim3((unsigned)n_waves), dim3(kWave), Geo<8>::lds_bytes(Geo<8>::kAuxSorted), stream, p);
  else if (lane_events == 32)
    hipLaunchKernelGGL((fold_sorted_kernel<32>), dim3((unsigned)n_waves), dim3(kWave), Geo<32>::lds_bytes(Geo<32>::kAuxSorted), stream, p);
  else
    hipLaunchKernelGGL((fold_sorted_kernel<16>), dim3((unsigned)n_waves), dim3(kWave), Geo<16>::lds_bytes(Geo<16>::kAuxSorted), stream, p);
  return hipGetLastError();
}

}  // namespace surge
