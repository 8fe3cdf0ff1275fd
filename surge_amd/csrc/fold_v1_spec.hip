// fold_v1_spec.hip — the v1 fold kernels compiled for one op table (hiprtc; host code only, no kernel is defined here).
//
// What fold_slots.hip does for ABI v2, for the op table of ABI v1: the kernels' own device source (fold_flat_device.h,
// fold_lane_device.h), compiled once per distinct op table and process with the table's words as compile-time masks
// (fold_device.h, SURGE_V1_SPEC).  The flat kernel is the one of the v1 folds that is bound by its instruction stream (lane
// transformers: ~97 VALU instructions per event against 55 in the lane-per-aggregate kernels); the others run at the
// transport's pace.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "replay_internal.h"

namespace surge {
namespace {

struct V1Masks {
  uint32_t word[kTableWords];  // [k] bit e: word k of entry e is non-zero (k < 15)
  uint32_t throws, deletes;    // TW_FLAGS bit 0 / bit 16 per entry
};

// false: a word holds something a bit per entry cannot express (not an op table fill_params writes)
bool v1_masks(const uint32_t (*table)[kTableWords], V1Masks* m) {
  std::memset(m, 0, sizeof(*m));
  for (int e = 0; e < kTableEntries; ++e) {
    for (int k = 0; k < TW_FLAGS; ++k) {
      const uint32_t w = table[e][k];
      if (w != 0u && w != (k == TW_EVC ? 1u : ~0u)) return false;
      if (w) m->word[k] |= 1u << e;
    }
    const uint32_t f = table[e][TW_FLAGS];
    if (f & ~0x10001u) return false;
    if (f & 1u) m->throws |= 1u << e;
    if (f & 0x10000u) m->deletes |= 1u << e;
  }
  return true;
}

}  // namespace

// The program handed to hiprtc for one op table: the masks, then either the flat kernel (V1_FLAT: fold_flat_device.h — K3
// appends, AUTO on logs of few long rows) or the lane-per-row kernels (V1_LANES: fold_lane_device.h — SORTED, CHUNKED, ROWS).
// Two programs, not one: a handle that only ever appends micro-batches never pays for the lane kernels' compile and the
// other way round; each is cached on disk by its text (rtc.cpp).
std::string v1_spec_source(const uint32_t (*table)[kTableWords], int kind) {
  V1Masks m;
  if (!v1_masks(table, &m)) return std::string();
  std::string s = "#define SURGE_V1_SPEC 1\n#define SURGE_V1_MASK(k) (";
  char b[64];
  for (int k = 0; k < TW_FLAGS; ++k) {
    std::snprintf(b, sizeof b, "(k) == %d ? 0x%xu : ", k, m.word[k]);
    s += b;
  }
  s += "0u)\n";
  std::snprintf(b, sizeof b, "#define SURGE_V1_THROWS 0x%xu\n", m.throws);
  s += b;
  std::snprintf(b, sizeof b, "#define SURGE_V1_DELETES 0x%xu\n", m.deletes);
  s += b;
#ifdef SURGE_EXPERIMENTS  // experiment builds of the library only (scripts/build_experiments_lib.py): extra #defines for the program, "A=1;B=2"
  if (const char* extra = std::getenv("SURGE_REPLAY_RTC_EXTRA")) {
    std::string e = extra;
    size_t pos = 0;
    while (pos < e.size()) {
      size_t semi = e.find(';', pos);
      if (semi == std::string::npos) semi = e.size();
      std::string d = e.substr(pos, semi - pos);
      const size_t eq = d.find('=');
      if (!d.empty()) s += "#define " + (eq == std::string::npos ? d : d.substr(0, eq) + " " + d.substr(eq + 1)) + "\n";
      pos = semi + 1;
    }
  }
#endif
  if (kind == V1_FLAT) {
    s += R"SRC(
#include "fold_flat_device.h"
using namespace surge;
extern "C" __global__ void __launch_bounds__(64) surge_v1_flat8(const FoldParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fold_flat_body<MODE_FLAT, 8>(p, smem);
}
extern "C" __global__ void __launch_bounds__(64) surge_v1_flat16(const FoldParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fold_flat_body<MODE_FLAT, 16>(p, smem);
}
)SRC";
  } else {
    // (register budgets as in fold_chunked.hip: two waves per SIMD with 16 KiB tiles, three with 8 KiB tiles)
    s += R"SRC(
#include "fold_lane_device.h"
using namespace surge;
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) surge_v1_sorted8(const FoldParams p) {
  ChunkTable t;
  t.v_start = nullptr; t.v_len = nullptr; t.v_info = nullptr; t.v_dest = nullptr; t.n_vrows = 0; t.side = nullptr;
  chunk_walk<8, true, true>(p, t);
}
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) surge_v1_sorted16(const FoldParams p) {
  ChunkTable t;
  t.v_start = nullptr; t.v_len = nullptr; t.v_info = nullptr; t.v_dest = nullptr; t.n_vrows = 0; t.side = nullptr;
  chunk_walk<16, true, true>(p, t);
}
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1))) surge_v1_sorted32(const FoldParams p) {
  ChunkTable t;
  t.v_start = nullptr; t.v_len = nullptr; t.v_info = nullptr; t.v_dest = nullptr; t.n_vrows = 0; t.side = nullptr;
  chunk_walk<32, true, true>(p, t);
}
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) surge_v1_chunked8(const ChunkArgs a) {
  chunk_walk<8, false, true>(a.p, a.t);
}
extern "C" __global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) surge_v1_chunked16(const ChunkArgs a) {
  chunk_walk<16, false, true>(a.p, a.t);
}
extern "C" __global__ void __launch_bounds__(64) surge_v1_rows8(const FoldParams p) {
  __shared__ __attribute__((aligned(16))) char lds_ev[Geo<8>::kTileBytes];
  fold_rows_body<8, true>(p, lds_ev, nullptr);
}
extern "C" __global__ void __launch_bounds__(64) surge_v1_rows16(const FoldParams p) {
  __shared__ __attribute__((aligned(16))) char lds_ev[Geo<16>::kTileBytes];
  fold_rows_body<16, true>(p, lds_ev, nullptr);
}
)SRC";
  }
  return s;
}

bool v1_kernels_acquire(const uint32_t (*table)[kTableWords], int device, int kind, V1Kernels* out, std::string* why) {
  if (rtc_disabled(why)) return false;  // (asked first: with the knob at 0 that is the reason a handle reports, whatever the lane knob says)
  if (kind == V1_LANES) {
    // Opt-in (SURGE_REPLAY_RTC_LANES=1).  Measured in round 6 on the 10 M-aggregate log, one box, A/B/A
    // (profiles/r06_lane_spec_*.jsonl): SORTED takes 12.2 ms whatever its walk costs — compiled for the built-in schema (53 VALU
    // per event), for the Counter fixture's own schema (20), or with the arithmetic REMOVED (an experiment build that only moves
    // the events): 12.19 / 12.22 / 12.20 ms, at 8- and 16-event lanes, from six resident waves per CU up.  The kernel runs at
    // the pace of its transport — 64 row pieces per load instruction, gathered from anywhere in the log — not of its
    // instruction stream; compiling the walk buys nothing there (CHUNKED on one GPU's C4 shard: -1 %; ROWS on C2: +1.5 %).
    // So the default stays the ahead-of-time kernels; the compiled ones are kept, fuzzed against the oracle, for hosts whose
    // schemas or shapes differ.  (Their first version was 13 - 29 % SLOWER: hiprtc's compiler puts an s_waitcnt vmcnt(0) in front
    // of every LDS read that follows an LDS-DMA load, which serialised the sixteen loads of a tile — fold_lane_device.h, issue().)
    const char* v = std::getenv("SURGE_REPLAY_RTC_LANES");
    if (!v || std::atoi(v) == 0) {
      *why = "off (SURGE_REPLAY_RTC_LANES=1 compiles them)";
      return false;
    }
  }
  V1Masks m;
  if (!v1_masks(table, &m)) {
    *why = "the op table holds words the specialised build cannot express";
    return false;
  }
  std::string key = std::string(kind == V1_FLAT ? "v1flat:" : "v1lanes:") + std::string((const char*)&m, sizeof(m));
#ifdef SURGE_EXPERIMENTS
  if (const char* extra = std::getenv("SURGE_REPLAY_RTC_EXTRA")) key += std::string("+") + extra;
#endif
  const auto source = [&] { return v1_spec_source(table, kind); };
  if (kind == V1_FLAT) {
    const RtcModule* mod = rtc_module_acquire(key, device, source, {"surge_v1_flat8", "surge_v1_flat16"}, why);
    if (!mod) return false;
    out->flat8 = mod->fn[0]; out->flat16 = mod->fn[1];
    out->compile_ms = mod->compile_ms;
    return true;
  }
  const RtcModule* mod = rtc_module_acquire(key, device, source, {"surge_v1_sorted8", "surge_v1_sorted16", "surge_v1_sorted32", "surge_v1_chunked8",
                                                                  "surge_v1_chunked16", "surge_v1_rows8", "surge_v1_rows16"}, why);
  if (!mod) return false;
  out->sorted8 = mod->fn[0]; out->sorted16 = mod->fn[1]; out->sorted32 = mod->fn[2]; out->chunked8 = mod->fn[3];
  out->chunked16 = mod->fn[4]; out->rows8 = mod->fn[5]; out->rows16 = mod->fn[6];
  out->compile_ms = mod->compile_ms;
  return true;
}

}  // namespace surge
