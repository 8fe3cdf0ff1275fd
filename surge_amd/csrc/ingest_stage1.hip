// ingest_stage1.hip — stage 1 of a push of the device decoder (ingest_decoder_internal.h): where the push's bytes go on the
// device, what its slot has to hold, the copies and the launches of the stage units ingest_crc / ingest_lz4 /
// ingest_records .hip — all on the slot's own stream.  Nothing here reads or writes the key table.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "ingest_decoder_internal.h"

using namespace surge::ingest;
using namespace surge::ingest::host;

namespace {

int32_t slot_scratch(surge_device_decoder* d, PushSlot& s, int64_t n_rec) {
  const size_t R = (size_t)n_rec;
  DCHK(d, s.meta.reserve(R * sizeof(RecMeta), false, s.stream));
  if (!d->states) DCHK(d, s.ev_tmp.reserve(R * 16, false, s.stream));
  if (!d->states) DCHK(d, s.f64_list.reserve(R * 4, false, s.stream));
  static const ErrorCell kZero{~0ull, 0u, 0u, ~0u, ~0u, 0u, ~0u};  // (the source of an asynchronous copy: it must outlive the call)
  DCHK(d, hipMemcpyAsync(s.d_err.p, &kZero, sizeof(kZero), hipMemcpyHostToDevice, s.stream));
  return OK;
}

int32_t slot_pinned(surge_device_decoder* d, PushSlot& s, size_t bytes) {
  if (bytes <= s.pinned_cap) return OK;
  if (s.pinned) (void)hipHostFree(s.pinned);
  s.pinned = nullptr;
  s.pinned_cap = 0;
  bytes += bytes / 4 + 65536;  // (room to spare: the next fetch's tables are a few per cent larger or smaller)
  DCHK(d, hipHostMalloc(&s.pinned, bytes, hipHostMallocDefault));
  s.pinned_cap = bytes;
  return OK;
}

// SURGE_DBG_DECODE=<lz4 mode><section mode> (two digits; timing experiments only — see Lz4Work::dbg / JsonCtx::dbg; a
// lz4 mode needs a section mode, since the sections' bytes are then not the topic's)
int32_t dbg_decode() {
#ifdef SURGE_EXPERIMENTS  // this hook makes the decoder deliver records that are NOT the topic's: experiment builds of the library only
  static const int32_t v = [] {
    const char* e = std::getenv("SURGE_DBG_DECODE");
    const int32_t x = e ? std::atoi(e) : 0;
    return (x >= 10 && x % 10 == 0) ? x + 1 : x;
  }();
  return v;
#else
  return 0;
#endif
}

// what the value decoder needs besides the value: the template on the device, the mode, and the envelope the decoder's
// template names (h_tmpl: validated at create)
JsonCtx json_ctx(const surge_device_decoder* d, int32_t dbg) {
  return JsonCtx{d->json ? (const EvjDevice*)d->d_tmpl.p : nullptr, (const surge::F64ParseTable*)d->d_ptab.p, dbg, (int16_t)(d->states ? 1 : 0),
                 d->json ? (int16_t)d->h_tmpl.envelope : (int16_t)0};
}

// SURGE_DBG_TIMING: the host time every step of stage 1 took, to stderr
struct Laps {
  const bool on = std::getenv("SURGE_DBG_TIMING") != nullptr;
  double mark = on ? now_us() : 0.0;
  static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void lap(const char* what) {
    const double t = on ? now_us() : 0.0;
    if (on) std::fprintf(stderr, "[surge dbg] stage1 %-14s %8.1f us\n", what, t - mark);
    mark = t;
  }
};

// Where a wire push's bytes go on the device: the span of each part's arena the push needs, one after the other (16-byte
// aligned), then the sections the host decompressed (`extra`), then — from area_base on — the LZ4 frames the device decompresses
// and, behind those (snappy_base), the snappy sections'.
struct WireLayout {
  struct Part {
    int64_t lo, len, dev;  // the span [lo, lo + len) of the caller's arena goes to `dev` of the slot's bytes
    bool in_place;         // ... straight out of the arena: it is page-locked (surge_ingest_use_pinned_arena)
  };
  std::vector<Part> parts;
  std::vector<uint8_t> extra;
  int64_t total_sections = 0, n_rec = 0, n_raw = 0;
  int32_t max_recs = 0;  // of one batch of this push (section_kernel's workgroup size)
  int64_t area_base() const { return (n_raw + (int64_t)extra.size() + 15) & ~15ll; }
};

struct SlotNeeds {  // what a slot's buffers have to hold for a push
  size_t bytes, sections, crc_spans, floors, pinned;
  int64_t n_rec;
  Lz4ScratchBytes lz4, snappy;
};

size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

// Section::byte_off while a push is planned: -1 - x = x bytes into the LZ4 area, kSnappyMark - x = x bytes into the snappy area
constexpr int64_t kSnappyMark = -(1ll << 62);

// step 1: the parts' spans and the push's section table (s.h_secs)
int32_t layout_sections(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const surge_batch_section* const* sections, const int64_t* n_sections, WireLayout& L) {
  try {
    s.h_secs.resize((size_t)L.total_sections);
    L.parts.resize((size_t)n_parts);
  } catch (const std::bad_alloc&) {
    return dfail(d, E_NOMEM, "out of host memory");
  }
  int64_t at = 0;
  for (int32_t p = 0; p < n_parts; ++p) {
    int64_t lo = INT64_MAX, hi = 0;
    for (int64_t i = 0; i < n_sections[p]; ++i) {
      const surge_batch_section& in = sections[p][i];
      if (in.byte_off < 0 || in.byte_len < 0 || in.n_records < 0) return dfail(d, E_INVALID, "negative section field");
      const int64_t crc_prefix = (in.codec & SURGE_SECTION_CRC_PENDING) ? 8 : (in.codec & SURGE_SECTION_CRC_WIRE) ? 44 : 0;
      if (crc_prefix && (in.byte_off < crc_prefix || in.byte_len >= (1ll << 31) - 64)) return dfail(d, E_INVALID, "a CRC-pending section without the bytes in front of it");
      lo = in.byte_off - crc_prefix < lo ? in.byte_off - crc_prefix : lo;
      hi = in.byte_off + in.byte_len > hi ? in.byte_off + in.byte_len : hi;
    }
    if (n_sections[p] == 0) lo = hi = 0;
    L.parts[(size_t)p] = WireLayout::Part{lo, hi - lo, L.n_raw, false};
    for (int64_t i = 0; i < n_sections[p]; ++i, ++at) {
      const surge_batch_section& in = sections[p][i];
      s.h_secs[(size_t)at] = Section{L.n_raw + (in.byte_off - lo), in.byte_len, in.base_offset, in.n_records, 0, L.n_rec};
      L.n_rec += in.n_records;
      L.max_recs = in.n_records > L.max_recs ? in.n_records : L.max_recs;
    }
    L.n_raw = (L.n_raw + (hi - lo) + 15) & ~15ll;
  }
  return OK;
}

// step 2: one walk over the sections' first bytes on the host — the CRC spans the device finishes (s.h_crc) and the LZ4
// frames' blocks (s.lz4: ingest_lz4.hip reads the frames) and the snappy sections' chunks (s.snappy: ingest_snappy.hip)
int32_t plan_frames(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                    const int64_t* n_sections, WireLayout& L) {
  try {
    s.lz4.clear();
    s.snappy.clear();
    s.snappy_host_sections = 0;
    s.h_crc.clear();
    int64_t at = 0;
    for (int32_t p = 0; p < n_parts; ++p) {
      for (int64_t i = 0; i < n_sections[p]; ++i, ++at) {
        const surge_batch_section& in = sections[p][i];
        // (the frame headers were written by the framing threads, on other cores: one cache miss per batch — 1.2 ms per
        // 7000-batch push — unless they are asked for ahead of time)
        // ... the lines this walk reads of a section: its first bytes (and, framed in place, the crc field 44 bytes in front of
        // them), and its last words (where lz4_plan_section's walk over a frame ends)
        if (i + 16 < n_sections[p]) {
          const surge_batch_section& nx = sections[p][i + 16];
          __builtin_prefetch(bytes[p] + nx.byte_off - ((nx.codec & SURGE_SECTION_CRC_WIRE) ? 44 : 0));
          __builtin_prefetch(bytes[p] + nx.byte_off + 16);
          if (nx.byte_len > 64) __builtin_prefetch(bytes[p] + nx.byte_off + nx.byte_len - 8);
        }
        Section& sec = s.h_secs[(size_t)at];
        if (in.codec & SURGE_SECTION_CRC_PENDING) {  // {crc, register after the header bytes}, written by the framer in front of the section
          uint32_t pre[2];
          std::memcpy(pre, bytes[p] + in.byte_off - 8, 8);
          s.h_crc.push_back(CrcSpan{sec.byte_off, (int32_t)in.byte_len, (int32_t)at, pre[0], pre[1]});
        } else if (in.codec & SURGE_SECTION_CRC_WIRE) {  // the batch as received: its crc field (big-endian), then the 40 header bytes it covers, then the section
          const uint8_t* c = bytes[p] + in.byte_off - 44;
          const uint32_t expect = ((uint32_t)c[0] << 24) | ((uint32_t)c[1] << 16) | ((uint32_t)c[2] << 8) | c[3];
          s.h_crc.push_back(CrcSpan{sec.byte_off - 40, (int32_t)in.byte_len + 40, (int32_t)at, expect, ~0u});
        }
        if (((in.codec & 0xff) != 3 && (in.codec & 0xff) != 2) || in.n_records == 0) continue;
        const size_t ex = L.extra.size();
        int64_t area_off = 0;
        if ((in.codec & 0xff) == 2) {
          const char* why = "";
          switch (snappy_plan_section(s.snappy, bytes[p] + in.byte_off, in.byte_len, sec.byte_off, (int32_t)at, &area_off, L.extra, &why)) {
            case LZ4_ON_DEVICE:  // (resolved below, behind the LZ4 frames' area: kSnappyMark tells the two apart)
              sec.byte_off = kSnappyMark - area_off;
              sec.byte_len = 0;
              break;
            case LZ4_ON_HOST:
              sec.byte_off = L.n_raw + (int64_t)ex;
              sec.byte_len = (int64_t)(L.extra.size() - ex);
              ++s.snappy_host_sections;
              break;
            case LZ4_TOO_LARGE:
            case LZ4_BAD_FRAME: return dfail(d, SURGE_E_CORRUPT, std::string(why) + " (the section at base offset " + std::to_string(in.base_offset) + ")");
          }
          continue;
        }
        switch (lz4_plan_section(s.lz4, bytes[p] + in.byte_off, in.byte_len, sec.byte_off, (int32_t)at, &area_off, L.extra)) {
          case LZ4_ON_DEVICE:  // byte_off: resolved below, once the raw spans' final size is known; byte_len: set by the kernel that decodes the frame's last block
            sec.byte_off = -1 - area_off;
            sec.byte_len = 0;
            break;
          case LZ4_ON_HOST:
            sec.byte_off = L.n_raw + (int64_t)ex;
            sec.byte_len = (int64_t)(L.extra.size() - ex);
            break;
          case LZ4_TOO_LARGE: return dfail(d, SURGE_E_CORRUPT, "LZ4 batch expands beyond 2 GiB");
          case LZ4_BAD_FRAME: return dfail(d, SURGE_E_CORRUPT, "bad LZ4 frame in the section at base offset " + std::to_string(in.base_offset));
        }
      }
    }
  } catch (const std::bad_alloc&) {
    return dfail(d, E_NOMEM, "out of host memory");
  }
  if (s.lz4.blocks.size() >= (1ull << 31)) return dfail(d, E_UNSUPPORTED, "more than 2^31 LZ4 blocks in one push: push fewer sections at a time");
  if (s.snappy.blocks.size() >= (1ull << 31)) return dfail(d, E_UNSUPPORTED, "more than 2^31 snappy chunks in one push: push fewer sections at a time");
  for (Section& sc : s.h_secs) {
    if (sc.byte_off <= kSnappyMark) sc.byte_off = L.area_base() + s.lz4.area + (kSnappyMark - sc.byte_off);
    else if (sc.byte_off < 0) sc.byte_off = L.area_base() + (-1 - sc.byte_off);
  }
  return OK;
}

// step 3: what the push needs of a slot.  A part goes straight out of the caller's arena when that is page-locked, else
// through the slot's own pinned staging (one extra host copy); the section, block and CRC tables travel through the staging
// too: a copy from pageable memory waits for the stream (1.4 ms of host time per push went there)
SlotNeeds slot_needs(const PushSlot& s, const uint8_t* const* bytes, WireLayout& L) {
  SlotNeeds n;
  n.bytes = (size_t)(L.area_base() + s.lz4.area + s.snappy.area) + 64;
  n.sections = sizeof(Section) * s.h_secs.size();
  n.crc_spans = sizeof(CrcSpan) * s.h_crc.size();
  n.n_rec = L.n_rec;
  n.lz4 = lz4_scratch_bytes(s.lz4);
  n.snappy = lz4_scratch_bytes(s.snappy);
  n.floors = 8 * s.h_floors.size();
  n.pinned = pad16(L.extra.size()) + n.sections + n.lz4.blocks + pad16(n.snappy.blocks) + pad16(n.crc_spans) + pad16(n.floors) + 64;
  for (size_t p = 0; p < L.parts.size(); ++p) {
    WireLayout::Part& part = L.parts[p];
    if (part.len == 0) continue;
    hipPointerAttribute_t attr;
    part.in_place = hipPointerGetAttributes(&attr, bytes[p] + part.lo) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // a pageable pointer makes hipPointerGetAttributes fail: not an error of this call
    if (!part.in_place) n.pinned += pad16((size_t)part.len);
  }
  return n;
}

int32_t size_slot(surge_device_decoder* d, PushSlot& t, const SlotNeeds& n) {
  const size_t per_event = d->states ? 0 : (size_t)n.n_rec;  // (a state decoder decodes no value)
  const std::pair<Buf*, size_t> device[] = {{&t.d_bytes, n.bytes}, {&t.d_sections, n.sections}, {&t.meta, (size_t)n.n_rec * sizeof(RecMeta)}, {&t.ev_tmp, per_event * 16},
                                            {&t.f64_list, per_event * 4}, {&t.crc_spans, n.crc_spans}, {&t.d_floors, n.floors}, {&t.lz4_blocks, n.lz4.blocks}, {&t.lz4_sizes, n.lz4.state},
                                            {&t.lz4_nseq, n.lz4.n_seq}, {&t.lz4_seq, n.lz4.seq}, {&t.lz4_cls, n.lz4.cls}, {&t.sn_blocks, n.snappy.blocks},
                                            {&t.sn_sizes, n.snappy.state}, {&t.sn_nseq, n.snappy.n_seq}, {&t.sn_seq, n.snappy.seq}, {&t.sn_cls, n.snappy.cls}};
  for (const auto& b : device) DCHK(d, b.first->reserve(b.second, false, t.stream));
  return slot_pinned(d, t, n.pinned);
}

// The FIRST wire push of a decoder sizes every slot like its own: the fetches of a recovery are alike, and a slot that sizes
// its buffers when its turn comes does so in the middle of the pipeline (an allocation per buffer, a hipFree — a device-wide
// wait — for every one that grows, and milliseconds to page-lock its staging).
void warm_idle_slots(surge_device_decoder* d, PushSlot& s, const SlotNeeds& n) {
  if (d->slots_sized) return;
  d->slots_sized = true;
  // (only while nothing else is in flight — the decoder's first push as a rule: no other slot is then being read by a push or by
  // the thread that finishes pushes; a slot whose last push was finished without a wait is left alone too)
  {
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->n_pending != 0) return;
  }
  for (PushSlot& t : d->slots)
    if (&t != &s && !t.busy && !t.released_valid && size_slot(d, t, n) != OK) (void)hipGetLastError();  // (best effort: a slot that could not be sized now reports it when its turn comes)
}

// step 4: everything the kernels read, to the device on the slot's stream
int32_t stage_and_copy(surge_device_decoder* d, PushSlot& s, const uint8_t* const* bytes, const WireLayout& L) {
  hipStream_t st = s.stream;
  size_t staged = 0;
  auto stage = [&](const void* src, size_t len) -> const uint8_t* {
    uint8_t* at = (uint8_t*)s.pinned + staged;
    std::memcpy(at, src, len);
    staged += pad16(len);
    return at;
  };
  for (size_t p = 0; p < L.parts.size(); ++p) {
    const WireLayout::Part& part = L.parts[p];
    if (part.len == 0) continue;
    const uint8_t* src = bytes[p] + part.lo;
    if (!part.in_place) src = stage(src, (size_t)part.len);
    DCHK(d, hipMemcpyAsync((uint8_t*)s.d_bytes.p + part.dev, src, (size_t)part.len, hipMemcpyHostToDevice, st));
  }
  if (!L.extra.empty()) DCHK(d, hipMemcpyAsync((uint8_t*)s.d_bytes.p + L.n_raw, stage(L.extra.data(), L.extra.size()), L.extra.size(), hipMemcpyHostToDevice, st));
  const size_t sec_bytes = sizeof(Section) * s.h_secs.size(), crc_bytes = sizeof(CrcSpan) * s.h_crc.size(), blk_bytes = sizeof(Lz4Block) * s.lz4.blocks.size();
  DCHK(d, hipMemcpyAsync(s.d_sections.p, stage(s.h_secs.data(), sec_bytes), sec_bytes, hipMemcpyHostToDevice, st));
  if (crc_bytes) DCHK(d, hipMemcpyAsync(s.crc_spans.p, stage(s.h_crc.data(), crc_bytes), crc_bytes, hipMemcpyHostToDevice, st));
  if (blk_bytes) DCHK(d, hipMemcpyAsync(s.lz4_blocks.p, stage(s.lz4.blocks.data(), blk_bytes), blk_bytes, hipMemcpyHostToDevice, st));
  const size_t sn_bytes = sizeof(Lz4Block) * s.snappy.blocks.size();
  if (sn_bytes) DCHK(d, hipMemcpyAsync(s.sn_blocks.p, stage(s.snappy.blocks.data(), sn_bytes), sn_bytes, hipMemcpyHostToDevice, st));
  const size_t floor_bytes = 8 * s.h_floors.size();
  if (floor_bytes) DCHK(d, hipMemcpyAsync(s.d_floors.p, stage(s.h_floors.data(), floor_bytes), floor_bytes, hipMemcpyHostToDevice, st));
  return OK;
}

// the sparse floors list as the record stage reads it (s.h_floors): one int64 per section of the push, INT64_MIN where there is
// none; empty for a push without floors.  `section` counts through the parts' sections in push order.
int32_t expand_floors(surge_device_decoder* d, PushSlot& s, int64_t total_sections, int64_t n_floors, const surge_section_floor* floors) {
  s.h_floors.clear();
  if (n_floors == 0) return OK;
  if (d->states) return dfail(d, SURGE_E_STATE, "a state decoder reads its topic from the beginning: floors belong to an events decoder");
  try {
    s.h_floors.assign((size_t)total_sections, INT64_MIN);
  } catch (const std::bad_alloc&) {
    return dfail(d, E_NOMEM, "out of host memory");
  }
  for (int64_t i = 0; i < n_floors; ++i) {
    if (floors[i].section < 0 || floors[i].section >= total_sections) return dfail(d, E_INVALID, "a floor names section " + std::to_string(floors[i].section) + ": the push has " + std::to_string(total_sections));
    int64_t& f = s.h_floors[(size_t)floors[i].section];
    f = floors[i].first_offset > f ? floors[i].first_offset : f;
  }
  return OK;
}

}  // namespace

// Stage 1 of a wire push: the parts' records sections to the device, LZ4 blocks decoded, every record chained, parsed and
// its value decoded — records below their section's floor passed over (n_floors > 0: the floored instantiations of the record stage).
int32_t surge::ingest::host::stage1_wire(surge_device_decoder* d, PushSlot& s, int32_t n_parts, const uint8_t* const* bytes, const surge_batch_section* const* sections,
                    const int64_t* n_sections, int64_t n_floors, const surge_section_floor* floors) {
  Laps laps;
  const uint64_t seed = d->seed.load();
  WireLayout L;
  for (int32_t p = 0; p < n_parts; ++p) {
    if (n_sections[p] < 0 || (n_sections[p] > 0 && (!bytes[p] || !sections[p]))) return dfail(d, E_INVALID, "bad argument");
    L.total_sections += n_sections[p];
  }
  s.n_rec = 0;
  s.wire = true;
  s.snappy.clear();  // (stage 2 counts what this push planned: nothing, should it end before plan_frames)
  s.snappy_host_sections = 0;
  if (L.total_sections >= (1ll << 31)) return dfail(d, E_UNSUPPORTED, "more than 2^31 batches in one push");
  int32_t rc = expand_floors(d, s, L.total_sections, n_floors, floors);
  if (rc != OK || L.total_sections == 0) return rc;
  rc = layout_sections(d, s, n_parts, sections, n_sections, L);
  if (rc != OK || L.n_rec == 0) return rc;
  if (L.n_rec >= (1ll << 32) - 1) return dfail(d, E_UNSUPPORTED, "more than 2^32 - 2 records in one push: push fewer sections at a time");
  rc = plan_frames(d, s, n_parts, bytes, sections, n_sections, L);
  if (rc != OK) return rc;
  laps.lap("walk sections");
  const SlotNeeds needs = slot_needs(s, bytes, L);
  warm_idle_slots(d, s, needs);
  rc = size_slot(d, s, needs);
  if (rc == OK) rc = slot_scratch(d, s, L.n_rec);
  if (rc == OK) laps.lap("reserve");
  if (rc == OK) rc = stage_and_copy(d, s, bytes, L);
  if (rc != OK) return rc;
  hipStream_t st = s.stream;
  const uint8_t* dby = (const uint8_t*)s.d_bytes.p;
  Section* dsec = (Section*)s.d_sections.p;
  ErrorCell* derr = (ErrorCell*)s.d_err.p;
  // the batches' CRC-32C, finished where their bytes now are (the host ran it over the 40 header bytes only)
  if (!s.h_crc.empty()) DCHK(d, launch_crc(dby, (const CrcSpan*)s.crc_spans.p, (int32_t)s.h_crc.size(), derr, st));
  laps.lap("copies");
  Lz4Work w{dbg_decode() / 10, (int32_t*)s.lz4_sizes.p, (int32_t*)s.lz4_nseq.p, (uint2*)s.lz4_seq.p, (int32_t*)s.lz4_cls.p, nullptr};
  DCHK(d, launch_lz4(s.lz4, dby, (uint8_t*)s.d_bytes.p + L.area_base(), (const Lz4Block*)s.lz4_blocks.p, w, dsec, derr, st));
  laps.lap("lz4 launches");
  Lz4Work ws{0, (int32_t*)s.sn_sizes.p, (int32_t*)s.sn_nseq.p, (uint2*)s.sn_seq.p, (int32_t*)s.sn_cls.p, nullptr};
  DCHK(d, launch_snappy(s.snappy, dby, (uint8_t*)s.d_bytes.p + L.area_base() + s.lz4.area, (const Lz4Block*)s.sn_blocks.p, ws, dsec, derr, st));
  laps.lap("snappy launches");
  const JsonCtx jc = json_ctx(d, dbg_decode() % 10);
  DCHK(d, launch_sections(dby, dsec, L.total_sections, L.max_recs, seed, jc, (RecMeta*)s.meta.p, (uint4*)s.ev_tmp.p, (uint32_t*)s.f64_list.p, derr,
                          s.h_floors.empty() ? nullptr : (const int64_t*)s.d_floors.p, st));
  laps.lap("section launches");
  s.n_rec = L.n_rec;
  s.seed = seed;
  return OK;
}

// Stage 1 of a push of records that are already framed
int32_t surge::ingest::host::stage1_records(surge_device_decoder* d, PushSlot& s, const uint8_t* keys, const int64_t* key_off, const uint8_t* values,
                                            const int64_t* value_off, const int64_t* offsets, int64_t n) {
  s.n_rec = 0;
  s.wire = false;
  const uint64_t seed = d->seed.load();
  if (n == 0) return OK;
  if (n >= (1ll << 32) - 1) return dfail(d, E_UNSUPPORTED, "more than 2^32 - 2 records in one push");
  const int64_t kb = key_off[n] - key_off[0], vb = value_off[n] - value_off[0];
  if (kb < 0 || vb < 0 || (kb > 0 && !keys) || (vb > 0 && !values)) return dfail(d, E_INVALID, "bad key / value spans");
  for (int64_t i = 0; i < n; ++i)  // (the kernels index the staged bytes with these: no launch on offsets that run backwards)
    if (key_off[i + 1] < key_off[i] || value_off[i + 1] < value_off[i]) return dfail(d, E_INVALID, "key_off / value_off must not decrease (record " + std::to_string(i) + ")");
  hipStream_t st = s.stream;
  const size_t n_bytes = (size_t)(kb + vb), off_bytes = (size_t)(n + 1) * 8;
  const size_t stage = n_bytes + 2 * off_bytes + (offsets ? (size_t)n * 8 : 0) + 64;
  DCHK(d, s.d_bytes.reserve(n_bytes + 16, false, st));
  DCHK(d, s.rec_a.reserve(off_bytes, false, st));  // the device copies of key_off / value_off / offsets
  DCHK(d, s.rec_b.reserve(off_bytes, false, st));
  DCHK(d, s.rec_c.reserve((size_t)n * 8 + 8, false, st));
  {
    int32_t rc = slot_scratch(d, s, n);
    if (rc == OK) rc = slot_pinned(d, s, stage);
    if (rc != OK) return rc;
  }
  // pinned staging: [keys][values][key_off (rebased)][value_off (rebased)][offsets]
  uint8_t* pin = (uint8_t*)s.pinned;
  if (kb) std::memcpy(pin, keys + key_off[0], (size_t)kb);
  if (vb) std::memcpy(pin + kb, values + value_off[0], (size_t)vb);
  int64_t* p_ko = (int64_t*)(pin + ((n_bytes + 7) & ~(size_t)7));
  int64_t* p_vo = p_ko + (n + 1);
  int64_t* p_of = p_vo + (n + 1);
  for (int64_t i = 0; i <= n; ++i) { p_ko[i] = key_off[i] - key_off[0]; p_vo[i] = value_off[i] - value_off[0]; }
  if (offsets) std::memcpy(p_of, offsets, (size_t)n * 8);
  if (n_bytes) DCHK(d, hipMemcpyAsync(s.d_bytes.p, pin, n_bytes, hipMemcpyHostToDevice, st));
  DCHK(d, hipMemcpyAsync(s.rec_a.p, p_ko, off_bytes, hipMemcpyHostToDevice, st));
  DCHK(d, hipMemcpyAsync(s.rec_b.p, p_vo, off_bytes, hipMemcpyHostToDevice, st));
  if (offsets) DCHK(d, hipMemcpyAsync(s.rec_c.p, p_of, (size_t)n * 8, hipMemcpyHostToDevice, st));
  DCHK(d, launch_records((const uint8_t*)s.d_bytes.p, (const int64_t*)s.rec_a.p, (const int64_t*)s.rec_b.p, offsets ? (const int64_t*)s.rec_c.p : nullptr, kb, n, seed,
                         json_ctx(d, 0), (RecMeta*)s.meta.p, (uint4*)s.ev_tmp.p, (uint32_t*)s.f64_list.p, (ErrorCell*)s.d_err.p, st));
  s.n_rec = n;
  s.seed = seed;
  return OK;
}
