// ingest_internal.h — what the units of the host framer share (ingest.cpp: the single-partition framer, surge_ingest_*;
// ingest_group.cpp: the partition group, surge_ingest_group_*): status codes, the batch-header reader, the arena, the framer's
// object and the few functions of the framer the group calls.  Host only and internal, like ingest_decoder_internal.h: not part
// of the C ABI (that is include/surge_ingest.h).  What runs once per batch or per record stays inline here or inside ingest.cpp;
// the group reaches a member's feed and drain through surge_ingest_feed / surge_ingest_drain_sections, the CRC-32C (crc32c.cpp)
// through surge_crc32c.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

#include "../../include/surge_ingest.h"

namespace surge {
namespace ingest {
namespace framer __attribute__((visibility("hidden"))) {

constexpr int32_t OK = 0, E_INVALID = -1, E_STATE = -2, E_NOMEM = -4, E_UNSUPPORTED = -5;  // (include/surge_replay.h's SURGE_E_*)

// surge_ingest_counters' eight slots, in the order include/surge_ingest.h gives them
enum Counter { C_BATCHES, C_RECORDS_DECODED, C_RECORDS_DELIVERED, C_RECORDS_ABORTED, C_CONTROL_BATCHES, C_FLUSH_SKIPPED, C_BYTES_DECOMPRESSED,
               C_OPEN_TRANSACTIONS, C_COUNT };
static_assert(C_COUNT == 8, "surge_ingest_counters hands out int64_t[8]");

struct Rec {
  int64_t offset, key_off, value_off, agg_idx;
  int32_t key_len, value_len;
};

struct Batch {
  int64_t producer_id = -1;
  int decided = 1;  // 0 pending (open transaction), 1 committed / non-transactional, 2 aborted
  std::vector<Rec> recs;
  size_t next = 0;  // first record not yet drained
  // FRAMES mode (device decode): the batch's records section, verbatim, inside the arena
  int64_t sect_off = -1, sect_len = 0, base_offset = 0;
  int32_t count = 0, sect_codec = 0;
  // SURGE_INGEST_DEVICE_CRC: bytes in front of the section that travel with it (sect_off points at them): 8 = {crc, register after
  // the header bytes} written by the framer; 44 = the batch's own crc field and the 40 header bytes it covers, as received
  // (in-place framing: the device runs the whole CRC)
  int32_t crc_prefix = 0;
  int64_t last_offset = 0;  // baseOffset + lastOffsetDelta (compaction leaves the header's as they were written)
};

// A record batch's header (message format v2: the 61 bytes in front of the records section).
struct BatchHeader {
  int64_t base_offset, producer_id;
  int32_t batch_len, count;  // batch_len: the bytes behind the length field (the batch spans 12 + batch_len)
  int32_t last_offset_delta;
  uint32_t crc;
  int16_t attrs;
  uint8_t magic;
  const uint8_t *crc_from, *recs;  // what the CRC-32C covers (attributes .. end of the batch); the records section
  int64_t crc_len, recs_len;
  int64_t size() const { return 12 + (int64_t)batch_len; }
  int codec() const { return attrs & 7; }
  bool transactional() const { return attrs & 0x10; }
  bool control() const { return attrs & 0x20; }
};

// What stands at data + pos: a whole batch; a cut one (fewer than 12 bytes, or fewer than its length says: wait for more); or
// a length below the v2 header's.  Every walk over a buffer's batches takes its stop rule from here.
enum class HeaderRead { WHOLE, CUT, SHORT };
constexpr int32_t kHeaderBehindLength = 49;  // partitionLeaderEpoch .. recordCount

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

// ... the length field alone (the first 12 bytes of the header are all it reads)
inline HeaderRead read_batch_length(const uint8_t* data, int64_t len, int64_t pos, int32_t* batch_len) {
  if (len - pos < 12) return HeaderRead::CUT;
  *batch_len = (int32_t)be32(data + pos + 8);
  if (*batch_len < kHeaderBehindLength) return HeaderRead::SHORT;
  return len - pos - 12 < *batch_len ? HeaderRead::CUT : HeaderRead::WHOLE;
}

// ... and the header (of a WHOLE batch every field lies inside it, whatever the magic byte says the layout is)
inline HeaderRead read_batch_header(const uint8_t* data, int64_t len, int64_t pos, BatchHeader* h) {
  const HeaderRead got = read_batch_length(data, len, pos, &h->batch_len);
  if (got != HeaderRead::WHOLE) return got;
  const uint8_t* p = data + pos;
  h->base_offset = (int64_t)be64(p);
  h->magic = p[16];  // behind partitionLeaderEpoch
  h->crc = be32(p + 17);
  h->crc_from = p + 21;
  h->crc_len = (int64_t)h->batch_len - 9;
  h->attrs = (int16_t)((p[21] << 8) | p[22]);
  h->last_offset_delta = (int32_t)be32(p + 23);
  h->producer_id = (int64_t)be64(p + 43);  // behind baseTimestamp, maxTimestamp
  h->count = (int32_t)be32(p + 57);        // behind producerEpoch, baseSequence
  h->recs = p + 61;
  h->recs_len = (int64_t)h->batch_len - kHeaderBehindLength;
  return got;
}

// The byte arena records / sections are copied into: a growable buffer whose memory comes from a pluggable allocator, so
// that a device decoder can have it PAGE-LOCKED (surge_ingest_set_allocator: its H2D copy then reads the arena in place
// instead of staging it through a pinned buffer of its own).
struct SliceOverflow : std::bad_alloc {};  // an external arena (a slice of a group's slab) is full

struct Arena {
  uint8_t* p = nullptr;
  size_t n = 0, cap = 0;
  void* (*alloc)(size_t) = nullptr;
  void (*release)(void*) = nullptr;
  bool external = false;  // a view into memory someone else owns (a slice of a surge_ingest_group's slab): never grown, never freed
  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() {
    if (p && !external) (release ? release : std::free)(p);
  }
  void view(uint8_t* at, size_t bytes) { external = true; p = at; cap = bytes; n = 0; }
  size_t size() const { return n; }
  const uint8_t* data() const { return p; }
  uint8_t* data() { return p; }
  void clear() { n = 0; }
  // Three ways to choose a capacity over one re-allocation step (surge_ingest_group_slab_bytes shows the capacities).
  void reserve(size_t want) {  // room for `want` bytes in one allocation, with half as much again to spare; the contents stay
    if (want <= cap) return;
    size_t c = cap ? cap : (size_t)1 << 16;
    while (c < want) c += c / 2 + 4096;
    regrow(c, n);
  }
  void reserve_exact(size_t want) {  // exactly `want` bytes and EMPTY when it has to grow (a group's slabs: page-locked memory is not cheap)
    if (want <= cap) return;
    regrow(want, 0);
  }
  void append(const uint8_t* src, size_t len) {  // doubles its way up
    if (n + len > cap) {
      // a group sizes its members' slices for the whole feed; only host-side LZ4 (a group without SURGE_INGEST_DEVICE_LZ4)
      // can outgrow one: surge_ingest_group_feed undoes the feed and runs it again with more room
      if (external) throw SliceOverflow();
      size_t c = cap ? cap * 2 : (size_t)1 << 16;
      while (c < n + len) c *= 2;
      regrow(c, n);
    }
    if (len) std::memcpy(p + n, src, len);
    n += len;
  }

  // Where the arenas [first, last) take their memory from, as long as none of them holds any (false: one does, nothing was changed —
  // surge_ingest_set_allocator and surge_ingest_group_set_allocator each refuse in their own words, through their own channel)
  static bool set_allocator(Arena* first, Arena* last, void* (*alloc)(size_t), void (*release)(void*)) {
    for (const Arena* a = first; a != last; ++a)
      if (a->cap) return false;
    for (Arena* a = first; a != last; ++a) { a->alloc = alloc; a->release = release; }
    return true;
  }

 private:
  void regrow(size_t c, size_t keep) {  // `c` bytes from the allocator; the first `keep` bytes move along
    uint8_t* fresh = (uint8_t*)(alloc ? alloc(c) : std::malloc(c));
    if (!fresh) throw std::bad_alloc();
    if (keep) std::memcpy(fresh, p, keep);
    if (p) (release ? release : std::free)(p);
    p = fresh;
    n = keep;
    cap = c;
  }
};

// What the group calls of ingest.cpp beside its exports.  fail: sets the handle's error text (g may be null) and the calling thread's
// (surge_ingest_last_error(NULL) / surge_ingest_group_last_error(NULL) read it); returns `code`
int32_t fail(surge_ingest* g, int32_t code, const std::string& m);
int64_t position_of(const surge_ingest* g);  // the offset a consumer resumes from (surge_ingest_position)

}  // namespace framer
}  // namespace ingest
}  // namespace surge

// (the C ABI's name for the framer stays in the global namespace; that its members are hidden types is intended)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"
struct surge_ingest {
  using Arena = surge::ingest::framer::Arena;
  using Batch = surge::ingest::framer::Batch;
  int isolation = SURGE_INGEST_READ_COMMITTED;
  bool frames = false;  // SURGE_INGEST_FRAMES: records are not parsed here, their sections go to a surge_device_decoder
  bool device_lz4 = false;  // SURGE_INGEST_DEVICE_LZ4: ... and LZ4 frames stay compressed (the device decoder undoes them)
  bool device_crc = false;  // SURGE_INGEST_DEVICE_CRC: ... and a data batch's CRC-32C is finished and compared on the device
  bool inplace = false;     // (a group's in-place feed) `data` lies inside the slab this member's slice is a view of: sections stay where they were received
  std::string err;
  // FRAMES mode rotates through six arenas, one per feed: the sections a drain handed out stay where they are while
  // the next FIVE feeds fill the others, so host threads can frame fetches i + 1 .. i + 5 while a device decoder still
  // reads fetch i (surge_device_decoder_push_async keeps up to five pushes in flight).  The other modes only ever use
  // the first.
  static constexpr int kArenas = 6;
  Arena arenas[kArenas];
  int cur = 0;
  bool handed_out = false;  // a drain has handed out spans of arenas[cur] since the last switch
  int crc_threads = 1;      // surge_ingest_set_threads: host threads that verify the batches' CRC-32C of one feed
  // a member of a surge_ingest_group frames every feed into the slice of the group's slab it is given for that feed
  bool grouped = false;
  Arena ext[kArenas];
  uint8_t* ext_next = nullptr;
  size_t ext_next_cap = 0;
  bool slice_overflow = false;  // the last feed ran out of its slice (host-side LZ4 in a group: the group retries with more room)
  Arena& arena_now() { return grouped ? ext[cur] : arenas[cur]; }
  const Arena& arena_now() const { return grouped ? ext[cur] : arenas[cur]; }
  std::deque<Batch> queue;
  int64_t queued_section_bytes() const {  // the bytes of the sections a FRAMES framer still holds (open transactions, batches not drained yet)
    int64_t queued = 0;
    for (const Batch& qb : queue) queued += qb.sect_off >= 0 ? qb.sect_len : 0;
    return queued;
  }
  std::vector<std::string> keys;   // aggregate ids in first-seen order
  std::vector<uint64_t> key_hash;  // their hashes
  std::vector<int64_t> slots;      // open-addressing index over keys (power-of-two size, -1 = empty)
  std::vector<uint8_t> scratch;
  int64_t counters[surge::ingest::framer::C_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
  // surge_ingest_set_start_offset: where a consumer that has sought into the partition begins, and how far this one has come
  struct Start {
    int64_t first = 0;             // records below it are not delivered (<= 0: no start)
    bool passed = false;           // a batch that reaches the start has been handed out: the floor is inert from here on
    bool fed = false;              // (the start is set before the first feed)
    int64_t next_offset = -1;      // the offset behind the last batch a feed took (-1: none yet)
    int64_t discarded_batches = 0, dropped_records = 0;  // surge_ingest_below_start
    int64_t floored_section = -1;  // the section of the last drain_sections that straddles the start (-1: none)
    bool live() const { return first > 0 && !passed; }
    // What a live start means for one batch, wherever batches are handed out: it lies below the start as a whole and is never delivered;
    // or it reaches it — the first that does is the one that can straddle it, and the floor is inert behind it.  (... and for one record)
    bool below(const Batch& b) const { return b.last_offset < first; }
    bool below(int64_t offset) const { return offset < first; }
    bool straddled_by(const Batch& b) const { return b.base_offset < first && !below(b); }
  } start;
};
#pragma GCC diagnostic pop
