// ingest.cpp — events-topic ingest, host side of libsurge_replay.so.
// Kafka RecordBatch v2 + read_committed, restated from the published formats (kafka-clients 3.2.3 is not vendored with the
// reference: parity unpinned, see include/surge_ingest.h).  The LZ4 frames of compressed batches are read by lz4_frame.cpp.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <time.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#endif
#include <pthread.h>
#include <thread>
#include <vector>

#include "../../include/surge_ingest.h"

namespace {

constexpr int32_t OK = 0, E_INVALID = -1, E_NOMEM = -4, E_UNSUPPORTED = -5;

// surge_ingest_counters' eight slots, in the order include/surge_ingest.h gives them
enum Counter { C_BATCHES, C_RECORDS_DECODED, C_RECORDS_DELIVERED, C_RECORDS_ABORTED, C_CONTROL_BATCHES, C_FLUSH_SKIPPED, C_BYTES_DECOMPRESSED,
               C_OPEN_TRANSACTIONS, C_COUNT };
static_assert(C_COUNT == 8, "surge_ingest_counters hands out int64_t[8]");

thread_local std::string g_err;

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

struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;  // Castagnoli, reflected
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xff];
  }
};

const CrcTables& crc_tables() {
  static const CrcTables tables;  // initialised once, thread-safe (one decoder per partition thread)
  return tables;
}

#if defined(__x86_64__)
// The CRC32 instruction computes exactly this polynomial, 8 bytes per instruction with a latency of 3 cycles and a
// throughput of one per cycle: ONE dependent chain leaves two thirds of the unit idle (4.3 GB/s measured).  So a long
// buffer is cut into three equal blocks whose CRCs run interleaved in one loop; block A's register is then advanced
// over the length of B ("crc of A followed by |B| zero bytes", a linear map applied through four 256-entry tables built
// once from the byte table) and xor-ed into B's, likewise into C's — the classic three-way scheme of Intel's white paper
// / Mark Adler's crc32c.c, restated.
constexpr int64_t kCrcLong = 8192, kCrcShort = 256;

struct CrcShift {
  uint32_t t[4][256];
  // t[k][n]: the register value (n << 8k) after `len` zero bytes
  explicit CrcShift(int64_t len) {
    const CrcTables& T = crc_tables();
    for (int k = 0; k < 4; ++k)
      for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n << (8 * k);
        for (int64_t i = 0; i < len; ++i) c = (c >> 8) ^ T.t[0][c & 0xff];
        t[k][n] = c;
      }
  }
  uint32_t apply(uint32_t c) const { return t[0][c & 0xff] ^ t[1][(c >> 8) & 0xff] ^ t[2][(c >> 16) & 0xff] ^ t[3][c >> 24]; }
};

// three interleaved chains over data[0 .. 3 block), joined; returns the register after all three blocks
__attribute__((target("sse4.2"))) uint64_t crc32c_three_way(uint64_t c0, const uint8_t* data, int64_t block, const CrcShift& sh) {
  uint64_t c1 = 0, c2 = 0;
  const uint8_t* a = data;
  const uint8_t* b = data + block;
  const uint8_t* c = data + 2 * block;
  for (int64_t i = 0; i < block; i += 8) {
    uint64_t va, vb, vc;
    std::memcpy(&va, a + i, 8);
    std::memcpy(&vb, b + i, 8);
    std::memcpy(&vc, c + i, 8);
    c0 = __builtin_ia32_crc32di(c0, va);
    c1 = __builtin_ia32_crc32di(c1, vb);
    c2 = __builtin_ia32_crc32di(c2, vc);
  }
  c0 = sh.apply((uint32_t)c0) ^ c1;
  c0 = sh.apply((uint32_t)c0) ^ c2;
  return c0;
}

__attribute__((target("sse4.2"))) uint32_t crc32c_hw(const uint8_t* data, int64_t len) {
  static const CrcShift shift_long(kCrcLong), shift_short(kCrcShort);
  uint64_t c0 = 0xffffffffu;
  for (; len >= 3 * kCrcLong; data += 3 * kCrcLong, len -= 3 * kCrcLong) c0 = crc32c_three_way(c0, data, kCrcLong, shift_long);
  for (; len >= 3 * kCrcShort; data += 3 * kCrcShort, len -= 3 * kCrcShort) c0 = crc32c_three_way(c0, data, kCrcShort, shift_short);
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t v;
    std::memcpy(&v, data + i, 8);
    c0 = __builtin_ia32_crc32di(c0, v);
  }
  uint32_t c32 = (uint32_t)c0;
  for (; i < len; ++i) c32 = __builtin_ia32_crc32qi(c32, data[i]);
  return c32 ^ 0xffffffffu;
}
#endif

struct Reader {
  const uint8_t* p;
  const uint8_t* end;
  bool ok = true;
  bool need(int64_t n) {
    if (!ok || end - p < n) { ok = false; return false; }
    return true;
  }
  uint8_t u8() { return need(1) ? *p++ : 0; }
  // zig-zag varint (protobuf style), as Kafka's ByteUtils.readVarlong
  int64_t varlong() {
    uint64_t v = 0;
    int shift = 0;
    while (true) {
      if (!need(1) || shift > 63) { ok = false; return 0; }
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7f) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }
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

}  // namespace

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

struct surge_ingest {
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
  std::vector<std::string> keys;   // aggregate ids in first-seen order
  std::vector<uint64_t> key_hash;  // their hashes
  std::vector<int64_t> slots;      // open-addressing index over keys (power-of-two size, -1 = empty)
  std::vector<uint8_t> scratch;
  int64_t counters[C_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
  // surge_ingest_set_start_offset: where a consumer that has sought into the partition begins, and how far this one has come
  struct Start {
    int64_t first = 0;             // records below it are not delivered (<= 0: no start)
    bool passed = false;           // a batch that reaches the start has been handed out: the floor is inert from here on
    bool fed = false;              // (the start is set before the first feed)
    int64_t next_offset = -1;      // the offset behind the last batch a feed took (-1: none yet)
    int64_t discarded_batches = 0, dropped_records = 0;  // surge_ingest_below_start
    int64_t floored_section = -1;  // the section of the last drain_sections that straddles the start (-1: none)
    bool live() const { return first > 0 && !passed; }
  } start;
};

namespace {

int32_t fail(surge_ingest* g, int32_t code, const std::string& m) {
  if (g) g->err = m;
  g_err = m;
  return code;
}

inline uint64_t hash_bytes(const uint8_t* p, size_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
  while (n >= 8) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    h = (h ^ v) * 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    p += 8;
    n -= 8;
  }
  uint64_t v = 0;
  if (n > 0) std::memcpy(&v, p, n);  // an empty key in an empty arena has a null pointer
  h = (h ^ v) * 0xD6E8FEB86659FD93ull;
  return h ^ (h >> 29);
}

void rehash(surge_ingest* g, size_t new_cap) {
  g->slots.assign(new_cap, -1);
  const size_t mask = new_cap - 1;
  for (size_t i = 0; i < g->keys.size(); ++i) {
    size_t s = (size_t)g->key_hash[i] & mask;
    while (g->slots[s] >= 0) s = (s + 1) & mask;
    g->slots[s] = (int64_t)i;
  }
}

int64_t intern(surge_ingest* g, const uint8_t* key, int32_t len) {
  size_t n = 0;
  while (n < (size_t)len && key[n] != (uint8_t)':') ++n;  // PartitionStringUpToColon
  if (g->slots.empty()) rehash(g, 1024);
  const uint64_t h = hash_bytes(key, n);
  size_t mask = g->slots.size() - 1;
  for (size_t s = (size_t)h & mask;; s = (s + 1) & mask) {
    const int64_t i = g->slots[s];
    if (i < 0) break;
    if (g->key_hash[(size_t)i] == h && g->keys[(size_t)i].size() == n && std::memcmp(g->keys[(size_t)i].data(), key, n) == 0) return i;
  }
  const int64_t idx = (int64_t)g->keys.size();
  g->keys.emplace_back((const char*)key, n);
  g->key_hash.push_back(h);
  if ((g->keys.size() + 1) * 2 > g->slots.size()) {
    rehash(g, g->slots.size() * 2);
  } else {
    size_t s = (size_t)h & mask;
    while (g->slots[s] >= 0) s = (s + 1) & mask;
    g->slots[s] = idx;
  }
  return idx;
}

// dense aggregate index of a record that is being delivered
inline int64_t deliver_idx(surge_ingest* g, Rec& r) {
  if (r.agg_idx == -2) r.agg_idx = intern(g, g->arena_now().data() + r.key_off, r.key_len);
  return r.agg_idx;
}

// number of records deliverable from the head of the queue
int64_t ready_count(const surge_ingest* g) {
  int64_t n = 0;
  bool live = g->start.live();
  for (const Batch& b : g->queue) {
    if (b.decided == 0) break;  // an open transaction: nothing behind it is stable yet
    if (b.decided != 1) continue;
    if (!live) {
      n += b.sect_off >= 0 ? (int64_t)b.count : (int64_t)(b.recs.size() - b.next);
      continue;
    }
    // below the start nothing is deliverable (of a section that straddles it the device decides: all of it counts)
    if (b.sect_off >= 0) n += b.last_offset >= g->start.first ? (int64_t)b.count : 0;
    else for (size_t i = b.next; i < b.recs.size(); ++i) n += b.recs[i].offset >= g->start.first;
    live = b.last_offset < g->start.first;
  }
  return n;
}

// h's records, as they stand at data[0, len), into b (a control batch's: the marker's type into *control_type)
int32_t parse_records(surge_ingest* g, Batch& b, const BatchHeader& h, const uint8_t* data, int64_t len, int* control_type) {
  Reader r{data, data + len};
  const bool control = h.control();
  if (h.count > 0 && !control) b.recs.reserve((size_t)(h.count < 65536 ? h.count : 65536));
  for (int32_t i = 0; i < h.count; ++i) {
    const int64_t rlen = r.varlong();
    if (!r.ok || rlen < 0 || !r.need(rlen)) return fail(g, SURGE_E_CORRUPT, "record length runs past the batch");
    Reader q{r.p, r.p + rlen};
    r.p += rlen;
    (void)q.u8();        // attributes
    (void)q.varlong();   // timestampDelta
    const int64_t offset_delta = q.varlong();
    const int64_t klen = q.varlong();
    if (!q.ok || klen < -1 || (klen >= 0 && !q.need(klen))) return fail(g, SURGE_E_CORRUPT, "bad record key");
    const uint8_t* key = q.p;
    if (klen > 0) q.p += klen;
    const int64_t vlen = q.varlong();
    if (!q.ok || vlen < -1 || (vlen >= 0 && !q.need(vlen))) return fail(g, SURGE_E_CORRUPT, "bad record value");
    const uint8_t* val = q.p;
    if (vlen > 0) q.p += vlen;
    const int64_t n_headers = q.varlong();
    if (!q.ok || n_headers < 0) return fail(g, SURGE_E_CORRUPT, "bad header count");
    for (int64_t hdr = 0; hdr < n_headers; ++hdr) {
      const int64_t hk = q.varlong();
      if (!q.ok || hk < 0 || !q.need(hk)) return fail(g, SURGE_E_CORRUPT, "bad header key");
      q.p += hk;
      const int64_t hv = q.varlong();
      if (!q.ok || hv < -1 || (hv > 0 && !q.need(hv))) return fail(g, SURGE_E_CORRUPT, "bad header value");
      if (hv > 0) q.p += hv;
    }
    g->counters[C_RECORDS_DECODED] += 1;
    if (control) {
      // control record key: version int16, type int16 (0 = ABORT, 1 = COMMIT)
      if (klen >= 4) *control_type = (key[2] << 8) | key[3];
      continue;
    }
    if (klen == 0 && vlen == 0) {  // the producer's "flush" record (KafkaProducerActorImpl.scala:322-329)
      if (g->start.live() && h.base_offset + offset_delta < g->start.first) {  // below the start it is dropped like any record
        g->counters[C_RECORDS_DECODED] -= 1;
        g->start.dropped_records += 1;
      } else {
        g->counters[C_FLUSH_SKIPPED] += 1;
      }
      continue;
    }
    Rec rec;
    rec.offset = h.base_offset + offset_delta;
    rec.key_len = (int32_t)klen;
    rec.value_len = (int32_t)vlen;
    rec.key_off = (int64_t)g->arena_now().size();
    if (klen > 0) g->arena_now().append(key, (size_t)klen);
    rec.value_off = (int64_t)g->arena_now().size();
    if (vlen > 0) g->arena_now().append(val, (size_t)vlen);
    rec.agg_idx = klen >= 0 ? -2 : -1;  // -2: interned when the record is DELIVERED (drain): the keys of aborted or
                                        // still-open transactions never enter the key table
    b.recs.push_back(rec);
  }
  return OK;
}

// the bytes of the sections a FRAMES framer still holds (open transactions, batches not drained yet)
int64_t queued_section_bytes(const surge_ingest& g) {
  int64_t queued = 0;
  for (const Batch& qb : g.queue) queued += qb.sect_off >= 0 ? qb.sect_len : 0;
  return queued;
}

// The records deliverable from the head of the queue, up to `max` of them: the walk stops at an open transaction (nothing
// behind it is stable yet) and passes aborted batches.  fn(rec, k) gets the k-th of them and answers false to refuse it,
// which ends the walk with -1; otherwise the count comes back.  kPop: what was visited leaves the queue, and the batches
// that are exhausted or aborted in front of it go with it; without it the queue stays as it is.
// A start offset (surge_ingest_set_start_offset): records below it are passed over, unseen by fn, until a batch that reaches
// the start has been visited to its end; the popping walk counts them (and the batches that lie below the start as a whole).
template <bool kPop, class Fn>
inline int64_t visit_ready(surge_ingest* g, int64_t max, Fn&& fn) {
  int64_t n = 0;
  size_t at = 0;  // (a popping walk only ever looks at the front)
  surge_ingest::Start& st = g->start;
  bool live = st.live();
  while ((n < max || live) && at < g->queue.size()) {  // (below a live start the walk goes on without room: what it passes over takes none)
    Batch& b = g->queue[at];
    if (b.decided == 0) break;
    if (b.decided == 1) {
      size_t i = b.next;
      for (; i < b.recs.size(); ++i) {
        if (live && b.recs[i].offset < st.first) {
          if (kPop) { g->counters[C_RECORDS_DECODED] -= 1; st.dropped_records += 1; }
          continue;
        }
        if (n == max) break;
        if (!fn(b.recs[i], n)) return -1;
        ++n;
      }
      if (kPop) b.next = i;
      if (i < b.recs.size()) break;  // no room for the batch's next record
      if (live && i == b.recs.size()) {
        if (b.last_offset >= st.first) live = false;
        else if (kPop) st.discarded_batches += 1;
      }
    }
    if (!kPop) ++at;
    else if (b.decided == 2 || b.next == b.recs.size()) g->queue.pop_front();
  }
  if (kPop && !live) st.passed = st.first > 0;
  return n;
}

// The offset a consumer resumes from: behind the last batch a feed took, in front of whatever the queue still holds to be
// delivered — an open transaction, committed batches not drained yet (aborted ones are already decided) — and never below
// the start.
int64_t position_of(const surge_ingest* g) {
  int64_t pos = g->start.next_offset < 0 ? 0 : g->start.next_offset;
  for (const Batch& b : g->queue) {
    if (b.decided == 2) continue;
    pos = (b.sect_off < 0 && b.next > 0 && b.next < b.recs.size()) ? b.recs[b.next].offset : b.base_offset;
    break;
  }
  return pos < g->start.first ? g->start.first : pos;
}

constexpr const char* kFramesOnly = "this decoder frames batches for a surge_device_decoder (SURGE_INGEST_FRAMES): use surge_ingest_drain_sections";

int32_t delivered(surge_ingest* g, int64_t n, int64_t* n_out) {
  g->counters[C_RECORDS_DELIVERED] += n;
  *n_out = n;
  return OK;
}

// For each whole batch at the front of data[0, len) whether its CRC-32C holds.  The walk stops where surge_ingest_feed's
// stops for good — both read their headers with read_batch_header — so verdict k is batch k's.
void verify_crcs_in_parallel(const uint8_t* data, int64_t len, int n_threads, std::vector<uint8_t>* ok) try {
  std::vector<BatchHeader> heads;
  BatchHeader h;
  for (int64_t pos = 0; read_batch_header(data, len, pos, &h) == HeaderRead::WHOLE && h.magic == 2; pos += h.size()) heads.push_back(h);
  ok->assign(heads.size(), 0);
  if (heads.empty()) return;
  (void)surge_crc32c((const uint8_t*)"", 0);  // initialise the dispatch / tables before threads race for them
  std::atomic<size_t> next{0};
  auto work = [&]() {
    constexpr size_t kGrab = 32;
    for (size_t b = next.fetch_add(kGrab); b < heads.size(); b = next.fetch_add(kGrab))
      for (size_t k = b; k < heads.size() && k < b + kGrab; ++k) (*ok)[k] = surge_crc32c(heads[k].crc_from, heads[k].crc_len) == heads[k].crc;
  };
  std::vector<std::thread> th;
  try {
    for (int t = 1; t < n_threads; ++t) th.emplace_back(work);
  } catch (...) {  // the threads that did start, and this one, do the work
  }
  work();
  for (std::thread& t : th) t.join();
} catch (...) {  // no memory for the lists: no verdicts, the walk computes the CRCs itself
  ok->clear();
}

// FRAMES, a feed that follows a drain (or any feed of a group's member): on to the next arena.  The sections still queued (open
// transactions, undrained batches) move along, the ones the last drain handed out stay untouched in the arena this feed leaves
// behind (valid through the five feeds after it).
void rotate_arena(surge_ingest* g, int64_t feed_len) {
  const int to = (g->cur + 1) % surge_ingest::kArenas;
  Arena& next = g->grouped ? g->ext[to] : g->arenas[to];
  const Arena& prev = g->arena_now();
  if (g->grouped) {
    next.view(g->ext_next, g->ext_next_cap);
  } else {  // room for the whole feed at once: a page-locked arena that doubles its way up costs an allocation per step
    next.clear();
    next.reserve((size_t)queued_section_bytes(*g) + (size_t)feed_len);
  }
  for (Batch& qb : g->queue) {
    if (qb.sect_off < 0) continue;
    const int64_t at = (int64_t)next.size();
    next.append(prev.data() + qb.sect_off, (size_t)qb.sect_len);
    qb.sect_off = at;
  }
  g->cur = to;
  g->handed_out = false;
}

// An lz4 batch's frame, decompressed on the host into g->scratch: *recs / *recs_len then name the records themselves.
int32_t host_lz4(surge_ingest* g, const uint8_t** recs, int64_t* recs_len) {
  // first guess: the frame's content-size field when the producer wrote one, else 8x (Kafka's LZ4 output
  // stream omits it); a too-small guess comes back as -6 (out of space) and is grown, never as "corrupt"
  const uint8_t* frame = *recs;
  const int64_t frame_len = *recs_len;
  int64_t cap = frame_len * 8 + 1024;
  if (frame_len >= 15 && (frame[4] & 0x08)) {
    uint64_t cs = 0;
    for (int k = 7; k >= 0; --k) cs = (cs << 8) | frame[6 + k];
    if (cs > 0 && cs <= (1ull << 31)) cap = (int64_t)cs;
  }
  int64_t got;
  while (true) {
    g->scratch.resize((size_t)cap);
    got = surge_lz4_frame_decompress(frame, frame_len, g->scratch.data(), cap);
    if (got != -6) break;
    cap *= 4;
    if (cap > (1ll << 31)) return fail(g, SURGE_E_CORRUPT, "LZ4 batch expands beyond 2 GiB");
  }
  if (got < 0) return fail(g, SURGE_E_CORRUPT, "bad LZ4 frame in record batch");
  g->counters[C_BYTES_DECOMPRESSED] += got;
  *recs = g->scratch.data();
  *recs_len = got;
  return OK;
}

// FRAMES: a data batch's records section travels as it is (the device chains and parses the records): copied into the arena,
// with defer_crc behind the 8-byte prefix; or, in place, left where the fetch response was received (inside the slab this
// slice is a view of), with defer_crc together with the 44 bytes in front of it (Batch::crc_prefix).
void place_section(surge_ingest* g, Batch& b, const BatchHeader& h, const uint8_t* recs, int64_t recs_len, int sect_codec, bool defer_crc) {
  Arena& arena = g->arena_now();
  b.base_offset = h.base_offset;
  b.count = h.count;
  b.sect_codec = sect_codec;
  if (g->inplace) {
    b.crc_prefix = defer_crc ? 44 : 0;
    b.sect_off = (int64_t)(recs - arena.data()) - b.crc_prefix;
  } else {
    b.sect_off = (int64_t)arena.size();
    if (defer_crc) {
      const uint32_t pre[2] = {h.crc, ~surge_crc32c(h.crc_from, 40)};  // the register (not finalised) after attributes .. recordCount
      arena.append((const uint8_t*)pre, 8);
      b.crc_prefix = 8;
    }
    arena.append(recs, (size_t)recs_len);
  }
  b.sect_len = recs_len + b.crc_prefix;
  g->counters[C_RECORDS_DECODED] += h.count;
}

// An ABORT (0) / COMMIT (1) marker ends its producer's open transaction.  *n_open: the open transactions' batches in the queue
// — few; the marker looks for its producer's among them from the back and stops at the oldest open one (the first version
// walked the whole queue per marker: every batch of the feed).
void apply_marker(surge_ingest* g, int64_t producer_id, int control_type, int64_t* n_open) {
  int64_t still_to_see = *n_open;
  for (auto qb = g->queue.rbegin(); qb != g->queue.rend() && still_to_see > 0; ++qb) {
    if (qb->decided != 0) continue;
    --still_to_see;
    if (qb->producer_id != producer_id) continue;
    qb->decided = control_type == 1 ? 1 : 2;
    --*n_open;
    if (control_type == 0) g->counters[C_RECORDS_ABORTED] += qb->sect_off >= 0 ? (int64_t)qb->count : (int64_t)qb->recs.size();
  }
}

// One whole batch of a feed: checked, its records parsed (or, FRAMES, its section placed), queued; a marker decides the
// transactions it ends.  crc_verdict: the batch's CRC-32C verified up front (null: not yet).
int32_t take_batch(surge_ingest* g, const BatchHeader& h, const uint8_t* crc_verdict, int64_t* n_open) {
  if (h.magic != 2) return fail(g, E_UNSUPPORTED, "only message format v2 (magic 2) is supported");
  // SURGE_INGEST_DEVICE_CRC: the CRC of a data batch is only STARTED here — over the 40 header bytes it covers in front of the
  // records section (place_section) — and finished where the section's bytes go anyway: on the device.  What this thread
  // still touches of a batch is its header.
  const bool defer_crc = g->device_crc && !h.control();
  if (!defer_crc && !(crc_verdict ? *crc_verdict != 0 : surge_crc32c(h.crc_from, h.crc_len) == h.crc))
    return fail(g, SURGE_E_CORRUPT, "record batch CRC-32C mismatch");
  if (h.count < 0) return fail(g, SURGE_E_CORRUPT, "truncated batch header");
  // (a header that is only verified later, on the device, must not drive anything out of bounds before that: a record takes
  // at least 7 bytes, and LZ4 expands at most 255 x)
  if (defer_crc && (int64_t)h.count > (h.recs_len / 7 + 1) * (h.codec() ? 255 : 1))
    return fail(g, SURGE_E_CORRUPT, "recordCount impossible for the batch's size (damaged header)");
  const uint8_t* recs = h.recs;
  int64_t recs_len = h.recs_len;
  int sect_codec = 0;
  if (h.codec() == 3 && g->device_lz4 && !h.control()) {
    sect_codec = 3;  // the frame travels as it is: the device decoder walks its blocks and decodes them on the GPU
  } else if (h.codec() == 3 && g->inplace && !h.control()) {
    return fail(g, E_UNSUPPORTED, "an in-place feed leaves the sections where they were received: lz4 topics need SURGE_INGEST_DEVICE_LZ4");
  } else if (h.codec() == 3) {
    const int32_t rc = host_lz4(g, &recs, &recs_len);
    if (rc != OK) return rc;
  } else if (h.codec() != 0) {
    return fail(g, E_UNSUPPORTED, "compression codec not supported (only none and lz4; the reference publishes lz4)");
  }
  Batch b;
  b.producer_id = h.producer_id;
  b.base_offset = h.base_offset;
  b.last_offset = h.base_offset + h.last_offset_delta;
  int control_type = -1;
  if (g->frames && !h.control()) {
    if (defer_crc && recs != h.recs) return fail(g, E_UNSUPPORTED, "SURGE_INGEST_DEVICE_CRC needs the sections to travel as they are on the wire (SURGE_INGEST_DEVICE_LZ4 for lz4 topics)");
    place_section(g, b, h, recs, recs_len, sect_codec, defer_crc);
  } else {
    const int32_t rc = parse_records(g, b, h, recs, recs_len, &control_type);
    if (rc != OK) return rc;
  }
  g->counters[C_BATCHES] += 1;
  g->start.next_offset = b.last_offset + 1;
  if (h.control()) {
    g->counters[C_CONTROL_BATCHES] += 1;
    if (control_type == 0 || control_type == 1) apply_marker(g, h.producer_id, control_type, n_open);
    return OK;
  }
  b.decided = (h.transactional() && g->isolation == SURGE_INGEST_READ_COMMITTED) ? 0 : 1;
  if (!b.recs.empty() || b.count > 0) {
    *n_open += b.decided == 0;
    g->queue.push_back(std::move(b));
  }
  return OK;
}

// surge_ingest_feed's walk.  *pos: where the first batch not consumed begins — a failure in batch k leaves batches 0..k-1 of
// this buffer decoded and queued: they are reported as consumed, so a caller that retries (or skips the bad batch) never
// feeds them twice.  What throws (no memory, a full slice) leaves *pos where it stands.
int32_t feed_batches(surge_ingest* g, const uint8_t* data, int64_t len, int64_t* pos) {
  if (g->frames && (g->handed_out || g->grouped)) {
    rotate_arena(g, len);  // (a feed that follows no drain keeps appending where the last one stopped: nothing is copied)
  } else if (g->queue.empty()) {
    // nothing queued and (FRAMES: no span of this arena handed out since the switch) nothing to keep: start over
    g->arena_now().clear();
  }
  // With more than one CRC thread the batches' checksums are verified up front, in parallel (a batch's CRC depends on
  // nothing but its own bytes; the walk below then looks the verdicts up in order, so what is reported, and when, is
  // exactly what the one-thread walk reports).
  std::vector<uint8_t> crc_ok;
  if (g->crc_threads > 1 && len >= (1 << 20) && !g->device_crc) verify_crcs_in_parallel(data, len, g->crc_threads, &crc_ok);
  int64_t n_open = 0;
  for (const Batch& qb : g->queue) n_open += qb.decided == 0;
  BatchHeader h;
  for (size_t batch_no = 0;; ++batch_no, *pos += h.size()) {
    const HeaderRead got = read_batch_header(data, len, *pos, &h);
    if (got == HeaderRead::SHORT) return fail(g, SURGE_E_CORRUPT, "batchLength below the v2 header size");
    if (got == HeaderRead::CUT) break;  // partial batch: wait for more bytes
    __builtin_prefetch(h.recs + h.recs_len);  // the next batch's header: a fresh cache line every few KB of a buffer that was just received
    __builtin_prefetch(h.recs + h.recs_len + 64);
    const int32_t rc = take_batch(g, h, batch_no < crc_ok.size() ? &crc_ok[batch_no] : nullptr, &n_open);
    if (rc != OK) return rc;
  }
  g->counters[C_OPEN_TRANSACTIONS] = n_open;
  return OK;
}

}  // namespace

extern "C" {

uint32_t surge_crc32c(const uint8_t* data, int64_t len) {
#if defined(__x86_64__)
  static const bool have_hw = __builtin_cpu_supports("sse4.2");
  if (have_hw) return crc32c_hw(data, len);
#endif
  const CrcTables& T = crc_tables();
  uint32_t c = 0xffffffffu;
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) {  // slicing-by-8
    const uint32_t lo = c ^ ((uint32_t)data[i] | ((uint32_t)data[i + 1] << 8) | ((uint32_t)data[i + 2] << 16) | ((uint32_t)data[i + 3] << 24));
    c = T.t[7][lo & 0xff] ^ T.t[6][(lo >> 8) & 0xff] ^ T.t[5][(lo >> 16) & 0xff] ^ T.t[4][lo >> 24] ^
        T.t[3][data[i + 4]] ^ T.t[2][data[i + 5]] ^ T.t[1][data[i + 6]] ^ T.t[0][data[i + 7]];
  }
  for (; i < len; ++i) c = (c >> 8) ^ T.t[0][(c ^ data[i]) & 0xff];
  return c ^ 0xffffffffu;
}

/* table walk only (tests compare it with the instruction path) */
uint32_t surge_crc32c_portable(const uint8_t* data, int64_t len) {
  const CrcTables& T = crc_tables();
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < len; ++i) c = (c >> 8) ^ T.t[0][(c ^ data[i]) & 0xff];
  return c ^ 0xffffffffu;
}

int32_t surge_ingest_create(int32_t isolation_level, surge_ingest** out) {
  if (!out) return fail(nullptr, E_INVALID, "out is NULL");
  *out = nullptr;
  const int32_t flags = isolation_level & (SURGE_INGEST_FRAMES | SURGE_INGEST_DEVICE_LZ4 | SURGE_INGEST_DEVICE_CRC);
  isolation_level &= ~flags;
  if (isolation_level != SURGE_INGEST_READ_UNCOMMITTED && isolation_level != SURGE_INGEST_READ_COMMITTED)
    return fail(nullptr, E_INVALID, "unknown isolation level");
  surge_ingest* g = new (std::nothrow) surge_ingest();
  if (!g) return fail(nullptr, E_NOMEM, "out of host memory");
  g->isolation = isolation_level;
  g->frames = flags != 0;
  g->device_lz4 = (flags & SURGE_INGEST_DEVICE_LZ4) != 0;
  g->device_crc = (flags & SURGE_INGEST_DEVICE_CRC) != 0;
  *out = g;
  return OK;
}

int32_t surge_ingest_destroy(surge_ingest* g) {
  delete g;
  return OK;
}

const char* surge_ingest_last_error(const surge_ingest* g) { return g ? g->err.c_str() : g_err.c_str(); }

int32_t surge_ingest_set_threads(surge_ingest* g, int32_t n_threads) {
  if (!g || n_threads < 1 || n_threads > 64) return fail(g, E_INVALID, "threads must be in 1 .. 64");
  g->crc_threads = n_threads;
  return OK;
}

int32_t surge_ingest_feed(surge_ingest* g, const uint8_t* data, int64_t len, int64_t* consumed_out) {
  if (!g) return fail(nullptr, E_INVALID, "handle is NULL");
  if (len < 0 || (!data && len > 0)) return fail(g, E_INVALID, "bad buffer");
  g->start.fed = true;
  int64_t pos = 0;
  int32_t rc;
  try {
    rc = feed_batches(g, data, len, &pos);
  } catch (const SliceOverflow&) {
    g->slice_overflow = true;
    rc = fail(g, E_NOMEM, "the group's slice for this partition is full");
  } catch (const std::bad_alloc&) {
    rc = fail(g, E_NOMEM, "out of host memory while decoding");
  }
  if (consumed_out) *consumed_out = pos;
  return rc;
}

int64_t surge_ingest_ready(const surge_ingest* g) { return g ? ready_count(g) : 0; }

int32_t surge_ingest_drain(surge_ingest* g, int64_t max, surge_ingest_record* out, int64_t* n_out) {
  if (!g || !n_out || max < 0 || (!out && max > 0)) return fail(g, E_INVALID, "bad argument");
  if (g->frames) return fail(g, -2, kFramesOnly);
  return delivered(g, visit_ready<true>(g, max, [&](Rec& r, int64_t k) {
    out[k].offset = r.offset; out[k].agg_idx = deliver_idx(g, r); out[k].key_off = r.key_off; out[k].key_len = r.key_len;
    out[k].value_len = r.value_len; out[k].value_off = r.value_off;
    return true;
  }), n_out);
}

const uint8_t* surge_ingest_arena(const surge_ingest* g) { return g ? g->arena_now().data() : nullptr; }

int32_t surge_ingest_set_allocator(surge_ingest* g, void* (*alloc)(size_t), void (*release)(void*)) {
  if (!g || !alloc != !release) return fail(g, E_INVALID, "bad argument");
  for (const Arena& a : g->arenas)
    if (a.cap) return fail(g, -2, "surge_ingest_set_allocator after the first feed");
  for (Arena& a : g->arenas) {
    a.alloc = alloc;
    a.release = release;
  }
  return OK;
}

// The two drains below are all or nothing: a first walk looks at (decodes) what the call would deliver and pops nothing, so a
// value that is refused leaves the queue as it was; the second walk delivers.
int32_t surge_ingest_drain_fixed16(surge_ingest* g, int64_t max, int64_t* agg_idx_out, void* events16_out,
                                   int64_t* offsets_out, int64_t* n_out) {
  if (!g || !n_out || max < 0 || ((!agg_idx_out || !events16_out) && max > 0)) return fail(g, E_INVALID, "bad argument");
  if (g->frames) return fail(g, -2, kFramesOnly);
  int32_t refused = OK;
  visit_ready<false>(g, max, [&](Rec& r, int64_t) {
    if (r.value_len == 16 && r.agg_idx != -1) return true;
    refused = fail(g, E_INVALID, "record value is not a 16-byte fixed event (or the key is null)");
    return false;
  });
  if (refused != OK) return refused;
  uint8_t* ev = (uint8_t*)events16_out;
  return delivered(g, visit_ready<true>(g, max, [&](Rec& r, int64_t k) {
    agg_idx_out[k] = deliver_idx(g, r);
    std::memcpy(ev + k * 16, g->arena_now().data() + r.value_off, 16);
    if (offsets_out) offsets_out[k] = r.offset;
    return true;
  }), n_out);
}

int32_t surge_ingest_drain_json(surge_ingest* g, int64_t max, const surge_event_json_template* tmpl, int64_t* agg_idx_out,
                                void* events16_out, int64_t* offsets_out, int64_t* n_out) {
  if (!g || !n_out || !tmpl || max < 0 || ((!agg_idx_out || !events16_out) && max > 0)) return fail(g, E_INVALID, "bad argument");
  if (g->frames) return fail(g, -2, kFramesOnly);
  if (surge_event_json_validate(tmpl) != 0) return fail(g, E_INVALID, std::string("event template: ") + surge_event_json_last_error());
  uint8_t* ev = (uint8_t*)events16_out;
  int32_t refused = OK;
  auto decode_keyed = [&](const Rec& r, uint8_t* out) {  // an enveloped value names its aggregate: the id the record is interned under (the key up to ':')
    const uint8_t* key = g->arena_now().data() + r.key_off;
    int64_t n = 0;
    while (n < r.key_len && key[n] != (uint8_t)':') ++n;  // PartitionStringUpToColon, as intern() cuts it
    return surge_event_json_decode_keyed(tmpl, key, n, g->arena_now().data() + r.value_off, r.value_len, out);
  };
  visit_ready<false>(g, max, [&](Rec& r, int64_t k) {
    if (r.agg_idx == -1 || r.value_len < 0) {
      refused = fail(g, SURGE_E_CORRUPT, "record at offset " + std::to_string(r.offset) + " has a null key or value (not an event)");
    } else if (decode_keyed(r, ev + k * 16) != OK) {
      refused = fail(g, SURGE_E_CORRUPT, "record at offset " + std::to_string(r.offset) + ": " + surge_event_json_last_error());
    }
    return refused == OK;
  });
  if (refused != OK) return refused;
  return delivered(g, visit_ready<true>(g, max, [&](Rec& r, int64_t k) {
    agg_idx_out[k] = deliver_idx(g, r);
    if (offsets_out) offsets_out[k] = r.offset;
    return true;
  }), n_out);
}

int32_t surge_ingest_drain_sections(surge_ingest* g, int64_t max_sections, surge_batch_section* out, int64_t* n_out) {
  if (!g || !n_out || max_sections < 0 || (!out && max_sections > 0)) return fail(g, E_INVALID, "bad argument");
  if (!g->frames) return fail(g, -2, "surge_ingest_drain_sections needs a decoder created with SURGE_INGEST_FRAMES");
  int64_t n = 0, recs = 0;
  surge_ingest::Start& st = g->start;
  st.floored_section = -1;
  while (n < max_sections && !g->queue.empty()) {
    Batch& b = g->queue.front();
    if (b.decided == 0) break;  // an open transaction: nothing behind it is stable yet
    if (b.decided == 1 && st.live() && b.last_offset < st.first) {  // below the start as a whole: never handed out
      g->counters[C_RECORDS_DECODED] -= b.count;
      st.discarded_batches += 1;
      st.dropped_records += b.count;
    } else if (b.decided == 1) {
      out[n].byte_off = b.sect_off + b.crc_prefix;
      out[n].byte_len = b.sect_len - b.crc_prefix;
      out[n].base_offset = b.base_offset;
      out[n].n_records = b.count;
      out[n].codec = b.sect_codec | (b.crc_prefix == 8 ? SURGE_SECTION_CRC_PENDING : b.crc_prefix == 44 ? SURGE_SECTION_CRC_WIRE : 0);
      if (st.live()) {  // the first batch that reaches the start: the one that can straddle it
        if (b.base_offset < st.first) {
          out[n].codec |= SURGE_SECTION_FLOORED;
          st.floored_section = n;
        }
        st.passed = true;
      }
      recs += b.count;
      ++n;
    }
    g->queue.pop_front();
  }
  g->counters[C_RECORDS_DELIVERED] += recs;  // handed to the device decoder (its own counters tell flush records from events)
  if (n > 0) g->handed_out = true;
  *n_out = n;
  return OK;
}

}  // extern "C" (the group's type)

// A consumer's partitions framed as ONE unit: every feed lays the partitions' records sections out in one slab — the
// group rotates through six, like a single framer's arenas — so a fetch response reaches the device in one copy.
//
// Threads: the group keeps a POOL of framing threads for its lifetime (started at the first feed that asks for them;
// a feed hands them one job and takes part in it itself) — a consumer feeds every couple of milliseconds, and creating
// and joining seven threads per feed cost more than some feeds' framing.
//
// Failure: a feed either frames every partition or leaves the group exactly as it was.  What a member's feed changes —
// its queue (open transactions move to the new slice), its counters, which arena is current — is saved before the feed
// (a FRAMES queue holds only the few batches of open transactions: cheap) and put back when any partition fails or the
// caller's section table is too small; the slab the failed feed wrote into is the one the next feed writes into again.
namespace {

struct FramingPool {
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  std::vector<std::thread> th;
  const std::function<void()>* job = nullptr;
  uint64_t gen = 0;
  int want = 0;     // workers 0 .. want-1 take part in the current job
  int pending = 0;  // ... and have not finished it yet
  bool stop = false;

  void worker(int idx) {
    char name[16];
    snprintf(name, sizeof name, "surge-frame-%d", idx);  // (shows in /proc/<pid>/task/*/comm: bench.py's per-thread CPU table)
    pthread_setname_np(pthread_self(), name);
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv_job.wait(lk, [&] { return stop || gen != seen; });
      if (stop) return;
      seen = gen;
      if (idx >= want) continue;
      const std::function<void()>* j = job;
      lk.unlock();
      (*j)();  // (catches everything itself)
      lk.lock();
      if (--pending == 0) cv_done.notify_one();
    }
  }
  // Runs `work` on this thread and on up to `helpers` pool threads; returns when all of them have left it.
  void run(const std::function<void()>& work, int helpers) {
    {
      std::lock_guard<std::mutex> lk(mu);
      while ((int)th.size() < helpers) {
        try {
          const int idx = (int)th.size();
          th.emplace_back([this, idx] { worker(idx); });
        } catch (...) {  // std::system_error: the threads that did start — and the caller — do the work
          break;
        }
      }
      if (helpers > (int)th.size()) helpers = (int)th.size();
      job = &work;
      want = pending = helpers;
      ++gen;
    }
    if (helpers > 0) cv_job.notify_all();
    work();
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
    job = nullptr;
  }
  ~FramingPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv_job.notify_all();
    for (std::thread& t : th) t.join();
  }
};


// what a group feed changes in a member, and is undone from (once per save: restore trades the queues)
struct MemberSave {
  std::deque<Batch> queue;
  int64_t counters[C_COUNT];
  int cur;
  bool handed_out;
  surge_ingest::Start start;
  void save(const surge_ingest& x) { queue = x.queue; std::memcpy(counters, x.counters, sizeof counters); cur = x.cur; handed_out = x.handed_out; start = x.start; }
  void restore(surge_ingest& x) { x.queue.swap(queue); std::memcpy(x.counters, counters, sizeof counters); x.cur = cur; x.handed_out = handed_out; x.start = start; }
};

}  // namespace

struct surge_ingest_group {
  std::vector<surge_ingest*> g;
  Arena slabs[surge_ingest::kArenas];
  int cur = 0;
  std::string err;
  std::vector<std::vector<surge_batch_section>> drained;
  std::vector<int64_t> off;
  std::vector<MemberSave> saved;
  std::vector<int32_t> status;
  std::vector<int64_t> consumed;
  std::vector<surge_section_floor> floors;  // of the last feed's sections (surge_ingest_group_take_floors)
  // in-place feeds (surge_ingest_group_receive_buffer): the slab the caller is receiving into and the room in front of the
  // receive region that the partitions' carried sections (open transactions) move into
  int recv_slab = -1;
  int64_t recv_carry = 0, recv_bytes = 0;
  std::atomic<int64_t> cpu_ns[2] = {{0}, {0}};  // thread CPU time spent in {receive copies, framing} since the group was created (surge_ingest_group_cpu_seconds)
  int64_t expand_hint = 1;  // the slice factor the last feed needed (host-side lz4: the topic's compression ratio does not change from feed to feed)
  FramingPool pool;
  ~surge_ingest_group() {
    for (surge_ingest* x : g) delete x;
  }
};

namespace {

int64_t thread_cpu_ns() {
  struct timespec ts;
  if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) != 0) return 0;
  return (int64_t)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}

// Every partition's slice of the next slab, 16-byte aligned: what the partition still holds (open transactions, batches not
// drained yet) + bytes[p] (nullptr: nothing).  off (nullable) gets the n + 1 slice bounds; the total comes back.
int64_t lay_out_slices(const surge_ingest_group* grp, const int64_t* bytes, int64_t times, int64_t* off) {
  int64_t total = 0;
  for (size_t p = 0; p < grp->g.size(); ++p) {
    if (off) off[p] = total;
    total = (total + queued_section_bytes(*grp->g[p]) + (bytes ? bytes[p] * times : 0) + 15) & ~15ll;
  }
  if (off) off[grp->g.size()] = total;
  return total;
}

// A slab with room for fewer than `want` bytes gets `roomy` — and so does every other slab when it is the group's FIRST.  OK or E_NOMEM.
// Page-locking a 30 - 45 MB slab takes 1.5 ms on a good day and 20 ms on a bad one (bytes -> states on the small-flush topic:
// two of a dozen runs lost a 24 ms fetch to it and with it two thirds of their rate).  Fetch responses of one consumer are
// alike, so a recovery pays for page-locking once, before its pipeline fills, not once per slab over its first six fetches.
int32_t size_slab(surge_ingest_group* grp, Arena& slab, size_t want, size_t roomy) try {
  if (slab.cap >= want) return OK;
  bool first = true;
  for (const Arena& a : grp->slabs) first = first && a.cap == 0;
  if (!first) slab.reserve_exact(roomy);
  else for (Arena& a : grp->slabs) a.reserve_exact(roomy);
  return OK;
} catch (const std::bad_alloc&) {
  grp->err = "out of host memory for the group's slab";
  return E_NOMEM;
}

// A fetch response's bytes into the slab with non-temporal stores.  What is written is read again by the framer — one header line
// per few KB, prefetched a batch ahead — and by the copy engine; a cached copy reads every destination line first (read for
// ownership: a third more memory traffic) and evicts what the other threads work on.  memcpy without AVX2 / on other hosts.
#if defined(__x86_64__) || defined(__i386__)
__attribute__((target("avx2"))) void stream_copy_avx2(uint8_t* to, const uint8_t* from, size_t n) {
  size_t head = (size_t)(-(intptr_t)to) & 31u;
  if (head > n) head = n;
  std::memcpy(to, from, head);
  to += head; from += head; n -= head;
  size_t i = 0;
  for (; i + 128 <= n; i += 128) {
    const __m256i a = _mm256_loadu_si256((const __m256i*)(from + i)), b = _mm256_loadu_si256((const __m256i*)(from + i + 32));
    const __m256i c = _mm256_loadu_si256((const __m256i*)(from + i + 64)), d = _mm256_loadu_si256((const __m256i*)(from + i + 96));
    _mm256_stream_si256((__m256i*)(to + i), a);
    _mm256_stream_si256((__m256i*)(to + i + 32), b);
    _mm256_stream_si256((__m256i*)(to + i + 64), c);
    _mm256_stream_si256((__m256i*)(to + i + 96), d);
  }
  _mm_sfence();
  std::memcpy(to + i, from + i, n - i);
}
#endif
void stream_copy(uint8_t* to, const uint8_t* from, size_t n) {
#if defined(__x86_64__) || defined(__i386__)
  static const bool avx2 = __builtin_cpu_supports("avx2") && std::getenv("SURGE_INGEST_RECEIVE_COPY") == nullptr;  // (any value: plain memcpy, for A/B)
  if (avx2 && n >= 4096) return stream_copy_avx2(to, from, n);
#endif
  std::memcpy(to, from, n);
}

// In place: every partition's bytes lie inside the region surge_ingest_group_receive_buffer handed out for this feed.  The
// sections then stay where they were received — the slab is not written at all beyond the few carried sections in front.
bool received_in_place(const surge_ingest_group* grp, const uint8_t* const* data, const int64_t* len) {
  if (grp->recv_slab != (grp->cur + 1) % surge_ingest::kArenas) return false;
  const uint8_t *lo = grp->slabs[grp->recv_slab].data() + grp->recv_carry, *hi = lo + grp->recv_bytes;
  bool any = false;
  for (size_t p = 0; p < grp->g.size(); ++p) {
    if (len[p] == 0) continue;
    any = true;
    if (data[p] < lo || data[p] + len[p] > hi) return false;
  }
  return any;
}

// A framing thread takes the partitions eight at a time and first walks their batch LENGTHS side by side — one step per partition
// in turn, the next header of each prefetched while the other seven take theirs: a batch header is a cache line nobody has
// touched since the response was received (with non-temporal stores: not in any cache), and a framer that meets them one
// after the other waits out a memory latency per batch — most of what a batch costs it.
constexpr int32_t kTogether = 8;
void touch_headers(const uint8_t* const* data, const int64_t* len, int32_t p0, int32_t p1) {
  int64_t at[kTogether];
  int32_t live = 0;
  for (int32_t p = p0; p < p1; ++p) {
    at[p - p0] = len[p] >= 12 ? 0 : -1;
    if (len[p] >= 12) { __builtin_prefetch(data[p]); ++live; }
  }
  while (live > 0) {
    for (int32_t p = p0; p < p1; ++p) {
      int64_t& pos = at[p - p0];
      if (pos < 0) continue;
      int32_t batch_len;
      if (read_batch_length(data[p], len[p], pos, &batch_len) != HeaderRead::WHOLE) { pos = -1; --live; continue; }  // (the real walk decides what a bad length means)
      pos += 12 + (int64_t)batch_len;
      __builtin_prefetch(data[p] + pos);
      __builtin_prefetch(data[p] + pos + 60);
    }
  }
}

// One partition's share of a group feed: its bytes framed into its slice of the slab, what is deliverable drained, the
// sections' offsets made the slab's.  The outcome goes into grp->status / consumed / drained (nothing may leave a thread).
void frame_partition(surge_ingest_group* grp, int32_t p, uint8_t* slab, const uint8_t* data, int64_t len, bool inplace) {
  surge_ingest* x = grp->g[(size_t)p];
  const int64_t slice_at = grp->off[(size_t)p];
  int32_t rc = OK;
  int64_t consumed = 0;
  try {
    x->ext_next = slab + slice_at;
    x->ext_next_cap = (size_t)(grp->off[(size_t)p + 1] - slice_at);
    x->slice_overflow = false;
    x->inplace = inplace;
    rc = surge_ingest_feed(x, data, len, &consumed);
    x->inplace = false;
    std::vector<surge_batch_section>& out = grp->drained[(size_t)p];
    out.clear();
    if (rc == OK && !x->queue.empty()) {
      out.resize(x->queue.size());
      int64_t got = 0;
      rc = surge_ingest_drain_sections(x, (int64_t)out.size(), out.data(), &got);
      out.resize(rc == OK ? (size_t)got : 0);
      for (surge_batch_section& sct : out) sct.byte_off += slice_at;
    }
  } catch (...) {
    rc = E_NOMEM;
  }
  grp->status[(size_t)p] = rc;
  grp->consumed[(size_t)p] = consumed;
}

// A group feed's set-up, with `expand` times the room for what is framed by copy: every member saved (what a failed feed is undone
// from), the slices laid out, the slab sized for them.  OK, or the status with the group's message set.
int32_t prepare_slab(surge_ingest_group* grp, Arena& slab, const int64_t* len, bool inplace, int64_t expand) {
  try {
    for (size_t p = 0; p < grp->g.size(); ++p) grp->saved[p].save(*grp->g[p]);
  } catch (const std::bad_alloc&) {
    grp->err = "out of host memory";
    return E_NOMEM;
  }
  const int64_t total = lay_out_slices(grp, inplace ? nullptr : len, expand, grp->off.data());
  if (inplace) {
    if (total <= grp->recv_carry) return OK;  // (always: nothing was fed between receive_buffer and this call)
    grp->err = "the partitions' carried sections outgrew the room surge_ingest_group_receive_buffer left for them";
    return E_INVALID;
  }
  slab.clear();
  return size_slab(grp, slab, (size_t)total + 16, (size_t)total + (size_t)total / 4 + 65536);
}

// ... and its framing: the partitions on `threads` threads, the calling one + the group's pool
void frame_partitions(surge_ingest_group* grp, uint8_t* slab, const uint8_t* const* data, const int64_t* len, int32_t threads, bool inplace) {
  const int32_t n = (int32_t)grp->g.size();
  std::atomic<int32_t> next{0};
  const std::function<void()> work = [&]() {
    const int64_t t0 = thread_cpu_ns();
    for (int32_t p0 = next.fetch_add(kTogether); p0 < n; p0 = next.fetch_add(kTogether)) {
      const int32_t p1 = p0 + kTogether < n ? p0 + kTogether : n;
      touch_headers(data, len, p0, p1);
      for (int32_t p = p0; p < p1; ++p) frame_partition(grp, p, slab, data[p], len[p], inplace);
    }
    grp->cpu_ns[1] += thread_cpu_ns() - t0;
  };
  grp->pool.run(work, (threads < 1 ? 1 : threads > n ? n : threads) - 1);
}

}  // namespace

extern "C" {

int32_t surge_ingest_group_create(int32_t n_partitions, int32_t isolation_level, surge_ingest_group** out) {
  if (!out) return fail(nullptr, E_INVALID, "out is NULL");
  *out = nullptr;
  if (n_partitions < 1 || n_partitions > (1 << 20)) return fail(nullptr, E_INVALID, "n_partitions out of range");
  surge_ingest_group* grp = nullptr;
  try {
    grp = new surge_ingest_group();
    grp->g.reserve((size_t)n_partitions);
    grp->drained.resize((size_t)n_partitions);
    grp->off.resize((size_t)n_partitions + 1);
    grp->saved.resize((size_t)n_partitions);
    grp->status.resize((size_t)n_partitions);
    grp->consumed.resize((size_t)n_partitions);
    for (int32_t p = 0; p < n_partitions; ++p) {
      surge_ingest* x = nullptr;
      const int32_t rc = surge_ingest_create(isolation_level | SURGE_INGEST_FRAMES, &x);
      if (rc != OK) {
        delete grp;
        return rc;
      }
      x->grouped = true;
      grp->g.push_back(x);
    }
  } catch (const std::bad_alloc&) {
    delete grp;
    return fail(nullptr, E_NOMEM, "out of host memory");
  }
  *out = grp;
  return OK;
}

int32_t surge_ingest_group_destroy(surge_ingest_group* grp) {
  delete grp;
  return OK;
}

const char* surge_ingest_group_last_error(const surge_ingest_group* grp) { return grp ? grp->err.c_str() : g_err.c_str(); }

int32_t surge_ingest_group_set_allocator(surge_ingest_group* grp, void* (*alloc)(size_t), void (*release)(void*)) {
  if (!grp || !alloc != !release) return fail(nullptr, E_INVALID, "bad argument");
  for (Arena& a : grp->slabs) {
    if (a.cap) { grp->err = "surge_ingest_group_set_allocator after the first feed"; return -2; }
    a.alloc = alloc;
    a.release = release;
  }
  return OK;
}

int64_t surge_ingest_group_queued_sections(const surge_ingest_group* grp) {
  if (!grp) return 0;
  int64_t n = 0;
  for (const surge_ingest* x : grp->g) n += (int64_t)x->queue.size();
  return n;
}

int32_t surge_ingest_group_slab_bytes(const surge_ingest_group* grp, int64_t* bytes_out, int32_t* custom_allocator_out) {
  if (!grp || !bytes_out) return E_INVALID;
  int64_t total = 0;
  bool custom = false;
  for (const Arena& a : grp->slabs) {
    total += (int64_t)a.cap;
    custom = custom || a.alloc != nullptr;
  }
  *bytes_out = total;
  if (custom_allocator_out) *custom_allocator_out = custom ? 1 : 0;
  return OK;
}

int32_t surge_ingest_group_cpu_seconds(const surge_ingest_group* grp, double out[2]) {
  if (!grp || !out) return E_INVALID;
  out[0] = (double)grp->cpu_ns[0].load() * 1e-9;
  out[1] = (double)grp->cpu_ns[1].load() * 1e-9;
  return OK;
}

int32_t surge_ingest_group_receive_buffer(surge_ingest_group* grp, int64_t bytes, uint8_t** buf_out) {
  if (!grp || !buf_out || bytes < 0) return fail(nullptr, E_INVALID, "bad argument");
  *buf_out = nullptr;
  const int next = (grp->cur + 1) % surge_ingest::kArenas;
  Arena& slab = grp->slabs[next];
  // room in front for what the partitions still hold (their carried sections move there), 16-byte aligned per partition
  const int64_t carry = (lay_out_slices(grp, nullptr, 0, nullptr) + 63) & ~63ll;
  slab.clear();
  const size_t want = (size_t)(carry + bytes) + 64;
  const int32_t rc = size_slab(grp, slab, want, want + want / 4 + 65536);
  if (rc != OK) return rc;
  grp->recv_slab = next;
  grp->recv_carry = carry;
  grp->recv_bytes = bytes;
  *buf_out = slab.data() + carry;
  return OK;
}

// For a host whose fetch responses lie elsewhere (a test harness, a consumer library that owns its buffers): the one copy a
// socket read would have made — every partition's bytes into the group's receive buffer, on `threads` threads (the calling
// thread + the group's pool), cut into pieces of 1 MiB — and where each partition's bytes now are.
int32_t surge_ingest_group_receive_copy(surge_ingest_group* grp, const uint8_t* const* data, const int64_t* len, int32_t threads, const uint8_t** placed_out) {
  if (!grp || !data || !len || !placed_out) return fail(nullptr, E_INVALID, "bad argument");
  const int32_t n = (int32_t)grp->g.size();
  int64_t total = 0;
  for (int32_t p = 0; p < n; ++p) {
    if (len[p] < 0 || (!data[p] && len[p] > 0)) { grp->err = "bad buffer for partition " + std::to_string(p); return E_INVALID; }
    total += len[p];
  }
  uint8_t* base = nullptr;
  const int32_t rc = surge_ingest_group_receive_buffer(grp, total, &base);
  if (rc != OK) return rc;
  struct Piece { uint8_t* to; const uint8_t* from; size_t n; };
  std::vector<Piece> pieces;
  try {
    int64_t at = 0;
    for (int32_t p = 0; p < n; ++p) {
      placed_out[p] = len[p] ? base + at : nullptr;
      for (int64_t o = 0; o < len[p]; o += 1 << 20) pieces.push_back(Piece{base + at + o, data[p] + o, (size_t)(len[p] - o < (1 << 20) ? len[p] - o : (1 << 20))});
      at += len[p];
    }
  } catch (const std::bad_alloc&) {
    grp->err = "out of host memory";
    return E_NOMEM;
  }
  std::atomic<size_t> next{0};
  const std::function<void()> work = [&]() {
    const int64_t t0 = thread_cpu_ns();
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= pieces.size()) break;
      stream_copy(pieces[k].to, pieces[k].from, pieces[k].n);
    }
    grp->cpu_ns[0] += thread_cpu_ns() - t0;
  };
  int32_t t = threads < 1 ? 1 : threads;
  if ((size_t)t > pieces.size()) t = (int32_t)(pieces.size() ? pieces.size() : 1);
  grp->pool.run(work, t - 1);
  return OK;
}

int32_t surge_ingest_group_feed(surge_ingest_group* grp, const uint8_t* const* data, const int64_t* len, int32_t threads, int64_t* consumed_out,
                                int64_t max_sections, surge_batch_section* sections_out, int64_t* n_sections_out, const uint8_t** slab_out) {
  if (!grp || !data || !len || !n_sections_out || !slab_out || max_sections < 0 || (!sections_out && max_sections > 0)) return fail(nullptr, E_INVALID, "bad argument");
  const int32_t n = (int32_t)grp->g.size();
  *n_sections_out = 0;
  *slab_out = nullptr;
  grp->floors.clear();
  if (consumed_out) std::memset(consumed_out, 0, sizeof(int64_t) * (size_t)n);
  for (int32_t p = 0; p < n; ++p)
    if (len[p] < 0 || (!data[p] && len[p] > 0)) { grp->err = "bad buffer for partition " + std::to_string(p); return E_INVALID; }
  const int group_cur = grp->cur, group_next = (group_cur + 1) % surge_ingest::kArenas;
  const bool inplace = received_in_place(grp, data, len);
  grp->recv_slab = -1;
  Arena& slab = grp->slabs[group_next];
  auto undo = [&]() {
    for (int32_t p = 0; p < n; ++p) {
      grp->saved[(size_t)p].restore(*grp->g[(size_t)p]);
      grp->drained[(size_t)p].clear();
    }
    grp->cur = group_cur;
    if (inplace) grp->recv_slab = group_next;  // (the received bytes are still there: the caller may feed them again)
    if (consumed_out) std::memset(consumed_out, 0, sizeof(int64_t) * (size_t)n);
  };
  // Every partition's slice: what it still holds (open transactions, batches not drained yet) + this feed.  With
  // SURGE_INGEST_DEVICE_LZ4 a section is never longer than its batch; without it the host decompresses lz4 batches INTO the
  // slice, whose size is then only known afterwards: the feed is undone and run again with `expand` times the room.
  // (the trial starts from the factor the last feed needed, not from 1: a group without SURGE_INGEST_DEVICE_LZ4 on a compressed
  // topic otherwise framed — CRC, decompression and all — every fetch two or three times over, for ever; the factor is capped
  // at 256: an LZ4 block expands at most 255 x)
  for (int64_t expand = grp->expand_hint;; expand *= 4) {
    const int32_t rc = prepare_slab(grp, slab, len, inplace, expand);
    if (rc != OK) return rc;
    grp->cur = group_next;
    frame_partitions(grp, slab.data(), data, len, threads, inplace);
    int32_t first_bad = OK;
    bool overflow = false;
    int64_t need = 0;
    for (int32_t p = 0; p < n; ++p) {
      overflow |= grp->g[(size_t)p]->slice_overflow;
      need += (int64_t)grp->drained[(size_t)p].size();
      if (grp->status[(size_t)p] != OK && first_bad == OK) {
        first_bad = grp->status[(size_t)p];
        grp->err = "partition " + std::to_string(p) + ": " + grp->g[(size_t)p]->err;
      }
    }
    if (overflow && expand < 256) {
      undo();
      continue;
    }
    if (first_bad != OK) {
      undo();
      return first_bad;
    }
    grp->expand_hint = expand;
    if (need > max_sections) {
      undo();
      *n_sections_out = need;
      grp->err = "sections_out is too small: this feed delivers " + std::to_string(need) + " sections (n_sections_out; the feed was undone — call again with room for them)";
      return E_INVALID;
    }
    int64_t at = 0;
    for (int32_t p = 0; p < n; ++p) {
      for (const surge_batch_section& sct : grp->drained[(size_t)p]) {
        if (sct.codec & SURGE_SECTION_FLOORED) grp->floors.push_back(surge_section_floor{p, 0, at, grp->g[(size_t)p]->start.first});
        sections_out[at++] = sct;
      }
      if (consumed_out) consumed_out[p] = grp->consumed[(size_t)p];
    }
    *n_sections_out = at;
    *slab_out = slab.data();
    return OK;
  }
}

int32_t surge_ingest_group_counters(const surge_ingest_group* grp, int64_t out[8]) {
  if (!grp || !out) return E_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  for (const surge_ingest* x : grp->g)
    for (int i = 0; i < 8; ++i) out[i] += x->counters[i];
  return OK;
}

int64_t surge_ingest_key_count(const surge_ingest* g) { return g ? (int64_t)g->keys.size() : 0; }

int32_t surge_ingest_key(const surge_ingest* g, int64_t idx, const char** utf8_out, int64_t* len_out) {
  if (!g || !utf8_out || !len_out) return fail(nullptr, E_INVALID, "bad argument");
  if (idx < 0 || idx >= (int64_t)g->keys.size()) return E_INVALID;
  *utf8_out = g->keys[(size_t)idx].data();
  *len_out = (int64_t)g->keys[(size_t)idx].size();
  return OK;
}

int32_t surge_ingest_counters(const surge_ingest* g, int64_t out[8]) {
  if (!g || !out) return E_INVALID;
  for (int i = 0; i < 8; ++i) out[i] = g->counters[i];
  return OK;
}

}  // extern "C"

#include "ingest_start.h"  // start offsets, floors and positions: the exports (what they read is above)
