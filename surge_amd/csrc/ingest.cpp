// ingest.cpp — events-topic ingest, host side of libsurge_replay.so: the single-partition framer (surge_ingest_*).
// Kafka RecordBatch v2 + read_committed, restated from the published formats (kafka-clients 3.2.3 is not vendored with the
// reference: parity unpinned, see include/surge_ingest.h).  The LZ4 frames of compressed batches are read by lz4_frame.cpp, the
// CRC-32C is crc32c.cpp's; a consumer's partitions framed as one unit are ingest_group.cpp's (what the units share: ingest_internal.h).
#include <atomic>
#include <thread>

#include "ingest_internal.h"
#include "snappy_block.h"

using namespace surge::ingest::framer;

static thread_local std::string g_err;  // the calling thread's last message (surge_ingest_last_error(NULL))

int32_t surge::ingest::framer::fail(surge_ingest* g, int32_t code, const std::string& m) {
  if (g) g->err = m;
  g_err = m;
  return code;
}

namespace {

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

// The aggregate id a record is interned under: its key up to the first ':' (PartitionStringUpToColon)
inline size_t aggregate_id_len(const uint8_t* key, int32_t len) {
  size_t n = 0;
  while (n < (size_t)len && key[n] != (uint8_t)':') ++n;
  return n;
}

int64_t intern(surge_ingest* g, const uint8_t* key, int32_t len) {
  const size_t n = aggregate_id_len(key, len);
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
  const surge_ingest::Start& st = g->start;
  bool live = st.live();
  for (const Batch& b : g->queue) {
    if (b.decided == 0) break;  // an open transaction: nothing behind it is stable yet
    if (b.decided != 1) continue;
    if (!live) {
      n += b.sect_off >= 0 ? (int64_t)b.count : (int64_t)(b.recs.size() - b.next);
      continue;
    }
    // below the start nothing is deliverable (of a section that straddles it the device decides: all of it counts)
    if (b.sect_off >= 0) n += st.below(b) ? 0 : (int64_t)b.count;
    else for (size_t i = b.next; i < b.recs.size(); ++i) n += !st.below(b.recs[i].offset);
    live = st.below(b);
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
      if (g->start.live() && g->start.below(h.base_offset + offset_delta)) {  // below the start it is dropped like any record
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
        if (live && st.below(b.recs[i].offset)) {
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
        if (!st.below(b)) live = false;
        else if (kPop) st.discarded_batches += 1;
      }
    }
    if (!kPop) ++at;
    else if (b.decided == 2 || b.next == b.recs.size()) g->queue.pop_front();
  }
  if (kPop && !live) st.passed = st.first > 0;
  return n;
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
    next.reserve((size_t)g->queued_section_bytes() + (size_t)feed_len);
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

// A snappy batch's records section (snappy_block.h: framed chunks or one raw block), decompressed on the host into g->scratch.
// The preambles say what it holds before a byte is decoded, so there is no guess to grow; a refusal is worded by the header.
int32_t host_snappy(surge_ingest* g, const uint8_t** recs, int64_t* recs_len) {
  namespace sn = surge::snappy;
  int64_t total = 0, got = 0;
  sn::Status st = sn::frame_bound(*recs, *recs_len, &total);
  if (st == sn::SN_OK) {
    g->scratch.resize((size_t)total + 16);
    st = sn::frame_decompress(*recs, *recs_len, g->scratch.data(), total, &got);
  }
  if (st != sn::SN_OK) {
    const char* why = sn::status_name(st);
    return fail(g, SURGE_E_CORRUPT, why);
  }
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
  // at least 7 bytes, and LZ4 expands at most 255 x — a snappy element less: 64 bytes from a 3-byte copy)
  if (defer_crc && (int64_t)h.count > (h.recs_len / 7 + 1) * (h.codec() ? 255 : 1))
    return fail(g, SURGE_E_CORRUPT, "recordCount impossible for the batch's size (damaged header)");
  const uint8_t* recs = h.recs;
  int64_t recs_len = h.recs_len;
  int sect_codec = 0;
  const bool compressed = h.codec() == 3 || h.codec() == 2;  // lz4 (one frame) or snappy (chunks, or one raw block)
  if (compressed && g->device_lz4 && !h.control()) {
    sect_codec = h.codec();  // the section travels as it is: the device decoder walks its blocks / chunks and decodes them on the GPU
  } else if (compressed && g->inplace && !h.control()) {
    return fail(g, E_UNSUPPORTED, "an in-place feed leaves the sections where they were received: lz4 and snappy topics need SURGE_INGEST_DEVICE_LZ4");
  } else if (compressed) {
    const int32_t rc = h.codec() == 3 ? host_lz4(g, &recs, &recs_len) : host_snappy(g, &recs, &recs_len);
    if (rc != OK) return rc;
  } else if (h.codec() != 0) {
    return fail(g, E_UNSUPPORTED, "compression codec not supported (none, lz4 and snappy are read; gzip and zstd are not; the reference publishes lz4)");
  }
  Batch b;
  b.producer_id = h.producer_id;
  b.base_offset = h.base_offset;
  b.last_offset = h.base_offset + h.last_offset_delta;
  int control_type = -1;
  if (g->frames && !h.control()) {
    if (defer_crc && recs != h.recs) return fail(g, E_UNSUPPORTED, "SURGE_INGEST_DEVICE_CRC needs the sections to travel as they are on the wire (SURGE_INGEST_DEVICE_LZ4 for lz4 and snappy topics)");
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

// The offset a consumer resumes from: behind the last batch a feed took, in front of whatever the queue still holds to be
// delivered — an open transaction, committed batches not drained yet (aborted ones are already decided) — and never below
// the start.
int64_t surge::ingest::framer::position_of(const surge_ingest* g) {
  int64_t pos = g->start.next_offset < 0 ? 0 : g->start.next_offset;
  for (const Batch& b : g->queue) {
    if (b.decided == 2) continue;
    pos = (b.sect_off < 0 && b.next > 0 && b.next < b.recs.size()) ? b.recs[b.next].offset : b.base_offset;
    break;
  }
  return pos < g->start.first ? g->start.first : pos;
}

extern "C" {

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
  if (g->frames) return fail(g, E_STATE, kFramesOnly);
  return delivered(g, visit_ready<true>(g, max, [&](Rec& r, int64_t k) {
    out[k].offset = r.offset; out[k].agg_idx = deliver_idx(g, r); out[k].key_off = r.key_off; out[k].key_len = r.key_len;
    out[k].value_len = r.value_len; out[k].value_off = r.value_off;
    return true;
  }), n_out);
}

const uint8_t* surge_ingest_arena(const surge_ingest* g) { return g ? g->arena_now().data() : nullptr; }

int32_t surge_ingest_set_allocator(surge_ingest* g, void* (*alloc)(size_t), void (*release)(void*)) {
  if (!g || !alloc != !release) return fail(g, E_INVALID, "bad argument");
  if (!Arena::set_allocator(g->arenas, g->arenas + surge_ingest::kArenas, alloc, release)) return fail(g, E_STATE, "surge_ingest_set_allocator after the first feed");
  return OK;
}

// The two drains below are all or nothing: a first walk looks at (decodes) what the call would deliver and pops nothing, so a
// value that is refused leaves the queue as it was; the second walk delivers.
int32_t surge_ingest_drain_fixed16(surge_ingest* g, int64_t max, int64_t* agg_idx_out, void* events16_out,
                                   int64_t* offsets_out, int64_t* n_out) {
  if (!g || !n_out || max < 0 || ((!agg_idx_out || !events16_out) && max > 0)) return fail(g, E_INVALID, "bad argument");
  if (g->frames) return fail(g, E_STATE, kFramesOnly);
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
  if (g->frames) return fail(g, E_STATE, kFramesOnly);
  if (surge_event_json_validate(tmpl) != 0) return fail(g, E_INVALID, std::string("event template: ") + surge_event_json_last_error());
  uint8_t* ev = (uint8_t*)events16_out;
  int32_t refused = OK;
  auto decode_keyed = [&](const Rec& r, uint8_t* out) {  // an enveloped value names its aggregate: the id the record is interned under (the key up to ':')
    const uint8_t* key = g->arena_now().data() + r.key_off;
    return surge_event_json_decode_keyed(tmpl, key, (int64_t)aggregate_id_len(key, r.key_len), g->arena_now().data() + r.value_off, r.value_len, out);
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
  if (!g->frames) return fail(g, E_STATE, "surge_ingest_drain_sections needs a decoder created with SURGE_INGEST_FRAMES");
  int64_t n = 0, recs = 0;
  surge_ingest::Start& st = g->start;
  st.floored_section = -1;
  while (n < max_sections && !g->queue.empty()) {
    Batch& b = g->queue.front();
    if (b.decided == 0) break;  // an open transaction: nothing behind it is stable yet
    if (b.decided == 1 && st.live() && st.below(b)) {  // below the start as a whole: never handed out
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
        if (st.straddled_by(b)) {
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

// ---- start offsets, floors and positions: the exports.  What a start offset DOES is above, where batches are handed out:
// surge_ingest::Start's predicates in visit_ready, ready_count, parse_records' flush record and surge_ingest_drain_sections.
int32_t surge_ingest_set_start_offset(surge_ingest* g, int64_t first_offset) {
  if (!g) return fail(nullptr, E_INVALID, "handle is NULL");
  if (g->start.fed) return fail(g, E_STATE, "surge_ingest_set_start_offset after the first feed");
  g->start.first = first_offset > 0 ? first_offset : 0;
  return OK;
}

int64_t surge_ingest_position(const surge_ingest* g) { return g ? position_of(g) : 0; }

int32_t surge_ingest_take_floors(surge_ingest* g, int64_t max, surge_section_floor* out, int64_t* n_out) {
  if (!g || !n_out || max < 0 || (!out && max > 0)) return fail(g, E_INVALID, "bad argument");
  *n_out = g->start.floored_section >= 0 ? 1 : 0;
  if (*n_out > max) return fail(g, E_INVALID, "floors table too small (n_out entries are needed)");
  if (*n_out) out[0] = surge_section_floor{0, 0, g->start.floored_section, g->start.first};
  return OK;
}

int32_t surge_ingest_below_start(const surge_ingest* g, int64_t out[2]) {
  if (!g || !out) return E_INVALID;
  out[0] = g->start.discarded_batches;
  out[1] = g->start.dropped_records;
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
  for (int i = 0; i < C_COUNT; ++i) out[i] = g->counters[i];
  return OK;
}

}  // extern "C"
