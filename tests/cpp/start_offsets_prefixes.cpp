// start_offsets_prefixes.cpp — the host framer's start offsets, floors list and positions (surge_amd/csrc/ingest.cpp, ingest_group.cpp:
// surge_ingest_set_start_offset, _take_floors, _position, _below_start and the group's forms) under -fsanitize=address,undefined.
// A small topic that straddles every kind of start — batches of 1, 2 and 7 records, a compaction gap, a flush record, a committed
// and an aborted transaction, uncompressed and lz4 — is fed as every prefix of its bytes (each in a malloc of EXACTLY its length,
// so one byte too far is a heap-buffer-overflow report) and as seeded mutations with the batches' CRCs made good again, with every
// start the cases of tests/test_start_offsets.py name; through the host drains, the FRAMES drain and a group.  What must hold
// whatever the bytes: no delivered offset below the start, offsets ascending, at most one floored section and the floors list
// naming exactly it, the position never below the start.  Built and run stand-alone by tests/test_start_offsets.py; never loaded
// into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "surge_ingest.h"

namespace {

std::string varint(int64_t v) {
  uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
  std::string out;
  while (z >= 0x80) { out.push_back((char)((z & 0x7F) | 0x80)); z >>= 7; }
  out.push_back((char)z);
  return out;
}

void be(std::string& s, uint64_t v, int bytes) {
  for (int i = bytes - 1; i >= 0; --i) s.push_back((char)((v >> (8 * i)) & 0xff));
}

std::string record(int64_t delta, const std::string& key, const std::string& value) {
  std::string body;
  body.push_back(0);
  body += varint(0) + varint(delta) + varint((int64_t)key.size()) + key + varint((int64_t)value.size()) + value + varint(0);
  return varint((int64_t)body.size()) + body;
}

struct Rec { int64_t delta; std::string key, value; };

void seal(std::string& batch) {  // the CRC-32C over attributes .. end, into its field
  const uint32_t crc = surge_crc32c((const uint8_t*)batch.data() + 21, (int64_t)batch.size() - 21);
  for (int i = 0; i < 4; ++i) batch[17 + i] = (char)((crc >> (8 * (3 - i))) & 0xff);
}

std::string batch(int64_t base, const std::vector<Rec>& recs, int32_t last_delta, bool lz4, int64_t pid, bool control) {
  std::string body;
  for (const Rec& r : recs) body += record(r.delta, r.key, r.value);
  if (lz4) {
    std::vector<uint8_t> frame((size_t)surge_lz4_frame_bound((int64_t)body.size()));
    const int64_t n = surge_lz4_frame_compress((const uint8_t*)body.data(), (int64_t)body.size(), frame.data(), (int64_t)frame.size());
    if (n < 0) { std::printf("FAIL: lz4 writer\n"); std::exit(1); }
    body.assign((const char*)frame.data(), (size_t)n);
  }
  std::string b;
  be(b, (uint64_t)base, 8);
  be(b, (uint64_t)(49 + body.size()), 4);
  be(b, 0, 4);  // partitionLeaderEpoch
  b.push_back(2);
  be(b, 0, 4);  // crc
  be(b, (uint64_t)((lz4 ? 3 : 0) | (pid >= 0 ? 0x10 : 0) | (control ? 0x20 : 0)), 2);
  be(b, (uint64_t)(uint32_t)last_delta, 4);
  be(b, 0, 8);
  be(b, 0, 8);
  be(b, (uint64_t)pid, 8);
  be(b, 0, 2);
  be(b, (uint64_t)(uint32_t)-1, 4);
  be(b, (uint64_t)recs.size(), 4);
  b += body;
  seal(b);
  return b;
}

std::string marker(int64_t offset, int64_t pid, int commit) {
  std::string key, value;
  be(key, 0, 2); be(key, (uint64_t)commit, 2);
  be(value, 0, 2); be(value, 0, 4);
  return batch(offset, {Rec{0, key, value}}, 0, false, pid, true);
}

std::string ev16(uint32_t seq) {
  std::string v(16, '\0');
  v[0] = 1;
  std::memcpy(&v[4], &seq, 4);
  return v;
}

struct Topic {
  std::string bytes;
  std::vector<size_t> batch_at;  // where each batch begins
  int64_t end = 0;
};

Topic make_topic(bool lz4) {
  Topic t;
  auto add = [&](const std::string& b) { t.batch_at.push_back(t.bytes.size()); t.bytes += b; };
  auto recs = [&](int64_t base, int n, int gone_a = -1, int gone_b = -1) {
    std::vector<Rec> out;
    for (int d = 0; d < n; ++d)
      if (d != gone_a && d != gone_b) out.push_back(Rec{d, "agg-" + std::to_string((base + d) % 5) + ":" + std::to_string(base + d), ev16((uint32_t)(base + d))});
    return out;
  };
  add(batch(0, recs(0, 1), 0, lz4, -1, false));
  add(batch(1, recs(1, 2), 1, lz4, -1, false));
  std::vector<Rec> seven = recs(3, 7, 3, 6);  // offsets 3 .. 9; 6 and 9 are gone (compaction)
  seven[1] = Rec{1, "", ""};                  // the flush record, offset 4
  add(batch(3, seven, 6, lz4, -1, false));
  add(batch(10, recs(10, 7), 6, lz4, 7, false));  // a committed transaction of two batches: 10 .. 18, marker 19
  add(batch(17, recs(17, 2), 1, lz4, 7, false));
  add(marker(19, 7, 1));
  add(batch(20, recs(20, 2), 1, lz4, 8, false));  // an aborted one: 20 .. 22, marker 23
  add(batch(22, recs(22, 1), 0, lz4, 8, false));
  add(marker(23, 8, 0));
  add(batch(24, recs(24, 7), 6, lz4, -1, false));
  t.end = 31;
  return t;
}

int64_t g_cases = 0, g_delivered = 0;
bool g_strict = true;  // the topic is the writer's: offsets ascend (a mutated one may run them backwards, where a floor that has been passed stays inert)

#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    if (!(cond)) { std::printf("FAIL %s:%d: %s (start %lld, len %zu)\n", __FILE__, __LINE__, #cond, (long long)start, len); std::exit(1); } \
  } while (0)

surge_event_json_template no_type_template() {
  surge_event_json_template t;
  std::memset(&t, 0, sizeof(t));
  t.n_types = 1;
  t.types[0].event_type = 1;
  return t;
}

// one buffer, one start, one way of draining: mode 0 drain, 1 drain_fixed16, 2 drain_json, 3 FRAMES sections, 4 FRAMES | DEVICE_LZ4 | DEVICE_CRC
void run_single(const uint8_t* data, size_t len, int64_t start, int mode, size_t cut) {
  ++g_cases;
  surge_ingest* g = nullptr;
  const int32_t flags = mode == 3 ? SURGE_INGEST_FRAMES : mode == 4 ? (SURGE_INGEST_FRAMES | SURGE_INGEST_DEVICE_LZ4 | SURGE_INGEST_DEVICE_CRC) : 0;
  REQUIRE(surge_ingest_create(SURGE_INGEST_READ_COMMITTED | flags, &g) == 0);
  REQUIRE(surge_ingest_set_start_offset(g, start) == 0);
  int64_t last = -1, floored = 0;
  size_t fed = 0;
  std::vector<uint8_t> carry;
  for (int round = 0; round < 2; ++round) {  // the buffer in two feeds, cut at `cut`: each piece in a malloc of exactly its length
    const size_t upto = round == 0 ? (cut < len ? cut : len) : len;
    std::vector<uint8_t> piece(carry);
    piece.insert(piece.end(), data + fed, data + upto);
    fed = upto;
    uint8_t* exact = (uint8_t*)std::malloc(piece.size() ? piece.size() : 1);
    if (!piece.empty()) std::memcpy(exact, piece.data(), piece.size());
    int64_t consumed = 0;
    const int32_t rc = surge_ingest_feed(g, exact, (int64_t)piece.size(), &consumed);
    REQUIRE(consumed >= 0 && (size_t)consumed <= piece.size());
    carry.assign(piece.begin() + consumed, piece.end());
    if (round == 0) REQUIRE(surge_ingest_set_start_offset(g, start) == -2);  // after the first feed: refused
    if (rc != 0) carry.clear();
    const int64_t ready = surge_ingest_ready(g);
    REQUIRE(ready >= 0);
    if (mode >= 3) {
      std::vector<surge_batch_section> secs(len / 61 + 2);  // (a batch is at least its 61-byte header; `ready` counts records, and a mutated recordCount is taken at its word here)
      int64_t n = 0;
      REQUIRE(surge_ingest_drain_sections(g, (int64_t)secs.size(), secs.data(), &n) == 0);
      surge_section_floor fl[2];
      int64_t n_fl = 0;
      REQUIRE(surge_ingest_take_floors(g, 2, fl, &n_fl) == 0 && n_fl <= 1);
      int64_t flagged = -1;
      for (int64_t i = 0; i < n; ++i) {
        REQUIRE(secs[i].byte_off >= 0 && secs[i].byte_len >= 0);
        if (secs[i].codec & SURGE_SECTION_FLOORED) { REQUIRE(flagged < 0); flagged = i; }
        (void)*(volatile const uint8_t*)(surge_ingest_arena(g) + secs[i].byte_off + (secs[i].byte_len ? secs[i].byte_len - 1 : 0));
      }
      REQUIRE((n_fl == 1) == (flagged >= 0));
      if (n_fl == 1) REQUIRE(fl[0].section == flagged && fl[0].first_offset == start && fl[0].part == 0 && secs[flagged].base_offset < start);
      floored += n_fl;
      g_delivered += n;
    } else if (mode == 0) {
      std::vector<surge_ingest_record> out((size_t)ready + 1);
      int64_t n = 0;
      REQUIRE(surge_ingest_drain(g, ready, out.data(), &n) == 0 && n == ready);
      for (int64_t i = 0; i < n; ++i) {
        if (g_strict) REQUIRE(out[i].offset > last && (start <= 0 || out[i].offset >= start));
        last = out[i].offset;
      }
      g_delivered += n;
    } else {
      std::vector<int64_t> agg((size_t)ready + 1), off((size_t)ready + 1);
      std::vector<uint8_t> ev(((size_t)ready + 1) * 16);
      int64_t n = 0;
      const surge_event_json_template tmpl = no_type_template();
      const int32_t drc = mode == 1 ? surge_ingest_drain_fixed16(g, ready, agg.data(), ev.data(), off.data(), &n)
                                    : surge_ingest_drain_json(g, ready, &tmpl, agg.data(), ev.data(), off.data(), &n);
      if (drc == 0) {
        REQUIRE(n == ready);
        for (int64_t i = 0; i < n; ++i) REQUIRE(!g_strict || start <= 0 || off[i] >= start);
        g_delivered += n;
      }
    }
    std::free(exact);
    const int64_t pos = surge_ingest_position(g);
    REQUIRE(pos >= 0 && (start <= 0 || pos >= start));
  }
  REQUIRE(floored <= 1);
  int64_t below[2] = {-1, -1};
  REQUIRE(surge_ingest_below_start(g, below) == 0 && below[0] >= 0 && below[1] >= 0);
  if (start <= 0) REQUIRE(below[0] == 0 && below[1] == 0);
  surge_ingest_destroy(g);
}

// the same buffer as two partitions of a group with two different starts
void run_group(const uint8_t* data, size_t len, int64_t start) {
  ++g_cases;
  surge_ingest_group* grp = nullptr;
  REQUIRE(surge_ingest_group_create(2, SURGE_INGEST_READ_COMMITTED | SURGE_INGEST_DEVICE_LZ4, &grp) == 0);
  const int64_t starts[2] = {start, 0};
  REQUIRE(surge_ingest_group_set_start_offsets(grp, starts) == 0);
  uint8_t* exact = (uint8_t*)std::malloc(len ? len : 1);
  std::memcpy(exact, data, len);
  const uint8_t* parts[2] = {exact, exact};
  const int64_t lens[2] = {(int64_t)len, (int64_t)len};
  std::vector<surge_batch_section> secs(len / 61 * 2 + 4);
  int64_t consumed[2], n = 0;
  const uint8_t* slab = nullptr;
  const int32_t rc = surge_ingest_group_feed(grp, parts, lens, 2, consumed, (int64_t)secs.size(), secs.data(), &n, &slab);
  surge_section_floor fl[2];
  int64_t n_fl = -1;
  REQUIRE(surge_ingest_group_take_floors(grp, 2, fl, &n_fl) == 0 && n_fl >= 0 && n_fl <= 1);
  if (rc == 0) {
    int64_t flagged = 0;
    for (int64_t i = 0; i < n; ++i) flagged += (secs[i].codec & SURGE_SECTION_FLOORED) ? 1 : 0;
    REQUIRE(flagged == n_fl);
    if (n_fl) REQUIRE(fl[0].part == 0 && fl[0].section >= 0 && fl[0].section < n && (secs[fl[0].section].codec & SURGE_SECTION_FLOORED) && fl[0].first_offset == start);
    REQUIRE(surge_ingest_group_set_start_offsets(grp, starts) == -2);
  } else {
    REQUIRE(n_fl == 0);  // a feed that fails is undone: no floors of it
  }
  int64_t pos[2] = {-1, -1}, below[2];
  REQUIRE(surge_ingest_group_positions(grp, pos) == 0 && pos[1] >= 0 && pos[0] >= (start > 0 ? start : 0));
  REQUIRE(surge_ingest_group_below_start(grp, below) == 0 && below[0] >= 0);
  std::free(exact);
  surge_ingest_group_destroy(grp);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

}  // namespace

int main() {
  const int64_t starts[] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 16, 17, 18, 19, 20, 21, 23, 24, 25, 30, 31, 400};
  for (int lz4 = 0; lz4 < 2; ++lz4) {
    g_strict = true;
    const Topic t = make_topic(lz4 != 0);
    const uint8_t* data = (const uint8_t*)t.bytes.data();
    const size_t n_starts = sizeof(starts) / sizeof(starts[0]);
    // every prefix — a fetch that cuts the topic anywhere: the cut batch waits for more bytes — each with three of the starts and two
    // of the drains in turn; then every start with every drain over the whole topic, fed in two pieces cut at and inside every batch
    for (size_t len = 0; len <= t.bytes.size(); ++len)
      for (size_t k = 0; k < 3; ++k) run_single(data, len, starts[(len + 7 * k) % n_starts], (int)((len + k) % 5), len / 2);
    for (int64_t start : starts) {
      const size_t len = t.bytes.size();
      for (int m = 0; m < 5; ++m)
        for (size_t at : t.batch_at) { run_single(data, len, start, m, at); run_single(data, len, start, m, at + 30); }
      for (size_t at : t.batch_at) run_group(data, at, start);
      run_group(data, len, start);
    }
    // the whole topic delivers what the writer wrote from the start on (uncompressed and lz4 alike)
    for (int64_t start : starts) {
      surge_ingest* g = nullptr;
      surge_ingest_create(SURGE_INGEST_READ_COMMITTED, &g);
      surge_ingest_set_start_offset(g, start);
      int64_t consumed = 0;
      size_t len = t.bytes.size();
      REQUIRE(surge_ingest_feed(g, data, (int64_t)len, &consumed) == 0);
      surge_ingest_record out[64];
      int64_t n = 0;
      REQUIRE(surge_ingest_drain(g, 64, out, &n) == 0);
      int64_t want = 0;
      const int64_t offs[] = {0, 1, 2, 3, 5, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 24, 25, 26, 27, 28, 29, 30};  // no flush (4), no gaps (6, 9), nothing aborted
      for (int64_t o : offs) {
        if (o < start) continue;
        REQUIRE(want < n && out[want].offset == o);
        ++want;
      }
      REQUIRE(n == want && surge_ingest_position(g) == (start > t.end ? start : t.end));
      surge_ingest_destroy(g);
    }
    g_strict = false;
    // seeded mutations: bytes of the headers and record sections the framer branches on, the CRCs made good again
    for (int k = 0; k < 4000; ++k) {
      std::string m = t.bytes;
      const int edits = 1 + (int)(rnd() % 3);
      for (int e = 0; e < edits; ++e) {
        const size_t b = rnd() % t.batch_at.size();
        const size_t lo = t.batch_at[b], hi = b + 1 < t.batch_at.size() ? t.batch_at[b + 1] : m.size();
        const uint32_t what = rnd() % 4;
        size_t at = what == 0 ? lo + rnd() % 8             // baseOffset
                    : what == 1 ? lo + 21 + rnd() % 6      // attributes, lastOffsetDelta
                    : what == 2 ? lo + 57 + rnd() % 4      // recordCount
                                : lo + 61 + rnd() % (hi - lo - 61);  // the records
        m[at] = (char)(what == 0 ? rnd() % 64 : rnd());
      }
      for (size_t b = 0; b < t.batch_at.size(); ++b) {
        const size_t lo = t.batch_at[b], hi = b + 1 < t.batch_at.size() ? t.batch_at[b + 1] : m.size();
        std::string one = m.substr(lo, hi - lo);
        seal(one);
        m.replace(lo, hi - lo, one);
      }
      const int64_t start = starts[rnd() % (sizeof(starts) / sizeof(starts[0]))];
      size_t len = m.size();
      run_single((const uint8_t*)m.data(), len, start, (int)(rnd() % 5), rnd() % len);
      if (k % 8 == 0) run_group((const uint8_t*)m.data(), len, start);
    }
  }
  std::printf("PASS: %lld cases, %lld records / sections delivered\n", (long long)g_cases, (long long)g_delivered);
  return 0;
}
