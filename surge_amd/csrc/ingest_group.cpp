// ingest_group.cpp — surge_ingest_group (include/surge_ingest.h): a consumer's partitions framed as ONE unit, one FRAMES framer
// (ingest.cpp) per partition.  Every feed lays the partitions' records sections out in one slab — the group rotates through
// six, like a single framer's arenas — so a fetch response reaches the device in one copy.  A member is fed and drained through
// surge_ingest_feed / surge_ingest_drain_sections; what else the group touches of it is in ingest_internal.h.
//
// Threads: the group keeps a POOL of framing threads for its lifetime (started at the first feed that asks for them;
// a feed hands them one job and takes part in it itself) — a consumer feeds every couple of milliseconds, and creating
// and joining seven threads per feed cost more than some feeds' framing.
//
// Failure: a feed either frames every partition or leaves the group exactly as it was.  What a member's feed changes —
// its queue (open transactions move to the new slice), its counters, which arena is current — is saved before the feed
// (a FRAMES queue holds only the few batches of open transactions: cheap) and put back when any partition fails or the
// caller's section table is too small; the slab the failed feed wrote into is the one the next feed writes into again.
#include <pthread.h>
#include <time.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#endif

#include "ingest_internal.h"

using namespace surge::ingest::framer;

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

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"  // (as for surge_ingest)
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
#pragma GCC diagnostic pop

namespace {

// The group's fail(): its own text only (the calling thread's, surge_ingest_group_last_error(NULL), stays what it was)
int32_t fail_group(surge_ingest_group* grp, int32_t code, const std::string& m) {
  grp->err = m;
  return code;
}

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
    total = (total + grp->g[p]->queued_section_bytes() + (bytes ? bytes[p] * times : 0) + 15) & ~15ll;
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
  return fail_group(grp, E_NOMEM, "out of host memory for the group's slab");
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

// What a receive copy and a feed are given: per partition a length and, where it is not 0, bytes.  Their sum, or -1 with the group's message set.
int64_t buffers_total(surge_ingest_group* grp, const uint8_t* const* data, const int64_t* len) {
  int64_t total = 0;
  for (size_t p = 0; p < grp->g.size(); ++p) {
    if (len[p] < 0 || (!data[p] && len[p] > 0)) return fail_group(grp, -1, "bad buffer for partition " + std::to_string(p));
    total += len[p];
  }
  return total;
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
    return fail_group(grp, E_NOMEM, "out of host memory");
  }
  const int64_t total = lay_out_slices(grp, inplace ? nullptr : len, expand, grp->off.data());
  if (inplace) {
    if (total <= grp->recv_carry) return OK;  // (always: nothing was fed between receive_buffer and this call)
    return fail_group(grp, E_INVALID, "the partitions' carried sections outgrew the room surge_ingest_group_receive_buffer left for them");
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

const char* surge_ingest_group_last_error(const surge_ingest_group* grp) { return grp ? grp->err.c_str() : surge_ingest_last_error(nullptr); }

int32_t surge_ingest_group_set_allocator(surge_ingest_group* grp, void* (*alloc)(size_t), void (*release)(void*)) {
  if (!grp || !alloc != !release) return fail(nullptr, E_INVALID, "bad argument");  // pinned: the group's own text stays what it was
  if (!Arena::set_allocator(grp->slabs, grp->slabs + surge_ingest::kArenas, alloc, release)) return fail_group(grp, E_STATE, "surge_ingest_group_set_allocator after the first feed");
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
  if (!grp || !buf_out || bytes < 0) return fail(nullptr, E_INVALID, "bad argument");  // pinned: the group's own text stays what it was
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
  if (!grp || !data || !len || !placed_out) return fail(nullptr, E_INVALID, "bad argument");  // pinned: the group's own text stays what it was
  const int32_t n = (int32_t)grp->g.size();
  const int64_t total = buffers_total(grp, data, len);
  if (total < 0) return E_INVALID;
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
    return fail_group(grp, E_NOMEM, "out of host memory");
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
  if (!grp || !data || !len || !n_sections_out || !slab_out || max_sections < 0 || (!sections_out && max_sections > 0)) return fail(nullptr, E_INVALID, "bad argument");  // pinned: the group's own text stays what it was
  const int32_t n = (int32_t)grp->g.size();
  *n_sections_out = 0;
  *slab_out = nullptr;
  grp->floors.clear();
  if (consumed_out) std::memset(consumed_out, 0, sizeof(int64_t) * (size_t)n);
  if (buffers_total(grp, data, len) < 0) return E_INVALID;
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
  // at 256: an LZ4 block expands at most 255 x, and a snappy block less — its densest element is a 3-byte copy of 64 bytes,
  // under 22 x — so the same cap covers a group on a snappy topic)
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
      return fail_group(grp, E_INVALID, "sections_out is too small: this feed delivers " + std::to_string(need) + " sections (n_sections_out; the feed was undone — call again with room for them)");
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
  for (int i = 0; i < C_COUNT; ++i) out[i] = 0;
  for (const surge_ingest* x : grp->g)
    for (int i = 0; i < C_COUNT; ++i) out[i] += x->counters[i];
  return OK;
}

// ---- start offsets, floors and positions for a group: one entry per partition (the floors of a feed are collected in surge_ingest_group_feed)
int32_t surge_ingest_group_set_start_offsets(surge_ingest_group* grp, const int64_t* first_offset) {
  if (!grp || !first_offset) return fail(nullptr, E_INVALID, "bad argument");  // pinned: the group's own text stays what it was
  for (const surge_ingest* x : grp->g)
    if (x->start.fed) return fail_group(grp, E_STATE, "surge_ingest_group_set_start_offsets after the first feed");
  for (size_t p = 0; p < grp->g.size(); ++p) grp->g[p]->start.first = first_offset[p] > 0 ? first_offset[p] : 0;
  return OK;
}

int32_t surge_ingest_group_positions(const surge_ingest_group* grp, int64_t* out) {
  if (!grp || !out) return E_INVALID;
  for (size_t p = 0; p < grp->g.size(); ++p) out[p] = position_of(grp->g[p]);
  return OK;
}

int32_t surge_ingest_group_take_floors(surge_ingest_group* grp, int64_t max, surge_section_floor* out, int64_t* n_out) {
  if (!grp || !n_out || max < 0 || (!out && max > 0)) return fail(nullptr, E_INVALID, "bad argument");  // pinned: the group's own text stays what it was
  *n_out = (int64_t)grp->floors.size();
  if (*n_out > max) return fail_group(grp, E_INVALID, "floors table too small (n_out entries are needed)");
  for (size_t i = 0; i < grp->floors.size(); ++i) out[i] = grp->floors[i];
  return OK;
}

int32_t surge_ingest_group_below_start(const surge_ingest_group* grp, int64_t out[2]) {
  if (!grp || !out) return E_INVALID;
  out[0] = out[1] = 0;
  for (const surge_ingest* x : grp->g) {
    out[0] += x->start.discarded_batches;
    out[1] += x->start.dropped_records;
  }
  return OK;
}

}  // extern "C"
