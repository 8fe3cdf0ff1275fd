// ingest_intern.hip — the device decoder's interning stage: aggregate ids -> dense indices, and the compaction of the delivered
// records into the result arrays.
//   probe      one thread per record: open-addressing insert-or-find by hash (atomicCAS); a NEW slot remembers its first record
//   flag       one thread per record: key bytes compared with what the slot stands for (a 64-bit hash collision is detected,
//              not trusted); the first record of every new key and the delivered records are flagged
//   scans      (rocPRIM) the new keys' ids in first-delivered order — the host decoder's order — and arena offsets; the
//              delivered records' positions in the result arrays
//   assign     the new keys' bytes to the device key arena, their ids into their slots
//   finalize   one thread per delivered record: aggregate index from its slot, event and offset to the result arrays
//   (state mode) value scan + value gather: the delivered records' value bytes out of the push's bytes into one buffer
//   lookup     (no push in flight) one thread per queried id: find only — the table is read, never written
// The control flow around these — the retry after a collision, what is checked before anything is committed, the commit order —
// is stage 2 of the decoder (ingest_stage2.hip); this unit launches what it is told to.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ingest_device.h"

namespace surge {
namespace ingest {
namespace {

__global__ void table_clear_kernel(TableSlot* __restrict__ s, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ((uint4*)s)[i] = make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu);
}

// n bytes at a == n bytes at b?  Sixteen bytes a round, every load of a round in flight at once (the first version compared
// byte by byte and stopped at the first difference: two dependent single-byte loads per byte — 110 us per 10^6 records on
// 13-byte ids, 550 us on 36-byte UUIDs, profiles/r06_e2e_*_depth1_kernel_stats.csv).  Reads at most 7 bytes past either end
// (the staged bytes and the key arena both end 16 bytes after their last byte).
__device__ __forceinline__ bool keys_equal(const uint8_t* a, const uint8_t* b, int n) {
  uint32_t diff = 0u;
  for (int i = 0; i < n; i += 16) {
    uint32_t x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int left = n - i - 4 * k;
      x[k] = left > 0 ? load4(a + i + 4 * k) ^ load4(b + i + 4 * k) : 0u;
      if (left < 4 && left > 0) x[k] &= (1u << (8 * left)) - 1u;
    }
    diff |= x[0] | x[1] | x[2] | x[3];
  }
  return diff == 0u;
}

// insert-or-find by hash; a slot this push inserts remembers its first record
__global__ void probe_kernel(RecMeta* __restrict__ meta, int64_t n_rec, Table t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec) return;
  if (meta[i].status != RS_OK) return;
  const unsigned long long h = meta[i].hash;
  uint64_t s = h & t.mask;
  while (true) {
    const unsigned long long old = atomicCAS(&t.s[s].hash, 0ull, h);
    if (old == 0ull || old == h) break;
    s = (s + 1) & t.mask;
  }
  meta[i].slot = (uint32_t)s;
  if (t.s[s].key_id == 0xffffffffu) atomicMin(&t.s[s].first_rec, (uint32_t)i);
}

// Per record: is it the first record of a key this push discovers (those get the next ids, in record order: the host
// decoder's first-delivered numbering — an exclusive scan of the flags, no sort); does its key equal, byte for byte, the
// key its slot stands for (the key arena for a known key, the slot's first record for a new one): a 64-bit hash
// collision is detected here, before anything of the push is committed.  first[i] = flag << 40 | key length (scanned:
// id rank and arena offset in one pass); keep[i] = the record is delivered.
__global__ void flag_kernel(const RecMeta* __restrict__ meta, int64_t n_rec, const uint8_t* __restrict__ bytes, Table t, const uint8_t* __restrict__ arena,
                            const int64_t* __restrict__ key_off, unsigned long long* __restrict__ first, uint32_t* __restrict__ keep, ErrorCell* err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_rec) return;
  unsigned long long f = 0ull;
  uint32_t k = 0u;
  if (i < n_rec) {
    const RecMeta m = meta[i];
    if (m.status == RS_OK) {
      const uint32_t id = t.s[m.slot].key_id;
      const uint8_t* kp = bytes + m.key_off;
      bool same;
      if (id != 0xffffffffu) {
        const int64_t a0 = key_off[id], a1 = key_off[id + 1];
        same = a1 - a0 == m.key_len && keys_equal(arena + a0, kp, m.key_len);
      } else {
        const uint32_t fr = t.s[m.slot].first_rec;
        if ((int64_t)fr == i) {
          same = true;
          f = (1ull << 40) | (unsigned long long)(uint32_t)m.key_len;
        } else {
          const RecMeta o = meta[fr];
          const uint8_t* op = bytes + o.key_off;
          same = o.key_len == m.key_len && keys_equal(op, kp, m.key_len);
        }
      }
      if (same) k = 1u; else report(err, i, RS_COLLISION);
    }
  }
  first[i] = f;  // (entry n_rec = 0: the scans' totals land there)
  keep[i] = k;
}

// the keys this push discovered: id = n_keys + rank, bytes to the arena; their slots stop being "new"
__global__ void assign_kernel(const RecMeta* __restrict__ meta, int64_t n_rec, const uint8_t* __restrict__ bytes, const unsigned long long* __restrict__ first,
                              const unsigned long long* __restrict__ first_scan, int64_t n_keys, int64_t arena_base, Table t, uint8_t* __restrict__ arena,
                              int64_t* __restrict__ key_off, unsigned long long* __restrict__ key_hash) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec || first[i] == 0ull) return;
  const RecMeta m = meta[i];
  const unsigned long long sc = first_scan[i];
  const int64_t id = n_keys + (int64_t)(sc >> 40);
  const int64_t dst = arena_base + (int64_t)(sc & ((1ull << 40) - 1));
  for (int b = 0; b < m.key_len; ++b) arena[dst + b] = bytes[m.key_off + b];
  key_off[id + 1] = dst + m.key_len;
  key_hash[id] = m.hash;
  t.s[m.slot].key_id = (uint32_t)id;
  t.s[m.slot].first_rec = 0xffffffffu;
}

// delivered records -> the result arrays (aggregate index from the record's slot)
__global__ void finalize_kernel(const RecMeta* __restrict__ meta, int64_t n_rec, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, Table t,
                                const uint4* __restrict__ ev_tmp, int64_t out_base, int64_t* __restrict__ agg_out, uint4* __restrict__ ev_out,
                                int64_t* __restrict__ off_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec || !keep[i]) return;
  const int64_t o = out_base + pos[i];
  agg_out[o] = (int64_t)t.s[meta[i].slot].key_id;
  if (ev_out) ev_out[o] = ev_tmp[i];  // (state mode has no events: the values follow by value_gather_kernel)
  off_out[o] = meta[i].offset;
}

// a push that fails after its keys were probed takes them out again: slots it inserted go back to empty (they only ever
// occupied slots that were empty before, so the table is what it was)
__global__ void rollback_kernel(const RecMeta* __restrict__ meta, int64_t n_rec, Table t) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec || meta[i].status != RS_OK) return;
  const uint32_t s = meta[i].slot;
  if (t.s[s].key_id == 0xffffffffu) {
    t.s[s].hash = 0ull;
    t.s[s].first_rec = 0xffffffffu;
  }
}

__global__ void rehash_kernel(const unsigned long long* __restrict__ key_hash, int64_t n_keys, Table t) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_keys) return;
  const unsigned long long h = key_hash[id];
  uint64_t s = h & t.mask;
  // (two known keys that collide under a new seed share a hash and get two slots: lookups of the second then find the
  // first, flag_kernel reports the mismatch and the table is re-seeded once more)
  while (atomicCAS(&t.s[s].hash, 0ull, h) != 0ull) s = (s + 1) & t.mask;
  t.s[s].key_id = (uint32_t)id;
}

// after a re-seed: every known key's hash from its bytes in the arena, every record's from its key in the staged bytes
__global__ void rekey_keys_kernel(const uint8_t* __restrict__ arena, const int64_t* __restrict__ key_off, int64_t n_keys, uint64_t seed,
                                  unsigned long long* __restrict__ key_hash) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_keys) return;
  key_hash[id] = hash_key(arena + key_off[id], (int)(key_off[id + 1] - key_off[id]), seed);
}
__global__ void rekey_records_kernel(RecMeta* __restrict__ meta, int64_t n_rec, const uint8_t* __restrict__ bytes, uint64_t seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rec || meta[i].status != RS_OK) return;
  meta[i].hash = hash_key(bytes + meta[i].key_off, meta[i].key_len, seed);
}

// The read side of the table: query i = ids[id_off[i] .. id_off[i + 1]) -> its dense index, or -1.  One query per thread.  The id is
// hashed under the seed in use and probed linearly from its home slot, wrapping at the table's end: an empty slot ends the probe
// (a miss), a slot with the id's hash is compared with the arena — length, then bytes — and only byte equality is a hit; an
// equal hash over other bytes goes on probing (after a re-seed two known keys may share a hash and own two slots).  No atomics,
// no stores to the table: any number of lookups may run while no push is in flight.  The probe is bounded by the slot count, so
// it ends on any table; a query whose offsets do not describe a length in [0, 2^31) is a miss.
__global__ void __launch_bounds__(256) lookup_kernel(const uint8_t* __restrict__ ids, const int64_t* __restrict__ id_off, int64_t n, Table t, const uint8_t* __restrict__ arena,
                                                    const int64_t* __restrict__ key_off, uint64_t seed, int64_t* __restrict__ idx_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = id_off[i], len = id_off[i + 1] - o;
  int64_t found = -1;
  if (o >= 0 && len >= 0 && len < (1ll << 31)) {
    const uint8_t* p = ids + o;
    const unsigned long long h = hash_key(p, (int)len, seed);
    uint64_t s = h & t.mask;
    for (uint64_t step = 0; step <= t.mask; ++step) {
      const uint4 e = ((const uint4*)t.s)[s];  // one 16-byte load: {hash, key_id, first_rec}
      const unsigned long long eh = ((unsigned long long)e.y << 32) | e.x;
      if (eh == 0ull) break;
      if (eh == h && e.z != 0xffffffffu) {
        const int64_t a0 = key_off[e.z], a1 = key_off[e.z + 1];
        if (a1 - a0 == len && keys_equal(arena + a0, p, (int)len)) {
          found = (int64_t)e.z;
          break;
        }
      }
      s = (s + 1) & t.mask;
    }
  }
  idx_out[i] = found;
}

// ---- state mode: the delivered records' values -> one contiguous buffer --------------------------------------------------------
// A push's staged / decompressed bytes are written again by the slot's next push, so the values a state decoder keeps have to
// move: behind what earlier pushes delivered, one after the other in delivery order, value_off in front of each.

// vlen[i] = the bytes record i adds to the values (0 for a record that is not delivered, and for the closing entry n_rec)
__global__ void value_len_kernel(const RecMeta* __restrict__ meta, int64_t n_rec, const uint32_t* __restrict__ keep, unsigned long long* __restrict__ vlen) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_rec) return;
  vlen[i] = (i < n_rec && keep[i]) ? (unsigned long long)(uint32_t)meta[i].val_len : 0ull;
}

// per delivered record: where its value goes (value_off, absolute) and where it lies in the push's bytes (val_src, by position in the push)
__global__ void value_off_kernel(const RecMeta* __restrict__ meta, int64_t n_rec, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                                 const unsigned long long* __restrict__ vscan, int64_t out_base, int64_t val_base, int64_t* __restrict__ value_off,
                                 int64_t* __restrict__ val_src) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_rec) return;
  if (i == n_rec) { value_off[out_base + pos[n_rec]] = val_base + (int64_t)vscan[n_rec]; return; }  // (pos[n_rec] = records delivered)
  if (!keep[i]) return;
  value_off[out_base + pos[i]] = val_base + (int64_t)vscan[i];
  val_src[pos[i]] = meta[i].val_off;
}

// The gather.  The work is split by OUTPUT bytes: a workgroup owns a run of kGatherRecs consecutive delivered records — their
// output span [D0, D1) is contiguous — and its lanes take the span's aligned 16-byte pieces, not the records: a lane finds the
// record(s) its piece comes from in the run's offsets (LDS, binary search), puts the bytes together with load4 and stores one
// aligned uint4; values of 30 bytes and one value of a megabyte keep every lane equally busy.  What lies in front of the first
// and behind the last aligned piece (< 16 bytes each) is stored byte by byte: nothing outside [D0, D1) is written.
struct GatherRun {
  int64_t dst[kGatherRecs + 1];  // value_off of the run's records and the closing entry (absolute, in the values buffer)
  int64_t src[kGatherRecs];      // where each value lies in the push's bytes
  int32_t n;
};

__device__ __forceinline__ void gather_run_load(GatherRun& run, int64_t first, int64_t kept, const int64_t* __restrict__ value_off, const int64_t* __restrict__ val_src) {
  const int64_t left = kept - first;
  const int32_t n = left < kGatherRecs ? (int32_t)left : kGatherRecs;
  for (int32_t k = threadIdx.x; k <= n; k += blockDim.x) {
    run.dst[k] = value_off[first + k];
    if (k < n) run.src[k] = val_src[first + k];
  }
  if (threadIdx.x == 0) run.n = n;
}

// the record of the run that holds output byte p (D0 <= p < D1): the first whose end lies behind p (records without bytes never qualify)
__device__ __forceinline__ int32_t gather_find(const GatherRun& run, int64_t p) {
  int32_t lo = 0, hi = run.n - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (run.dst[mid + 1] > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ uint32_t gather_byte(const GatherRun& run, const uint8_t* __restrict__ bytes, int64_t p, int32_t& r) {
  while (run.dst[r + 1] <= p) ++r;  // (p < D1 = dst[n]: ends at a record with bytes)
  return bytes[run.src[r] + (p - run.dst[r])];
}

// the aligned piece [p, p + 16) of the run's span
__device__ __forceinline__ void gather_piece(const GatherRun& run, const uint8_t* __restrict__ bytes, int64_t p, uint8_t* __restrict__ values) {
  int32_t r = gather_find(run, p);
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t q = p + 4 * k;
    while (run.dst[r + 1] <= q) ++r;
    if (q + 4 <= run.dst[r + 1]) {  // the dword lies in one value: one unaligned load (reads at most 7 bytes behind it: the staged bytes' slack)
      w[k] = load4(bytes + run.src[r] + (q - run.dst[r]));
    } else {                        // it straddles values: byte by byte
      int32_t rr = r;
      uint32_t v = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) v |= gather_byte(run, bytes, q + b, rr) << (8 * b);
      w[k] = v;
    }
  }
  *(uint4*)(values + p) = make_uint4(w[0], w[1], w[2], w[3]);
}

// One workgroup per run.  It copies the head and tail bytes and the first kGatherOwn bytes' worth of pieces; a run whose span is
// longer (one value of a megabyte among short ones) lists itself for value_gather_long_kernel, which splits the rest over a whole
// grid: the decision is the workgroup's, not a lane's, and no lane ever copies a long value alone.
__global__ void __launch_bounds__(256) value_gather_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ value_off, const int64_t* __restrict__ val_src,
                                                          int64_t kept, uint8_t* __restrict__ values, uint32_t* __restrict__ long_runs) {
  __shared__ GatherRun run;
  gather_run_load(run, (int64_t)blockIdx.x * kGatherRecs, kept, value_off, val_src);
  __syncthreads();
  const int64_t d0 = run.dst[0], d1 = run.dst[run.n];
  if (d1 <= d0) return;  // tombstones only
  const int64_t a0 = (d0 + 15) & ~15ll;                    // the first aligned piece starts here (if it fits)
  const int64_t n_pieces = a0 < d1 ? (d1 - a0) >> 4 : 0;
  const int64_t own = n_pieces < (kGatherOwn >> 4) ? n_pieces : (kGatherOwn >> 4);
  for (int64_t j = threadIdx.x; j < own; j += blockDim.x) gather_piece(run, bytes, a0 + 16 * j, values);
  // head [d0, min(a0, d1)) and tail [a0 + 16 n_pieces, d1): lanes of the last wave, one byte each
  const int64_t head_end = a0 < d1 ? a0 : d1, tail = a0 < d1 ? a0 + 16 * n_pieces : d1;
  const int t = (int)threadIdx.x - 192;
  if (t >= 0 && t < 16 && d0 + t < head_end) { int32_t r = gather_find(run, d0 + t); values[d0 + t] = (uint8_t)gather_byte(run, bytes, d0 + t, r); }
  if (t >= 16 && t < 32 && tail + (t - 16) < d1) { int32_t r = gather_find(run, tail + (t - 16)); values[tail + (t - 16)] = (uint8_t)gather_byte(run, bytes, tail + (t - 16), r); }
  if (threadIdx.x == 0 && n_pieces > own) long_runs[1 + atomicAdd(&long_runs[0], 1u)] = blockIdx.x;  // (at most one entry per workgroup: the list holds them all)
}

// the pieces behind the first kGatherOwn bytes of the listed runs, every run split over the whole grid
__global__ void __launch_bounds__(256) value_gather_long_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ value_off, const int64_t* __restrict__ val_src,
                                                               int64_t kept, uint8_t* __restrict__ values, const uint32_t* __restrict__ long_runs) {
  __shared__ GatherRun run;
  const uint32_t n_long = long_runs[0];
  for (uint32_t k = 0; k < n_long; ++k) {  // (uniform: every workgroup walks the same list)
    __syncthreads();  // the last run's readers are through
    gather_run_load(run, (int64_t)long_runs[1 + k] * kGatherRecs, kept, value_off, val_src);
    __syncthreads();
    const int64_t d0 = run.dst[0], d1 = run.dst[run.n];
    const int64_t a0 = (d0 + 15) & ~15ll;
    const int64_t n_pieces = a0 < d1 ? (d1 - a0) >> 4 : 0;
    for (int64_t j = (kGatherOwn >> 4) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_pieces; j += (int64_t)gridDim.x * blockDim.x)
      gather_piece(run, bytes, a0 + 16 * j, values);
  }
}

// one thread per item, 256 to a workgroup
#define LAUNCH_1D(kernel, n, st, ...) hipLaunchKernelGGL(kernel, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__)

}  // namespace

hipError_t intern_temp_bytes(int64_t n_rec, size_t* bytes, hipStream_t st) {
  const size_t R = (size_t)n_rec;
  size_t tb_a = 0, tb_b = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, tb_a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, R + 1, rocprim::plus<unsigned long long>(), st);
  if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tb_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, R + 1, rocprim::plus<uint32_t>(), st);
  *bytes = tb_a > tb_b ? tb_a : tb_b;
  return e;
}

void launch_table_build(const KeyTable& k, hipStream_t st) {
  LAUNCH_1D(table_clear_kernel, k.t.mask + 1, st, k.t.s, k.t.mask + 1);
  if (k.n_keys > 0) LAUNCH_1D(rehash_kernel, k.n_keys, st, (const unsigned long long*)k.key_hash, k.n_keys, k.t);
}

void launch_rekey_records(RecMeta* meta, int64_t n_rec, const uint8_t* bytes, uint64_t seed, hipStream_t st) {
  LAUNCH_1D(rekey_records_kernel, n_rec, st, meta, n_rec, bytes, seed);
}

hipError_t launch_intern_probe(RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const KeyTable& k, const InternScratch& sc, ErrorCell* err, hipStream_t st) {
  const size_t R = (size_t)n_rec;
  LAUNCH_1D(probe_kernel, n_rec, st, meta, n_rec, k.t);
  LAUNCH_1D(flag_kernel, n_rec + 1, st, (const RecMeta*)meta, n_rec, bytes, k.t, (const uint8_t*)k.arena, (const int64_t*)k.key_off, sc.first, sc.keep, err);
  size_t tb = sc.temp_bytes;
  hipError_t e = rocprim::exclusive_scan(sc.temp, tb, (const unsigned long long*)sc.first, sc.first_scan, 0ull, R + 1, rocprim::plus<unsigned long long>(), st);
  tb = sc.temp_bytes;
  return e != hipSuccess ? e : rocprim::exclusive_scan(sc.temp, tb, (const uint32_t*)sc.keep, sc.keep_pos, 0u, R + 1, rocprim::plus<uint32_t>(), st);
}

void launch_intern_reseed(RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const KeyTable& k, uint64_t seed, hipStream_t st) {
  launch_intern_rollback(meta, n_rec, k.t, st);
  LAUNCH_1D(table_clear_kernel, k.t.mask + 1, st, k.t.s, k.t.mask + 1);
  if (k.n_keys > 0) {
    LAUNCH_1D(rekey_keys_kernel, k.n_keys, st, (const uint8_t*)k.arena, (const int64_t*)k.key_off, k.n_keys, seed, k.key_hash);
    LAUNCH_1D(rehash_kernel, k.n_keys, st, (const unsigned long long*)k.key_hash, k.n_keys, k.t);
  }
  launch_rekey_records(meta, n_rec, bytes, seed, st);
}

void launch_intern_commit(const RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const KeyTable& k, const InternScratch& sc, int64_t n_new,
                          const uint4* ev_tmp, int64_t out_base, int64_t* agg_out, uint4* ev_out, int64_t* off_out, hipStream_t st) {
  if (n_new > 0)
    LAUNCH_1D(assign_kernel, n_rec, st, meta, n_rec, bytes, (const unsigned long long*)sc.first, (const unsigned long long*)sc.first_scan, k.n_keys, k.arena_bytes, k.t,
              k.arena, k.key_off, k.key_hash);
  LAUNCH_1D(finalize_kernel, n_rec, st, meta, n_rec, (const uint32_t*)sc.keep, (const uint32_t*)sc.keep_pos, k.t, ev_tmp, out_base, agg_out, ev_out, off_out);
}

void launch_intern_rollback(const RecMeta* meta, int64_t n_rec, const Table& t, hipStream_t st) { LAUNCH_1D(rollback_kernel, n_rec, st, meta, n_rec, t); }

hipError_t launch_lookup(const uint8_t* ids, const int64_t* id_off, int64_t n, const KeyTable& k, uint64_t seed, int64_t* idx_out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (k.n_keys == 0 || !k.t.s) return hipMemsetAsync(idx_out, 0xff, (size_t)n * 8, st);  // nothing interned: every query misses (-1)
  LAUNCH_1D(lookup_kernel, n, st, ids, id_off, n, k.t, (const uint8_t*)k.arena, (const int64_t*)k.key_off, seed, idx_out);
  return hipGetLastError();
}

hipError_t launch_value_scan(const RecMeta* meta, int64_t n_rec, const InternScratch& sc, const StateScratch& ss, hipStream_t st) {
  LAUNCH_1D(value_len_kernel, n_rec + 1, st, meta, n_rec, (const uint32_t*)sc.keep, ss.vlen);
  size_t tb = sc.temp_bytes;
  return rocprim::exclusive_scan(sc.temp, tb, (const unsigned long long*)ss.vlen, ss.vscan, 0ull, (size_t)n_rec + 1, rocprim::plus<unsigned long long>(), st);
}

hipError_t launch_value_gather(const RecMeta* meta, int64_t n_rec, const uint8_t* bytes, const InternScratch& sc, const StateScratch& ss, int64_t kept, int64_t out_base,
                               int64_t val_base, int64_t* value_off, uint8_t* values, hipStream_t st) {
  LAUNCH_1D(value_off_kernel, n_rec + 1, st, meta, n_rec, (const uint32_t*)sc.keep, (const uint32_t*)sc.keep_pos, (const unsigned long long*)ss.vscan, out_base, val_base,
            value_off, ss.val_src);
  if (kept <= 0) return hipGetLastError();
  const hipError_t e = hipMemsetAsync(ss.long_runs, 0, 4, st);
  if (e != hipSuccess) return e;
  const unsigned n_runs = (unsigned)((kept + kGatherRecs - 1) / kGatherRecs);
  hipLaunchKernelGGL(value_gather_kernel, dim3(n_runs), dim3(256), 0, st, bytes, (const int64_t*)(value_off + out_base), (const int64_t*)ss.val_src, kept, values, ss.long_runs);
  // (1024 workgroups: four per CU; with no run listed each reads one word and ends)
  hipLaunchKernelGGL(value_gather_long_kernel, dim3(1024), dim3(256), 0, st, bytes, (const int64_t*)(value_off + out_base), (const int64_t*)ss.val_src, kept, values,
                     (const uint32_t*)ss.long_runs);
  return hipGetLastError();
}

}  // namespace ingest
}  // namespace surge
