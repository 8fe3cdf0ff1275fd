// ingest_intern.hip — the device decoder's interning stage: aggregate ids -> dense indices, and the compaction of the delivered
// records into the result arrays.
//   probe      one thread per record: open-addressing insert-or-find by hash (atomicCAS); a NEW slot remembers its first record
//   flag       one thread per record: key bytes compared with what the slot stands for (a 64-bit hash collision is detected,
//              not trusted); the first record of every new key and the delivered records are flagged
//   scans      (rocPRIM) the new keys' ids in first-delivered order — the host decoder's order — and arena offsets; the
//              delivered records' positions in the result arrays
//   assign     the new keys' bytes to the device key arena, their ids into their slots
//   finalize   one thread per delivered record: aggregate index from its slot, event and offset to the result arrays
// The control flow around these — the retry after a collision, what is checked before anything is committed, the commit order —
// is stage 2 of the decoder (ingest_decoder.hip); this unit launches what it is told to.
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
  ev_out[o] = ev_tmp[i];
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

}  // namespace ingest
}  // namespace surge
