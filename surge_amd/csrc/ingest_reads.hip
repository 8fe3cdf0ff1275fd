// ingest_reads.hip — the device decoder's key table read between pushes (ingest_decoder_internal.h, ReadsState): the ids
// and their offsets as they lie (surge_device_decoder_keys / _key_table), id -> dense index or -1
// (surge_device_decoder_lookup[_device], lookup_kernel), and the table in key order: surge_device_decoder_key_order /
// _range_device / _gather_keys_device over ingest_order.hip's kernels, with the order's pass loop (ensure_order).  A read
// needs every push finished and a decoder no push has poisoned: readable() is that gate.
#include "ingest_decoder_internal.h"

using namespace surge::ingest;
using namespace surge::ingest::host;

namespace {

// every push is finished (a slot the push in flight inserted has no id yet, and its stage 2 may move the table or its hash function)
int32_t pushes_finished(surge_device_decoder* d) { return d->n_pending != 0 ? refuse_pending(d, kNoIdsYet) : OK; }

// ... and none has left the tables in an unknown state
int32_t readable(surge_device_decoder* d) {
  const int32_t rc = pushes_finished(d);
  if (rc != OK) return rc;
  return d->poisoned ? refuse_poisoned(d) : OK;
}

// reads.order.idx = the dense indices in key order, built when the table has grown since the last build.  Most significant chunk
// first: a pass sorts every key by (its group, its next four bytes, how many it has left), then the groups are re-numbered; the
// loop ends when every group is one key.  (Unique keys: a group of several holds only keys that go on, so that is after at most
// ceil(max_len / 4) + 1 passes; a pass in which no key had a byte left ends it whatever the table holds.)  Eight bytes come
// back per pass.  The scratch — 28 bytes per key and rocPRIM's — goes when the build is over; the order stays, 8 bytes per key.
int32_t ensure_order(surge_device_decoder* d) {
  ReadsState::Order& order = d->reads.order;
  const int64_t n = d->n_keys;
  if (order.keys == n) return OK;
  if (n > kOrderMaxKeys) return dfail(d, E_UNSUPPORTED, "more than 2^29 aggregate ids: the key order sorts 29 bits of group");
  hipStream_t st = d->stream;
  order.keys = -1;
  int64_t passes = 0;
  if (n > 0) {
    DCHK(d, order.idx.reserve((size_t)n * 8, false, st));
    Buf key_a, key_b, idx_a, idx_b, grp, flag, live, temp;
    OrderScratch sc{};
    DCHK(d, order_temp_bytes(n, &sc.temp_bytes, st));
    DCHK(d, key_a.reserve((size_t)n * 8, false, st));
    DCHK(d, key_b.reserve((size_t)n * 8, false, st));
    for (Buf* b : {&idx_a, &idx_b, &grp, &flag}) DCHK(d, b->reserve((size_t)n * 4, false, st));
    DCHK(d, live.reserve(4, false, st));
    DCHK(d, temp.reserve(sc.temp_bytes ? sc.temp_bytes : 1, false, st));
    sc.key_in = (unsigned long long*)key_a.p;
    sc.key_out = (unsigned long long*)key_b.p;
    sc.idx_in = (uint32_t*)idx_a.p;
    sc.idx_out = (uint32_t*)idx_b.p;
    sc.grp = (uint32_t*)grp.p;
    sc.flag = (uint32_t*)flag.p;
    sc.live = (uint32_t*)live.p;
    sc.temp = temp.p;
    DCHK(d, launch_order_init(sc, n, st));
    int64_t groups = 1;
    while (groups < n) {
      int group_bits = 0;
      while ((1ll << group_bits) < groups) ++group_bits;
      DCHK(d, launch_order_pass(keys_of(d), passes, group_bits, sc, st));
      ++passes;
      uint32_t last_group = 0, had_bytes = 0;
      DCHK(d, hipMemcpyAsync(&last_group, sc.grp + (n - 1), 4, hipMemcpyDeviceToHost, st));
      DCHK(d, hipMemcpyAsync(&had_bytes, sc.live, 4, hipMemcpyDeviceToHost, st));
      DCHK(d, hipStreamSynchronize(st));
      groups = (int64_t)last_group + 1;
      if (!had_bytes) break;
    }
    DCHK(d, launch_order_finish(sc, n, (int64_t*)order.idx.p, st));
    DCHK(d, hipStreamSynchronize(st));  // (the scratch is freed on the way out)
    if (groups < n) return dfail(d, SURGE_E_CORRUPT, "the key table holds the same id twice");
  }
  order.keys = n;
  order.passes = passes;
  return OK;
}

}  // namespace

extern "C" {

int32_t surge_device_decoder_keys(surge_device_decoder* d, uint8_t* utf8_out, int64_t utf8_capacity, int64_t* key_off_out, int64_t* n_keys_out,
                                  int64_t* utf8_bytes_out) {
  if (!d) return refuse_null_decoder();
  if (n_keys_out) *n_keys_out = d->n_keys;
  if (utf8_bytes_out) *utf8_bytes_out = d->arena_bytes;
  if (!utf8_out && !key_off_out) return OK;  // size query
  if (utf8_capacity < d->arena_bytes) return dfail(d, E_INVALID, "utf8_out is too small (see *utf8_bytes_out)");
  DeviceScope scope(d->device);
  DCHK(d, hipStreamSynchronize(d->stream));
  if (utf8_out && d->arena_bytes > 0) DCHK(d, hipMemcpy(utf8_out, d->arena.p, (size_t)d->arena_bytes, hipMemcpyDeviceToHost));
  if (key_off_out) DCHK(d, hipMemcpy(key_off_out, d->key_off.p, (size_t)(d->n_keys + 1) * 8, hipMemcpyDeviceToHost));
  return OK;
}

int32_t surge_device_decoder_key_table(surge_device_decoder* d, const uint8_t** d_utf8, const int64_t** d_key_off) {
  if (!d) return refuse_null_decoder();
  if (d_utf8) *d_utf8 = (const uint8_t*)d->arena.p;
  if (d_key_off) *d_key_off = (const int64_t*)d->key_off.p;
  return OK;
}

int32_t surge_device_decoder_lookup_device(surge_device_decoder* d, const uint8_t* d_ids_utf8, const int64_t* d_id_off, int64_t n, int64_t* d_idx_out) {
  if (!d) return refuse_null_decoder();
  if (n < 0 || (n > 0 && (!d_ids_utf8 || !d_id_off || !d_idx_out))) return dfail(d, E_INVALID, "bad argument");
  const int32_t rc = readable(d);
  if (rc != OK) return rc;
  if (n == 0) return OK;
  DeviceScope scope(d->device);
  DCHK(d, launch_lookup(d_ids_utf8, d_id_off, n, keys_of(d), d->seed, d_idx_out, d->stream));
  return OK;
}

// (the queries are staged behind the pending test alone: what a poisoned decoder answers, surge_device_decoder_lookup_device says)
int32_t surge_device_decoder_lookup(surge_device_decoder* d, const uint8_t* ids_utf8, const int64_t* id_off, int64_t n, int64_t* idx_out) {
  if (!d) return refuse_null_decoder();
  if (n < 0 || (n > 0 && (!ids_utf8 || !id_off || !idx_out))) return dfail(d, E_INVALID, "bad argument");
  {
    const int32_t rc = pushes_finished(d);
    if (rc != OK) return rc;
  }
  if (n == 0) return OK;
  const int64_t first = id_off[0];
  if (first < 0) return dfail(d, E_INVALID, "id_off[0] is negative");
  std::vector<int64_t> off;
  try { off.resize((size_t)n + 1); } catch (const std::bad_alloc&) { return dfail(d, E_NOMEM, "out of host memory"); }
  for (int64_t i = 0; i <= n; ++i) {  // (the staged bytes begin at the first id)
    if (i > 0 && (id_off[i] < id_off[i - 1] || id_off[i] - id_off[i - 1] >= (1ll << 31))) return dfail(d, E_INVALID, "id_off must not decrease, and an id is shorter than 2^31 bytes");
    off[(size_t)i] = id_off[i] - first;
  }
  const size_t bytes = (size_t)off[(size_t)n];
  DeviceScope scope(d->device);
  hipStream_t st = d->stream;
  ReadsState::Lookup& lk = d->reads.lookup;
  DCHK(d, lk.ids.reserve(bytes + 16, false, st));  // (the 16 bytes of slack keys_equal's loads may touch)
  DCHK(d, lk.off.reserve((size_t)(n + 1) * 8, false, st));
  DCHK(d, lk.idx.reserve((size_t)n * 8, false, st));
  if (bytes) DCHK(d, hipMemcpyAsync(lk.ids.p, ids_utf8 + first, bytes, hipMemcpyHostToDevice, st));
  DCHK(d, hipMemcpyAsync(lk.off.p, off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  const int32_t rc = surge_device_decoder_lookup_device(d, (const uint8_t*)lk.ids.p, (const int64_t*)lk.off.p, n, (int64_t*)lk.idx.p);
  if (rc == OK) DCHK(d, hipMemcpyAsync(idx_out, lk.idx.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  DCHK(d, hipStreamSynchronize(st));  // (off is this call's)
  return rc;
}

// ---- reads in key order (ingest_order.hip) -------------------------------------------------------------------------------------
int32_t surge_device_decoder_key_order(surge_device_decoder* d, const int64_t** d_order, int64_t* n_keys_out, int64_t* passes_out) {
  if (!d) return refuse_null_decoder();
  int32_t rc = readable(d);
  if (rc != OK) return rc;
  DeviceScope scope(d->device);
  if ((rc = ensure_order(d)) != OK) return rc;
  if (d_order) *d_order = d->n_keys ? (const int64_t*)d->reads.order.idx.p : nullptr;
  if (n_keys_out) *n_keys_out = d->n_keys;
  if (passes_out) *passes_out = d->reads.order.passes;
  return OK;
}

int32_t surge_device_decoder_range_device(surge_device_decoder* d, const uint8_t* from_utf8, int64_t from_len, const uint8_t* to_utf8, int64_t to_len,
                                          int64_t* d_rows_out, int64_t capacity, int64_t* n_out) {
  // (what the numbers alone decide comes first: it is refused the same with and without a decoder)
  if (from_len < 0 || to_len < 0 || capacity < 0) return dfail(d, E_INVALID, "a negative length or capacity");
  if (!d) return refuse_null_decoder();
  if (!n_out) return dfail(d, E_INVALID, "bad argument");
  if (from_len >= (1ll << 31) || to_len >= (1ll << 31)) return dfail(d, E_INVALID, "a bound is shorter than 2^31 bytes");
  int32_t rc = readable(d);
  if (rc != OK) return rc;
  *n_out = 0;
  if (d->n_keys == 0) return OK;
  DeviceScope scope(d->device);
  if ((rc = ensure_order(d)) != OK) return rc;
  hipStream_t st = d->stream;
  ReadsState::Range& rg = d->reads.range;
  const int64_t* const order = (const int64_t*)d->reads.order.idx.p;
  // the two bounds, each with the 16 bytes behind it that the compare's loads may touch; a NULL bound has the length -1
  const int64_t fl = from_utf8 ? from_len : -1, tl = to_utf8 ? to_len : -1;
  const int64_t to_at = ((fl > 0 ? fl : 0) + 15) / 16 * 16 + 16;
  DCHK(d, rg.bounds.reserve((size_t)(to_at + (tl > 0 ? tl : 0) + 16), false, st));
  DCHK(d, rg.lo_hi.reserve(16, false, st));
  if (fl > 0) DCHK(d, hipMemcpyAsync(rg.bounds.p, from_utf8, (size_t)fl, hipMemcpyHostToDevice, st));
  if (tl > 0) DCHK(d, hipMemcpyAsync((uint8_t*)rg.bounds.p + to_at, to_utf8, (size_t)tl, hipMemcpyHostToDevice, st));
  DCHK(d, launch_order_bounds(keys_of(d), order, (const uint8_t*)rg.bounds.p, fl, to_at, tl, (int64_t*)rg.lo_hi.p, st));
  int64_t lo_hi[2] = {0, 0};
  DCHK(d, hipMemcpyAsync(lo_hi, rg.lo_hi.p, 16, hipMemcpyDeviceToHost, st));
  DCHK(d, hipStreamSynchronize(st));
  if (lo_hi[0] < 0 || lo_hi[1] > d->n_keys) return dfail(d, E_DEVICE, "the bound search left the key order");
  const int64_t n = lo_hi[1] > lo_hi[0] ? lo_hi[1] - lo_hi[0] : 0;  // (from > to: nothing)
  *n_out = n;
  if (n > capacity) return dfail(d, SURGE_E_RANGE, "d_rows_out is too small (see *n_out)");
  if (n == 0) return OK;
  if (!d_rows_out) return dfail(d, E_INVALID, "d_rows_out is NULL");
  DCHK(d, hipMemcpyAsync(d_rows_out, order + lo_hi[0], (size_t)n * 8, hipMemcpyDeviceToDevice, st));
  DCHK(d, hipStreamSynchronize(st));
  return OK;
}

int32_t surge_device_decoder_gather_keys_device(surge_device_decoder* d, const int64_t* d_rows, int64_t n, uint8_t* d_utf8_out, int64_t utf8_capacity,
                                                int64_t* d_off_out, int64_t* total_bytes_out) {
  if (n < 0 || utf8_capacity < 0) return dfail(d, E_INVALID, "a negative length or capacity");
  if (!d) return refuse_null_decoder();
  if (!d_off_out || (n > 0 && !d_rows)) return dfail(d, E_INVALID, "bad argument");
  const int32_t rc = readable(d);
  if (rc != OK) return rc;
  DeviceScope scope(d->device);
  hipStream_t st = d->stream;
  ReadsState::Gather& gk = d->reads.gather;
  KeyGatherScratch sc{};
  DCHK(d, key_gather_temp_bytes(n, &sc.temp_bytes, st));
  DCHK(d, gk.len.reserve((size_t)(n + 1) * 8, false, st));
  DCHK(d, gk.at.reserve((size_t)(n + 1) * 8, false, st));
  DCHK(d, gk.bad.reserve(4, false, st));
  DCHK(d, gk.temp.reserve(sc.temp_bytes ? sc.temp_bytes : 1, false, st));
  sc.len = (unsigned long long*)gk.len.p;
  sc.at = (unsigned long long*)gk.at.p;
  sc.bad = (uint32_t*)gk.bad.p;
  sc.temp = gk.temp.p;
  DCHK(d, launch_key_lengths(keys_of(d), d_rows, n, sc, st));
  unsigned long long total = 0;
  uint32_t bad = 0;
  DCHK(d, hipMemcpyAsync(&total, sc.at + n, 8, hipMemcpyDeviceToHost, st));
  DCHK(d, hipMemcpyAsync(&bad, sc.bad, 4, hipMemcpyDeviceToHost, st));
  DCHK(d, hipStreamSynchronize(st));
  if (bad) return dfail(d, E_INVALID, "a row is outside [0, n_keys)");
  if (total_bytes_out) *total_bytes_out = (int64_t)total;
  if ((int64_t)total > utf8_capacity) return dfail(d, SURGE_E_RANGE, "d_utf8_out is too small (see *total_bytes_out)");
  if (total > 0 && !d_utf8_out) return dfail(d, E_INVALID, "d_utf8_out is NULL");
  DCHK(d, launch_key_gather(keys_of(d), d_rows, n, sc, d_utf8_out, d_off_out, st));
  DCHK(d, hipStreamSynchronize(st));
  return OK;
}

}  // extern "C"
