// device_framer.hip — the host object of the device framer (surge_device_framer_*, include/surge_snapshot.h): the handle's
// lifecycle, the C exports, the steps of a publish and the host CRC pass.
//
// Steps (all on the framer's stream): select the changed aggregates (rocPRIM select) -> their partition + base size ->
// stable radix sort by partition -> the three scans -> batches per partition (count, then emit at scanned offsets) ->
// one thread per record writes its bytes, one per batch its 61-byte header -> one device -> host copy -> host CRCs.
// (LZ4 mode puts compress_and_pack, frame_lz4.hip, between the records and the headers.)
//
// The host waits for the device three times per publish, five in LZ4 mode: for the count of selected records (select_records),
// for the batch and byte totals (cut_batches), [LZ4: for the block count and for the compressed spans (compress_and_pack),]
// and for the bytes in page-locked memory (headers_and_copy_out).  A scan whose scratch has to grow waits once more
// (scan_in_place, frame_internal.h).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "../../include/surge_ingest.h"  // surge_crc32c
#include "frame_internal.h"

using namespace surge::frame;
using namespace surge::frame::host;

namespace {

// 1. the arguments: refused before anything is touched
int32_t check_arguments(surge_device_framer* f, int64_t n_aggregates, const uint8_t* d_kind, const int32_t* d_partition, const int64_t* d_key_off,
                        const uint8_t** bytes_out, const int64_t** part_byte_off_out) {
  if (!f) return ffail(nullptr, E_INVALID, "framer is NULL");
  if (n_aggregates < 0 || n_aggregates > (1ll << 32) - 2 || !bytes_out || !part_byte_off_out)
    return ffail(f, E_INVALID, "bad argument");
  if (n_aggregates > 0 && (!d_kind || !d_partition || !d_key_off)) return ffail(f, E_INVALID, "NULL device buffer");
  return OK;
}

// 2. the changed aggregates, in index order: f->sel, and pub.n_sel of them (one wait); clears the bad-input word
int32_t select_records(surge_device_framer* f, Publish& pub) {
  hipStream_t st = f->stream;
  FCHK(f, f->sel.room((size_t)pub.n));
  FCHK(f, f->n_sel.room(2));
  FCHK(f, f->bad.room(4));
  size_t tb_select = 0;
  FCHK(f, select_changed(nullptr, tb_select, pub.kind, f->sel.ptr(), f->n_sel.ptr(), pub.n, st));
  FCHK(f, f->temp.reserve(tb_select));  // (nothing is in flight: the previous publish ended with a wait)
  FCHK(f, hipMemsetAsync(f->bad.ptr(), 0, 4, st));
  FCHK(f, select_changed(f->temp.p, tb_select, pub.kind, f->sel.ptr(), f->n_sel.ptr(), pub.n, st));
  FCHK(f, hipMemcpyAsync(&pub.n_sel, f->n_sel.ptr(), 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  return OK;
}

// 3. partition + base size per record, stable sort by partition, the three scanned sizes, every partition's first record:
// pub.order, pub.c1 .. c3, f->pstart.  Nothing is in flight when it begins (select_records waited), so the scratch is sized
// here for the sort and for the scans of n_sel + 1 without a wait; the three scans then find it large enough.
int32_t plan_records(surge_device_framer* f, Publish& pub) {
  hipStream_t st = f->stream;
  const int32_t P = f->n_part;
  const int64_t n_sel = pub.n_sel;
  if (n_sel > 0xfffffff0ll) return ffail(f, E_RANGE, "more than 2^32 records in one publish");
  unsigned bits = 1;
  while ((1ll << bits) < P) ++bits;
  size_t tb_sort = 0, tb_scan = 0;
  FCHK(f, sort_by_partition(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n_sel, bits, st));
  FCHK(f, scan_exclusive(nullptr, tb_scan, nullptr, (size_t)n_sel + 1, st));
  FCHK(f, f->temp.reserve(tb_sort > tb_scan ? tb_sort : tb_scan));
  for (Dev<uint32_t>* b : {&f->keys_a, &f->keys_b, &f->vals_a, &f->vals_b, &f->base}) FCHK(f, b->room((size_t)n_sel));
  FCHK(f, f->c.room((size_t)(n_sel + 1) * 3));
  FCHK(f, f->pstart.room((size_t)P + 1));
  FCHK(f, f->nb.room((size_t)P + 1));
  FCHK(f, f->pbytes.room((size_t)P + 1));
  FCHK(f, f->d_next.room((size_t)P));
  launch_frame_size(f->sel.ptr(), n_sel, pub.kind, pub.partition, P, pub.key_off, pub.val_off, pub.keys_utf8 != nullptr, pub.values != nullptr,
                    f->keys_a.ptr(), f->vals_a.ptr(), f->base.ptr(), f->bad.ptr(), st);
  FCHK(f, sort_by_partition(f->temp.p, tb_sort, f->keys_a.ptr(), f->keys_b.ptr(), f->vals_a.ptr(), f->vals_b.ptr(), n_sel, bits, st));
  pub.order = f->vals_b.ptr();
  pub.c1 = f->c.ptr();
  pub.c2 = pub.c1 + (n_sel + 1);
  pub.c3 = pub.c2 + (n_sel + 1);
  launch_frame_sizes3(pub.order, f->base.ptr(), n_sel, pub.c1, pub.c2, pub.c3, st);
  for (int64_t* cv : {pub.c1, pub.c2, pub.c3})
    if (const int32_t rc = scan_in_place(f, cv, (size_t)n_sel + 1)) return rc;
  launch_frame_pstart(f->keys_b.ptr(), n_sel, P, f->pstart.ptr(), st);
  return OK;
}

// 4. the batches of every partition: count, scan, emit.  One wait, for the totals (pub.n_batches, pub.n_bytes), the bad-input
// word of step 3's size kernel and the spans of the uncompressed output (f->part_byte_off); then f->batches on the device.
// Leaves f->nb as every partition's first batch.
int32_t cut_batches(surge_device_framer* f, Publish& pub) {
  hipStream_t st = f->stream;
  const int32_t P = f->n_part;
  int64_t* nb = f->nb.ptr();
  int64_t* pbytes = f->pbytes.ptr();
  FCHK(f, hipMemcpyAsync(f->d_next.ptr(), f->next_offset.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
  launch_frame_batches(f->pstart.ptr(), P, pub.c1, pub.c2, pub.c3, f->max_records, f->max_bytes, f->d_next.ptr(), false, nb, pbytes, nullptr, st);
  FCHK(f, hipMemsetAsync(nb + P, 0, 8, st));
  FCHK(f, hipMemsetAsync(pbytes + P, 0, 8, st));
  if (const int32_t rc = scan_in_place(f, nb, (size_t)P + 1)) return rc;  // (P + 1 <= 2^20 + 1 elements: the scratch sized for n_sel + 1 may be smaller)
  if (const int32_t rc = scan_in_place(f, pbytes, (size_t)P + 1)) return rc;
  int64_t totals[2] = {0, 0};
  FCHK(f, hipMemcpyAsync(&totals[0], nb + P, 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipMemcpyAsync(&totals[1], pbytes + P, 8, hipMemcpyDeviceToHost, st));
  uint32_t bad = 0;
  FCHK(f, hipMemcpyAsync(&bad, f->bad.ptr(), 4, hipMemcpyDeviceToHost, st));
  FCHK(f, hipMemcpyAsync(f->part_byte_off.data(), pbytes, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  if (bad)
    return ffail(f, E_RANGE, "a changed aggregate has an unknown kind, a partition outside [0, n_partitions), a negative key / value span, or bytes in a table that was passed as NULL");
  FCHK(f, f->batches.room((size_t)totals[0]));
  FCHK(f, f->out.room((size_t)totals[1]));
  try {
    f->h_batches.resize((size_t)totals[0]);
  } catch (const std::bad_alloc&) {
    return ffail(f, E_NOMEM, "out of host memory");
  }
  pub.n_batches = totals[0];
  pub.n_bytes = pub.uncompressed_bytes = totals[1];
  launch_frame_batches(f->pstart.ptr(), P, pub.c1, pub.c2, pub.c3, f->max_records, f->max_bytes, f->d_next.ptr(), true, nb, pbytes, f->batches.ptr(), st);
  return OK;
}

// 5. the records, into the uncompressed layout: pub.d_final = f->out
int32_t write_records(surge_device_framer* f, Publish& pub) {
  launch_frame_write(f->batches.ptr(), pub.n_batches, pub.order, f->sel.ptr(), pub.n_sel, pub.kind, f->base.ptr(), pub.c1, pub.c2, pub.c3, pub.keys_utf8,
                     pub.key_off, pub.values, pub.val_off, f->out.ptr(), f->stream);
  pub.d_final = f->out.ptr();
  return OK;
}

// 7. the batch headers, then the output and the batch table to the host (one wait): f->pinned, f->h_batches
int32_t headers_and_copy_out(surge_device_framer* f, const Publish& pub) {
  hipStream_t st = f->stream;
  FCHK(f, f->pinned.reserve((size_t)pub.n_bytes));
  launch_frame_header(f->batches.ptr(), pub.n_batches, pub.timestamp_ms, f->codec, pub.d_final, st);
  FCHK(f, hipGetLastError());
  FCHK(f, hipMemcpyAsync(f->pinned.p, pub.d_final, (size_t)pub.n_bytes, hipMemcpyDeviceToHost, st));
  FCHK(f, hipMemcpyAsync(f->h_batches.data(), f->batches.ptr(), (size_t)pub.n_batches * sizeof(Batch), hipMemcpyDeviceToHost, st));
  FCHK(f, hipStreamSynchronize(st));
  return OK;
}

// 8. CRC-32C of every batch (attributes .. end), on the host's crc32 instruction, batches spread over a few threads
int32_t host_crcs(uint8_t* base, const std::vector<Batch>& hb, int64_t n_batches, int64_t n_bytes) {
  (void)surge_crc32c((const uint8_t*)"", 0);  // initialise the dispatch before threads race for it
  std::atomic<int64_t> next{0};
  auto work = [&]() {
    for (int64_t i = next.fetch_add(1); i < n_batches; i = next.fetch_add(1)) {
      uint8_t* o = base + hb[(size_t)i].out_off;
      const uint32_t crc = surge_crc32c(o + 21, (int64_t)(kHeader - 21) + hb[(size_t)i].records_bytes);
      o[17] = (uint8_t)(crc >> 24); o[18] = (uint8_t)(crc >> 16); o[19] = (uint8_t)(crc >> 8); o[20] = (uint8_t)crc;
    }
  };
  unsigned hw = std::thread::hardware_concurrency();
  int n_threads = (int)(hw ? hw : 1);
  if (n_threads > 8) n_threads = 8;
  if ((int64_t)n_threads > n_batches) n_threads = (int)n_batches;
  if (n_bytes < (4 << 20)) n_threads = 1;
  std::vector<std::thread> th;
  try {
    for (int t = 1; t < n_threads; ++t) th.emplace_back(work);
  } catch (...) {  // the threads that did start, and this one, do the work
  }
  work();
  for (std::thread& t : th) t.join();
  return OK;
}

// Steps 2 to 8 in the order of their device work.  An empty publish (no aggregates, or none changed) is a success that leaves
// pub without batches; nothing here writes the caller's outputs or advances the handle (surge_device_framer_frame commits).
int32_t run_steps(surge_device_framer* f, Publish& pub) {
  if (pub.n == 0) return OK;
  if (const int32_t rc = select_records(f, pub)) return rc;
  if (pub.n_sel == 0) return OK;
  if (const int32_t rc = plan_records(f, pub)) return rc;
  if (const int32_t rc = cut_batches(f, pub)) return rc;
  if (const int32_t rc = write_records(f, pub)) return rc;
  if (f->codec == SURGE_SNAPSHOT_CODEC_LZ4)
    if (const int32_t rc = compress_and_pack(f, pub)) return rc;
  if (const int32_t rc = headers_and_copy_out(f, pub)) return rc;
  return host_crcs(f->pinned.p, f->h_batches, pub.n_batches, pub.n_bytes);
}

}  // namespace

extern "C" {

int32_t surge_device_framer_create(int32_t device_id, void* hip_stream, int32_t n_partitions, int32_t max_records_per_batch, int64_t max_batch_bytes,
                                   surge_device_framer** out) {
  if (!out) return ffail(nullptr, E_INVALID, "out is NULL");
  *out = nullptr;
  if (n_partitions <= 0 || n_partitions > (1 << 20) || max_records_per_batch < 0 || max_records_per_batch > kD3 || max_batch_bytes < 0)
    return ffail(nullptr, E_INVALID, "bad argument (partitions in 1 .. 2^20, at most 2^20 records per batch)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device_id < 0 || device_id >= n_dev)
    return ffail(nullptr, E_DEVICE, "no usable HIP device (the device framer has no CPU fallback: use surge_snapshot_writer_append)");
  surge_device_framer* f = new (std::nothrow) surge_device_framer();
  if (!f) return ffail(nullptr, E_NOMEM, "out of host memory");
  f->device = device_id;
  f->stream = (hipStream_t)hip_stream;
  f->n_part = n_partitions;
  if (max_records_per_batch > 0) f->max_records = max_records_per_batch;
  if (max_batch_bytes > 0) f->max_bytes = max_batch_bytes;
  try {
    f->next_offset.assign((size_t)n_partitions, 0);
    f->part_byte_off.assign((size_t)n_partitions + 1, 0);
  } catch (const std::bad_alloc&) {
    delete f;
    return ffail(nullptr, E_NOMEM, "out of host memory");
  }
  *out = f;
  return OK;
}

int32_t surge_device_framer_destroy(surge_device_framer* f) {
  if (!f) return OK;
  Guard g(f->device);
  (void)hipStreamSynchronize(f->stream);
  delete f;  // its buffers go with it: the device is current and the stream has drained
  return OK;
}

const char* surge_device_framer_last_error(const surge_device_framer* f) { return f ? f->err.c_str() : g_frame_err.c_str(); }

int32_t surge_device_framer_set_compression(surge_device_framer* f, int32_t codec) {
  if (!f) return ffail(nullptr, E_INVALID, "framer is NULL");
  if (codec != SURGE_SNAPSHOT_CODEC_NONE && codec != SURGE_SNAPSHOT_CODEC_LZ4)
    return ffail(f, E_INVALID, "unknown codec (the device framer writes uncompressed or LZ4 batches)");
  f->codec = codec;
  return OK;
}

int32_t surge_device_framer_next_offsets(const surge_device_framer* f, int64_t* out) {
  if (!f || !out) return ffail(nullptr, E_INVALID, "bad argument");
  std::memcpy(out, f->next_offset.data(), f->next_offset.size() * 8);
  return OK;
}

int64_t surge_device_framer_uncompressed_bytes(const surge_device_framer* f) { return f ? f->uncompressed_bytes : -1; }

int32_t surge_device_framer_frame(surge_device_framer* f, int64_t n_aggregates, const uint8_t* d_kind, const int32_t* d_partition,
                                  const uint8_t* d_keys_utf8, const int64_t* d_key_off, const uint8_t* d_values, const int64_t* d_val_off,
                                  int64_t timestamp_ms, const uint8_t** bytes_out, const int64_t** part_byte_off_out, int64_t* n_records_out,
                                  int64_t* n_batches_out) {
  if (const int32_t rc = check_arguments(f, n_aggregates, d_kind, d_partition, d_key_off, bytes_out, part_byte_off_out)) return rc;
  Guard g(f->device);
  Publish pub;
  pub.n = n_aggregates;
  pub.kind = d_kind;
  pub.partition = d_partition;
  pub.keys_utf8 = d_keys_utf8;
  pub.key_off = d_key_off;
  pub.values = d_values;
  pub.val_off = d_val_off;
  pub.timestamp_ms = timestamp_ms;
  const int32_t rc = run_steps(f, pub);
  // 9. commit, the one place that writes the caller's outputs and advances the handle.  A publish that was refused commits as
  // an empty one does: no partition has a span, the counts are zero, no offset advances, and the two pointers are valid.
  if (rc != OK) pub = Publish{};
  if (pub.n_batches == 0) std::fill(f->part_byte_off.begin(), f->part_byte_off.end(), 0);  // (else the spans are the last step's)
  for (int64_t i = 0; i < pub.n_batches; ++i) f->next_offset[(size_t)f->h_batches[(size_t)i].partition] += f->h_batches[(size_t)i].count;
  f->uncompressed_bytes = pub.uncompressed_bytes;
  *bytes_out = f->pinned.p;
  *part_byte_off_out = f->part_byte_off.data();
  if (n_records_out) *n_records_out = pub.n_sel;
  if (n_batches_out) *n_batches_out = pub.n_batches;
  return rc;
}

}  // extern "C"
