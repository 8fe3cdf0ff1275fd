// engine_states.hip — reading and writing the resident states: snapshot / get / gather, the encoders, the decoder of
// serialized state text and its string columns, the published snapshot (delta / commit / invalidate), pack / unpack.
#include <cstring>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "f64_text.h"
#include "state_parse.h"

using namespace surge;

extern "C" {

int32_t surge_replay_snapshot(surge_replay_handle* h, void* states_out, uint8_t* present_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "snapshot before load_csr/bind_device_csr");
  if (h->st.n_folds == 0) return fail(h, SURGE_E_STATE, "snapshot before fold");
  DeviceGuard g(h->device);
  std::unique_lock<std::shared_mutex> lk(h->mu);
  const int64_t epoch = h->fold_epoch.load();
  const size_t bytes = (size_t)h->n_agg * 64;
  try {
    h->mirror.resize(bytes);
  } catch (const std::bad_alloc&) {
    return fail(h, SURGE_E_NOMEM, "out of host memory for the snapshot mirror");
  }
  if (bytes) {
    HIPCHK(h, hipMemcpyAsync(h->mirror.data(), h->d_state, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  h->mirror_epoch = epoch;
  int64_t poisoned = 0;
  for (int64_t a = 0; a < h->n_agg; ++a) {
    uint32_t fl;
    std::memcpy(&fl, h->mirror.data() + a * 64 + 36, 4);
    if (present_out) present_out[a] = (uint8_t)(fl & SURGE_STATE_PRESENT);
    poisoned += (fl & SURGE_STATE_POISONED) ? 1 : 0;
  }
  h->st.n_poisoned = poisoned;
  if (states_out && bytes) std::memcpy(states_out, h->mirror.data(), bytes);
  return SURGE_OK;
}

int32_t surge_replay_get(surge_replay_handle* h, int64_t agg_idx, void* state64_out, uint8_t* present_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!state64_out) return fail(h, SURGE_E_INVALID, "state64_out is NULL");
  if (!h->bound || h->st.n_folds == 0) return fail(h, SURGE_E_STATE, "get before fold");
  if (agg_idx < 0 || agg_idx >= h->n_agg) return fail(h, SURGE_E_RANGE, "aggregate index out of range");
  bool served = false;
  {
    std::shared_lock<std::shared_mutex> lk(h->mu);
    if (h->mirror_epoch == h->fold_epoch.load()) {
      std::memcpy(state64_out, h->mirror.data() + agg_idx * 64, 64);
      served = true;
    }
  }
  if (!served) {  // no mirror for this fold epoch: one device read at a time
    std::unique_lock<std::shared_mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIPCHK(h, hipMemcpyAsync(state64_out, h->d_state + agg_idx * 4, 64, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (present_out) {
    uint32_t fl;
    std::memcpy(&fl, (const uint8_t*)state64_out + 36, 4);
    *present_out = (uint8_t)(fl & SURGE_STATE_PRESENT);
  }
  return SURGE_OK;
}

int32_t surge_replay_gather(surge_replay_handle* h, const int64_t* agg_idx, int64_t n, void* states_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound || h->st.n_folds == 0) return fail(h, SURGE_E_STATE, "gather before fold");
  if (n < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n == 0) return SURGE_OK;
  if (!agg_idx || !states_out) return fail(h, SURGE_E_INVALID, "NULL buffer");
  for (int64_t i = 0; i < n; ++i)
    if (agg_idx[i] < 0 || agg_idx[i] >= h->n_agg) return fail(h, SURGE_E_RANGE, "aggregate index out of range");
  DeviceGuard g(h->device);
  HIPCHK(h, h->gather_idx.reserve((size_t)n * 8));
  HIPCHK(h, h->gather_out.reserve((size_t)n * 64));
  HIPCHK(h, hipMemcpyAsync(h->gather_idx.ptr, agg_idx, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_gather_states(h->d_state, (const int64_t*)h->gather_idx.ptr, n, (uint4*)h->gather_out.ptr, h->stream));
  HIPCHK(h, hipMemcpyAsync(states_out, h->gather_out.ptr, (size_t)n * 64, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SURGE_OK;
}

// what both encoders check before they touch the device, and the tables their kernels read
static int32_t encode_prepare(surge_replay_handle* h, const surge_json_template* tmpl) {
  if (tmpl->n_parts == 0 || tmpl->n_parts > SURGE_JSON_MAX_PARTS) return fail(h, SURGE_E_INVALID, "template.n_parts out of range");
  bool uses_f64 = false;
  for (uint32_t i = 0; i < tmpl->n_parts; ++i) {
    const auto& pt = tmpl->part[i];
    if (pt.kind > SURGE_JP_STR) return fail(h, SURGE_E_UNSUPPORTED, "unknown template part kind");
    if (pt.kind == SURGE_JP_LITERAL && (pt.lit_off > 256 || pt.lit_len > 256 - pt.lit_off)) return fail(h, SURGE_E_INVALID, "literal out of range");
    if (pt.kind == SURGE_JP_STR) {
      if (pt.field_offset >= SURGE_JSON_STRING_COLUMNS || !h->json_side.str_off[pt.field_offset])
        return fail(h, SURGE_E_INVALID, "SURGE_JP_STR names a string column that was not set (surge_replay_set_encode_strings)");
    } else if (pt.kind >= SURGE_JP_I32) {
      const uint32_t width = (pt.kind == SURGE_JP_I64 || pt.kind == SURGE_JP_F64) ? 8u : 4u;
      if (pt.field_offset + width > 64u || pt.field_offset % width) return fail(h, SURGE_E_INVALID, "field outside the 64-byte state or misaligned");
    }
    uses_f64 = uses_f64 || pt.kind == SURGE_JP_F64;
  }
  return uses_f64 ? 1 : 0;
}

static int32_t encode_tables(surge_replay_handle* h, bool uses_f64) {
  if (uses_f64 && !h->json_side.f64) {  // the power-of-5 tables of the Double text: one 10.7 KB copy per handle
    HIPCHK(h, h->f64_tables.reserve(sizeof(F64Tables)));
    HIPCHK(h, hipMemcpy(h->f64_tables.ptr, f64_tables_host(), sizeof(F64Tables), hipMemcpyHostToDevice));
    h->json_side.f64 = (const F64Tables*)h->f64_tables.ptr;
  }
  if (!h->json_side.not_a_number) {  // two counters: aggregates without a number text, rows outside the state (the rows encoders)
    HIPCHK(h, h->nan_count.reserve(16));
    h->json_side.not_a_number = (unsigned long long*)h->nan_count.ptr;
  }
  HIPCHK(h, hipMemsetAsync(h->nan_count.ptr, 0, 16, h->stream));
  return SURGE_OK;
}

static int32_t encode_states(surge_replay_handle* h, const surge_json_template* tmpl, const uint8_t* d_keys_utf8,
                             const int64_t* d_key_off, uint8_t* d_out, int64_t out_capacity, int64_t* d_out_off,
                             int64_t* total_bytes_out, uint32_t envelope) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound || h->st.n_folds == 0) return fail(h, SURGE_E_STATE, "encode_json before fold");
  if (!tmpl || !d_key_off || !d_out_off || !total_bytes_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  const int32_t uses_f64 = encode_prepare(h, tmpl);
  if (uses_f64 < 0) return uses_f64;
  *total_bytes_out = 0;
  if (h->n_agg == 0) return SURGE_OK;
  DeviceGuard g(h->device);
  SURGE_TRY(encode_tables(h, uses_f64 != 0));
  const int64_t nb = (h->n_agg + 1023) / 1024;
  HIPCHK(h, h->scan_totals.reserve((size_t)(nb + 1) * 8));
  HIPCHK(h, launch_json_encode(*tmpl, h->d_state, h->n_agg, d_keys_utf8, d_key_off, d_out_off, (int64_t*)h->scan_totals.ptr,
                               d_out, false, envelope, h->encode_filter, h->json_side, h->stream));
  int64_t total = 0;
  unsigned long long not_numbers = 0;
  HIPCHK(h, hipMemcpyAsync(&total, (int64_t*)h->scan_totals.ptr + nb, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&not_numbers, h->nan_count.ptr, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpyAsync(d_out_off + h->n_agg, &total, 8, hipMemcpyHostToDevice, h->stream));
  *total_bytes_out = total;
  if (total > out_capacity) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return fail(h, SURGE_E_RANGE, "output buffer too small for the encoded snapshot");
  }
  if (total > 0 && !d_out) return fail(h, SURGE_E_INVALID, "d_out is NULL");
  HIPCHK(h, launch_json_encode(*tmpl, h->d_state, h->n_agg, d_keys_utf8, d_key_off, d_out_off, (int64_t*)h->scan_totals.ptr,
                               d_out, true, envelope, h->encode_filter, h->json_side, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (not_numbers)
    return fail(h, SURGE_E_UNSUPPORTED, std::to_string(not_numbers) + " aggregate(s) hold a NaN / infinite Double: no JSON number exists (the "
                                        "reference's writeState throws); they were encoded as zero bytes, everything else is valid");
  return SURGE_OK;
}

// The encoders over a row list: the same two passes, over n_rows output slots.  Pass 1 leaves its lengths in the handle's own
// scratch, so a call that is refused — a row outside the state, a buffer too small — has written nothing the caller owns.
static int32_t encode_rows(surge_replay_handle* h, const surge_json_template* tmpl, const uint8_t* d_keys_utf8, const int64_t* d_key_off,
                           const int64_t* d_rows, int64_t n_rows, uint8_t* d_out, int64_t out_capacity, int64_t* d_out_off, uint8_t* d_kind_out,
                           int64_t* total_bytes_out, uint32_t envelope) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound || h->st.n_folds == 0) return fail(h, SURGE_E_STATE, "encode_json_rows before fold");
  if (!tmpl || !d_out_off || !total_bytes_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  if (n_rows < 0 || out_capacity < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_rows > 0 && (!d_rows || !d_key_off)) return fail(h, SURGE_E_INVALID, "NULL argument");
  const int32_t uses_f64 = encode_prepare(h, tmpl);
  if (uses_f64 < 0) return uses_f64;
  *total_bytes_out = 0;
  DeviceGuard g(h->device);
  if (n_rows == 0) {
    HIPCHK(h, hipMemsetAsync(d_out_off, 0, 8, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SURGE_OK;
  }
  SURGE_TRY(encode_tables(h, uses_f64 != 0));
  const int64_t nb = (n_rows + 1023) / 1024;
  HIPCHK(h, h->scan_totals.reserve((size_t)(nb + 1) * 8));
  HIPCHK(h, h->rows_off.reserve_roomy((size_t)(n_rows + 1) * 8));
  int64_t* off = (int64_t*)h->rows_off.ptr;
  const JsonRows rw{d_rows, h->n_agg, d_kind_out, (unsigned long long*)h->nan_count.ptr + 1};
  HIPCHK(h, launch_json_encode(*tmpl, h->d_state, n_rows, d_keys_utf8, d_key_off, off, (int64_t*)h->scan_totals.ptr, d_out, false, envelope, nullptr,
                               h->json_side, h->stream, &rw));
  int64_t total = 0;
  unsigned long long counts[2] = {0, 0};  // rows without a number text, rows outside the state
  HIPCHK(h, hipMemcpyAsync(&total, (int64_t*)h->scan_totals.ptr + nb, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(counts, h->nan_count.ptr, 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (counts[1])
    return fail(h, SURGE_E_INVALID, std::to_string(counts[1]) + " row(s) outside [-1, n_agg = " + std::to_string(h->n_agg) + "): nothing was written");
  *total_bytes_out = total;
  if (total > out_capacity) return fail(h, SURGE_E_RANGE, "output buffer too small for the encoded rows");
  if (total > 0 && !d_out) return fail(h, SURGE_E_INVALID, "d_out is NULL");
  HIPCHK(h, hipMemcpyAsync(off + n_rows, &total, 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_out_off, off, (size_t)(n_rows + 1) * 8, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, launch_json_encode(*tmpl, h->d_state, n_rows, d_keys_utf8, d_key_off, off, (int64_t*)h->scan_totals.ptr, d_out, true, envelope, nullptr,
                               h->json_side, h->stream, &rw));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (counts[0])
    return fail(h, SURGE_E_UNSUPPORTED, std::to_string(counts[0]) + " row(s) name an aggregate that holds a NaN / infinite Double: no JSON number exists (the "
                                        "reference's writeState throws); they were encoded as zero bytes (SURGE_READ_NOT_A_NUMBER), everything else is valid");
  return SURGE_OK;
}

int32_t surge_replay_set_encode_strings(surge_replay_handle* h, int32_t column, const uint8_t* d_utf8, const int64_t* d_off) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return fail(h, SURGE_E_INVALID, "string column out of range");
  h->json_side.str[column] = d_utf8;
  h->json_side.str_off[column] = d_off;
  return SURGE_OK;
}

int32_t surge_replay_encode_json(surge_replay_handle* h, const surge_json_template* tmpl, const uint8_t* d_keys_utf8,
                                 const int64_t* d_key_off, uint8_t* d_out, int64_t out_capacity, int64_t* d_out_off,
                                 int64_t* total_bytes_out) {
  return encode_states(h, tmpl, d_keys_utf8, d_key_off, d_out, out_capacity, d_out_off, total_bytes_out, 0u);
}

int32_t surge_replay_encode_protobuf_state(surge_replay_handle* h, const surge_json_template* payload_tmpl,
                                           const uint8_t* d_keys_utf8, const int64_t* d_key_off, uint8_t* d_out,
                                           int64_t out_capacity, int64_t* d_out_off, int64_t* total_bytes_out) {
  return encode_states(h, payload_tmpl, d_keys_utf8, d_key_off, d_out, out_capacity, d_out_off, total_bytes_out, 1u);
}

int32_t surge_replay_encode_json_rows(surge_replay_handle* h, const surge_json_template* tmpl, const uint8_t* d_keys_utf8, const int64_t* d_key_off,
                                      const int64_t* d_rows, int64_t n_rows, uint8_t* d_out, int64_t out_capacity, int64_t* d_out_off, uint8_t* d_kind_out,
                                      int64_t* total_bytes_out) {
  return encode_rows(h, tmpl, d_keys_utf8, d_key_off, d_rows, n_rows, d_out, out_capacity, d_out_off, d_kind_out, total_bytes_out, 0u);
}

int32_t surge_replay_encode_protobuf_state_rows(surge_replay_handle* h, const surge_json_template* payload_tmpl, const uint8_t* d_keys_utf8,
                                                const int64_t* d_key_off, const int64_t* d_rows, int64_t n_rows, uint8_t* d_out, int64_t out_capacity,
                                                int64_t* d_out_off, uint8_t* d_kind_out, int64_t* total_bytes_out) {
  return encode_rows(h, payload_tmpl, d_keys_utf8, d_key_off, d_rows, n_rows, d_out, out_capacity, d_out_off, d_kind_out, total_bytes_out, 1u);
}

int32_t surge_replay_set_decode_base(surge_replay_handle* h, const void* state64) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (state64) std::memcpy(h->decode_base, state64, 64); else std::memset(h->decode_base, 0, 64);
  return SURGE_OK;
}

int32_t surge_replay_set_decode_mode(surge_replay_handle* h, int32_t mode) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (mode != SURGE_STATE_READ_STRICT && mode != SURGE_STATE_READ_LENIENT) return fail(h, SURGE_E_INVALID, "unknown decode mode (SURGE_STATE_READ_*)");
  h->decode_mode = mode;
  return SURGE_OK;
}

// envelope: every value is a protobuf State message around the template's text (surge_replay_decode_protobuf_states)
static int32_t decode_states(surge_replay_handle* h, const surge_json_template* tmpl, const uint8_t* d_values, const int64_t* d_value_off,
                             int64_t n_records, const uint8_t* d_keys_utf8, const int64_t* d_key_off, const int64_t* d_agg_idx, int64_t n_agg,
                             void* d_states64, uint8_t* d_status_out, int64_t* d_str_span_out, int64_t counts_out[4], bool envelope) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (h->v2) return fail(h, SURGE_E_UNSUPPORTED, envelope ? "decode_protobuf_states serves ABI v1 handles (a slot schema keeps its presence word elsewhere)" : "decode_json_states serves ABI v1 handles (a slot schema keeps its presence word elsewhere)");
  if (const char* why = state_template_problem(tmpl)) return fail(h, SURGE_E_INVALID, why);
  const bool lenient = h->decode_mode == SURGE_STATE_READ_LENIENT;
  StateFieldTable fields{};
  if (lenient) {  // the template as the lenient parser reads it: refused here, before anything is launched
    uint32_t bad_part = 0;
    if (const char* why = state_field_table(tmpl, &fields, &bad_part))
      return fail(h, SURGE_E_UNSUPPORTED, std::string("the lenient decode mode cannot read this template: ") + why + " (part " + std::to_string(bad_part) + ")");
  }
  if (!counts_out) return fail(h, SURGE_E_INVALID, "counts_out is NULL");
  counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
  if (n_records < 0 || n_agg < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (!d_agg_idx && n_records > n_agg) return fail(h, SURGE_E_INVALID, "more records than aggregates and no d_agg_idx");
  if ((d_keys_utf8 && !d_key_off)) return fail(h, SURGE_E_INVALID, "d_keys_utf8 without d_key_off");
  if (n_records == 0) return SURGE_OK;
  if (!d_value_off || !d_states64) return fail(h, SURGE_E_INVALID, "NULL argument");
  if ((uintptr_t)d_states64 & 15u) return fail(h, SURGE_E_INVALID, "d_states64 is not 16-byte aligned");
  DeviceGuard g(h->device);
  if (!h->sd_ptab.ptr) {  // the Eisel-Lemire table of the Double parser: one 10.4 KB copy per handle
    HIPCHK(h, h->sd_ptab.reserve(sizeof(F64ParseTable)));
    HIPCHK(h, hipMemcpy(h->sd_ptab.ptr, f64_parse_table_host(), sizeof(F64ParseTable), hipMemcpyHostToDevice));
  }
  HIPCHK(h, h->sd_counts.reserve(SD_N_COUNTS * 8));
  if (d_agg_idx) HIPCHK(h, h->sd_last.reserve_roomy((size_t)n_agg * 8));
  if (!d_status_out) HIPCHK(h, h->sd_status.reserve_roomy((size_t)n_records));  // (the re-parse below finds its records by status)
  StateDecodeParams p{};
  p.values = d_values; p.value_off = d_value_off; p.n_records = n_records;
  p.keys = d_keys_utf8; p.key_off = d_key_off;
  p.agg_idx = d_agg_idx; p.last1 = (unsigned long long*)h->sd_last.ptr; p.n_agg = n_agg;
  p.states = (uint4*)d_states64;
  p.status = d_status_out ? d_status_out : (uint8_t*)h->sd_status.ptr;
  p.spans = d_str_span_out;
  p.ptab = (const F64ParseTable*)h->sd_ptab.ptr;
  p.counts = (unsigned long long*)h->sd_counts.ptr;
  p.envelope = envelope;
  p.lenient = lenient;
  // the base row, without the bytes the template names and the flags word: the kernel ORs it into the parsed row
  alignas(16) uint8_t base[64];
  std::memcpy(base, h->decode_base, 64);
  std::memset(base + 36, 0, 4);
  for (uint32_t i = 0; i < tmpl->n_parts; ++i) {
    const uint32_t k = tmpl->part[i].kind;
    if (k >= SURGE_JP_I32 && k <= SURGE_JP_F64) std::memset(base + tmpl->part[i].field_offset, 0, (k == SURGE_JP_I64 || k == SURGE_JP_F64) ? 8 : 4);
  }
  std::memcpy(p.base, base, 64);
  // rows of the handle's own resident state change: what the host mirror holds is no longer the current fold epoch's
  const uint4* s0 = (const uint4*)d_states64;
  const bool resident = h->d_state && s0 < h->d_state + h->n_agg * 4 && h->d_state < s0 + n_agg * 4;
  std::unique_lock<std::shared_mutex> lk(h->mu, std::defer_lock);
  if (resident) lk.lock();
  HIPCHK(h, launch_state_decode(*tmpl, p, h->stream, lenient ? &fields : nullptr));
  unsigned long long c[SD_N_COUNTS] = {0};
  HIPCHK(h, hipMemcpyAsync(c, p.counts, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (c[SD_BAD_INDEX])
    return fail(h, SURGE_E_INVALID, std::to_string(c[SD_BAD_INDEX]) + " d_agg_idx entr(y/ies) outside [0, n_agg): nothing was written");
  if (resident) h->fold_epoch.fetch_add(1);
  int64_t refused = (int64_t)c[SD_REFUSED], first_refused = refused ? (int64_t)c[SD_FIRST_REFUSED] : -1, written = (int64_t)c[SD_WRITTEN];
  int32_t first_status = 0;
  if (c[SD_AMBIGUOUS]) {
    // the rare Double the Eisel-Lemire product cannot decide (or one of more than 19 digits): those records come back and
    // go through the host export (strtod), as the device decoder of events hands its undecided records back
    std::vector<uint8_t> status((size_t)n_records);
    std::vector<int64_t> off((size_t)n_records + 1), agg;
    HIPCHK(h, hipMemcpyAsync(status.data(), p.status, (size_t)n_records, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(off.data(), d_value_off, ((size_t)n_records + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    if (d_agg_idx) {
      agg.resize((size_t)n_records);
      HIPCHK(h, hipMemcpyAsync(agg.data(), d_agg_idx, (size_t)n_records * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<uint8_t> text, key;
    for (int64_t r = 0; r < n_records; ++r) {
      if (status[(size_t)r] != SURGE_STATE_DECODE_AMBIGUOUS) continue;
      const int64_t a = d_agg_idx ? agg[(size_t)r] : r;
      text.resize((size_t)(off[(size_t)r + 1] - off[(size_t)r]));
      HIPCHK(h, hipMemcpyAsync(text.data(), d_values + off[(size_t)r], text.size(), hipMemcpyDeviceToHost, h->stream));
      int64_t key_len = -1;
      if (d_key_off) {
        int64_t ko[2];
        HIPCHK(h, hipMemcpyAsync(ko, d_key_off + a, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        key_len = ko[1] - ko[0];
        key.resize((size_t)key_len);
        if (key_len > 0) HIPCHK(h, hipMemcpyAsync(key.data(), d_keys_utf8 + ko[0], (size_t)key_len, hipMemcpyDeviceToHost, h->stream));
      }
      HIPCHK(h, hipStreamSynchronize(h->stream));
      alignas(16) uint8_t row[64];
      int64_t span[2 * SURGE_JSON_STRING_COLUMNS];
      // (in envelope mode the span comes back relative to the value, as the kernel reports it)
      const auto host_decode = lenient ? (envelope ? surge_decode_protobuf_state_lenient : surge_decode_json_state_lenient)
                                       : (envelope ? surge_decode_protobuf_state : surge_decode_json_state);
      const int32_t rc = host_decode(tmpl, text.data(), (int64_t)text.size(), key.data(), key_len, row, span);
      const uint8_t st = (uint8_t)(rc < 0 ? SURGE_STATE_DECODE_NUMBER : rc);
      if (rc == SURGE_STATE_DECODE_OK) {
        for (int b = 0; b < 64; ++b) row[b] |= base[b];
        HIPCHK(h, hipMemcpyAsync((uint8_t*)d_states64 + a * 64, row, 64, hipMemcpyHostToDevice, h->stream));
        if (d_str_span_out) HIPCHK(h, hipMemcpyAsync(d_str_span_out + r * (2 * SURGE_JSON_STRING_COLUMNS), span, sizeof(span), hipMemcpyHostToDevice, h->stream));
        ++written;
      } else {
        ++refused;
        if (first_refused < 0 || r < first_refused) first_refused = r;
      }
      HIPCHK(h, hipMemcpyAsync(p.status + r, &st, 1, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));  // (row / span / st are this iteration's)
    }
  }
  counts_out[0] = written;
  counts_out[1] = (int64_t)c[SD_TOMBSTONES];
  counts_out[2] = refused;
  counts_out[3] = (int64_t)c[SD_AMBIGUOUS];
  if (refused) {
    uint8_t st = 0;
    HIPCHK(h, hipMemcpyAsync(&st, p.status + first_refused, 1, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    first_status = st;
    return fail(h, SURGE_E_CORRUPT, std::to_string(refused) + " state value(s) were refused (their rows are untouched), the first at record " +
                                    std::to_string(first_refused) + " with status " + std::to_string(first_status) +
                                    " (SURGE_STATE_DECODE_*); everything else was decoded");
  }
  return SURGE_OK;
}

int32_t surge_replay_decode_json_states(surge_replay_handle* h, const surge_json_template* tmpl, const uint8_t* d_values,
                                        const int64_t* d_value_off, int64_t n_records, const uint8_t* d_keys_utf8,
                                        const int64_t* d_key_off, const int64_t* d_agg_idx, int64_t n_agg, void* d_states64,
                                        uint8_t* d_status_out, int64_t* d_str_span_out, int64_t counts_out[4]) {
  return decode_states(h, tmpl, d_values, d_value_off, n_records, d_keys_utf8, d_key_off, d_agg_idx, n_agg, d_states64, d_status_out, d_str_span_out,
                       counts_out, false);
}

int32_t surge_replay_decode_protobuf_states(surge_replay_handle* h, const surge_json_template* payload_tmpl, const uint8_t* d_values,
                                            const int64_t* d_value_off, int64_t n_records, const uint8_t* d_keys_utf8,
                                            const int64_t* d_key_off, const int64_t* d_agg_idx, int64_t n_agg, void* d_states64,
                                            uint8_t* d_status_out, int64_t* d_str_span_out, int64_t counts_out[4]) {
  return decode_states(h, payload_tmpl, d_values, d_value_off, n_records, d_keys_utf8, d_key_off, d_agg_idx, n_agg, d_states64, d_status_out,
                       d_str_span_out, counts_out, true);
}

int32_t surge_replay_merge_state_strings(surge_replay_handle* h, int32_t column, const uint8_t* d_values, const int64_t* d_value_off, int64_t n_records,
                                         const int64_t* d_agg_idx, const uint8_t* d_status, const int64_t* d_str_span, const uint8_t* d_prev_utf8,
                                         const int64_t* d_prev_off, int64_t n_prev, int64_t n_agg, uint8_t* d_out_utf8, int64_t out_capacity,
                                         int64_t* d_out_off, int64_t* total_bytes_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (column < 0 || column >= SURGE_JSON_STRING_COLUMNS) return fail(h, SURGE_E_INVALID, "string column out of range");
  if (n_records < 0 || n_prev < 0 || out_capacity < 0) return fail(h, SURGE_E_INVALID, "negative size");
  if (n_agg < n_prev) return fail(h, SURGE_E_INVALID, "n_agg is below n_prev: a column never shrinks");
  if (!d_out_off || !total_bytes_out) return fail(h, SURGE_E_INVALID, "NULL argument");
  if (n_prev > 0 && !d_prev_off) return fail(h, SURGE_E_INVALID, "d_prev_off is NULL");
  if (n_records > 0 && (!d_value_off || !d_status || !d_str_span)) return fail(h, SURGE_E_INVALID, "NULL argument");
  if (!d_agg_idx && n_records > n_agg) return fail(h, SURGE_E_INVALID, "more records than aggregates and no d_agg_idx");
  *total_bytes_out = 0;
  DeviceGuard g(h->device);
  StateStringsParams p{};
  p.values = d_values; p.value_off = d_value_off; p.n_records = n_records;
  p.agg_idx = d_agg_idx; p.status = d_status; p.spans = d_str_span; p.column = column;
  p.n_agg = n_agg;
  p.prev = d_prev_utf8; p.prev_off = d_prev_off; p.n_prev = n_prev;
  p.out = d_out_utf8; p.out_off = d_out_off;
  if (n_records > 0) {  // the winners first, and with them the indices: an entry outside [0, n_agg) ends the call before anything is written
    HIPCHK(h, h->sd_counts.reserve(SD_N_COUNTS * 8));
    HIPCHK(h, h->sd_last.reserve_roomy((size_t)n_agg * 8));
    p.win1 = (unsigned long long*)h->sd_last.ptr;
    unsigned long long* d_bad = (unsigned long long*)h->sd_counts.ptr + SD_BAD_INDEX;
    unsigned long long bad = 0;
    HIPCHK(h, launch_state_strings_winners(p, d_bad, h->stream));
    HIPCHK(h, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad) return fail(h, SURGE_E_INVALID, std::to_string(bad) + " d_agg_idx entr(y/ies) outside [0, n_agg): nothing was written");
  }
  const int64_t nb = (n_agg + 1023) / 1024;
  int64_t total = 0;
  if (n_agg > 0) {
    HIPCHK(h, h->scan_totals.reserve((size_t)(nb + 1) * 8));
    HIPCHK(h, launch_state_strings_pass(p, false, h->stream));
    HIPCHK(h, launch_scan_lengths_i64(d_out_off, n_agg, (int64_t*)h->scan_totals.ptr, h->stream));
    HIPCHK(h, hipMemcpyAsync(&total, (int64_t*)h->scan_totals.ptr + nb, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  HIPCHK(h, hipMemcpyAsync(d_out_off + n_agg, &total, 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *total_bytes_out = total;
  if (total > out_capacity) return fail(h, SURGE_E_RANGE, "output buffer too small for the string column");
  if (total > 0 && !d_out_utf8) return fail(h, SURGE_E_INVALID, "d_out_utf8 is NULL");
  if (total > 0) {
    HIPCHK(h, launch_state_strings_pass(p, true, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return SURGE_OK;
}

int32_t surge_replay_snapshot_delta(surge_replay_handle* h, uint8_t* d_kind_out, int64_t* n_values_out, int64_t* n_tombstones_out,
                                    int32_t commit) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound || h->st.n_folds == 0) return fail(h, SURGE_E_STATE, "snapshot_delta before fold");
  if (!d_kind_out && h->n_agg > 0) return fail(h, SURGE_E_INVALID, "d_kind_out is NULL");
  DeviceGuard g(h->device);
  if (h->published_n < h->n_agg) {  // first use, or the resident state grew: new aggregates have never been published
    const size_t want = (size_t)h->n_agg * 64;
    if (want > h->published.cap) {
      void* fresh = nullptr;
      size_t cap = h->published.cap * 2 > want ? h->published.cap * 2 : want;
      HIPCHK(h, hipMalloc(&fresh, cap));
      if (h->published_n > 0)
        HIPCHK(h, hipMemcpyAsync(fresh, h->published.ptr, (size_t)h->published_n * 64, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (h->published.ptr) (void)hipFree(h->published.ptr);
      h->published.ptr = fresh;
      h->published.cap = cap;
    }
    HIPCHK(h, hipMemsetAsync((char*)h->published.ptr + (size_t)h->published_n * 64, 0, (size_t)(h->n_agg - h->published_n) * 64, h->stream));
    h->published_n = h->n_agg;
  }
  HIPCHK(h, h->poison_count.reserve(16));
  HIPCHK(h, launch_snapshot_delta(h->d_state, (uint4*)h->published.ptr, h->n_agg, d_kind_out, (unsigned long long*)h->poison_count.ptr,
                                  commit != 0, h->v2, h->stream));
  unsigned long long c[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(c, h->poison_count.ptr, 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (n_values_out) *n_values_out = (int64_t)c[0];
  if (n_tombstones_out) *n_tombstones_out = (int64_t)c[1];
  h->delta_epoch = h->fold_epoch.load();
  h->delta_n = h->n_agg;
  return SURGE_OK;
}

int32_t surge_replay_snapshot_commit(surge_replay_handle* h, const uint8_t* d_kind) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound || h->published_n < h->n_agg) return fail(h, SURGE_E_STATE, "snapshot_commit without a preceding snapshot_delta");
  if (!d_kind && h->n_agg > 0) return fail(h, SURGE_E_INVALID, "d_kind is NULL");
  // the commit copies the CURRENT states of the reported aggregates into the baseline: after a fold / append / grow they
  // are no longer the states that were encoded, and a newer state would count as published without ever being emitted
  if (h->delta_epoch != h->fold_epoch.load() || h->delta_n != h->n_agg)
    return fail(h, SURGE_E_STATE, "snapshot_commit: the resident state changed since the snapshot_delta whose kinds these are "
                                  "(fold / append / grow in between); take a new delta");
  DeviceGuard g(h->device);
  HIPCHK(h, launch_snapshot_commit(h->d_state, (uint4*)h->published.ptr, h->n_agg, d_kind, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SURGE_OK;
}

int32_t surge_replay_snapshot_invalidate(surge_replay_handle* h, const uint8_t* d_kind) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound || h->delta_n < 0 || h->published_n < h->delta_n) return fail(h, SURGE_E_STATE, "snapshot_invalidate without a preceding snapshot_delta");
  if (!d_kind && h->delta_n > 0) return fail(h, SURGE_E_INVALID, "d_kind is NULL");
  DeviceGuard g(h->device);
  // d_kind holds delta_n entries: the store may have grown (and folded) since; the aggregates added later have no
  // baseline to invalidate, and invalidating an older aggregate only makes the next delta report it again
  HIPCHK(h, launch_snapshot_invalidate((uint4*)h->published.ptr, h->delta_n, d_kind, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SURGE_OK;
}

int32_t surge_replay_set_encode_filter(surge_replay_handle* h, const uint8_t* d_kind) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  h->encode_filter = d_kind;
  return SURGE_OK;
}

int32_t surge_replay_device_state(surge_replay_handle* h, void** d_states, int64_t* n_agg) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "device_state before load_csr/bind_device_csr");
  if (d_states) *d_states = h->d_state;
  if (n_agg) *n_agg = h->n_agg;
  return SURGE_OK;
}

int32_t surge_replay_set_state_out(surge_replay_handle* h, void* d_state_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(h, SURGE_E_STATE, "set_state_out before load_csr/bind_device_csr");
  if (!d_state_out || ((uintptr_t)d_state_out & 15)) return fail(h, SURGE_E_INVALID, "state buffer must be non-NULL and 16-byte aligned");
  h->d_state = (uint4*)d_state_out;
  h->fold_epoch.fetch_add(1);
  return SURGE_OK;
}

int32_t surge_replay_pack_states(surge_replay_handle* h, const void* d_states64, int64_t n, void* d_packed40, void* hip_stream) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n < 0 || (n > 0 && (!d_states64 || !d_packed40))) return fail(h, SURGE_E_INVALID, "bad argument");
  if (((uintptr_t)d_states64 & 7) || ((uintptr_t)d_packed40 & 7)) return fail(h, SURGE_E_INVALID, "buffers must be 8-byte aligned");
  DeviceGuard g(h->device);
  HIPCHK(h, launch_pack_states(d_states64, n, d_packed40, false, hip_stream ? (hipStream_t)hip_stream : h->stream));
  return SURGE_OK;
}

int32_t surge_replay_unpack_states(surge_replay_handle* h, const void* d_packed40, int64_t n, void* d_states64, void* hip_stream) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (n < 0 || (n > 0 && (!d_states64 || !d_packed40))) return fail(h, SURGE_E_INVALID, "bad argument");
  if (((uintptr_t)d_states64 & 7) || ((uintptr_t)d_packed40 & 7)) return fail(h, SURGE_E_INVALID, "buffers must be 8-byte aligned");
  DeviceGuard g(h->device);
  HIPCHK(h, launch_pack_states(d_packed40, n, d_states64, true, hip_stream ? (hipStream_t)hip_stream : h->stream));
  return SURGE_OK;
}

}  // extern "C"
