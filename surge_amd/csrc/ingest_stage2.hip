// ingest_stage2.hip — stage 2 of a push of the device decoder (ingest_decoder_internal.h): everything behind the per-record
// metadata and decoded values — interning, compaction, append — on the decoder's stream, one push after the other.  The
// kernels are ingest_intern.hip's; this unit says what is launched when, and names a push's failure.
#include "ingest_decoder_internal.h"

using namespace surge::ingest;
using namespace surge::ingest::host;

namespace {

// what is wrong with a record, one text per status (ingest_device.h)
const char* const kWhyBad[] = {"", "", "has a null key or value (not an event)", "is malformed (a length runs past its record or batch)",
                               "is not the JSON object the event template describes", "names an event type the template does not know",
                               "lacks a field the template names, or the field is not the number it should be", "is not a 16-byte fixed event", "",
                               "collides with another key on its 64-bit hash",
                               "has an empty, non-null value under a key (a state record carries a value or the null of a tombstone)",
                               "is not the protobuf Event envelope the event template names ([aggregateId] [payload] and nothing else)",
                               "names another aggregateId in its envelope than the aggregate id of its key", "",
                               "lacks a string field its event class names (kept event strings), or that string is not a valid JSON string"};
static_assert(sizeof(kWhyBad) / sizeof(kWhyBad[0]) == RS_COUNT, "one text per record status");
const char* why_bad(uint32_t status) { return status < RS_COUNT ? kWhyBad[status] : "is bad"; }

// The offset of record `rec` of a wire push that the record stage found malformed: it gives up on such a record before it
// keeps its offset, so it is read here — section -> record -> offset — from the section's bytes as the device has them (an
// LZ4 section exists decompressed there only): the length varints up to the record, then its head.  false: not recovered.
bool malformed_record_offset(const PushSlot& s, int64_t rec, int64_t* offset) {
  size_t si = 0;
  while (si + 1 < s.h_secs.size() && s.h_secs[si + 1].rec_first <= rec) ++si;
  Section sec;
  std::vector<uint8_t> sb;
  if (si >= s.h_secs.size() || hipMemcpy(&sec, (const Section*)s.d_sections.p + si, sizeof(sec), hipMemcpyDeviceToHost) != hipSuccess || sec.byte_len <= 0 ||
      sec.byte_len >= (1ll << 31))
    return false;
  try { sb.resize((size_t)sec.byte_len); } catch (const std::bad_alloc&) { return false; }
  if (hipMemcpy(sb.data(), (const uint8_t*)s.d_bytes.p + sec.byte_off, sb.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
  size_t pos = 0;
  auto varlong = [&](int64_t* v) -> bool {
    uint64_t u = 0;
    for (int shift = 0; shift <= 63; shift += 7) {
      if (pos >= sb.size()) return false;
      const uint8_t b = sb[pos++];
      u |= (uint64_t)(b & 0x7f) << shift;
      if (!(b & 0x80)) { *v = (int64_t)(u >> 1) ^ -(int64_t)(u & 1); return true; }
    }
    return false;
  };
  int64_t len = 0, ts = 0, delta = 0;
  bool ok = true;
  for (int64_t k = sec.rec_first; ok && k < rec; ++k) {
    ok = varlong(&len) && len >= 0 && (uint64_t)len <= sb.size() - pos;
    if (ok) pos += (size_t)len;
  }
  if (!(ok && varlong(&len) && pos < sb.size() && (++pos, varlong(&ts)) && varlong(&delta))) return false;
  *offset = sec.base_offset + delta;
  return true;
}

// One push's stage 2: the names its steps share, and the steps in the order stage2() takes them.
struct Stage2 {
  surge_device_decoder* const d;
  PushSlot& s;
  EventStringsState& ev;  // kept event strings (ingest_columns.hip arms and merges them)
  const int64_t n_rec;
  const hipStream_t st;  // the decoder's
  const size_t R;
  const uint8_t* const dby;  // the slot's bytes, error cell and per-record metadata, as stage 1 left them
  ErrorCell* const derr;
  RecMeta* const dmeta;
  InternScratch scratch{};
  StateScratch values{};
  // what the push discovered (the middle wait brings it back): errors, new keys << 40 | their bytes, delivered records, their value bytes
  ErrorCell ec{};
  unsigned long long first_total = 0, val_total = 0;
  uint32_t kept = 0;
  int64_t n_new = 0, new_bytes = 0;
  // kept event strings (ingest_strings.hip): what the select found, the selected values' bytes
  StringsCell strings_cell{};
  int64_t n_sel = 0, sel_bytes = 0;

  Stage2(surge_device_decoder* d_, PushSlot& s_)
      : d(d_), s(s_), ev(d_->strings.ev), n_rec(s_.n_rec), st(d_->stream), R((size_t)s_.n_rec), dby((const uint8_t*)s_.d_bytes.p), derr((ErrorCell*)s_.d_err.p), dmeta((RecMeta*)s_.meta.p) {}

  // scratch (nothing of the push is in the table yet: an allocation failure here needs no rollback)
  int32_t reserve_scratch() {
    DCHK(d, d->first.reserve((R + 1) * 8, false, st));
    DCHK(d, d->first_scan.reserve((R + 1) * 8, false, st));
    DCHK(d, d->keep.reserve((R + 1) * 4, false, st));
    DCHK(d, d->keep_pos.reserve((R + 1) * 4, false, st));
    size_t temp_bytes = 0;
    DCHK(d, intern_temp_bytes(n_rec, &temp_bytes, st));
    DCHK(d, d->temp.reserve(temp_bytes, false, st));
    if (d->states) {
      DCHK(d, d->vlen.reserve((R + 1) * 8, false, st));
      DCHK(d, d->vscan.reserve((R + 1) * 8, false, st));
    }
    if (ev.armed) {
      const size_t n_blocks = (R + kStringsBlock - 1) / kStringsBlock;
      DCHK(d, ev.select.seg.reserve(n_blocks * kStringsBlock * 4, false, st));
      DCHK(d, ev.select.count.reserve(n_blocks * 4, false, st));
      DCHK(d, ev.select.base.reserve(n_blocks * 4, false, st));
      DCHK(d, ev.select.cell.reserve(sizeof(StringsCell), false, st));
    }
    const int32_t rc = ensure_table(d, n_rec);
    if (rc != OK) return rc;
    scratch = InternScratch{(unsigned long long*)d->first.p, (unsigned long long*)d->first_scan.p, (uint32_t*)d->keep.p, (uint32_t*)d->keep_pos.p, d->temp.p, d->temp.cap};
    values = StateScratch{(unsigned long long*)d->vlen.p, (unsigned long long*)d->vscan.p, nullptr, nullptr};
    return OK;
  }

  // behind stage 1 of the slot: probe the table, bring back what the push discovered — the FIRST synchronisation — and, on
  // a detected collision, re-seed and go again
  int32_t probe() {
    PCHK(d, hipStreamWaitEvent(st, s.done, 0));
    if (s.seed != d->seed) launch_rekey_records(dmeta, n_rec, dby, d->seed, st);  // the table was re-seeded after this push's stage 1 hashed its keys
    for (int attempt = 0;; ++attempt) {
      PCHK(d, launch_intern_probe(dmeta, n_rec, dby, keys_of(d), scratch, derr, st));
      if (d->states) {  // the delivered records' value lengths, scanned: where each value goes, and how many bytes the push adds
        PCHK(d, launch_value_scan(dmeta, n_rec, scratch, values, st));
        PCHK(d, hipMemcpyAsync(&val_total, values.vscan + R, 8, hipMemcpyDeviceToHost, st));
      }
      if (ev.armed) {  // the kept records whose class carries a string, and how many they are
        PCHK(d, hipMemsetAsync(ev.select.cell.p, 0, sizeof(StringsCell), st));
        PCHK(d, launch_strings_select(scratch.keep, (const uint4*)s.ev_tmp.p, n_rec, ev.types, strings_select(), st));
        PCHK(d, hipMemcpyAsync(&strings_cell, ev.select.cell.p, sizeof(strings_cell), hipMemcpyDeviceToHost, st));
      }
      PCHK(d, hipMemcpyAsync(&ec, derr, sizeof(ec), hipMemcpyDeviceToHost, st));
      PCHK(d, hipMemcpyAsync(&first_total, (unsigned long long*)d->first_scan.p + R, 8, hipMemcpyDeviceToHost, st));
      PCHK(d, hipMemcpyAsync(&kept, (uint32_t*)d->keep_pos.p + R, 4, hipMemcpyDeviceToHost, st));
      PCHK(d, wait_stream(d, st));
      if (ec.lz4_bad == ~0u && ec.snappy_bad == ~0u && ec.crc_bad == ~0u && ec.first_bad != ~0ull && (uint32_t)(ec.first_bad & 0xff) == RS_COLLISION && attempt < 3) {
        // Two different keys share a 64-bit hash (about 3 in a million pushes at 10^7 keys): the table gets another hash
        // function — every known key re-hashed from its bytes in the arena, the push's records from theirs — and the push
        // goes through again.  Nothing of it was committed.
        d->seed = (d->seed & ~(1ull << 63)) + 1;
        ++d->reseeds;
        launch_intern_reseed(dmeta, n_rec, dby, keys_of(d), d->seed, st);
        s.h_err = ErrorCell{~0ull, 0u, ec.n_f64_host, ~0u, ~0u, ec.n_below, ~0u};
        PCHK(d, hipMemcpyAsync(derr, &s.h_err, sizeof(s.h_err), hipMemcpyHostToDevice, st));
        continue;
      }
      break;
    }
    d->counters[0] += n_rec;
    n_new = (int64_t)(first_total >> 40);
    new_bytes = (int64_t)(first_total & ((1ull << 40) - 1));
    n_sel = ev.armed ? (int64_t)strings_cell.n_sel : 0;
    return OK;
  }

  StringsSelect strings_select() const { return StringsSelect{(uint32_t*)ev.select.seg.p, (uint32_t*)ev.select.count.p, (uint32_t*)ev.select.base.p, (StringsCell*)ev.select.cell.p}; }

  // kept event strings, a push that selected records: their list, their strings validated by the rule where stage 1 left the
  // values — spans and statuses go straight behind what is pending — and the bytes their values take; the wait brings a refusal
  // back while nothing of the push is committed (a push that selected nothing has none of this)
  int32_t validate_strings() {
    const size_t keep_n = (size_t)(ev.pend.n + n_sel);
    hipError_t e = ev.select.sel.reserve((size_t)n_sel * 4, false, st);
    if (e == hipSuccess) e = ev.select.lens.reserve((size_t)n_sel * 8, false, st);
    if (e == hipSuccess) e = ev.select.totals.reserve((((size_t)n_sel + 1023) / 1024 + 1) * 8, false, st);
    if (e == hipSuccess) e = ev.pend.off.reserve((keep_n + 1) * 8, true, st);
    if (e == hipSuccess) e = ev.pend.rows.reserve(keep_n * 8, true, st);
    if (e == hipSuccess) e = ev.pend.spans.reserve(keep_n * (2 * SURGE_JSON_STRING_COLUMNS) * 8, true, st);
    for (int c = 0; c < SURGE_JSON_STRING_COLUMNS && e == hipSuccess; ++c) e = ev.pend.status[c].reserve(keep_n, true, st);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string("growing the kept event strings: ") + hipGetErrorString(e));
    int64_t* const lens = (int64_t*)ev.select.lens.p;
    int64_t* const totals = (int64_t*)ev.select.totals.p;
    PCHK(d, launch_strings_list(dmeta, n_rec, strings_select(), (uint32_t*)ev.select.sel.p, lens, st));
    PCHK(d, launch_strings_spans(ev.rule.p, dmeta, dby, (const uint32_t*)ev.select.sel.p, n_sel, ev.pending(), derr, st));
    PCHK(d, launch_strings_scan(lens, n_sel, totals, st));
    PCHK(d, hipMemcpyAsync(&sel_bytes, totals + (n_sel + 1023) / 1024, 8, hipMemcpyDeviceToHost, st));
    PCHK(d, hipMemcpyAsync(&ec, derr, sizeof(ec), hipMemcpyDeviceToHost, st));
    PCHK(d, wait_stream(d, st));
    return OK;
  }

  // nothing of this push is delivered and no key it discovered stays interned
  int32_t fail(int32_t code, const std::string& why) {
    launch_intern_rollback(dmeta, n_rec, keys_of(d).t, st);
    PCHK(d, hipStreamSynchronize(st));
    return dfail(d, code, why);
  }

  bool found_bad() const { return ec.crc_bad != ~0u || ec.lz4_bad != ~0u || ec.snappy_bad != ~0u || ec.first_bad != ~0ull; }

  // the push as a whole fails with its first bad batch or record, by name
  int32_t name_failure() {
    auto base_offset_of = [&](uint32_t section) { return std::to_string(section < s.h_secs.size() ? s.h_secs[section].base_offset : -1); };
    if (ec.crc_bad != ~0u) return fail(SURGE_E_CORRUPT, "record batch CRC-32C mismatch (verified on the device) in the batch at base offset " + base_offset_of(ec.crc_bad));
    if (ec.lz4_bad != ~0u)
      return fail(SURGE_E_CORRUPT, "bad LZ4 frame in the batch at base offset " + base_offset_of(ec.lz4_bad) + " (malformed sequence, or a block that is not 64 KiB where it must be)");
    if (ec.snappy_bad != ~0u)
      return fail(SURGE_E_CORRUPT, "bad snappy chunk in the batch at base offset " + base_offset_of(ec.snappy_bad) +
                                       " (an element that runs past the chunk, offset 0 or beyond the output, or output that misses the preamble's length)");
    const int64_t rec = (int64_t)(ec.first_bad >> 8);
    const uint32_t status = (uint32_t)(ec.first_bad & 0xff);
    RecMeta m;
    PCHK(d, hipMemcpy(&m, dmeta + rec, sizeof(m), hipMemcpyDeviceToHost));
    if (status == RS_MALFORMED && s.wire) {
      (void)malformed_record_offset(s, rec, &m.offset);
      (void)hipGetLastError();
    }
    return fail(status == RS_COLLISION ? E_UNSUPPORTED : SURGE_E_CORRUPT, "record " + std::to_string(rec) + " of the push (offset " + std::to_string(m.offset) + ") " +
                                                                             why_bad(status) + (status == RS_COLLISION ? " under four hash functions in a row" : ""));
  }

  // everything that can fail for want of memory, before the first commit
  int32_t grow() {
    hipError_t e = hipSuccess;
    if (n_new > 0) {
      e = d->key_off.reserve((size_t)(d->n_keys + n_new + 1) * 8, true, st);
      if (e == hipSuccess) e = d->key_hash.reserve((size_t)(d->n_keys + n_new) * 8, true, st);
      if (e == hipSuccess) e = d->arena.reserve((size_t)(d->arena_bytes + new_bytes) + 16, true, st);
    }
    if (e == hipSuccess) e = d->r_agg.reserve((size_t)(d->n_records + kept) * 8 + 16, true, st);
    if (e == hipSuccess && !d->states) e = d->r_ev.reserve((size_t)(d->n_records + kept) * 16 + 16, true, st);
    if (d->states) {  // (the values buffer ends at least 64 bytes behind its last value)
      const size_t n_runs = ((size_t)kept + kGatherRecs - 1) / kGatherRecs;
      if (e == hipSuccess) e = d->r_val_off.reserve((size_t)(d->n_records + kept + 1) * 8 + 16, true, st);
      if (e == hipSuccess) e = d->r_val.reserve((size_t)(d->val_bytes + (int64_t)val_total) + 64, true, st);
      if (e == hipSuccess) e = d->val_src.reserve((size_t)kept * 8 + 16, false, st);
      if (e == hipSuccess) e = d->long_runs.reserve((n_runs + 1) * 4, false, st);
    }
    if (e == hipSuccess) e = d->r_off.reserve((size_t)(d->n_records + kept) * 8 + 16, true, st);
    if (e == hipSuccess && n_sel > 0) e = ev.pend.val.reserve((size_t)(ev.pend.bytes + sel_bytes) + 64, true, st);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? E_NOMEM : E_DEVICE, std::string("growing the key table / result arrays: ") + hipGetErrorString(e));
    return OK;
  }

  // the new keys get their ids and arena bytes, the delivered records go to the result arrays (state mode: their values too)
  int32_t commit_and_gather() {
    if (d->consumed_valid) {  // an asynchronous consumer of the last results (surge_replay_append_decoded_async) reads the arrays finalize_kernel writes
      PCHK(d, hipStreamWaitEvent(st, d->consumed, 0));
      d->consumed_valid = false;
    }
    launch_intern_commit(dmeta, n_rec, dby, keys_of(d), scratch, n_new, (const uint4*)s.ev_tmp.p, d->n_records, (int64_t*)d->r_agg.p, d->states ? nullptr : (uint4*)d->r_ev.p,
                         (int64_t*)d->r_off.p, st);
    PCHK(d, hipGetLastError());
    if (d->states) {  // the values leave the slot's bytes (its next push writes those again) for the result's own buffer
      values.val_src = (int64_t*)d->val_src.p;
      values.long_runs = (uint32_t*)d->long_runs.p;
      PCHK(d, launch_value_gather(dmeta, n_rec, dby, scratch, values, kept, d->n_records, d->val_bytes, (int64_t*)d->r_val_off.p, (uint8_t*)d->r_val.p, st));
      d->val_bytes += (int64_t)val_total;
    }
    if (n_sel > 0) {  // the selected records' values leave the slot's bytes too, their rows beside them
      PCHK(d, launch_strings_gather(dmeta, dby, (const uint32_t*)ev.select.sel.p, (const int64_t*)ev.select.lens.p, n_sel, sel_bytes, (const uint32_t*)d->keep_pos.p,
                                    (const int64_t*)d->r_agg.p + d->n_records, ev.pending(), st));
      ev.pend.n += n_sel;
      ev.pend.bytes += sel_bytes;
    }
    d->n_keys += n_new;
    d->arena_bytes += new_bytes;
    return OK;
  }

  // Doubles the fast parser could not decide (more than 19 digits, or one of Eisel-Lemire's rare ambiguous products):
  // the host parses exactly those values with the library's host decoder and patches the payload in place
  int32_t patch_host_doubles() {
    if (ec.n_f64_host == 0) return OK;
    PCHK(d, hipStreamSynchronize(st));  // the results have to be in place before the payloads are patched
    std::vector<uint32_t> list(ec.n_f64_host);
    PCHK(d, hipMemcpy(list.data(), s.f64_list.p, (size_t)ec.n_f64_host * 4, hipMemcpyDeviceToHost));
    for (uint32_t i : list) {
      RecMeta m;
      uint32_t pos = 0;
      PCHK(d, hipMemcpy(&m, dmeta + i, sizeof(m), hipMemcpyDeviceToHost));
      PCHK(d, hipMemcpy(&pos, (uint32_t*)d->keep_pos.p + i, 4, hipMemcpyDeviceToHost));
      uint8_t ev[16];
      std::vector<uint8_t> value((size_t)m.val_len + 1);
      PCHK(d, hipMemcpy(value.data(), dby + m.val_off, (size_t)m.val_len, hipMemcpyDeviceToHost));  // (an LZ4 section exists decompressed on the device only)
      if (surge_event_json_decode(&d->h_tmpl, value.data(), m.val_len, ev) != 0)  // (the whole value and the template with its envelope; the device compared the id, accepted the number's spelling and its length: cannot happen)
        return poison(d, dfail(d, SURGE_E_CORRUPT, "record at offset " + std::to_string(m.offset) + ": " + surge_event_json_last_error()));
      PCHK(d, hipMemcpy((uint8_t*)d->r_ev.p + (size_t)(d->n_records + pos) * 16, ev, 16, hipMemcpyHostToDevice));
    }
    d->counters[3] += ec.n_f64_host;
    return OK;
  }

  // the books, and the SECOND synchronisation — or, without it, the point of the stream the slot's next stage 1 waits for
  int32_t close(bool wait) {
    d->chain_fallbacks += ec.reserved;
    d->n_records += kept;
    d->counters[1] += kept;
    d->counters[2] += n_rec - kept - ec.n_below;
    d->below_floor += ec.n_below;
    ++d->pushes;
    if (s.wire) {
      d->snappy_device_chunks += (int64_t)s.snappy.blocks.size();
      d->snappy_host_sections += s.snappy_host_sections;
    }
    if (wait) {
      PCHK(d, wait_stream(d, st));
    } else {  // the slot's buffers are read until here: its next stage 1 waits for this point of the stream
      PCHK(d, hipEventRecord(s.released, st));
      s.released_valid = true;
    }
    return OK;
  }
};

}  // namespace

// Two synchronisations: one in the middle (what the push discovered: errors, new keys, their bytes, delivered records —
// everything the allocations behind it need), one at the end.  Nothing is committed before the first: a push that fails
// takes the keys it probed out of the table again (rollback_kernel), so a failed push leaves the decoder exactly as it was.
// wait = false leaves the second synchronisation out: the results are complete in the order of the decoder's stream
// (surge_device_decoder_push_finish_async).
int32_t surge::ingest::host::stage2(surge_device_decoder* d, PushSlot& s, bool wait) {
  if (s.n_rec == 0) return OK;
  Stage2 push(d, s);
  int32_t rc = push.reserve_scratch();
  if (rc == OK) rc = push.probe();
  if (rc == OK && push.found_bad()) return push.name_failure();
  if (rc == OK && push.n_sel > 0) {
    rc = push.validate_strings();
    if (rc == OK && push.found_bad()) return push.name_failure();
  }
  if (rc == OK) rc = push.grow();
  if (rc == OK) rc = push.commit_and_gather();
  if (rc == OK) rc = push.patch_host_doubles();
  if (rc == OK) rc = push.close(wait);
  // more pending than the bound: the columns are merged now (the merge waits for the stream)
  if (rc == OK && push.ev.armed && push.ev.pend.n > push.ev.pend.bound) rc = merge_event_strings(d);
  return rc;
}
