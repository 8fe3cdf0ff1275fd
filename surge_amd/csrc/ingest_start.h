// ingest_start.h — the exports of the host framer's start offsets, floors list and positions (include/surge_ingest.h, "start
// offsets and positions").  Part of ingest.cpp's translation unit — included at its end: surge_ingest, surge_ingest_group and
// position_of are that file's.  A file of its own because ingest.cpp's messages are held, one by one, to a recorded trace of the
// framer (tests/test_ingest_trace.py over tests/ingest_trace.py) that predates these calls; their refusals are tested where
// the calls are (tests/test_start_offsets.py).  What a start offset DOES is in ingest.cpp, where batches are handed out:
// visit_ready, ready_count, parse_records' flush record, surge_ingest_drain_sections, surge_ingest_group_feed's floors.
#pragma once

extern "C" {

int32_t surge_ingest_set_start_offset(surge_ingest* g, int64_t first_offset) {
  if (!g) return fail(nullptr, E_INVALID, "handle is NULL");
  if (g->start.fed) return fail(g, -2, "surge_ingest_set_start_offset after the first feed");
  g->start.first = first_offset > 0 ? first_offset : 0;
  return OK;
}

int32_t surge_ingest_group_set_start_offsets(surge_ingest_group* grp, const int64_t* first_offset) {
  if (!grp || !first_offset) return fail(nullptr, E_INVALID, "bad argument");
  for (const surge_ingest* x : grp->g)
    if (x->start.fed) { grp->err = "surge_ingest_group_set_start_offsets after the first feed"; return -2; }
  for (size_t p = 0; p < grp->g.size(); ++p) grp->g[p]->start.first = first_offset[p] > 0 ? first_offset[p] : 0;
  return OK;
}

int64_t surge_ingest_position(const surge_ingest* g) { return g ? position_of(g) : 0; }

int32_t surge_ingest_group_positions(const surge_ingest_group* grp, int64_t* out) {
  if (!grp || !out) return E_INVALID;
  for (size_t p = 0; p < grp->g.size(); ++p) out[p] = position_of(grp->g[p]);
  return OK;
}

int32_t surge_ingest_take_floors(surge_ingest* g, int64_t max, surge_section_floor* out, int64_t* n_out) {
  if (!g || !n_out || max < 0 || (!out && max > 0)) return fail(g, E_INVALID, "bad argument");
  *n_out = g->start.floored_section >= 0 ? 1 : 0;
  if (*n_out > max) return fail(g, E_INVALID, "floors table too small (n_out entries are needed)");
  if (*n_out) out[0] = surge_section_floor{0, 0, g->start.floored_section, g->start.first};
  return OK;
}

int32_t surge_ingest_group_take_floors(surge_ingest_group* grp, int64_t max, surge_section_floor* out, int64_t* n_out) {
  if (!grp || !n_out || max < 0 || (!out && max > 0)) return fail(nullptr, E_INVALID, "bad argument");
  *n_out = (int64_t)grp->floors.size();
  if (*n_out > max) { grp->err = "floors table too small (n_out entries are needed)"; return E_INVALID; }
  for (size_t i = 0; i < grp->floors.size(); ++i) out[i] = grp->floors[i];
  return OK;
}

int32_t surge_ingest_below_start(const surge_ingest* g, int64_t out[2]) {
  if (!g || !out) return E_INVALID;
  out[0] = g->start.discarded_batches;
  out[1] = g->start.dropped_records;
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
