// engine_comm.hip — the snapshot exchange between handles: the surge_replay_comm_* / allgather / gathered entry points over
// comm.hip.
#include <string>
#include <vector>

#include "engine_internal.h"

using namespace surge;

extern "C" {

int32_t surge_replay_comm_unique_id(uint8_t id_out[SURGE_COMM_ID_BYTES]) {
  if (!id_out) return fail(nullptr, SURGE_E_INVALID, "id_out is NULL");
  std::string err;
  const int32_t rc = comm_unique_id(id_out, &err);
  return rc == SURGE_OK ? rc : fail(nullptr, rc, err);
}

int32_t surge_replay_comm_init(surge_replay_handle* h, int32_t rank, int32_t world, const uint8_t id[SURGE_COMM_ID_BYTES]) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!id) return fail(h, SURGE_E_INVALID, "id is NULL");
  if (h->comm) return fail(h, SURGE_E_STATE, "the handle already has a communicator (surge_replay_comm_destroy first)");
  DeviceGuard g(h->device);
  std::string err;
  const int32_t rc = comm_create(h->device, rank, world, id, &h->comm, &err);
  if (rc == SURGE_OK) h->comm_world = world;
  return rc == SURGE_OK ? rc : fail(h, rc, err);
}

int32_t surge_replay_comm_destroy(surge_replay_handle* h) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  DeviceGuard g(h->device);
  if (h->comm) comm_destroy(h->comm);
  h->comm = nullptr;
  return SURGE_OK;
}

int32_t surge_replay_comm_info(surge_replay_handle* h, int32_t* rank, int32_t* world, int32_t* rccl_version, const char** library) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->comm) return fail(h, SURGE_E_STATE, "no communicator: surge_replay_comm_init first");
  return comm_info(h->comm, rank, world, rccl_version, library);
}

int32_t surge_replay_comm_counts(surge_replay_handle* h, int64_t n_local, int64_t* counts_out, int64_t* max_count_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->comm) return fail(h, SURGE_E_STATE, "no communicator: surge_replay_comm_init first");
  if (n_local < 0) return fail(h, SURGE_E_INVALID, "negative size");
  DeviceGuard g(h->device);
  std::string err;
  const int32_t rc = comm_counts(h->comm, n_local, counts_out, max_count_out, true, &err);
  return rc == SURGE_OK ? rc : fail(h, rc, err);
}

int32_t surge_replay_allgather_snapshot(surge_replay_handle* h, const void* d_states, int64_t n_local, void* d_out,
                                        int64_t rows_per_rank, int32_t slot, int32_t mode) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->comm) return fail(h, SURGE_E_STATE, "no communicator: surge_replay_comm_init first");
  if (mode != SURGE_GATHER_P2P && mode != SURGE_GATHER_ALLGATHER && mode != SURGE_GATHER_P2P_RAW) return fail(h, SURGE_E_INVALID, "unknown gather mode");
  if (!d_states) {
    if (!h->bound) return fail(h, SURGE_E_STATE, "allgather_snapshot of the resident state before load_csr/bind_device_csr");
    if (n_local > h->n_agg) return fail(h, SURGE_E_RANGE, "n_local exceeds the resident state");
    d_states = h->d_state;
  }
  if (((uintptr_t)d_states & 7) || ((uintptr_t)d_out & 7)) return fail(h, SURGE_E_INVALID, "buffers must be 8-byte aligned");
  if (slot < 0 || slot > 1) return fail(h, SURGE_E_INVALID, "slot must be 0 or 1");
  DeviceGuard g(h->device);
  std::string err;
  if (!d_out) {  // the handle keeps the gathered snapshot (hosts without device pointers)
    int64_t mx = 0;
    const int32_t rc0 = comm_counts(h->comm, n_local, nullptr, &mx, false, &err);
    if (rc0 != SURGE_OK) return fail(h, rc0, err);
    rows_per_rank = mx;
    HIPCHK(h, hipStreamSynchronize(h->stream));  // a reallocation must not pull the buffer from under an earlier exchange
    {
      std::string e2;
      (void)comm_wait(h->comm, h->stream, slot, true, &e2);
    }
    HIPCHK(h, h->gathered[slot].reserve((size_t)h->comm_world * (size_t)(mx > 0 ? mx : 1) * 64));
    h->gathered_rows[slot] = mx;
    d_out = h->gathered[slot].ptr;
  }
  const int32_t rc = comm_allgather(h->comm, h->stream, d_states, n_local, d_out, rows_per_rank, slot, mode, !h->v2 && mode != SURGE_GATHER_P2P_RAW, &err);
  return rc == SURGE_OK ? rc : fail(h, rc, err);
}

int32_t surge_replay_allgather(surge_replay_handle* const* hs, int32_t n, const int64_t* n_local, void* const* d_out,
                               int64_t rows_per_rank, int32_t slot) {
  if (!hs || n < 1) return fail(nullptr, SURGE_E_INVALID, "no handles");
  for (int32_t r = 0; r < n; ++r)
    if (!hs[r]) return fail(nullptr, SURGE_E_INVALID, "a handle is NULL");
  surge_replay_handle* h0 = hs[0];
  if (slot < 0 || slot > 1) return fail(h0, SURGE_E_INVALID, "slot must be 0 or 1");
  std::vector<int64_t> counts((size_t)n);
  std::vector<CommState*> cs((size_t)n);
  std::vector<hipStream_t> streams((size_t)n);
  std::vector<const void*> src((size_t)n);
  std::vector<void*> dst((size_t)n);
  int64_t mx = 0;
  for (int32_t r = 0; r < n; ++r) {
    surge_replay_handle* h = hs[r];
    for (int32_t q = 0; q < r; ++q)
      if (hs[q] == h) return fail(h0, SURGE_E_INVALID, "a handle appears twice in the group");
    if (!h->bound) return fail(h0, SURGE_E_STATE, "allgather before load_csr/bind_device_csr on every handle");
    if (h->v2 != h0->v2) return fail(h0, SURGE_E_INVALID, "v1 and v2 handles cannot share a group");
    if (h->comm && !comm_is_local(h->comm)) return fail(h0, SURGE_E_STATE, "a handle holds an RCCL rank (surge_replay_comm_destroy first)");
    counts[(size_t)r] = n_local ? n_local[r] : h->n_agg;
    if (counts[(size_t)r] < 0 || counts[(size_t)r] > h->n_agg) return fail(h0, SURGE_E_RANGE, "n_local outside the resident state");
    mx = counts[(size_t)r] > mx ? counts[(size_t)r] : mx;
    if (d_out && (!d_out[r] || ((uintptr_t)d_out[r] & 7))) return fail(h0, SURGE_E_INVALID, "d_out entries must be non-NULL and 8-byte aligned");
  }
  if (!d_out) rows_per_rank = mx;
  std::string err;
  for (int32_t r = 0; r < n; ++r) {
    surge_replay_handle* h = hs[r];
    DeviceGuard g(h->device);
    int32_t cr = -1, cw = -1;
    if (h->comm) (void)comm_info(h->comm, &cr, &cw, nullptr, nullptr);
    if (h->comm && (cr != r || cw != n)) {  // the group changed shape
      comm_destroy(h->comm);
      h->comm = nullptr;
    }
    if (!h->comm) {
      const int32_t rc = comm_create_local(h->device, r, n, &h->comm, &err);
      if (rc != SURGE_OK) return fail(h0, rc, err);
      h->comm_world = n;
    }
    if (!d_out) {
      HIPCHK(h0, hipStreamSynchronize(h->stream));  // a reallocation must not pull the buffer from under an earlier exchange
      std::string e2;
      (void)comm_wait(h->comm, h->stream, slot, true, &e2);
      HIPCHK(h0, h->gathered[slot].reserve((size_t)n * (size_t)(mx > 0 ? mx : 1) * 64));
      h->gathered_rows[slot] = mx;
      dst[(size_t)r] = h->gathered[slot].ptr;
    } else {
      dst[(size_t)r] = d_out[r];
    }
    cs[(size_t)r] = h->comm;
    streams[(size_t)r] = h->stream;
    src[(size_t)r] = h->d_state;
  }
  const int32_t rc = comm_allgather_local(cs.data(), streams.data(), src.data(), counts.data(), dst.data(), rows_per_rank, n, slot, !h0->v2, &err);
  return rc == SURGE_OK ? rc : fail(h0, rc, err);
}

int32_t surge_replay_gathered(surge_replay_handle* h, int32_t slot, void** d_out, int64_t* rows_per_rank) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (slot < 0 || slot > 1) return fail(h, SURGE_E_INVALID, "slot must be 0 or 1");
  if (!h->gathered[slot].ptr) return fail(h, SURGE_E_STATE, "no handle-owned gathered snapshot in this slot (allgather_snapshot with d_out = NULL first)");
  if (d_out) *d_out = h->gathered[slot].ptr;
  if (rows_per_rank) *rows_per_rank = h->gathered_rows[slot];
  return SURGE_OK;
}

int32_t surge_replay_gathered_read(surge_replay_handle* h, int32_t slot, int32_t rank, int64_t first_row, int64_t n_rows,
                                   void* states_out) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->comm) return fail(h, SURGE_E_STATE, "no communicator: surge_replay_comm_init first");
  if (slot < 0 || slot > 1) return fail(h, SURGE_E_INVALID, "slot must be 0 or 1");
  if (!h->gathered[slot].ptr) return fail(h, SURGE_E_STATE, "no handle-owned gathered snapshot in this slot");
  if (rank < 0 || rank >= h->comm_world || first_row < 0 || n_rows < 0 || first_row + n_rows > h->gathered_rows[slot])
    return fail(h, SURGE_E_RANGE, "rank / rows outside the gathered snapshot");
  if (n_rows == 0) return SURGE_OK;
  if (!states_out) return fail(h, SURGE_E_INVALID, "states_out is NULL");
  DeviceGuard g(h->device);
  std::string err;
  const int32_t rc = comm_wait(h->comm, h->stream, slot, true, &err);
  if (rc != SURGE_OK) return fail(h, rc, err);
  const char* src = (const char*)h->gathered[slot].ptr + ((size_t)rank * (size_t)h->gathered_rows[slot] + (size_t)first_row) * 64;
  HIPCHK(h, hipMemcpy(states_out, src, (size_t)n_rows * 64, hipMemcpyDeviceToHost));
  return SURGE_OK;
}

int32_t surge_replay_comm_wait(surge_replay_handle* h, int32_t slot, int32_t host_sync) {
  if (!h) return fail(nullptr, SURGE_E_INVALID, "handle is NULL");
  if (!h->comm) return fail(h, SURGE_E_STATE, "no communicator: surge_replay_comm_init first");
  DeviceGuard g(h->device);
  std::string err;
  const int32_t rc = comm_wait(h->comm, h->stream, slot, host_sync != 0, &err);
  return rc == SURGE_OK ? rc : fail(h, rc, err);
}

}  // extern "C"
