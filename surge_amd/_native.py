"""Builds and loads ``libsurge_replay.so`` (the C-ABI of ``include/surge_replay.h``) through ctypes.

There is no Python/CPU fallback for the fold: if the library cannot be built or loaded this
module raises, and every ``ReplayEngine`` call would fail loudly.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from typing import List, Optional

from .schema import CKernelInfo, CLayoutInfo, CSchema, CStats

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.abspath(os.path.join(_HERE, "..", "include"))
LIB_PATH = os.path.join(_HERE, "libsurge_replay.so")


def _read_sources() -> tuple:
    """The translation units, from ``csrc/SOURCES`` — the one list the Makefile reads too (tests/test_abi.py)."""
    with open(os.path.join(CSRC, "SOURCES")) as f:
        return tuple(ln.strip() for ln in f if ln.strip() and not ln.startswith("#"))


SOURCES = _read_sources()
# every header a translation unit may include or rtc.cpp embeds (.incbin): a change to any of them rebuilds every object
HEADERS = tuple(sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))) + tuple(
    os.path.join(INCLUDE, f) for f in ("surge_replay.h", "surge_ingest.h", "surge_snapshot.h"))

_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32

# One table per header: every symbol it declares, name -> (argtypes, restype).  The export tuples below are these tables' keys
# (tests/test_abi.py holds them against the headers) and ``load()`` sets the signatures from them: a new export is named once.
#: ``include/surge_replay.h``
REPLAY_H = {
    "surge_replay_default_schema": ([ctypes.POINTER(CSchema)], _i32),
    "surge_replay_create": ([ctypes.POINTER(CSchema), _i32, ctypes.POINTER(_vp)], _i32),
    "surge_replay_create_v2": ([_vp, _i32, ctypes.POINTER(_vp)], _i32),
    "surge_replay_kernel_info": ([_vp, ctypes.POINTER(CKernelInfo)], _i32),
    "surge_replay_compile_schema_v2": ([_vp, ctypes.c_char_p, _vp, _i64, ctypes.POINTER(_i64)], _i32),
    "surge_replay_compile_schema": ([_vp, ctypes.c_char_p, _vp, _i64, ctypes.POINTER(_i64)], _i32),
    "surge_replay_destroy": ([_vp], _i32),
    "surge_replay_last_error": ([_vp], ctypes.c_char_p),
    "surge_replay_set_stream": ([_vp, _vp], _i32),
    "surge_replay_get_stream": ([_vp, ctypes.POINTER(_vp)], _i32),
    "surge_replay_synchronize": ([_vp], _i32),
    "surge_replay_load_csr": ([_vp, _vp, _i64, _vp, _i64, _vp], _i32),
    "surge_replay_bind_device_csr": ([_vp, _vp, _i64, _vp, _i64, _vp, _vp], _i32),
    "surge_replay_fold": ([_vp, _i32], _i32),
    "surge_replay_prepare": ([_vp, _i32], _i32),
    "surge_replay_layout_info": ([_vp, ctypes.POINTER(CLayoutInfo)], _i32),
    "surge_replay_index_order": ([_vp, _i32, _vp, _i64, ctypes.POINTER(_i64)], _i32),
    "surge_replay_stage_reserve": ([_vp, _i64], _i32),
    "surge_replay_stage_events_device": ([_vp, _vp, _vp, _i64], _i32),
    "surge_replay_staged": ([_vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_pack_staged": ([_vp, _i64], _i32),
    "surge_replay_bound_log": ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_replay_append_fold": ([_vp, _vp, _vp, _i64, _vp, _i64], _i32),
    "surge_replay_append_fold_device": ([_vp, _vp, _vp, _i64, _vp, _i64], _i32),
    "surge_replay_append_events": ([_vp, _vp, _vp, _i64], _i32),
    "surge_replay_append_events_device": ([_vp, _vp, _vp, _i64], _i32),
    "surge_replay_get": ([_vp, _i64, _vp, ctypes.POINTER(ctypes.c_uint8)], _i32),
    "surge_replay_gather": ([_vp, _vp, _i64, _vp], _i32),
    "surge_replay_snapshot": ([_vp, _vp, _vp], _i32),
    "surge_replay_device_state": ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_i64)], _i32),
    "surge_replay_snapshot_delta": ([_vp, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i32], _i32),
    "surge_replay_set_encode_filter": ([_vp, _vp], _i32),
    "surge_replay_snapshot_commit": ([_vp, _vp], _i32),
    "surge_replay_snapshot_invalidate": ([_vp, _vp], _i32),
    "surge_replay_set_encode_strings": ([_vp, _i32, _vp, _vp], _i32),
    "surge_format_f64_json": ([ctypes.c_uint64, _vp, _i32], _i32),
    "surge_format_f64_json_many": ([_vp, _i64, _vp, _i64, _vp], _i64),
    "surge_replay_encode_json": ([_vp, _vp, _vp, _vp, _vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_encode_protobuf_state": ([_vp, _vp, _vp, _vp, _vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_encode_json_rows": ([_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_encode_protobuf_state_rows": ([_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_decode_json_states": ([_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, ctypes.POINTER(_i64 * 4)], _i32),
    "surge_replay_set_decode_base": ([_vp, _vp], _i32),
    "surge_replay_set_decode_mode": ([_vp, _i32], _i32),
    "surge_replay_decode_protobuf_states": ([_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, ctypes.POINTER(_i64 * 4)], _i32),
    "surge_decode_json_state": ([_vp, _vp, _i64, _vp, _i64, _vp, _vp], _i32),
    "surge_decode_protobuf_state": ([_vp, _vp, _i64, _vp, _i64, _vp, _vp], _i32),
    "surge_decode_json_state_lenient": ([_vp, _vp, _i64, _vp, _i64, _vp, _vp], _i32),
    "surge_decode_protobuf_state_lenient": ([_vp, _vp, _i64, _vp, _i64, _vp, _vp], _i32),
    "surge_unescape_json_string": ([_vp, _i64, _vp, _i64], _i64),
    "surge_replay_merge_state_strings": ([_vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_pack_states": ([_vp, _vp, _i64, _vp, _vp], _i32),
    "surge_replay_unpack_states": ([_vp, _vp, _i64, _vp, _vp], _i32),
    "surge_replay_partition_hash": ([_vp, _vp, _i64, _i32, _vp], _i32),
    "surge_replay_partition_hash_device": ([_vp, _vp, _vp, _i64, _i32, _vp], _i32),
    "surge_replay_partition_hash_up_to_colon": ([_vp, _vp, _i64, _i32, _vp], _i32),
    "surge_replay_partition_hash_up_to_colon_device": ([_vp, _vp, _vp, _i64, _i32, _vp], _i32),
    "surge_replay_partition_hash_utf8": ([_vp, _vp, _i64, _i32, _i32, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_partition_hash_utf8_device": ([_vp, _vp, _vp, _i64, _i32, _i32, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_set_state_out":([_vp, _vp], _i32),
    "surge_replay_grow": ([_vp, _i64], _i32),
    "surge_replay_comm_unique_id": ([_vp], _i32),
    "surge_replay_comm_init": ([_vp, _i32, _i32, _vp], _i32),
    "surge_replay_comm_destroy": ([_vp], _i32),
    "surge_replay_comm_info": ([_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(ctypes.c_char_p)], _i32),
    "surge_replay_comm_counts": ([_vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_replay_allgather_snapshot": ([_vp, _vp, _i64, _vp, _i64, _i32, _i32], _i32),
    "surge_replay_allgather": ([_vp, _i32, _vp, _vp, _i64, _i32], _i32),
    "surge_replay_comm_wait": ([_vp, _i32, _i32], _i32),
    "surge_replay_gathered": ([_vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64)], _i32),
    "surge_replay_gathered_read": ([_vp, _i32, _i32, _i64, _i64, _vp], _i32),
    "surge_replay_stats": ([_vp, ctypes.POINTER(CStats)], _i32),
    "surge_replay_stats_reset": ([_vp], _i32),
    "surge_replay_fold_times": ([_vp, _vp, _i64, ctypes.POINTER(_i64)], _i32),
    "surge_replay_stream_probe": ([_vp, _vp, _i64, ctypes.POINTER(ctypes.c_double)], _i32),
}

#: ``include/surge_ingest.h``
INGEST_H = {
    "surge_ingest_create": ([_i32, ctypes.POINTER(_vp)], _i32),
    "surge_ingest_destroy": ([_vp], _i32),
    "surge_ingest_last_error": ([_vp], ctypes.c_char_p),
    "surge_ingest_feed": ([_vp, _vp, _i64, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_set_threads": ([_vp, _i32], _i32),
    "surge_ingest_ready": ([_vp], _i64),
    "surge_ingest_drain": ([_vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_arena": ([_vp], _vp),
    "surge_ingest_drain_fixed16": ([_vp, _i64, _vp, _vp, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_drain_json": ([_vp, _i64, _vp, _vp, _vp, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_drain_sections": ([_vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_group_create": ([_i32, _i32, ctypes.POINTER(_vp)], _i32),
    "surge_ingest_group_destroy": ([_vp], _i32),
    "surge_ingest_group_last_error": ([_vp], ctypes.c_char_p),
    "surge_ingest_group_feed": ([_vp, _vp, _vp, _i32, _vp, _i64, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_vp)], _i32),
    "surge_ingest_group_receive_buffer": ([_vp, _i64, ctypes.POINTER(_vp)], _i32),
    "surge_ingest_group_receive_copy": ([_vp, _vp, _vp, _i32, _vp], _i32),
    "surge_ingest_group_cpu_seconds": ([_vp, ctypes.POINTER(ctypes.c_double * 2)], _i32),
    "surge_ingest_group_slab_bytes": ([_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i32)], _i32),
    "surge_ingest_group_queued_sections": ([_vp], _i64),
    "surge_ingest_group_counters": ([_vp, ctypes.POINTER(_i64 * 8)], _i32),
    "surge_ingest_group_set_allocator": ([_vp, _vp, _vp], _i32),
    "surge_ingest_group_use_pinned_slabs": ([_vp], _i32),
    "surge_ingest_set_allocator": ([_vp, _vp, _vp], _i32),
    "surge_ingest_use_pinned_arena": ([_vp], _i32),
    "surge_device_decoder_create": ([_i32, _vp, _vp, ctypes.POINTER(_vp)], _i32),
    "surge_device_decoder_create_states": ([_i32, _vp, ctypes.POINTER(_vp)], _i32),
    "surge_device_decoder_destroy": ([_vp], _i32),
    "surge_device_decoder_last_error": ([_vp], ctypes.c_char_p),
    "surge_device_decoder_push": ([_vp, _vp, _vp, _i64], _i32),
    "surge_device_decoder_push_records": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64], _i32),
    "surge_device_decoder_push_records_async": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64], _i32),
    "surge_device_decoder_push_async": ([_vp, _vp, _vp, _i64], _i32),
    "surge_device_decoder_push_parts_async": ([_vp, _i32, _vp, _vp, _vp], _i32),
    "surge_device_decoder_push_parts_floored_async": ([_vp, _i32, _vp, _vp, _vp, _i64, _vp], _i32),
    "surge_device_decoder_push_floored": ([_vp, _vp, _vp, _i64, _i64, _vp], _i32),
    "surge_device_decoder_below_floor": ([_vp, ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_continue_as_events": ([_vp, _vp], _i32),
    "surge_device_decoder_push_finish": ([_vp], _i32),
    "surge_device_decoder_push_finish_async": ([_vp], _i32),
    "surge_device_decoder_pending": ([_vp], _i32),
    "surge_device_decoder_reserve": ([_vp, _i64, _i64], _i32),
    "surge_device_decoder_result": ([_vp, ctypes.POINTER(_i64), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_state_result": ([_vp, ctypes.POINTER(_i64), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                           ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_clear": ([_vp], _i32),
    "surge_device_decoder_load_states": ([_vp, _vp, _vp, ctypes.POINTER(_i64 * 4)], _i32),
    "surge_device_decoder_load_protobuf_states": ([_vp, _vp, _vp, ctypes.POINTER(_i64 * 4)], _i32),
    "surge_device_decoder_keep_strings": ([_vp, _i32], _i32),
    "surge_device_decoder_state_strings": ([_vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_keep_event_strings": ([_vp, _vp], _i32),
    "surge_device_decoder_event_strings_next_column": ([_vp, _i32, ctypes.POINTER(_i64 * 3), ctypes.POINTER(_vp), ctypes.POINTER(_vp)], _i32),
    "surge_device_decoder_event_strings_pending": ([_vp, ctypes.POINTER(_i64 * 4), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp)], _i32),
    "surge_event_strings_validate": ([_vp, _vp], _i32),
    "surge_event_json_string_spans": ([_vp, _vp, _vp, _i64, _vp, _vp], _i32),
    "surge_replay_append_decoded": ([_vp, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_replay_append_decoded_async": ([_vp, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_replay_stage_decoded": ([_vp, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_keys": ([_vp, _vp, _i64, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_key_table": ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp)], _i32),
    "surge_device_decoder_lookup": ([_vp, _vp, _vp, _i64, _vp], _i32),
    "surge_device_decoder_lookup_device": ([_vp, _vp, _vp, _i64, _vp], _i32),
    "surge_device_decoder_range_device": ([_vp, _vp, _i64, _vp, _i64, _vp, _i64, ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_gather_keys_device": ([_vp, _vp, _i64, _vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_key_order": ([_vp, ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_device_decoder_counters": ([_vp, ctypes.POINTER(_i64 * 4)], _i32),
    "surge_device_decoder_stats": ([_vp, ctypes.POINTER(_i64 * 8)], _i32),
    "surge_device_decoder_route_stats": ([_vp, ctypes.POINTER(_i64 * 2)], _i32),
    "surge_event_json_validate": ([_vp], _i32),
    "surge_event_json_decode": ([_vp, _vp, _i64, _vp], _i32),
    "surge_event_json_decode_keyed": ([_vp, _vp, _i64, _vp, _i64, _vp], _i32),
    "surge_event_json_last_error": ([], ctypes.c_char_p),
    "surge_parse_f64_json": ([_vp, _i64, ctypes.POINTER(ctypes.c_uint64)], _i32),
    "surge_ingest_key_count": ([_vp], _i64),
    "surge_ingest_key": ([_vp, _i64, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_i64)], _i32),
    "surge_ingest_counters": ([_vp, ctypes.POINTER(_i64 * 8)], _i32),
    "surge_ingest_set_start_offset": ([_vp, _i64], _i32),
    "surge_ingest_take_floors": ([_vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_position": ([_vp], _i64),
    "surge_ingest_below_start": ([_vp, ctypes.POINTER(_i64 * 2)], _i32),
    "surge_ingest_group_set_start_offsets": ([_vp, _vp], _i32),
    "surge_ingest_group_take_floors": ([_vp, _i64, _vp, ctypes.POINTER(_i64)], _i32),
    "surge_ingest_group_positions": ([_vp, _vp], _i32),
    "surge_ingest_group_below_start": ([_vp, ctypes.POINTER(_i64 * 2)], _i32),
    "surge_crc32c": ([_vp, _i64], ctypes.c_uint32),
    "surge_crc32c_portable": ([_vp, _i64], ctypes.c_uint32),
    "surge_lz4_frame_decompress": ([_vp, _i64, _vp, _i64], _i64),
    "surge_lz4_frame_bound": ([_i64], _i64),
    "surge_lz4_frame_compress": ([_vp, _i64, _vp, _i64], _i64),
    "surge_xxh32": ([_vp, _i64, ctypes.c_uint32], ctypes.c_uint32),
}

#: the snappy reader: declared in ``include/surge_ingest.h`` behind the LZ4 frame's exports, in a table of its own (INGEST_H is
#: what tests/test_abi.py finds in that header by the prefixes it has always looked for); needs no handle and no device
SNAPPY_H = {
    "surge_snappy_uncompressed_length": ([_vp, _i64, ctypes.POINTER(_i32)], _i64),
    "surge_snappy_uncompress": ([_vp, _i64, _vp, _i64, ctypes.POINTER(_i32)], _i64),
    "surge_snappy_frame_bound": ([_vp, _i64, ctypes.POINTER(_i32)], _i64),
    "surge_snappy_frame_decompress": ([_vp, _i64, _vp, _i64, ctypes.POINTER(_i32)], _i64),
    "surge_snappy_status_name": ([_i32], ctypes.c_char_p),
}

#: ``include/surge_snapshot.h``
SNAPSHOT_H = {
    "surge_snapshot_writer_create": ([_i32, _i32, _i64, ctypes.POINTER(_vp)], _i32),
    "surge_snapshot_writer_destroy": ([_vp], _i32),
    "surge_snapshot_writer_last_error": ([_vp], ctypes.c_char_p),
    "surge_snapshot_writer_append": ([_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64], _i32),
    "surge_snapshot_writer_append_indexed": ([_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64], _i32),
    "surge_snapshot_writer_flush": ([_vp], _i32),
    "surge_snapshot_writer_partition": ([_vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_snapshot_writer_reset": ([_vp], _i32),
    "surge_snapshot_writer_set_compression": ([_vp, _i32], _i32),
    "surge_device_framer_create": ([_i32, _vp, _i32, _i32, _i64, ctypes.POINTER(_vp)], _i32),
    "surge_device_framer_destroy": ([_vp], _i32),
    "surge_device_framer_last_error": ([_vp], ctypes.c_char_p),
    "surge_device_framer_set_compression": ([_vp, _i32], _i32),
    "surge_device_framer_frame": ([_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i32),
    "surge_device_framer_next_offsets": ([_vp, _vp], _i32),
    "surge_device_framer_uncompressed_bytes": ([_vp], _i64),
}

#: the host half of the state decoder (declared in ``include/surge_replay.h``; needs no handle and no device)
STATE_EXPORTS = ("surge_decode_json_state", "surge_decode_protobuf_state", "surge_decode_json_state_lenient", "surge_decode_protobuf_state_lenient",
                 "surge_unescape_json_string")
#: which event class carries which string (declared in ``include/surge_ingest.h`` beside the two exports that use it)
EVENT_STRINGS_EXPORTS = ("surge_event_strings_validate",)
#: what each header declares beside those
EXPORTS = tuple(n for n in REPLAY_H if n not in STATE_EXPORTS)
INGEST_EXPORTS = tuple(n for n in INGEST_H if n not in EVENT_STRINGS_EXPORTS)
SNAPPY_EXPORTS = tuple(SNAPPY_H)
SNAPSHOT_EXPORTS = tuple(SNAPSHOT_H)

_lib: Optional[ctypes.CDLL] = None


class NativeLibraryError(RuntimeError):
    pass


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise NativeLibraryError("hipcc not found; cannot build libsurge_replay.so")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps: List[str] = [os.path.join(CSRC, s) for s in SOURCES] + list(HEADERS)
    return any(os.path.getmtime(d) > t for d in deps)


FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall")
OBJ_DIR = os.path.join(_HERE, "build")


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (the .so travels with the repo snapshot).

    One object per translation unit under ``surge_amd/build/`` (compiled side by side, only the ones older than their
    source or any header), then one link: the flags and the source list (``csrc/SOURCES``) are the Makefile's.
    """
    if not force and not needs_build():
        return LIB_PATH
    from concurrent.futures import ThreadPoolExecutor

    hipcc = _hipcc()
    os.makedirs(OBJ_DIR, exist_ok=True)
    newest_header = max(os.path.getmtime(h) for h in HEADERS)
    jobs = []
    for src in SOURCES:
        obj = os.path.join(OBJ_DIR, src + ".o")
        path = os.path.join(CSRC, src)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(path), newest_header):
            jobs.append((path, obj))

    def compile_one(job):
        path, obj = job
        # -I csrc: rtc.cpp embeds the device headers with .incbin
        cmd = [hipcc, *FLAGS, "-I" + INCLUDE, "-I" + CSRC, "-c", path, "-o", obj + ".tmp"]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode == 0:
            os.replace(obj + ".tmp", obj)
        return path, proc

    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
        for path, proc in pool.map(compile_one, jobs):
            if proc.returncode != 0:
                raise NativeLibraryError(f"hipcc failed on {path}:\n" + proc.stdout + proc.stderr)
            if verbose and (proc.stdout or proc.stderr):
                print(proc.stdout + proc.stderr)
    tmp = LIB_PATH + ".tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + [os.path.join(OBJ_DIR, s + ".o") for s in SOURCES] + ["-o", tmp]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise NativeLibraryError("link failed:\n" + proc.stdout + proc.stderr)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def load() -> ctypes.CDLL:
    """Load the library (building it first when the sources are newer).

    ``torch`` is imported first on purpose: its bundled ``libamdhip64.so`` has the same soname as
    the system one, and loading it first makes the library share torch's HIP runtime so device
    pointers and streams interoperate.
    """
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (side effect: loads torch's HIP runtime)
    except Exception:  # pragma: no cover - torch is optional for pure C hosts
        pass
    lib_path = os.environ.get("SURGE_REPLAY_LIB", LIB_PATH)  # experiments: load an alternative build
    if lib_path == LIB_PATH and needs_build():
        build()
    try:
        L = ctypes.CDLL(lib_path)
    except OSError as e:
        raise NativeLibraryError(f"cannot load {lib_path}: {e}") from e
    for table in (REPLAY_H, INGEST_H, SNAPSHOT_H, SNAPPY_H):
        for name, signature in table.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
            fn.argtypes, fn.restype = signature
    _lib = L
    return L
