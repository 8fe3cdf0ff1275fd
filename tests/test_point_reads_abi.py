"""The point-read exports (surge_device_decoder_lookup[_device], surge_replay_encode_json_rows / _protobuf_state_rows) without a
GPU: a NULL decoder or handle is refused before a device is touched, and the SURGE_READ_* kinds the header defines are the
constants Python reads the kinds array with."""
import ctypes
import os
import re

from surge_amd import _native, encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def test_a_null_decoder_is_invalid_through_both_lookups():
    lib = _native.load()
    ids = (ctypes.c_uint8 * 32)()
    off = (ctypes.c_int64 * 2)(0, 3)
    out = (ctypes.c_int64 * 1)(7)
    assert lib.surge_device_decoder_lookup(None, ids, off, 1, out) == E_INVALID
    assert lib.surge_device_decoder_lookup_device(None, ids, off, 1, out) == E_INVALID
    assert lib.surge_device_decoder_lookup(None, None, None, 0, None) == E_INVALID  # (also with nothing asked)
    assert out[0] == 7
    assert b"decoder is NULL" in lib.surge_device_decoder_last_error(None)


def test_a_null_handle_is_invalid_through_both_rows_encoders():
    lib = _native.load()
    t = encode.JsonTemplate.counter().to_c()
    total = ctypes.c_int64(-5)
    for fn in (lib.surge_replay_encode_json_rows, lib.surge_replay_encode_protobuf_state_rows):
        assert fn(None, ctypes.byref(t), None, None, None, 0, None, 0, None, None, ctypes.byref(total)) == E_INVALID
        assert total.value == -5
        assert b"handle is NULL" in lib.surge_replay_last_error(None)


def test_the_read_kinds_of_the_header_are_pythons():
    text = open(os.path.join(ROOT, "include", "surge_replay.h")).read()
    header = {name: int(value) for name, value in re.findall(r"#define\s+SURGE_READ_(\w+)\s+(\d+)", text)}
    assert header == {"MISS": encode.READ_MISS, "VALUE": encode.READ_VALUE, "NONE": encode.READ_NONE, "POISONED": encode.READ_POISONED,
                      "NOT_A_NUMBER": encode.READ_NOT_A_NUMBER}
    assert header == {"MISS": 0, "VALUE": 1, "NONE": 2, "POISONED": 3, "NOT_A_NUMBER": 4}  # (a C host compiled against the header holds these numbers: they do not move)


def test_the_four_exports_are_declared_and_loaded():
    for name in ("surge_replay_encode_json_rows", "surge_replay_encode_protobuf_state_rows"):
        assert name in _native.EXPORTS
    for name in ("surge_device_decoder_lookup", "surge_device_decoder_lookup_device"):
        assert name in _native.INGEST_EXPORTS
