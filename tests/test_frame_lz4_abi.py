"""The LZ4 mode of the device framer, as far as it can be checked without a GPU: the new call is declared, listed and
exported, refuses a NULL framer, and the Python wrapper refuses a codec it does not know before it touches the library."""
import ctypes
import os
import re

import pytest

from surge_amd import _native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "surge_snapshot.h")
SURGE_E_INVALID = -1


def test_set_compression_is_declared_listed_and_exported():
    text = open(HEADER).read()
    assert re.search(r"int32_t\s+surge_device_framer_set_compression\s*\(\s*surge_device_framer\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", text)
    assert "surge_device_framer_set_compression" in _native.SNAPSHOT_EXPORTS
    lib = _native.load()
    fn = lib.surge_device_framer_set_compression
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 2


def test_set_compression_refuses_a_null_framer():
    lib = _native.load()
    for codec in (0, 3, 1):
        assert lib.surge_device_framer_set_compression(None, codec) == SURGE_E_INVALID
    assert b"NULL" in lib.surge_device_framer_last_error(None)
    assert lib.surge_device_framer_uncompressed_bytes(None) == -1


def test_device_framer_refuses_an_unknown_codec_name_before_the_library_is_touched(monkeypatch):
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    assert DeviceFramer.CODECS == RecordBatchWriter.CODECS
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("the library was loaded for a codec name that cannot be valid"))
    with pytest.raises(ValueError):
        DeviceFramer(1, compression="zstd")
