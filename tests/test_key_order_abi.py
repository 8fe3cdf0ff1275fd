"""The key-order exports (surge_device_decoder_range_device / _gather_keys_device / _key_order) without a GPU: declared, loaded
and bound as the header declares them; a NULL decoder, a negative length and a negative capacity are refused before a device
is touched; and the pass rule the device follows (ingest_order.hip), restated in plain Python, gives ``sorted()`` on the
corpus the GPU test uses — which shows that the corpus reaches what it is there for: ties across a chunk boundary, keys that
differ only in how many bytes they have left, and a group that is still whole when the last pass ``ceil(max_len / 4)`` allows
begins."""
import ctypes
import os
import re

import key_order_cases as cases
from surge_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("surge_device_decoder_range_device", "surge_device_decoder_gather_keys_device", "surge_device_decoder_key_order")


def declared():
    """name -> the parameter types the header declares (text)."""
    text = open(os.path.join(ROOT, "include", "surge_ingest.h")).read()
    out = {}
    for name in NAMES:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name + " is not declared in include/surge_ingest.h"
        out[name] = [" ".join(p.split()[:-1]) for p in m.group(1).replace("\n", " ").split(",")]
    return out


def test_the_three_exports_are_declared_listed_and_in_the_library():
    lib = _native.load()
    for name in NAMES:
        assert name in declared() and name in _native.INGEST_EXPORTS
        assert getattr(lib, name) is not None


def test_the_ctypes_signatures_are_the_headers():
    lib = _native.load()
    as_ctypes = {"surge_device_decoder*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p, "const int64_t*": ctypes.c_void_p,
                 "int64_t": ctypes.c_int64, "const int64_t**": ctypes.POINTER(ctypes.c_void_p)}
    out_words = {("surge_device_decoder_range_device", 7), ("surge_device_decoder_gather_keys_device", 6), ("surge_device_decoder_key_order", 2),
                 ("surge_device_decoder_key_order", 3)}  # int64_t* parameters that are one word the call writes
    for name, params in declared().items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32
        assert len(fn.argtypes) == len(params), name
        for at, (have, text) in enumerate(zip(fn.argtypes, params)):
            want = ctypes.POINTER(ctypes.c_int64) if (name, at) in out_words else ctypes.c_void_p if text == "int64_t*" else as_ctypes[text]
            assert have is want, (name, at, text)


def test_null_and_negative_arguments_are_invalid_before_a_device_is_touched():
    lib = _native.load()
    n = ctypes.c_int64(-5)
    lo, hi = ctypes.create_string_buffer(b"a"), ctypes.create_string_buffer(b"b")
    assert lib.surge_device_decoder_range_device(None, lo, 1, hi, 1, None, 0, ctypes.byref(n)) == E_INVALID
    assert lib.surge_device_decoder_gather_keys_device(None, None, 0, None, 0, None, ctypes.byref(n)) == E_INVALID
    assert lib.surge_device_decoder_key_order(None, None, ctypes.byref(n), ctypes.byref(n)) == E_INVALID
    assert n.value == -5 and b"decoder is NULL" in lib.surge_device_decoder_last_error(None)
    # a negative length or capacity is refused on the numbers alone, in front of the look at the decoder: the text says which
    # check answered
    off = (ctypes.c_int64 * 2)()
    for args in ((lo, -1, hi, 1, None, 0), (lo, 1, hi, -1, None, 0), (lo, 1, hi, 1, None, -1)):
        assert lib.surge_device_decoder_range_device(None, *args, ctypes.byref(n)) == E_INVALID, args
        assert b"negative" in lib.surge_device_decoder_last_error(None)
    for count, capacity in ((-1, 0), (0, -1)):
        assert lib.surge_device_decoder_gather_keys_device(None, None, count, None, capacity, off, ctypes.byref(n)) == E_INVALID
        assert b"negative" in lib.surge_device_decoder_last_error(None)
    assert n.value == -5


def test_the_pass_rule_restated_is_sorted_on_the_corpus():
    keys = cases.corpus()
    order, passes, groups = cases.order_by_passes(keys)
    assert order == cases.expected_order(keys) and groups == len(keys)
    assert [keys[i] for i in order] == sorted(keys)
    # the corpus reaches the last pass: ceil(max_len / 4) of them, and one fewer leaves a group of several keys
    longest = max(len(k) for k in keys)
    assert longest == 255 and passes == (longest + 3) // 4 == 64
    assert cases.order_by_passes(keys, max_passes=passes - 1)[2] < len(keys)
    for n, seed in ((0, 1), (1, 2), (2, 3), (65, 4), (3000, 5)):
        keys = cases.random_keys(n, seed)
        order, passes, _ = cases.order_by_passes(keys)
        assert order == cases.expected_order(keys) and passes <= 13 // 4 + 1


def test_the_corpus_holds_what_it_claims():
    keys = set(cases.corpus())
    assert {b"", b"a", b"a\0", b"a\0\0"} <= keys  # proper prefixes that differ only in zero bytes
    for n in cases.STEM_LENGTHS:  # a shared prefix of exactly n bytes, 0x7f / 0x80 / 0xff deciding behind it
        stem = bytes([0x50 + n]) + b"q" * (n - 1)
        assert {stem, stem + b"\x7f", stem + b"\x80", stem + b"\xff"} <= keys
    assert sum(len(k) == 255 and k[:253] == cases.LONG for k in keys) == 4 and b"M" * 200 in keys
    assert {b"id", b"id!x", b"id:", b"id:~", b"id:\x7f", b"idx"} <= keys
    # a rule without the bytes-left component does not order this corpus: zero padding makes `a` and `a\0` one key
    padded = sorted(keys, key=lambda k: k.ljust(256, b"\0"))
    assert padded != sorted(keys) or len({k.ljust(256, b"\0") for k in keys}) < len(keys)
