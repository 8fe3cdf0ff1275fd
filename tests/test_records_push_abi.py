"""The asynchronous framed-records push without a GPU: ``surge_device_decoder_push_records_async`` is declared, listed and
exported; a NULL decoder is refused by name; ``DeviceDecoder.push_records`` / ``push_records_async`` hand lists of ``bytes`` and
``(data, off)`` arrays to the library as the same C arguments (checked against a stub library that copies what the pointers
point to) and refuse a poll whose sides do not match before the library is touched; the store's two recoveries from consumer
records refuse a model without the hook or without a template by name, before anything of the store is used.

On the parent commit the symbol and the methods do not exist: every test here fails there."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import records_push_cases as C
from surge_amd import _native
from surge_amd.device_decoder import DeviceDecoder, records_arguments
from surge_amd.ingest import IngestError
from surge_amd.store import GpuReplayStateStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "surge_device_decoder_push_records_async"


def test_the_export_is_declared_listed_and_in_the_built_library():
    header = open(os.path.join(ROOT, "include", "surge_ingest.h")).read()
    assert re.search(r"int32_t\s+" + NAME + r"\(surge_device_decoder\* d, const uint8_t\* keys, const int64_t\* key_off,", header)
    assert "may be reused or freed as soon as" in header  # the contract a wire push does not have
    assert NAME in _native.INGEST_EXPORTS
    lib = _native.load()
    assert getattr(lib, NAME).argtypes == getattr(lib, "surge_device_decoder_push_records").argtypes
    exported = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + NAME + r"\b", exported)


def test_a_null_decoder_is_invalid_with_the_null_decoder_message():
    lib = _native.load()
    keys, ko = C.arrays([b"a:1"])
    vals, vo = C.arrays([C.event16(1)])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.surge_device_decoder_push_records_async(None, p(keys), p(ko), p(vals), p(vo), None, 1) == -1  # SURGE_E_INVALID
    assert lib.surge_device_decoder_last_error(None) == b"decoder is NULL"
    assert lib.surge_device_decoder_push_records_async(None, None, None, None, None, None, 0) == -1  # (before n is looked at)


class StubLib:
    """Stands where the loaded library stands in a ``DeviceDecoder``: records what the two push exports are called with — the
    bytes and offsets behind the pointers, copied while the call lasts."""

    def __init__(self):
        self.calls = []

    def _record(self, name, h, keys, key_off, values, value_off, offsets, n):
        as_array = lambda p, count, ty: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ty)), shape=(count,)).copy()  # noqa: E731
        ko, vo = as_array(key_off, n + 1, ctypes.c_int64), as_array(value_off, n + 1, ctypes.c_int64)
        self.calls.append((name, h, n, ko.tolist(), vo.tolist(), as_array(keys, int(ko[-1]), ctypes.c_uint8).tobytes()[int(ko[0]):],
                           as_array(values, int(vo[-1]), ctypes.c_uint8).tobytes()[int(vo[0]):],
                           None if offsets is None else as_array(offsets, n, ctypes.c_int64).tolist()))
        return 0

    def surge_device_decoder_push_records(self, *a):
        return self._record("sync", *a)

    def surge_device_decoder_push_records_async(self, *a):
        return self._record("async", *a)

    def surge_device_decoder_last_error(self, h):
        return b""


def stub_decoder():
    d = object.__new__(DeviceDecoder)  # (no create: there is no device here)
    d._lib, d._h, d._inflight, d.states = StubLib(), ctypes.c_void_p(0x1234), [], False
    return d


def test_lists_and_arrays_become_the_same_c_arguments():
    keys = [b"a:1", b"", b"bb:22", b":x", b"long-id-" * 9 + b":7"]
    values = [C.value(1), b"", C.value(2, 40), C.event16(3), C.value(5)]
    offsets = [3, 4, 9, 10, 700]
    d = stub_decoder()
    d.push_records(keys, values, offsets)
    d.push_records(C.arrays(keys), C.arrays(values), np.asarray(offsets))
    d.push_records_async(keys, values, offsets)
    d.push_records_async(C.arrays(keys), C.arrays(values), np.asarray(offsets, dtype=np.int32))  # (any integer array: converted)
    d.push_records_async(keys, C.arrays(values))  # the two forms mix, and offsets=None is a NULL pointer
    calls = d._lib.calls
    assert [c[0] for c in calls] == ["sync", "sync", "async", "async", "async"]
    want = (d._h, 5, [0, 3, 3, 8, 10, 84], list(np.cumsum([0] + [len(v) for v in values])), b"".join(keys), b"".join(values))
    for c in calls:
        assert c[1:7] == want
    assert [c[7] for c in calls] == [offsets] * 4 + [None]
    assert len(d._inflight) == 3  # one entry per asynchronous push, for finish() to pop
    # a window of larger arrays: offsets that do not start at 0 are the library's to rebase
    kd, ko = C.arrays([b"zz"] + keys)
    vd, vo = C.arrays([b"yyyy"] + values)
    d.push_records_async((kd, ko[1:]), (vd, vo[1:]), offsets)
    assert d._lib.calls[-1][2:7] == (5, [o + 2 for o in want[2]], [o + 4 for o in want[3]], want[4], want[5])
    # None stands for an empty value (a consumer's tombstone); no record at all is no push in flight
    d.push_records_async([b"k"], [None], [0])
    assert d._lib.calls[-1][2:7] == (1, [0, 1], [0, 0], b"k", b"")
    before = len(d._inflight)
    d.push_records_async([], [])
    assert d._lib.calls[-1][2] == 0 and len(d._inflight) == before


@pytest.mark.parametrize("method", ["push_records", "push_records_async"])
def test_a_poll_whose_sides_do_not_match_is_refused_before_the_library_is_touched(method):
    d = stub_decoder()
    push = getattr(d, method)
    with pytest.raises(ValueError, match="2 keys for 1 values"):
        push([b"a:1", b"b:1"], [C.value(1)])
    with pytest.raises(ValueError, match="2 keys for 3 values"):
        push(C.arrays([b"a:1", b"b:1"]), C.arrays([C.value(1)] * 3))
    with pytest.raises(ValueError, match="1 offsets for 2 records"):
        push([b"a:1", b"b:1"], [C.value(1)] * 2, [7])
    with pytest.raises(ValueError, match="3 offsets for 2 records"):
        push([b"a:1", b"b:1"], [C.value(1)] * 2, np.arange(3))
    data, off = C.arrays([b"a:1", b"b:1"])
    with pytest.raises(ValueError, match="do not lie inside"):
        push((data[:4], off), [C.value(1)] * 2)  # offsets that run past the bytes given
    with pytest.raises(ValueError, match="n \\+ 1 entries"):
        push((data, off[:0]), [])
    assert d._lib.calls == [] and d._inflight == []
    assert records_arguments([b"k:1"], [b"v"])[0][-1] == 1


class _NoTemplateModel:
    def event_json_template(self):
        return None


def bare_store(model):
    """A store as far as the refusals need one: no engine, no device (they come before either is used)."""
    store = object.__new__(GpuReplayStateStore)
    store.model = model
    return store


def test_the_store_refuses_a_model_without_the_hook_or_without_a_template_by_name():
    from fixture_models import CounterBusinessLogic
    from surge_amd.encode import JsonTemplate

    counter = CounterBusinessLogic().command_model()
    assert getattr(counter, "event_string_fields", None) is None and counter.event_json_template() is not None
    json_poll = ([b"a:1"], [b'{"v":1}'], [0])
    store = bare_store(counter)
    with pytest.raises(ValueError, match=type(counter).__name__ + " has no event_string_fields"):
        store.restore_from_consumer_records([json_poll], keep_strings=True)
    with pytest.raises(ValueError, match=type(counter).__name__ + " has no event_string_fields"):
        store.restore_from_state_consumer_records([], template=JsonTemplate.bank_account(), keep_strings=True, events_polls=[json_poll], keep_event_strings=True)
    with pytest.raises(ValueError, match="keep_event_strings"):
        store.restore_from_state_consumer_records([], template=JsonTemplate.bank_account(), keep_strings=True, keep_event_strings=True)  # no events_polls
    with pytest.raises(ValueError, match="no STR part"):
        store.restore_from_state_consumer_records([], keep_strings=True)  # the Counter template has no string
    with pytest.raises(ValueError, match="depth"):
        store.restore_from_consumer_records([json_poll], depth=6)
    store = bare_store(_NoTemplateModel())
    for poll in (json_poll, (C.arrays([b"", b"a:1"]), C.arrays([b"", b'{"v":1}']), None)):  # (the flush record in front is not what is looked at)
        with pytest.raises(ValueError, match="event_json_template.*_NoTemplateModel has none"):
            store.restore_from_consumer_records([poll])
        with pytest.raises(ValueError, match="event_json_template.*_NoTemplateModel has none"):
            store.restore_from_state_consumer_records([], events_polls=[poll])
    assert not hasattr(store, "engine")  # nothing of a store was needed to say so


def test_ingest_error_is_what_a_refusal_of_the_library_raises_through_the_wrapper():
    class Refusing(StubLib):
        def surge_device_decoder_push_records_async(self, *a):
            return -2

        def surge_device_decoder_last_error(self, h):
            return b"every push slot holds an unfinished push"

    d = stub_decoder()
    d._lib = Refusing()
    with pytest.raises(IngestError, match="every push slot") as ei:
        d.push_records_async([b"a:1"], [C.event16(1)])
    assert ei.value.status == -2 and d._inflight == []  # a push that failed is not in flight
