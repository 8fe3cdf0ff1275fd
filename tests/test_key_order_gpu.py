"""-m gpu: the device decoder's key table in key order — ``key_order`` / ``range_rows`` / ``gather_keys``
(surge_device_decoder_key_order / _range_device / _gather_keys_device, ingest_order.hip).

Every expectation is the test's own: a row is an id's position in the list the test delivered, the order is Python's ``sorted``
over that list of ``bytes`` (unsigned bytes, a proper prefix first) and a range is two ``bisect`` calls over it
(``key_order_cases``).  Keys go in through ``push_records`` on a state decoder, whose id is the whole key: any byte may stand
anywhere in it."""
import ctypes

import numpy as np
import pytest

import kafka_wire as kw
import key_order_cases as cases
import start_offsets_gen as sgen
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE, E_RANGE = -1, -2, -6
VALUE = b'{"v":1}'


def deliver(d, keys, first_offset=0):
    """``keys`` as the keys of a state topic's records (a state decoder's id is the whole key)."""
    if keys:
        d.push_records(list(keys), [VALUE] * len(keys), list(range(first_offset, first_offset + len(keys))))
        d.clear()


def order_of(d):
    return d.key_order().cpu().tolist()


def rows_of(d, lo, hi):
    return d.range_rows(lo, hi).cpu().tolist()


@pytest.fixture(scope="module")
def held():
    keys = cases.corpus()
    with DeviceDecoder(states=True) as d:
        deliver(d, keys)
        assert d.n_keys == len(keys)
        yield d, keys


def test_the_corpus_in_key_order_and_back_as_bytes(held):
    import torch

    d, keys = held
    order = d.key_order()
    assert order.dtype == torch.int64 and order.is_cuda and order.cpu().tolist() == cases.expected_order(keys)
    assert d.order_passes == 64  # the 255-byte ids differ in byte 253: pass 63 decides them (test_key_order_abi.py restates the rule)
    assert d.gather_keys(order) == sorted(keys)
    assert rows_of(d, None, None) == cases.expected_order(keys)
    some = torch.tensor([5, 0, 5, len(keys) - 1], dtype=torch.int64, device=order.device)
    assert d.gather_keys(some) == [keys[5], keys[0], keys[5], keys[-1]] and d.gather_keys(some[:0]) == []


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 3000])
def test_key_counts_around_a_wave_a_block_and_beyond(n):
    keys = cases.random_keys(n, seed=100 + n)
    with DeviceDecoder(states=True) as d:
        deliver(d, keys)
        want = cases.expected_order(keys)
        assert order_of(d) == want and d.order_passes <= 4
        assert rows_of(d, None, None) == want
        assert d.gather_keys(d.key_order()) == sorted(keys)
        for lo, hi in ((b"", b"\x80"), (b"\x7f", b"\x7f\xff\xff"), (b"a", None), (None, b"a\0"), (b"\xff\xff", b"\x00")):
            assert rows_of(d, lo, hi) == cases.expected_range(keys, lo, hi), (lo, hi)


def test_the_deciding_chunk_at_each_of_the_16_arena_alignments():
    """The keys delivered in front move the pair's bytes through every alignment; the pair shares five bytes, so what decides
    lies in the second chunk, at arena offset ``lead + 4``."""
    stem = b"stem!"
    for lead in range(16):
        keys = [b"\xfe" * lead, stem + b"\x80", stem + b"\x7f", stem + b"\x7f\0", stem, b"t"]
        if lead == 0:
            keys[0] = b"\xfd"  # (an id of its own; the empty id is in the corpus)
            keys.insert(0, b"")
        with DeviceDecoder(states=True) as d:
            deliver(d, keys)
            assert order_of(d) == cases.expected_order(keys), lead
            assert rows_of(d, stem + b"\x7f", stem + b"\x80") == cases.expected_range(keys, stem + b"\x7f", stem + b"\x80")
            assert d.gather_keys(d.range_rows(stem, b"t")) == sorted(k for k in keys if stem <= k <= b"t")


def bounds_for(keys):
    srt = sorted(keys)
    longest = max(srt, key=len)
    out = [(None, None), (b"", None), (None, b""), (b"", b""), (srt[0], srt[-1]), (srt[3], srt[3]), (srt[3] + b"\0", srt[3] + b"\0"),
           (srt[5], srt[9]),                              # equal to a key at either end: both are in
           (srt[5] + b"\0", srt[9][:-1] if srt[9] else b""),  # between keys
           (b"a", b"a\0\0"), (b"a\0", b"a\0"), (b"a\0\0\0\0\0", b"a\x01"), (b"S", b"Sz"), (b"Sq", b"Sqq\x7f"),  # proper prefixes of keys as bounds
           (longest + b"\xff" * 8, None), (None, longest + b"\xff" * 8), (b"\xff" * 300, b"\xff" * 301),  # longer than every key
           (srt[9], srt[5]), (b"z", b"a"), (b"a\0", b"a"),    # from > to
           (b"L" * 253 + b"\x7f", b"L" * 253 + b"\x80z"), (b"M" * 197, b"M" * 200), (b"M" * 196, b"M" * 199),
           (b"id", b"id:~"), (b"id:", b"id:~"), (b"id", b"id:"), (b"id!", b"id:\x7e"), (b"idx", b"idx"), (b"ic", b"if")]
    return out


def test_bounds_against_bisect(held):
    d, keys = held
    for lo, hi in bounds_for(keys):
        assert rows_of(d, lo, hi) == cases.expected_range(keys, lo, hi), (lo, hi)
    assert rows_of(d, b"", None) == rows_of(d, None, None)  # the empty id is the least key: the same rows, by another way
    assert rows_of(d, None, b"") == [keys.index(b"")] and rows_of(d, b"z", b"a") == []
    # str bounds are their UTF-8
    assert rows_of(d, "id", "id:~") == cases.expected_range(keys, b"id", b"id:~")
    sub = d.gather_keys(d.range_rows(b"id", b"id:~"))
    # id!x lies inside the range (the substates filter drops it on the host); id:\x7f, id:~z and idx lie behind id:~
    assert sub == [b"id", b"id!x", b"id:", b"id:1", b"id:~"]


def raw_range(d, lo, hi, out, capacity):
    buf = lambda k: (None, 0) if k is None else (ctypes.create_string_buffer(k, len(k) + 1), len(k))  # noqa: E731
    (pl, nl), (ph, nh) = buf(lo), buf(hi)
    n = ctypes.c_int64(-1)
    rc = d._lib.surge_device_decoder_range_device(d._h, pl, nl, ph, nh, ctypes.c_void_p(out.data_ptr()) if out is not None else None, capacity, ctypes.byref(n))
    return rc, n.value


def test_a_capacity_one_too_small_writes_nothing_and_the_exact_one_is_enough(held):
    import torch

    d, keys = held
    dev = torch.device("cuda", d.device)
    want = cases.expected_range(keys, b"Sq", b"Wz")
    assert len(want) > 10
    out = torch.full((len(want) + 2,), -77, dtype=torch.int64, device=dev)
    rc, n = raw_range(d, b"Sq", b"Wz", out[1:], len(want) - 1)
    assert (rc, n) == (E_RANGE, len(want)) and out.cpu().tolist() == [-77] * (len(want) + 2)
    rc, n = raw_range(d, b"Sq", b"Wz", out[1:], len(want))
    assert (rc, n) == (0, len(want)) and out.cpu().tolist() == [-77] + want + [-77]
    assert raw_range(d, b"z", b"a", None, 0) == (0, 0)  # from > to needs no room
    assert raw_range(d, None, None, None, 0) == (E_RANGE, len(keys))


def raw_gather(d, rows, out, capacity, off):
    total = ctypes.c_int64(-1)
    rc = d._lib.surge_device_decoder_gather_keys_device(d._h, ctypes.c_void_p(rows.data_ptr()), int(rows.numel()), ctypes.c_void_p(out.data_ptr()), capacity,
                                                        ctypes.c_void_p(off.data_ptr()), ctypes.byref(total))
    return rc, total.value


def test_gather_keys_capacity_guards_and_a_bad_row(held):
    import torch

    d, keys = held
    dev = torch.device("cuda", d.device)
    picked = [keys.index(b"M" * 200), keys.index(b""), keys.index(b"id:~"), keys.index(b"a\0\0")]
    rows = torch.tensor(picked, dtype=torch.int64, device=dev)
    text = b"".join(keys[i] for i in picked)
    offs = np.cumsum([0] + [len(keys[i]) for i in picked]).tolist()
    out = torch.full((len(text) + 8,), 0xA5, dtype=torch.uint8, device=dev)
    off = torch.full((len(picked) + 3,), -77, dtype=torch.int64, device=dev)
    untouched = lambda: out.cpu().tolist() == [0xA5] * (len(text) + 8) and off.cpu().tolist() == [-77] * (len(picked) + 3)  # noqa: E731
    rc, total = raw_gather(d, rows, out[4:], len(text) - 1, off[1:])
    assert (rc, total) == (E_RANGE, len(text)) and untouched()
    for bad in (-1, len(keys), 1 << 40):
        rows_bad = torch.tensor(picked[:2] + [bad] + picked[2:], dtype=torch.int64, device=dev)
        rc, _ = raw_gather(d, rows_bad, out[4:], len(text) + 4, off[1:])
        assert rc == E_INVALID and untouched(), bad
    rc, total = raw_gather(d, rows, out[4:], len(text), off[1:])
    assert (rc, total) == (0, len(text))
    assert out.cpu().numpy().tobytes() == b"\xa5" * 4 + text + b"\xa5" * 4 and off.cpu().tolist() == [-77] + offs + [-77]
    with pytest.raises(IngestError) as ei:
        d.gather_keys(torch.tensor([0, len(keys)], dtype=torch.int64, device=dev))
    assert ei.value.status == E_INVALID


def test_a_push_that_interns_ids_rebuilds_the_order_and_clear_keeps_it():
    first, second = cases.random_keys(300, seed=21), [b"zz-%d" % i for i in range(40)] + [b"\x00\x00", b"\xff" * 9]
    first = [k for k in first if k not in second]
    with DeviceDecoder(states=True) as d:
        deliver(d, first)
        before = order_of(d)
        assert before == cases.expected_order(first)
        at, passes = d.key_order().data_ptr(), d.order_passes
        d.clear()
        deliver(d, first[:50], 1000)  # known ids only: nothing interned, nothing rebuilt
        assert d.n_keys == len(first) and order_of(d) == before and d.key_order().data_ptr() == at and d.order_passes == passes
        deliver(d, second + first[:5], 2000)
        both = first + second
        after = order_of(d)
        assert len(after) == len(both) != len(before) and after == cases.expected_order(both)
        assert rows_of(d, b"zz-1", b"zz-2") == cases.expected_range(both, b"zz-1", b"zz-2")
        assert d.gather_keys(d.key_order()) == sorted(both)


def test_a_reseed_of_the_hash_function_leaves_the_order_right(monkeypatch):
    monkeypatch.setenv("SURGE_INGEST_DEBUG_WEAK_HASH", "1")  # 8 bits of hash until the first re-seed
    ids = [b"agg-%d" % i for i in range(600)]
    with DeviceDecoder(None) as d:
        d.push_records([k + b":1" for k in ids[:3]], [sgen.fixed16(1, 1, 1)] * 3, [0, 1, 2])
        d.clear()
        assert order_of(d) == cases.expected_order(ids[:3])  # an order from before the re-seed
        d.push_records([k + b":1" for k in ids[3:]], [sgen.fixed16(1, 1, 1)] * 597, list(range(3, 600)))
        d.clear()
        assert d.stats()["hash_reseeds"] >= 1
        assert order_of(d) == cases.expected_order(ids)
        assert rows_of(d, b"agg-10", b"agg-19") == cases.expected_range(ids, b"agg-10", b"agg-19")
        assert d.lookup(ids[::7]).tolist() == list(range(0, 600, 7))  # the table still finds what the order lists


def test_a_state_decoder_continued_as_an_events_decoder():
    keys = [b"x", b"x:1", b"x:2", b"x!", b"xy", b"x:~z", b"t", b"t"]
    values = [VALUE] * 7 + [b""]  # t is written, then tombstoned: it stays in the order
    ids = keys[:7]
    with DeviceDecoder(states=True) as d:
        d.push_records(keys, values, list(range(8)))
        assert d.n_keys == 7
        d.clear()
        want = cases.expected_order(ids)
        assert order_of(d) == want
        d.continue_as_events(None)
        assert order_of(d) == want and rows_of(d, b"x", b"x:~") == cases.expected_range(ids, b"x", b"x:~")
        d.push_records([b"new:1", b"x:7", b"a:1"], [sgen.fixed16(1, 1, 1)] * 3, [0, 1, 2])  # events: the id is the key up to ':'
        d.clear()
        ids = ids + [b"new", b"a"]
        assert d.n_keys == 9 and order_of(d) == cases.expected_order(ids)
        assert d.gather_keys(d.range_rows(b"t", b"x:1")) == [b"t", b"x", b"x!", b"x:1"]


def test_an_empty_decoder_answers_no_rows():
    with DeviceDecoder(None) as d:
        assert order_of(d) == [] and rows_of(d, None, None) == [] and rows_of(d, b"a", b"b") == [] and d.order_passes == 0
        d.reserve(100, 4096)  # a table, and still no key in it
        assert order_of(d) == [] and rows_of(d, b"", None) == []
    with DeviceDecoder(states=True) as d:
        assert rows_of(d, None, None) == []


def test_state_while_a_push_is_unfinished_and_fine_after_finish():
    import torch

    wire = kw.record_batch(0, [(b"p%d:1" % i, sgen.fixed16(1, i + 1, 1)) for i in range(40)])
    with EventsTopicIngest(frames=True) as g, DeviceDecoder(None) as d:
        d.push_records([b"before:1"], [sgen.fixed16(1, 1, 1)], [0])
        d.clear()
        assert order_of(d) == [0]
        g.feed(wire)
        sections, arena = g.drain_sections()
        d.push_async((sections, arena))
        for call in (d.key_order, lambda: d.range_rows(None, None), lambda: d.gather_keys(torch.zeros(1, dtype=torch.int64, device=torch.device("cuda", d.device)))):
            with pytest.raises(IngestError) as ei:
                call()
            assert ei.value.status == E_STATE
        d.finish()
        d.clear()
        ids = [b"before"] + [b"p%d" % i for i in range(40)]
        assert order_of(d) == cases.expected_order(ids) and d.gather_keys(d.range_rows(b"p1", b"p2")) == sorted(k for k in ids if b"p1" <= k <= b"p2")
