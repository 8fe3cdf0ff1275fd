"""The state mode of the device decoder: state-topic bytes -> records on the device (``DeviceDecoder(states=True)``) ->
resident states (``load_states_into``) -> ``GpuReplayStateStore.restore_from_state_topic``.

The expectation is never the code under test: ``state_result()`` is held to the generator's own record lists
(``tests/state_topic_gen.py``, pinned on the host decoder by ``tests/test_state_topic_gen.py``), rows to ``decode_state_host``
of the compacted table.  Shapes are the smallest at which each path of the value gather is taken: its 256 records per
workgroup (-1, +0, +1, x2 + 1), the 64 KiB of its span a workgroup copies itself (+-1 byte around the next 16-byte piece),
every destination residue mod 16 and source residue mod 4."""
import ctypes
import json

import numpy as np
import pytest

import kafka_wire as kw
import state_topic_gen as gen
from oracle import oracle
from surge_amd import schema as S
from surge_amd import synth
from surge_amd.encode import JP_I32, JsonTemplate, decode_state_host
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine
from surge_amd.snapshot import StateRecord, compact

pytestmark = pytest.mark.gpu

COUNTER = JsonTemplate.counter()
GATHER_RECS = 256       # kGatherRecs (ingest_device.h): delivered records per workgroup of the value gather
GATHER_OWN = 64 << 10   # kGatherOwn: bytes of aligned pieces a workgroup copies itself; the rest goes to the grid-wide launch
GUARD = 0xEE


@pytest.fixture(scope="module")
def topics():
    return {c: gen.make_topic(compression=c) for c in ("lz4", "none")}


def framers(n):
    return [EventsTopicIngest(frames=True, device_lz4=True) for _ in range(n)]


def push_units(d, ingests, per_partition_units):
    """One push of these units (a list per partition); returns what it must deliver: partition after partition."""
    parts, expect = [], []
    for g, units in zip(ingests, per_partition_units):
        data, recs = gen.concat(units)
        g.feed(data)
        sec, arena = g.drain_sections()
        if sec.shape[0]:
            parts.append((sec, arena))
        expect += recs
    d.push_async(parts)
    d.finish()
    return expect


def push_batches(d, data):
    """One push of one partition's bytes through a framer of its own."""
    with EventsTopicIngest(frames=True, device_lz4=True) as g:
        g.feed(data)
        sec, arena = g.drain_sections()
        d.push_async([(sec, arena)])
        d.finish()


def check_result(d, expect, keys_before=()):
    """state_result() and the key table against the (offset, key, value | None) list in delivery order."""
    agg, values, value_off, offsets, n_keys = d.state_result()
    want_keys = list(dict.fromkeys(list(keys_before) + [k.decode("utf-8") for _, k, _ in expect]))  # first-delivered order
    assert d.keys() == want_keys and n_keys == len(want_keys)
    idx = {k: i for i, k in enumerate(want_keys)}
    assert agg.cpu().tolist() == [idx[k.decode("utf-8")] for _, k, _ in expect]
    assert offsets.cpu().tolist() == [o for o, _, _ in expect]
    lens = [len(v or b"") for _, _, v in expect]
    assert value_off.cpu().tolist() == [0] + list(np.cumsum(lens, dtype=np.int64)) if lens else value_off.cpu().tolist() == [0]
    assert values.cpu().numpy().tobytes() == b"".join(v or b"" for _, _, v in expect)
    return want_keys


# ---- 1: the record stage, wire path ------------------------------------------------------------------------------------
def test_the_fuzzed_topic_in_one_push_and_in_three(topics):
    units = topics["lz4"]
    everything = [r for u in units for r in gen.concat(u)[1]]
    assert any(v is None for _, _, v in everything)
    for n_push in (1, 3):
        ingests = framers(len(units))
        try:
            with DeviceDecoder(states=True) as d:
                expect = []
                for j in range(n_push):
                    expect += push_units(d, ingests, [gen.split(u, n_push)[j] for u in units])
                assert sorted(expect) == sorted(everything)  # aborted records absent, nothing else missing
                keys = check_result(d, expect)
                assert "a" in keys and "a:b" in keys  # two ids: the state topic's key is the id itself
                c = d.counters()
                assert c["flush_records_skipped"] == 1 and c["records_delivered"] == len(expect) and c["records_seen"] == len(expect) + 1
                _, _, value_off, _, _ = d.state_result()
                lens = (value_off[1:] - value_off[:-1]).cpu().numpy()
                assert [int(x) == 0 for x in lens] == [v is None for _, _, v in expect]  # tombstones have zero length
                with pytest.raises(IngestError) as ei:  # an events decoder's accessor
                    d.result()
                assert ei.value.status == -2
        finally:
            for g in ingests:
                g.close()


# ---- 2: the same records through push_records ----------------------------------------------------------------------------
def test_push_records_gives_the_same_result_with_empty_value_as_tombstone(topics):
    expect = [r for u in topics["lz4"] for r in gen.concat(u)[1]]
    with DeviceDecoder(states=True) as d:
        cut = len(expect) // 3
        for part in (expect[:cut], [(0, b"", b"")] + expect[cut:]):  # (a flush record arrives as empty key + empty value here too)
            d.push_records([k for _, k, _ in part], [v or b"" for _, _, v in part], [o for o, _, _ in part])
        check_result(d, expect)
        assert d.counters()["flush_records_skipped"] == 1


# ---- 3: refusals -----------------------------------------------------------------------------------------------------------
def _past_its_record(delta):
    """a record whose value length claims 100 bytes where 3 remain"""
    body = b"\x00" + kw.varint(0) + kw.varint(delta) + kw.varint(2) + b"zz" + kw.varint(100) + b"abc"
    return kw.varint(len(body)) + body


@pytest.mark.parametrize("case", ["null key", "empty value", "value past its record"])
def test_a_refused_record_fails_the_push_and_leaves_the_decoder_as_it_was(case):
    val = lambda k, c: oracle.counter_state_json(k, c, c)  # noqa: E731
    good_a = [(0, b"k0", val("k0", 1)), (1, b"k1", None), (3, b"k2", val("k2", 2))]
    good_b = [(0, b"k9", val("k9", 5)), (2, b"k0", None)]
    bad = {"null key": kw.record(2, None, val("x", 1)), "empty value": kw.record(2, b"fresh", b""), "value past its record": _past_its_record(2)}[case]
    with DeviceDecoder(states=True) as d:
        data, exp_a, _ = gen.compacted_batch(100, good_a, "lz4")
        push_batches(d, data)
        check_result(d, exp_a)
        raws = [kw.record(0, b"new-1", val("new-1", 1)), kw.record(1, b"k1", val("k1", 3)), bad, kw.record(5, b"new-2", None)]
        with pytest.raises(IngestError) as ei:
            push_batches(d, gen.batch(500, raws, 5, "lz4"))
        assert ei.value.status == -7 and "offset 502" in str(ei.value)  # SURGE_E_CORRUPT, naming the record's offset
        check_result(d, exp_a)  # the result and the keys unchanged: new-1 / new-2 were rolled back
        data, exp_b, _ = gen.compacted_batch(700, good_b, "none")
        push_batches(d, data)
        check_result(d, exp_a + exp_b)
        assert d.stats()["pushes"] == 2


# ---- 4: the value gather at its own edges ---------------------------------------------------------------------------------
def pattern(n, salt):
    return bytes((salt * 7 + i) & 0xFF or 1 for i in range(n)) if n < 4096 else ((np.arange(n, dtype=np.int64) * 131 + salt) % 251 + 1).astype(np.uint8).tobytes()


def records_of(lens, key_lens=None, first_key=0):
    """One record per key; value i has lens[i] bytes (0: a tombstone); key_lens sets the value's residue in the record"""
    out = []
    for i, n in enumerate(lens):
        kl = key_lens[i] if key_lens else 7
        key = (f"{first_key + i:x}".rjust(kl, "g")[-kl:] if kl >= 4 else "xyz"[:kl]).encode()  # (short keys repeat: the gather does not care)
        out.append((i, key, pattern(n, i) if n else None))
    return out


def run_gather_case(pushes):
    """``pushes``: lists of (delta, key, value | None), each one uncompressed batch.  Run once to size the buffers, clear, fill
    the values buffer and 64 bytes behind with a guard pattern, run again: the values are exact and the guard band is intact."""
    import torch

    with DeviceDecoder(states=True) as d:
        def go():
            expect, base = [], 0
            for recs in pushes:
                data, exp, base = gen.compacted_batch(base, recs, "none")
                push_batches(d, data)
                expect += exp
            return expect

        expect = go()
        total = sum(len(v or b"") for _, _, v in expect)
        _, values, value_off, _, _ = d.state_result()
        assert int(value_off[-1].item()) == total
        if total == 0:
            return
        ptr = values.data_ptr()

        def raw(n):  # the buffer ends at least 64 bytes behind its last value (surge_ingest.h)
            iface = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}
            return torch.as_tensor(type("_Span", (), {"__cuda_array_interface__": iface})(), device="cuda")

        d.clear()
        raw(total + 64).fill_(GUARD)
        torch.cuda.synchronize()
        keys = d.keys()
        assert go() == expect
        check_result(d, expect, keys_before=keys)
        assert d.state_result()[1].data_ptr() == ptr  # the same buffer: nothing grew
        got = raw(total + 64).cpu().numpy()
        assert got[:total].tobytes() == b"".join(v or b"" for _, _, v in expect)
        assert (got[total:] == GUARD).all()


EDGE_LENS = [0, 1, 15, 16, 17, 31, 32, 33]


@pytest.mark.parametrize("residue", range(16))
def test_gather_value_lengths_at_every_destination_and_source_residue(residue):
    # a preceding value of 0 .. 15 bytes sets the destination residue; key lengths 1 .. 4 (rotated) the source residue mod 4
    lens = [residue] + EDGE_LENS
    run_gather_case([records_of(lens, key_lens=[1 + (i + residue) % 4 for i in range(len(lens))])])


@pytest.mark.parametrize("n", [GATHER_RECS - 1, GATHER_RECS, GATHER_RECS + 1, 2 * GATHER_RECS + 1])
def test_gather_record_counts_around_a_workgroup(n):
    rng = np.random.default_rng(n)
    run_gather_case([records_of([int(x) for x in rng.integers(0, 41, size=n)])])


def test_gather_runs_of_tombstones():
    run_gather_case([records_of([0] * (GATHER_RECS + 44))])  # nothing but tombstones: no byte moves
    run_gather_case([records_of([0] * GATHER_RECS + [5, 0, 17])])  # a run that is all tombstones in front of one that is not
    lens = [0] + [9] * (GATHER_RECS - 2) + [0] + [0] + [21] * 10 + [0]  # a tombstone first and last in a workgroup, and in the next
    run_gather_case([records_of(lens)])


def test_gather_one_value_of_a_mebibyte_between_short_ones():
    run_gather_case([records_of([13, 40, 1 << 20, 7, 0, 33])])


@pytest.mark.parametrize("span", [GATHER_OWN - 1, GATHER_OWN, GATHER_OWN + 1, GATHER_OWN + 15, GATHER_OWN + 16, GATHER_OWN + 17])
def test_gather_a_run_whose_span_is_around_what_a_workgroup_copies_itself(span):
    lens = [601] * 100
    lens[-1] = span - sum(lens[:-1])
    assert sum(lens) == span and min(lens) > 0
    run_gather_case([records_of(lens)])
    run_gather_case([records_of([5]), records_of(lens, first_key=1000)])  # ... and behind a first push: the span starts at residue 5


@pytest.mark.parametrize("residue", range(16))
def test_gather_a_second_push_appended_at_every_destination_residue(residue):
    run_gather_case([records_of([48 + residue]), records_of(EDGE_LENS + [70], first_key=500)])


# ---- 5: LZ4 and uncompressed batches ------------------------------------------------------------------------------------------
def test_lz4_and_uncompressed_batches_give_identical_results(topics):
    got = {}
    for c in ("lz4", "none"):
        ingests = framers(len(topics[c]))
        try:
            with DeviceDecoder(states=True) as d:
                expect = push_units(d, ingests, topics[c])
                check_result(d, expect)
                agg, values, value_off, offsets, _ = d.state_result()
                got[c] = (agg.cpu().tolist(), values.cpu().numpy().tobytes(), value_off.cpu().tolist(), offsets.cpu().tolist(), d.keys())
        finally:
            for g in ingests:
                g.close()
    assert got["lz4"] == got["none"]


# ---- 6: load_states_into --------------------------------------------------------------------------------------------------------
def fresh_engine():
    eng = ReplayEngine()
    eng.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    eng.fold()
    return eng


def rows_of(eng):
    return eng.device_state().cpu().numpy()


MOCK_STATE = JsonTemplate((b'{"string":', "KEY", b',"int":', (JP_I32, 0), b"}"))  # MockState(string, int).toJsString


def test_load_states_the_reference_sequence_through_wire_bytes():
    # AggregateStateStoreKafkaStreamsSpec.scala:64-85: four keys piped in, then state1 again with another value
    seq = [("state1", 1), ("state2", 2), ("state3", 3), ("invalidValidation", 1), ("state1", 3)]
    recs = [(i, k.encode(), json.dumps({"string": k, "int": v}, separators=(",", ":")).encode()) for i, (k, v) in enumerate(seq)]
    with fresh_engine() as eng, DeviceDecoder(states=True) as d:
        push_batches(d, gen.compacted_batch(0, recs, "lz4")[0])
        assert d.load_states_into(eng, MOCK_STATE) == (4, 0, 0, 0)
        rows = rows_of(eng).view(S.STATE_DTYPE).reshape(-1)
        assert d.keys() == ["state1", "state2", "state3", "invalidValidation"] and list(rows["count"]) == [3, 2, 3, 1]
        assert d.state_result()[0].numel() == 0  # cleared


def expected_rows(keys, records):
    table = compact(StateRecord("state", 0, k.decode("utf-8"), v) for _, k, v in records)
    rows = np.zeros((len(keys), 64), dtype=np.uint8)  # deleted ids: 64 zero bytes
    for i, k in enumerate(keys):
        if k in table:
            rc, st, _ = decode_state_host(COUNTER, table[k], k)
            assert rc == 0
            rows[i] = np.frombuffer(st.tobytes(), dtype=np.uint8)
    return rows, table


@pytest.mark.parametrize("n_calls", [1, 3])
def test_load_states_of_the_fuzzed_topic_in_one_call_and_in_three(topics, n_calls):
    units = topics["lz4"]
    ingests = framers(len(units))
    try:
        with fresh_engine() as eng, DeviceDecoder(states=True) as d:
            delivered, totals = [], np.zeros(4, dtype=np.int64)
            for j in range(n_calls):
                delivered += push_units(d, ingests, [gen.split(u, n_calls)[j] for u in units])
                totals += np.array(d.load_states_into(eng, COUNTER))
            keys = d.keys()
            want, table = expected_rows(keys, delivered)
            got = rows_of(eng)
            assert got.shape == want.shape and (got == want).all()
            deleted = [i for i, k in enumerate(keys) if k not in table]
            assert len(deleted) >= 20 and not got[deleted].any()
            assert totals[2] == 0 and totals[0] + totals[1] >= len(keys)
            if n_calls == 1:
                assert (int(totals[0]), int(totals[1])) == (len(table), len(deleted))
    finally:
        for g in ingests:
            g.close()


def test_load_states_a_damaged_winner_is_named_by_its_topic_offset_and_a_damaged_loser_goes_unnoticed():
    val = lambda k, c: oracle.counter_state_json(k, c, c)  # noqa: E731
    recs = [(1000, b"k0", val("k0", 1)), (1003, b"k1", val("k1", 2)), (1004, b"k2", val("k2", 3)), (1010, b"k3", val("k3", 4)[:-3]),  # a loser
            (1042, b"k2", val("k2", 9)[:-1]),  # the winner of k2, damaged
            (1050, b"k3", val("k3", 8)), (1051, b"k4", None)]
    with fresh_engine() as eng, DeviceDecoder(states=True) as d:
        d.push_records([k for _, k, _ in recs], [v or b"" for _, _, v in recs], [o for o, _, _ in recs])
        eng.grow(5)
        eng.device_state().fill_(0xAB)
        __import__("torch").cuda.synchronize()
        with pytest.raises(IngestError) as ei:
            d.load_states_into(eng, COUNTER)
        assert ei.value.status == -7 and "topic offset 1042" in str(ei.value)
        assert d.state_result()[0].numel() == 0 and d.keys() == ["k0", "k1", "k2", "k3", "k4"]  # cleared, keys kept
        got = rows_of(eng)
        for i, (k, c) in enumerate([("k0", 1), ("k1", 2), ("k2", None), ("k3", 8)]):
            if c is None:
                assert (got[i] == 0xAB).all()  # the refused winner's row is untouched
            else:
                assert got[i].tobytes() == decode_state_host(COUNTER, val(k, c), k)[1].tobytes()
        assert not got[4].any()
        d.push_records([b"k2"], [val("k2", 11)], [1060])  # the decoder goes on
        assert d.load_states_into(eng, COUNTER) == (1, 0, 0, 0)
        assert rows_of(eng)[2].tobytes() == decode_state_host(COUNTER, val("k2", 11), "k2")[1].tobytes()


def test_the_two_kinds_of_decoder_refuse_each_others_hand_over():
    with fresh_engine() as eng:
        with DeviceDecoder() as events:
            with pytest.raises(IngestError) as ei:
                events.load_states_into(eng, COUNTER)
            assert ei.value.status == -2
            with pytest.raises(IngestError) as ei:
                events.state_result()
            assert ei.value.status == -2
        with DeviceDecoder(states=True) as states:
            states.push_records([b"k"], [oracle.counter_state_json("k", 1, 1)], [0])
            for call in (states.fold_into, lambda e: states.fold_into(e, wait=False), states.stage_into):
                with pytest.raises(IngestError) as ei:
                    call(eng)
                assert ei.value.status == -2  # SURGE_E_STATE


# ---- 7: resume through the store -------------------------------------------------------------------------------------------------
def test_resume_from_state_topic_bytes_plus_the_events_tail_equals_the_full_refold_and_the_oracle():
    """Counter model, 1500 Zipf aggregates.  Store A folds the head and publishes (LZ4, 4 partitions, and once more onto one
    partition), folds part of the tail and publishes the delta onto the same partitions; a fresh store reads the
    concatenated bytes and folds the rest of the tail.  Every byte of every row equals the one-shot fold and the CPU oracle."""
    import torch

    from fixture_models import CountDecremented, CounterBusinessLogic, CountIncremented, NoOpEvent
    from surge_amd.log import KeyTable, pack_events
    from surge_amd.snapshot import BulkSnapshotPublisher
    from surge_amd.store import GpuReplayStateStore

    n = 1500
    rng = np.random.default_rng(3)
    lens = np.minimum(synth.zipf_lengths(np.arange(n, dtype=np.int64), 3), 24) * (rng.random(n) < 0.9)
    ids = [f"agg-{i}" if i % 11 else f'q"{i}\\t\x05ü' for i in range(n)]
    owner = rng.permutation(np.repeat(np.arange(n), lens))
    seq = np.zeros(n, dtype=np.int64)
    events = []
    for a in owner:
        seq[a] += 1
        k = int(rng.integers(0, 3))
        arg = int(rng.integers(-50, 50))
        events.append(NoOpEvent(ids[a], int(seq[a])) if k == 0 else (CountIncremented if k == 1 else CountDecremented)(ids[a], arg, int(seq[a])))
    first_part = np.ceil(lens * rng.random(n)).astype(np.int64)
    first_part[-30:] = 0  # the last 30 ids first appear in the tail
    seen = np.zeros(n, dtype=np.int64)
    head, tail = [], []
    for a, e in zip(owner, events):
        seen[a] += 1
        (head if seen[a] <= first_part[a] else tail).append(e)
    tail_a, tail_b = tail[: len(tail) // 2], tail[len(tail) // 2:]
    bl = CounterBusinessLogic()
    model = bl.command_model()

    def key_table():
        kt = KeyTable()
        for k in ids:
            kt.intern(k)
        return kt

    stores, pubs = [], []
    try:
        a_store = GpuReplayStateStore(bl)
        stores.append(a_store)
        a_store.restore_log(pack_events(model, head, key_table()))
        pub1 = BulkSnapshotPublisher(a_store.engine, ids, 1, compression="lz4", device_compression=True)
        pub4 = BulkSnapshotPublisher(a_store.engine, ids, 4, compression="lz4", device_compression=True)
        pubs += [pub1, pub4]
        take = lambda out: {p: bytes(b) for p, b in out.items()}  # noqa: E731  (views of the framer's buffer: valid until the next publish)
        one_a, four_a = take(pub1.publish(commit=False)), take(pub4.publish())
        a_store.apply_events(tail_a)
        one_b, four_b = take(pub1.publish(commit=False)), take(pub4.publish())
        assert len(four_a) == 4 and len(four_b) == 4 and pub4.timings["values"] > 100
        a_rows = a_store.engine.snapshot()

        full = GpuReplayStateStore(bl)
        stores.append(full)
        full.keys = key_table()
        full.restore(head + tail)
        want = full.engine.snapshot()
        log = pack_events(model, head + tail, key_table())
        assert want.tobytes() == oracle.fold_csr(log.seg_off, log.events, None, model.event_algebra()).tobytes()

        def same_rows(store, rows_want):
            """the store's rows under ITS key table against rows indexed like `ids`; ids it never met are None there"""
            got = store.engine.snapshot()
            assert len(store.keys) == got.shape[0] and set(store.keys.keys) <= set(ids) and len(set(store.keys.keys)) == len(store.keys)
            for j, k in enumerate(ids):
                i = store.keys.get(k)
                w = rows_want[j].tobytes()
                assert (got[i].tobytes() if i is not None else bytes(64)) == w, k

        fetches4 = [[four_a.get(p) for p in range(4)], [four_b.get(p) for p in range(4)]]
        staged = GpuReplayStateStore(bl)  # the load alone, to look between the steps
        stores.append(staged)
        counts = staged.restore_from_state_topic(fetches4, n_partitions=4)
        assert counts["refused"] == 0 and counts["records_delivered"] == counts["records_seen"] > 1000 and counts["rows_written"] >= len(staged.keys)
        assert counts["tombstones"] == 0 and counts["batches"] > 4
        d_kind = torch.zeros(staged.engine.n_agg, dtype=torch.uint8, device="cuda")
        nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
        staged.engine._check(staged.engine._lib.surge_replay_snapshot_delta(staged.engine._h, ctypes.c_void_p(d_kind.data_ptr()), ctypes.byref(nv), ctypes.byref(nt), 0))
        assert (nv.value, nt.value) == (0, 0) and not d_kind.any()  # nothing to publish: what was loaded is the baseline
        same_rows(staged, a_rows)
        for k in (ids[3], ids[11], ids[700]):
            assert staged.get_aggregate_bytes(k) == a_store.get_aggregate_bytes(k)
        staged.apply_events(tail_b)
        same_rows(staged, want)

        resumed = GpuReplayStateStore(bl)  # in one call, tail included
        stores.append(resumed)
        resumed.restore_from_state_topic(fetches4, n_partitions=4, events_tail=tail_b)
        same_rows(resumed, want)

        single = GpuReplayStateStore(bl)  # the same topic on one partition
        stores.append(single)
        single.restore_from_state_topic([one_a[0], one_b[0]], events_tail=tail_b)
        same_rows(single, want)
    finally:
        for p in pubs:
            p.close()
        for s in stores:
            s.close()
