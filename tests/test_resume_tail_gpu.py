"""Resume on the device: the floored push of ``DeviceDecoder`` (``surge_device_decoder_push_parts_floored_async``: records below a
section's floor are passed over where records are parsed), a state decoder that continues as the events decoder of the same
aggregates (``continue_as_events``), and ``GpuReplayStateStore.restore_from_state_topic(events_fetches=...)`` — snapshot bytes,
then tail bytes.

The device is held to the host drain of the same bytes started at the same offset (``EventsTopicIngest(start_offset=...)``,
itself pinned on the writer's record list by tests/test_start_offsets.py); the stores to the full refold and the CPU oracle.
Everything is exact.  Section sizes are the four classes tests/test_event_envelope_gpu.py names."""
import ctypes
import uuid

import numpy as np
import pytest

import event_envelope_cases as cases
import kafka_wire as kw
import start_offsets_gen as sgen
from surge_amd import schema as S
from surge_amd.ingest import (ARG_I32, FLOOR_DTYPE, SECTION_DTYPE, SECTION_FLOORED, DeviceDecoder, EventJsonTemplate, EventsTopicIngest, IngestError,
                              PartitionedFramedFetches)
from test_event_envelope_gpu import check_store, device_result, padded_topic, same, sdk_history, sdk_topic, want_of

pytestmark = pytest.mark.gpu

SDK = cases.SDK
E_INVALID, E_STATE, E_CORRUPT = -1, -2, -7


def host_from(wire, template, start):
    """The pin: the host drain of ``wire`` started at ``start``."""
    with EventsTopicIngest(start_offset=start) as g:
        g.feed(wire)
        agg, ev, off = g.drain_json(template) if template is not None else g.drain_fixed16()
        return agg, ev, off, g.key_table().keys


def device_from(wire, template, framer_start, floors=None, device_lz4=True, device_crc=False):
    """Host framing started at ``framer_start`` + one floored push; ``floors``: instead of the framer's own list, ``(section,
    first_offset)`` pairs.  -> (result, below-floor count, counters, sections)"""
    with EventsTopicIngest(frames=True, device_lz4=device_lz4, device_crc=device_crc, start_offset=framer_start) as g, DeviceDecoder(template) as d:
        g.feed(wire)
        sections, arena = g.drain_sections()
        own = g.take_floors()
        if floors is not None:
            own = np.array([(0, 0, s, o) for s, o in floors], dtype=FLOOR_DTYPE)
        d.push(sections, arena, own)
        return device_result(d), d.below_floor(), d.counters(), sections.copy()


def straddled(n, value_bytes, compression="none", base=1000):
    """A small batch in front, the padded batch of ``n`` records at ``base`` (with a flush record as its third), one behind."""
    front = kw.record_batch(base - 10, [(b"front-%d:1" % i, cases.wrap(b"front-%d" % i, cases.amount_payload(i))) for i in range(5)], compression=compression)
    recs = []
    for i in range(n):
        aid = b"agg-%d" % (i % 37)
        recs.append((aid + b":%d" % i, cases.wrap(aid, cases.amount_payload(i * 7919 - 2**30, max(value_bytes, 40) + i % 5))))
    recs[2] = (b"", b"")
    behind = kw.record_batch(base + n, [(b"agg-3:x", cases.wrap(b"agg-3", cases.amount_payload(-3))), (b"late:1", cases.wrap(b"late", cases.amount_payload(9)))],
                             compression=compression)
    return front + kw.record_batch(base, recs, compression=compression) + behind


CLASSES = [(50, 100, 1, 8320), (100, 100, 8321, 16640), (150, 250, 16641, 65536), (200, 400, 65537, 1 << 20)]
CLASS_IDS = ["lds 8 KiB, 64 lanes", "lds 16 KiB, 128 lanes", "lds 64 KiB, 192 lanes", "global memory, 256 lanes"]


@pytest.mark.parametrize("n,value_bytes,lo,hi", CLASSES, ids=CLASS_IDS)
def test_the_floored_push_in_each_path_of_the_record_stage(n, value_bytes, lo, hi):
    base = 1000
    wire = straddled(n, value_bytes)
    for delta in sorted({0, 1, 2, 3, 63, 64, 65, n - 1, n} & set(range(n + 1))):
        host = host_from(wire, SDK, base + delta)
        if 0 < delta < n:  # the framer flags the batch and names it
            dev, below, counters, secs = device_from(wire, SDK, base + delta)
            assert (secs["codec"] & SECTION_FLOORED).tolist() == [1024, 0]
        else:  # the floor at the batch's first offset, and behind its last record: given by hand (a framer never hands those out floored)
            dev, below, counters, secs = device_from(wire, SDK, base, floors=[(0, base + delta)])
        assert lo <= int(secs["byte_len"][0]) <= hi
        same(host, dev)
        assert below == delta, delta  # (the flush record, delta 2, is one of them when it lies below)
        assert counters["flush_records_skipped"] == (1 if delta <= 2 else 0) and counters["records_delivered"] == host[0].shape[0]
        assert counters["records_seen"] == n + 2


@pytest.mark.parametrize("value_bytes", [40, 300], ids=["staged in LDS", "read from global memory"])
def test_a_floor_in_the_second_chaining_round(value_bytes):
    n, base = 300, 1000
    wire = straddled(n, value_bytes)
    for delta in (255, 256, 257, n - 1):
        dev, below, _, secs = device_from(wire, SDK, base + delta)
        same(host_from(wire, SDK, base + delta), dev)
        assert below == delta and (int(secs["byte_len"][0]) > 65536) == (value_bytes == 300)


@pytest.mark.parametrize("compression", ["none", "lz4"])
@pytest.mark.parametrize("device_crc", [False, True], ids=["host crc", "device crc"])
def test_lz4_and_uncompressed_host_and_device_crc_bare_and_fixed16(compression, device_crc):
    base = 1000
    for template, wire in ((SDK, straddled(70, 60, compression)), (sgen_template(), counter_topic(compression)), (None, sgen.standard_topic(compression).bytes)):
        starts = (base + 33, base + 69) if template is SDK else ((12, 44, 73, 81) if template is None else (3, 7))
        for s in starts:
            dev, below, _, secs = device_from(wire, template, s, device_crc=device_crc)
            host = host_from(wire, template, s)
            same(host, dev)
            assert np.count_nonzero(secs["codec"] & SECTION_FLOORED) <= 1 and (below > 0) == bool(np.any(secs["codec"] & SECTION_FLOORED))


def sgen_template():
    return EventJsonTemplate("_type", [("countIncremented", 1, "sequenceNumber", "incrementBy", ARG_I32)])


def counter_topic(compression):
    t = sgen.Topic(compression)
    t.data([(b"c%d:%d" % (i % 3, i), b'{"_type":"countIncremented","sequenceNumber":%d,"incrementBy":%d}' % (i, i + 1)) for i in range(9)])
    t.data([(b"c9:1", b'{"_type":"countIncremented","sequenceNumber":1,"incrementBy":5}')])
    return t.bytes


def test_by_copy_and_in_place_a_floored_and_an_unfloored_partition_in_one_push():
    t0, t1 = sgen.standard_topic("lz4"), sgen.standard_topic("none")
    starts = [44, 0]
    want = [host_from(t.bytes, None, s) for t, s in zip((t0, t1), starts)]
    for in_place in (False, True):
        with PartitionedFramedFetches([[t0.bytes, t1.bytes]], 2, threads=2, overlap=False, device_crc=True, in_place=in_place, start_offsets=starts) as framed, \
                DeviceDecoder(None) as d:
            item = next(iter(framed))
            assert item.floors["part"].tolist() == [0] and np.count_nonzero(item[0]["codec"] & SECTION_FLOORED) == 1
            d.push_async(item)
            d.finish()
            agg, ev, off, keys = device_result(d)
            assert d.below_floor() == len([r for r in t0.batches[3]["records"] if r[0] < 44])
        n0 = want[0][0].shape[0]
        assert off.tolist() == want[0][2].tolist() + want[1][2].tolist() and ev.tobytes() == want[0][1].tobytes() + want[1][1].tobytes()
        assert [keys[i] for i in agg[:n0]] == [want[0][3][i] for i in want[0][0]] and [keys[i] for i in agg[n0:]] == [want[1][3][i] for i in want[1][0]]


def bad_then_good(bad_key, bad_value, template):
    good = [(b"g%d:1" % i, cases.wrap(b"g%d" % i, b'{"x":1.5}' if template is cases.F64 else cases.amount_payload(i))) for i in range(4)]
    return kw.record_batch(500, [good[0], (bad_key, bad_value), good[1], good[2], good[3]], compression="lz4")


def test_values_that_would_not_decode_are_not_looked_at_below_the_floor_and_are_at_it():
    refused = cases.refused_cases()
    malformed, mismatch = refused[0], next(c for c in refused if c.reason == "mismatch")
    amb = cases.ambiguous_cases()[0]
    for c, template in ((malformed, SDK), (mismatch, SDK), (amb, cases.F64)):
        wire = bad_then_good(c.key, c.value, template)
        dev, below, counters, _ = device_from(wire, template, 502)  # the bad record is offset 501
        same(host_from(wire, template, 502), dev)
        assert below == 2 and counters["doubles_parsed_on_host"] == 0 and counters["records_delivered"] == 3
        if c is amb:  # at the floor it is handed back to the host, as ever
            dev, below, counters, _ = device_from(wire, template, 501)
            same(host_from(wire, template, 501), dev)
            assert below == 1 and counters["doubles_parsed_on_host"] == 1
        else:  # ... or fails the push, as ever — and the host drain with it
            with pytest.raises(IngestError) as ei:
                device_from(wire, template, 501)
            assert ei.value.status == E_CORRUPT and "(offset 501)" in str(ei.value) and cases.DEVICE_REASON[c.reason] in str(ei.value)
            with pytest.raises(IngestError):
                host_from(wire, template, 501)


def test_no_floors_through_the_new_entry_point_is_push_parts_async():
    from surge_amd import _native

    lib = _native.load()
    wire = straddled(70, 60, "lz4")
    got = []
    with EventsTopicIngest(frames=True, device_lz4=True) as g:
        g.feed(wire)
        sections, arena = g.drain_sections()
        secs = np.ascontiguousarray(sections, dtype=SECTION_DTYPE)
        one = lambda v, t: (t * 1)(v)  # noqa: E731
        for floored in (False, True):
            with DeviceDecoder(SDK) as d:
                args = (d._h, 1, one(arena, ctypes.c_void_p), one(secs.ctypes.data, ctypes.c_void_p), one(secs.shape[0], ctypes.c_int64))
                rc = lib.surge_device_decoder_push_parts_floored_async(*args, 0, None) if floored else lib.surge_device_decoder_push_parts_async(*args)
                assert rc == 0
                d.finish()
                got.append(device_result(d))
                assert d.below_floor() == 0
    same(got[0], got[1])
    with DeviceDecoder(states=True) as d, EventsTopicIngest(frames=True, start_offset=1003) as g:  # the state topic has no floor
        g.feed(straddled(10, 40))
        sections, arena = g.drain_sections()
        with pytest.raises(IngestError) as ei:
            d.push(sections, arena, g.take_floors())
        assert ei.value.status == E_STATE
    with DeviceDecoder(SDK) as d, EventsTopicIngest(frames=True) as g:  # a floor that names no section of the push
        g.feed(straddled(10, 40))
        sections, arena = g.drain_sections()
        with pytest.raises(IngestError) as ei:
            d.push(sections, arena, np.array([(0, 0, 3, 5)], dtype=FLOOR_DTYPE))
        assert ei.value.status == E_INVALID


# ---- a state decoder continues as an events decoder ---------------------------------------------------------------------------------
def state_ids(n=300):
    ids = [b"agg-%d" % i for i in range(n)]
    ids[5], ids[6], ids[7] = b"a:b", b"a", b"a:b:c"  # ids with a colon: in the table, never named by an event
    return ids


def loaded_state_decoder(ids, **kw_):
    d = DeviceDecoder(states=True, **kw_)
    values = [b"" if i % 9 == 4 else b'{"count":%d,"version":1}' % i for i in range(len(ids))]  # some tombstoned
    d.push_records(ids, values, list(range(len(ids))))
    assert d.n_keys == len(ids)
    d.clear()
    return d


def event16(seq, payload):
    return sgen.fixed16(1, seq, payload)


def test_a_state_decoder_continues_as_the_events_decoder_of_the_same_aggregates():
    ids = state_ids()
    index = {k: i for i, k in enumerate(ids)}
    tail_keys = [b"agg-17:1", b"agg-4:2", b"new-1:1", b"a:b:7", b"agg-13:9", b"new-2:1", b"new-1:2", b"a:1", b"agg-299", b"a:b:c:1", b"agg-4:3"]
    with loaded_state_decoder(ids) as d:
        d.continue_as_events(None)
        assert not d.states and d.n_keys == len(ids)
        d.push_records(tail_keys, [event16(i, i * 11) for i in range(len(tail_keys))], [1000 + i for i in range(len(tail_keys))])
        agg, ev, off, keys = device_result(d)
        want, fresh = [], {}
        for k in tail_keys:
            aid = k.split(b":", 1)[0]  # "a:b:7" is the id "a": the state id "a:b" can never be named by an event
            if aid not in index and aid not in fresh:
                fresh[aid] = len(ids) + len(fresh)  # new ids are numbered from the old key count on
            want.append(index.get(aid, fresh.get(aid)))
        assert agg.tolist() == want and want[3] == want[7] == want[9] == index[b"a"] and want[1] == 4  # (4 was tombstoned: re-created in its row)
        assert keys == [k.decode() for k in ids] + ["new-1", "new-2"] and off.tolist() == [1000 + i for i in range(len(tail_keys))]
        assert ev.tobytes() == b"".join(event16(i, i * 11) for i in range(len(tail_keys)))
        # state-only calls are refused from here on: each with arguments a state decoder would take
        from surge_amd.encode import JsonTemplate
        from surge_amd.replay import ReplayEngine

        with ReplayEngine() as eng:
            eng.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
            eng.fold()
            tmpl, counts, n = JsonTemplate.counter().to_c(), (ctypes.c_int64 * 4)(), ctypes.c_int64()
            lib = d._lib
            assert lib.surge_device_decoder_state_result(d._h, ctypes.byref(n), None, None, None, None, None) == E_STATE
            assert lib.surge_device_decoder_keep_strings(d._h, 1) == E_STATE
            assert lib.surge_device_decoder_load_states(d._h, eng._h, ctypes.byref(tmpl), ctypes.byref(counts)) == E_STATE
            assert lib.surge_device_decoder_load_protobuf_states(d._h, eng._h, ctypes.byref(tmpl), ctypes.byref(counts)) == E_STATE
        with pytest.raises(IngestError) as ei:
            d.continue_as_events(None)  # one-way: an events decoder is one already
        assert ei.value.status == E_STATE


def test_the_wire_path_and_a_template_after_the_switch():
    ids = [b"agg-%d" % i for i in range(40)]
    wire = straddled(50, 100)  # ids agg-0 .. agg-36, front-*, late
    with loaded_state_decoder(ids) as d, EventsTopicIngest(frames=True, start_offset=1010) as g:
        d.continue_as_events(SDK)
        g.feed(wire)
        sections, arena = g.drain_sections()
        d.push(sections, arena, g.take_floors())
        agg, ev, off, keys = device_result(d)
        host = host_from(wire, SDK, 1010)
        assert off.tolist() == host[2].tolist() and ev.tobytes() == host[1].tobytes()
        assert [keys[i] for i in agg] == [host[3][i] for i in host[0]] and keys[:40] == [k.decode() for k in ids] and keys[40:] == ["late"]
        assert d.below_floor() == 10


def test_each_refusal_of_the_switch():
    with DeviceDecoder(None) as d:  # an events decoder
        with pytest.raises(IngestError) as ei:
            d.continue_as_events(None)
        assert ei.value.status == E_STATE
    with DeviceDecoder(states=True) as d:  # records delivered and not loaded
        d.push_records([b"k"], [b'{"count":1,"version":1}'], [0])
        with pytest.raises(IngestError) as ei:
            d.continue_as_events(None)
        assert ei.value.status == E_STATE and d.states
        d.clear()
        d.continue_as_events(None)
    t = sgen.Topic().data([(b"k1", b'{"count":1,"version":1}')])
    with DeviceDecoder(states=True) as d, EventsTopicIngest(frames=True) as g:  # a push pending
        g.feed(t.bytes)
        d.push_async(g.drain_sections())
        with pytest.raises(IngestError) as ei:
            d.continue_as_events(None)
        assert ei.value.status == E_STATE
        d.finish()
        d.clear()
        d.continue_as_events(None)
    with loaded_state_decoder([b"x", b"y"]) as d:  # a template that does not validate: nothing changed
        bad = EventJsonTemplate("", [("", 1, "", "v", ARG_I32)])
        c = bad.to_c()
        c.envelope = 7
        rc = d._lib.surge_device_decoder_continue_as_events(d._h, ctypes.byref(c))
        assert rc == E_INVALID and d.states
        wide = EventJsonTemplate("_type", [("t%d" % i, i, "", "field%d" % i, ARG_I32) for i in range(9)])  # valid, but more names than the device tracks
        with pytest.raises(IngestError) as ei:
            d.continue_as_events(wide)
        assert ei.value.status == -5 and d.states
        d.push_records([b"z"], [b""], [5])  # still a state decoder: a tombstone is delivered
        assert d.n_keys == 3 and d.state_result()[0].tolist() == [2]


def test_a_reseed_after_the_switch_keeps_every_state_era_id_findable(monkeypatch):
    monkeypatch.setenv("SURGE_INGEST_DEBUG_WEAK_HASH", "1")  # the first hash function keeps 8 bits: collisions until the first re-seed
    for attempt in range(20):  # a dozen ids that do not collide among themselves under it, so that the re-seed comes AFTER the switch
        ids = [b"s%d-%d" % (attempt, i) for i in range(12)] + [b"p:q"]
        d = loaded_state_decoder(ids)
        if d.stats()["hash_reseeds"] == 0:
            break
        d.close()
    else:
        pytest.fail("no collision-free dozen in 20 attempts")
    with d:
        d.continue_as_events(None)
        fresh = [b"n%d:1" % i for i in range(300)]  # 300 new ids on 8 bits: collisions for certain
        d.push_records(fresh, [event16(1, i) for i in range(300)], list(range(300)))
        assert d.stats()["hash_reseeds"] >= 1 and d.stats()["hash_function"] >= 1
        d.clear()
        again = [k + b":2" for k in ids[:12]] + [b"p:3"]
        d.push_records(again, [event16(2, i) for i in range(13)], list(range(13)))
        agg = device_result(d)[0].tolist()
        assert agg[:12] == list(range(12)) and agg[12] == 13 + 300  # every state-era id is found in its row; "p:3" is the id "p", new ("p:q" is another)
        assert d.n_keys == 13 + 300 + 1 and d.keys()[:13] == [k.decode() for k in ids]


# ---- the store ------------------------------------------------------------------------------------------------------------------------
class Wire:
    """A history as its events topic: per partition the batches (transactional, lz4, one COMMIT each) with their offsets, so the
    bytes a consumer that seeks to ``o`` is sent and every event's offset are the writer's own."""

    def __init__(self, fmt, history, n_partitions, batch=40, pid=31):
        from surge_amd.kafka import partition_for_keys

        msgs = [fmt.write_event(e) for e in history]
        parts = partition_for_keys([m.key for m in msgs], n_partitions, up_to_colon=True) if n_partitions > 1 else np.zeros(len(msgs), dtype=np.int32)
        self.n = n_partitions
        self.batches = [[] for _ in range(n_partitions)]  # (bytes, base, last)
        self.offset_of = [None] * len(history)  # event index -> (partition, offset)
        for p in range(n_partitions):
            mine = [i for i, q in enumerate(parts) if q == p]
            off = 0
            for s in range(0, len(mine), batch):
                chunk = mine[s:s + batch]
                raw = kw.record_batch(off, [(msgs[i].key.encode(), msgs[i].value) for i in chunk], compression="lz4", transactional=True, producer_id=pid)
                self.batches[p].append((raw, off, off + len(chunk) - 1))
                for j, i in enumerate(chunk):
                    self.offset_of[i] = (p, off + j)
                off += len(chunk)
                self.batches[p].append((kw.control_batch(off, pid, kw.COMMIT), off, off))
                off += 1
        self.end = [b[-1][2] + 1 if b else 0 for b in self.batches]

    def bytes(self, p):
        return b"".join(raw for raw, _, _ in self.batches[p])

    def fetches(self, n_fetches, upto=None):
        """The topic cut wherever it falls into ``n_fetches`` responses (rows of one entry per partition)."""
        per = [self.bytes(p) for p in range(self.n)]
        rows = [[b[f * len(b) // n_fetches:(f + 1) * len(b) // n_fetches] or None for b in per] for f in range(n_fetches)]
        return rows if upto is None else rows[:upto]

    def sent_from(self, starts, n_fetches=2):
        """What a consumer that seeks to ``starts`` is sent: per partition the bytes from the batch that contains its start on."""
        per = [b"".join(raw for raw, _, last in self.batches[p] if last >= starts[p]) for p in range(self.n)]
        return [[b[f * len(b) // n_fetches:(f + 1) * len(b) // n_fetches] or None for b in per] for f in range(n_fetches)]

    def starts_behind(self, m):
        """Where each partition begins when the first ``m`` events of the history are in the snapshot."""
        starts = list(self.end)
        for i in range(len(self.offset_of) - 1, m - 1, -1):
            p, o = self.offset_of[i]
            starts[p] = o
        return starts


def positions_after(rows, n):
    """``positions()`` of a consumer that has framed the fetch responses ``rows``."""
    with PartitionedFramedFetches(rows, n, threads=2, overlap=False) as framed:
        for _ in framed:
            pass
        return framed.positions()


def counter_history(n_ids=300, n_events=2000, seed=5):
    from fixture_models import CountDecremented, CountIncremented, NoOpEvent

    rng = np.random.default_rng(seed)
    ids = [f"agg-{i}" if i % 11 else f'q"{i}\\t\x05ü' for i in range(n_ids)]
    seq = np.zeros(n_ids, dtype=np.int64)
    out = []
    for a in np.minimum(rng.zipf(1.3, size=n_events), n_ids) - 1:
        seq[a] += 1
        k, arg = int(rng.integers(0, 3)), int(rng.integers(-50, 50))
        out.append(NoOpEvent(ids[a], int(seq[a])) if k == 0 else (CountIncremented if k == 1 else CountDecremented)(ids[a], arg, int(seq[a])))
    return ids, out


@pytest.fixture(scope="module")
def counter_case():
    """The history, its wire, and the reference bytes per id: the full refold's, equal to the oracle's fold."""
    from fixture_models import CounterBusinessLogic
    from oracle import oracle
    from surge_amd.log import KeyTable, pack_events
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    model = bl.command_model()
    ids, history = counter_history()
    wire = Wire(bl.event_write_formatting(), history, 4)
    full = GpuReplayStateStore(bl)
    orc = GpuReplayStateStore(bl)
    try:
        full.restore_from_fetches(wire.fetches(4), n_partitions=4, framing_threads=2)
        kt = KeyTable()
        for k in ids:
            kt.intern(k)
        log = pack_events(model, history, kt)
        orc.keys = kt
        orc.restore_log(log)
        assert orc.engine.snapshot().tobytes() == oracle.fold_csr(log.seg_off, log.events, None, model.event_algebra()).tobytes()
        want = {k: orc.get_aggregate_bytes(k) for k in ids}
        assert {k: full.get_aggregate_bytes(k) for k in ids} == want and sum(w is not None for w in want.values()) > 100
    finally:
        full.close()
        orc.close()
    return bl, ids, history, wire, want


def published(store, n_partitions, **kw_):
    from surge_amd.snapshot import BulkSnapshotPublisher

    pub = BulkSnapshotPublisher(store.engine, store.keys.keys, n_partitions, compression="lz4", device_compression=True, **kw_)
    try:
        topic = {p: bytes(b) for p, b in pub.publish().items()}
    finally:
        pub.close()
    return [[topic.get(p) for p in range(n_partitions)]] if n_partitions > 1 else [topic[0]]


def test_counter_model_four_partitions_resumed_at_every_fetch_boundary_and_inside_a_batch(counter_case):
    from surge_amd.store import GpuReplayStateStore

    bl, ids, history, wire, want = counter_case
    n_fetches = 4
    cuts = [("fetch", k) for k in range(1, n_fetches + 1)] + [("event", 777), ("event", 1501)]
    for kind, k in cuts:
        a, resumed = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
        try:
            if kind == "fetch":  # publish at fetch k: the snapshot holds what the consumer had been handed, the positions say from where to go on
                a.restore_from_fetches(wire.fetches(n_fetches, upto=k), n_partitions=4, framing_threads=2)
                starts = positions_after(wire.fetches(n_fetches, upto=k), 4)
            else:  # a snapshot of the first k events: the first offsets lie inside batches
                a.restore(history[:k])
                starts = wire.starts_behind(k)
                assert any(all(base != s for _, base, _ in wire.batches[p]) for p, s in enumerate(starts))
            counts = resumed.restore_from_state_topic(published(a, 4), n_partitions=4, events_fetches=wire.sent_from(starts), events_from=starts, events_partitions=4,
                                                      framing_threads=2)
            assert counts["refused"] == 0 and counts["rows_written"] == len(a.keys)
            delivered = sum(1 for p, o in wire.offset_of if o >= starts[p])
            assert counts["tail_records_delivered"] == delivered, (kind, k)
            if kind == "event":
                assert delivered == len(history) - k and counts["tail_below_floor"] > 0
            for key in ids:
                assert resumed.get_aggregate_bytes(key) == want[key], (kind, k, key)
            assert set(resumed.keys.keys) <= set(ids) and len(resumed.keys) == resumed.engine.n_agg
        finally:
            a.close()
            resumed.close()


def test_single_partition_and_events_from_as_an_int():
    from fixture_models import CounterBusinessLogic
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    ids, history = counter_history(60, 500, seed=8)
    wire = Wire(bl.event_write_formatting(), history, 1, batch=70)
    k = 333
    full, a, resumed = GpuReplayStateStore(bl), GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        full.restore_from_fetches([wire.bytes(0)])
        a.restore(history[:k])
        start = wire.starts_behind(k)[0]
        tail = [row[0] for row in wire.sent_from([start], 3)]
        counts = resumed.restore_from_state_topic(published(a, 1), events_fetches=tail, events_from=start)
        assert counts["tail_records_delivered"] == len(history) - k and counts["tail_below_floor"] == start - [b for _, b, last in wire.batches[0] if last >= start][0]
        for key in ids:
            assert resumed.get_aggregate_bytes(key) == full.get_aggregate_bytes(key), key
    finally:
        for s in (full, a, resumed):
            s.close()


def test_the_sdk_sample_cycle_with_the_tail_as_bytes():
    from fixture_models import SdkSampleBusinessLogic
    from surge_amd.encode import JP_I32, JsonTemplate
    from surge_amd.store import GpuReplayStateStore

    state_tmpl = JsonTemplate((b'{"balance":', (JP_I32, 0), b"}"))
    ids1, h1 = sdk_history(120, 1200, 21)
    ids2, h2 = sdk_history(150, 900, 22, first_id=60)  # half of them new
    ids = sorted(set(ids1) | set(ids2))
    bl = SdkSampleBusinessLogic()
    wire = Wire(bl.event_write_formatting(), h1 + h2, 2, batch=70)
    e1, r2 = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        e1.restore(h1)
        starts = wire.starts_behind(len(h1))
        counts = r2.restore_from_state_topic(published(e1, 2, template=state_tmpl, envelope="protobuf_state"), n_partitions=2, template=state_tmpl,
                                             envelope="protobuf_state", events_fetches=wire.sent_from(starts, 3), events_from=starts, events_partitions=2, framing_threads=2)
        assert counts["tail_records_delivered"] == len(h2) and counts["tail_below_floor"] > 0 and counts["tail_doubles_parsed_on_host"] == 0
        check_store(r2, want_of(ids, h1 + h2))
    finally:
        e1.close()
        r2.close()


def test_bank_accounts_keep_their_strings_behind_a_tail_of_bytes():
    import state_strings_gen as strgen
    from fixture_models import BankAccount, BankAccountBusinessLogic, BankAccountCreated, BankAccountFormat, BankAccountUpdated
    from surge_amd.encode import JsonTemplate, encode_states, key_table_utf8
    from surge_amd.store import GpuReplayStateStore
    from test_state_strings_gpu import BANK, column_of, to_dev

    units, table = strgen.make_topic(compression="lz4")
    fetches = [[strgen.concat(strgen.split(part, 3)[j])[0] or None for part in units] for j in range(3)]
    fmt = BankAccountFormat()
    text_of = lambda k, t: fmt.write_state(BankAccount(uuid.UUID(k), t[0], t[1], t[2])).value  # noqa: E731
    live = next(k for k in table if table[k] and table[k][0] and table[k][1])
    other = next(k for k in table if table[k] and k != live)
    fresh_id = uuid.UUID(int=12345)
    below = [BankAccountUpdated(uuid.UUID(other), -1.0), BankAccountUpdated(uuid.UUID(live), -2.0)]  # offsets 0, 1: in the snapshot already
    tail = [BankAccountCreated(fresh_id, "Neu", "999", 5.0), BankAccountUpdated(uuid.UUID(live), 77.25)]
    evf = BankAccountBusinessLogic().event_write_formatting()
    msgs = [evf.write_event(e) for e in below + tail]
    wire = kw.record_batch(0, [(m.key.encode(), m.value) for m in msgs], compression="lz4")
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        counts = store.restore_from_state_topic(fetches, n_partitions=len(units), template=BANK, events_fetches=[wire], events_from=2)
        n = len(table)
        assert counts["tail_records_delivered"] == 2 and counts["tail_below_floor"] == 2 and store.engine.n_agg == n + 1
        assert store.get_aggregate_bytes(live) == text_of(live, (table[live][0], table[live][1], 77.25))
        assert store.get_aggregate_bytes(other) == text_of(other, table[other])  # the update below the floor was not folded again
        cols = store.state_string_columns()
        owners, codes = column_of(cols[0]), column_of(cols[1])
        assert len(owners) == n + 1 and owners[-1] == b"" and codes[-1] == b""  # as restore_from_fetches leaves a new id's strings
        keys = store.keys.keys
        assert keys[n] == str(fresh_id)
        data, off = key_table_utf8(keys)
        out, out_off = encode_states(store.engine, BANK, to_dev(data), to_dev(off), strings=cols)
        blob, o = out.cpu().numpy().tobytes(), out_off.cpu().tolist()
        for i, k in enumerate(keys[:n]):
            t = (table[k][0], table[k][1], 77.25) if k == live else table[k]
            assert blob[o[i]:o[i + 1]] == (text_of(k, t) if t else b""), k
    finally:
        store.close()


def test_events_tail_and_events_fetches_together_are_refused():
    from fixture_models import CounterBusinessLogic, NoOpEvent
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(CounterBusinessLogic())
    try:
        with pytest.raises(ValueError):
            store.restore_from_state_topic([], events_tail=[NoOpEvent("a", 1)], events_fetches=[b""])
        with pytest.raises(ValueError):
            store.restore_from_state_topic([], events_from=5)
    finally:
        store.close()


def test_a_tail_that_is_empty_behind_the_floors_leaves_exactly_the_snapshot(counter_case):
    from surge_amd.store import GpuReplayStateStore

    bl, ids, history, wire, want = counter_case
    a, plain, resumed = GpuReplayStateStore(bl), GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        a.restore(history[:900])
        topic = published(a, 4)
        plain.restore_from_state_topic(topic, n_partitions=4)
        last_batches = [[b"".join(raw for raw, _, _ in wire.batches[p][-2:]) for p in range(4)]]  # each partition's last batch and its marker: all below
        counts = resumed.restore_from_state_topic(topic, n_partitions=4, events_fetches=last_batches, events_from=wire.end, events_partitions=4, framing_threads=2)
        assert counts["tail_records_delivered"] == 0 and counts["tail_batches_discarded"] == 4
        assert resumed.keys.keys == plain.keys.keys
        for key in ids:
            assert resumed.get_aggregate_bytes(key) == plain.get_aggregate_bytes(key) == a.get_aggregate_bytes(key), key
    finally:
        for s in (a, plain, resumed):
            s.close()
