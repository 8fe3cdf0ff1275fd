"""The state-store seams (S1/S2) over the GPU replay, written after the reference's own store specs."""
import json
import uuid

import numpy as np
import pytest

from fixture_models import (
    BankAccountCommandModel, BankAccountCreated, BankAccountUpdated, BankAccountFormat, CounterBusinessLogic,
    CountDecremented, CountIncremented, ExceptionThrowingEvent, NoOpEvent, State,
)
from surge_amd.log import batch_groups, pack_events
from surge_amd.store import GpuReplayKeyValueStore, GpuReplayPersistencePlugin


# ---- CPU-only parts ----------------------------------------------------------------------------------
def test_ktable_semantics_last_write_wins_and_tombstones():
    # AggregateStateStoreKafkaStreamsSpec.scala:64-85 — pipe 4 keys, read back byte-equal; re-pipe key1 => overwritten
    store = GpuReplayPersistencePlugin().create_supplier("CounterAggregateAggregateStateStore")
    fmt = CounterBusinessLogic().aggregate_write_formatting()
    recs = {f"stateKey{i}": fmt.write_state(State(f"stateKey{i}", i, i)).value for i in range(1, 5)}
    for k, v in recs.items():
        store.put(k, v)
    for k, v in recs.items():
        assert store.get(k) == v
    updated = fmt.write_state(State("stateKey1", 3, 3)).value
    store.put("stateKey1", updated)
    assert store.get("stateKey1") == updated
    store.put("stateKey2", None)  # `null` value = tombstone (SurgeModel.scala:62)
    assert store.get("stateKey2") is None
    assert store.get("never-seen") is None


def test_key_value_store_read_api():
    # KafkaStreamsKeyValueStoreSpec.scala:37-91 — get / all / allValues / range("J","M") inclusive / approximateNumEntries
    store = GpuReplayKeyValueStore("s")
    for k in ["Alice", "Jane", "Kate", "Mike", "Zed"]:
        store.put(k, k.lower().encode())
    assert store.get("Jane") == b"jane" and store.get("Bob") is None
    assert [k for k, _ in store.range("J", "Mike")] == ["Jane", "Kate", "Mike"]
    assert [k for k, _ in store.range("J", "M")] == ["Jane", "Kate"]
    assert store.approximate_num_entries() == 5 and len(store.all_values()) == 5
    assert GpuReplayPersistencePlugin.enable_logging is False


def test_pack_events_orders_by_arrival_not_by_sequence_number():
    model = CounterBusinessLogic().command_model()
    # a NoOp consumes a sequence number without storing it, so "<id>:<seq>" keys can repeat
    events = [
        CountIncremented("a", 1, 1), CountIncremented("b", 5, 1), NoOpEvent("a", 2), CountDecremented("a", 3, 2),
        CountIncremented("b", 5, 2),
    ]
    log = pack_events(model, events, capacity=4)
    assert log.keys.keys == ["a", "b"] and log.n_aggregates == 4
    assert list(log.seg_off) == [0, 3, 5, 5, 5]
    assert list(log.events["seq"]) == [1, 2, 2, 1, 2]


def test_batch_groups_are_unique_and_order_preserving():
    import numpy as np

    from surge_amd import schema as S

    agg = np.array([5, 2, 5, 9, 2, 5])
    ev = S.make_events([1] * 6, [10, 20, 11, 30, 21, 12], [0] * 6)
    group_agg, group_off, sorted_ev = batch_groups(agg, ev)
    assert list(group_agg) == [2, 5, 9] and list(group_off) == [0, 2, 5, 6]
    assert list(sorted_ev["seq"]) == [20, 21, 10, 11, 12, 30]


# ---- GPU ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_get_aggregate_bytes_equals_write_state_of_the_host_fold():
    from surge_amd.store import AggregateInitializationException, GpuReplayStateStore

    bl = CounterBusinessLogic()
    model = bl.command_model()
    events = []
    for i in range(300):
        aid = f"agg-{i % 37}"
        events.append(CountIncremented(aid, i, i + 1) if i % 3 else CountDecremented(aid, 2, i + 1))
    events.insert(40, ExceptionThrowingEvent("agg-5", 41, RuntimeError("failed")))
    store = GpuReplayStateStore(bl)
    try:
        store.restore(events, capacity=64)
        for aid in {e.aggregateId for e in events}:
            if aid == "agg-5":
                with pytest.raises(AggregateInitializationException):
                    store.get_aggregate_bytes(aid)
                continue
            state = None
            for e in events:
                if e.aggregateId == aid:
                    state = model.handle_event(state, e)
            # drop-in: bytes == writeState(fold(...)).value (SURVEY §7 "serialized state format stays drop-in")
            assert store.get_aggregate_bytes(aid) == bl.aggregate_write_formatting().write_state(state).value
            assert bl.aggregate_read_formatting().read_state(store.get_aggregate_bytes(aid)) == state
        assert store.get_aggregate_bytes("no-such-aggregate") is None  # KTable miss
        # the plugin's store serves recovered state, later state-topic records override it
        kv = GpuReplayPersistencePlugin(store).create_supplier(store.store_name)
        assert kv.get("agg-1") == store.get_aggregate_bytes("agg-1")
        kv.put("agg-1", b"newer")
        assert kv.get("agg-1") == b"newer"
        # streaming micro-batch with a brand-new aggregate id
        more = [CountIncremented("agg-1", 10, 1000), CountIncremented("agg-new", 7, 1)]
        before = bl.aggregate_read_formatting().read_state(store.get_aggregate_bytes("agg-1"))
        store.apply_events(more)
        after = bl.aggregate_read_formatting().read_state(store.get_aggregate_bytes("agg-1"))
        assert (after.count, after.version) == (before.count + 10, 1000)
        assert bl.aggregate_read_formatting().read_state(store.get_aggregate_bytes("agg-new")) == State("agg-new", 7, 1)
    finally:
        store.close()


@pytest.mark.gpu
def test_bank_account_recovery_with_prior_snapshot():
    from surge_amd.command import SurgeCommandBusinessLogic
    from surge_amd.store import GpuReplayStateStore

    class BL(SurgeCommandBusinessLogic):
        aggregate_name = "BankAccount"

        def __init__(self):
            self.m, self.f = BankAccountCommandModel(), BankAccountFormat()

        def command_model(self):
            return self.m

        def aggregate_read_formatting(self):
            return self.f

        def aggregate_write_formatting(self):
            return self.f

    bl = BL()
    a, b, c = (uuid.UUID(int=i) for i in (1, 2, 3))
    prior = {str(c): bl.m.handle_event(None, BankAccountCreated(c, "Carol", "9", 5.0))}
    events = [
        BankAccountUpdated(b, 50.0),  # before Created: dropped (aggregate.map on None)
        BankAccountCreated(a, "Jane Doe", "1234", 1000.0),
        BankAccountUpdated(a, 1100.0),  # BankAccountCommandEngineSpec.scala:44-68
        BankAccountUpdated(c, 7.5),
    ]
    store = GpuReplayStateStore(bl)
    try:
        store.restore(events, prior=prior)
        got = json.loads(store.get_aggregate_bytes(str(a)))
        assert got == {"accountNumber": str(a), "accountOwner": "Jane Doe", "securityCode": "1234", "balance": 1100.0}
        assert store.get_aggregate_bytes(str(b)) is None
        assert json.loads(store.get_aggregate_bytes(str(c)))["balance"] == 7.5
    finally:
        store.close()


@pytest.mark.gpu
def test_incremental_snapshot_records_compact_to_the_full_refold():
    """Config C5 in miniature: micro-batches -> incremental state-topic records -> log compaction ==
    the KTable a full JVM-style re-fold would produce."""
    import random

    from surge_amd.snapshot import SnapshotWriter, compact
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    model = bl.command_model()
    rng = random.Random(4)
    ids = [f"agg-{i}" for i in range(200)]
    seqs = {k: 0 for k in ids}

    def batch(n):
        out = []
        for _ in range(n):
            k = rng.choice(ids)
            seqs[k] += 1
            out.append(CountIncremented(k, rng.randrange(-5, 50), seqs[k]) if rng.random() < 0.7 else CountDecremented(k, 3, seqs[k]))
        return out

    all_events, log = [], []
    store = GpuReplayStateStore(bl)
    try:
        first = batch(500)
        all_events += first
        store.restore(first, capacity=256)
        writer = SnapshotWriter(store, n_partitions=5)
        log += writer.full_snapshot()
        for _ in range(6):
            b = batch(300)
            all_events += b
            store.apply_events(b)
            log += writer.records_for(sorted({e.aggregateId for e in b}))  # only the touched aggregates
        table = compact(log)
        expect = {}
        for e in all_events:
            expect[e.aggregateId] = model.handle_event(expect.get(e.aggregateId), e)
        assert set(table) == set(expect)
        for k, st in expect.items():
            assert table[k] == bl.aggregate_write_formatting().write_state(st).value
        parts = {r.key: r.partition for r in log}
        from surge_amd.kafka import PartitionStringUpToColon

        assert all(p == PartitionStringUpToColon.instance.partition_for(k, 5) for k, p in parts.items())
    finally:
        store.close()


@pytest.mark.gpu
def test_recovery_from_raw_events_topic_bytes():
    """N1 end to end: lz4 record batches, one transaction per flush, an aborted flush, JSON event values
    (the Counter fixture's own writeEvent) -> ingest -> CSR -> GPU fold -> getAggregateBytes."""
    import kafka_wire as kw
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    model, fmt = bl.command_model(), bl.event_write_formatting()
    flushes = [
        ([CountIncremented("a", 1, 1), CountIncremented("b", 5, 1)], kw.COMMIT),
        ([CountIncremented("a", 1, 2)], kw.ABORT),            # never happened as far as consumers are concerned
        ([CountDecremented("b", 2, 2), NoOpEvent("c", 1)], kw.COMMIT),
        ([CountIncremented("a", 10, 2)], kw.COMMIT),
    ]
    wire, off = [], 0
    for events, outcome in flushes:
        msgs = [fmt.write_event(e) for e in events]
        wire.append(kw.record_batch(off, [(m.key.encode(), m.value) for m in msgs], compression="lz4", transactional=True, producer_id=5))
        off += len(msgs)
        wire.append(kw.control_batch(off, 5, outcome))
        off += 1
    store = GpuReplayStateStore(bl)
    try:
        counters = store.restore_from_topic(b"".join(wire))
        assert counters["records_aborted"] == 1 and counters["records_delivered"] == 5
        expect = {}
        for events, outcome in flushes:
            if outcome == kw.COMMIT:
                for e in events:
                    expect[e.aggregateId] = model.handle_event(expect.get(e.aggregateId), e)
        for k, st in expect.items():
            assert store.get_aggregate_bytes(k) == bl.aggregate_write_formatting().write_state(st).value
        assert expect["a"] == State("a", 11, 2)
    finally:
        store.close()


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [False, True])
def test_recovery_fetch_by_fetch_equals_recovery_from_the_whole_partition(overlap):
    """restore_from_fetches: the host frames fetch i + 1 while the GPU decodes / groups / folds fetch i; transactions
    that span fetches, a batch cut by a fetch boundary and aggregates that first appear late all end in the same store
    as one restore_from_topic over the concatenated bytes."""
    import random

    import kafka_wire as kw
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    fmt = bl.event_write_formatting()
    rnd = random.Random(11)
    seq = {}
    wire, off = [], 0
    for flush in range(60):
        events = []
        for _ in range(rnd.randrange(1, 120)):
            agg = "agg-%d" % rnd.randrange(40 + 25 * flush)  # the id space keeps growing: new aggregates in every fetch
            seq[agg] = seq.get(agg, 0) + 1
            events.append(rnd.choice([CountIncremented(agg, rnd.randrange(100), seq[agg]), CountDecremented(agg, rnd.randrange(100), seq[agg]),
                                      NoOpEvent(agg, seq[agg])]))
        msgs = [fmt.write_event(e) for e in events]
        txn = flush % 3 == 0
        wire.append(kw.record_batch(off, [(m.key.encode(), m.value) for m in msgs], compression=rnd.choice(["none", "lz4"]), transactional=txn, producer_id=5))
        off += len(msgs)
        if txn:
            wire.append(kw.control_batch(off, 5, kw.ABORT if flush % 9 == 0 else kw.COMMIT))
            off += 1
    whole = b"".join(wire)
    # fetch boundaries wherever they fall: inside batches, between a transaction's batch and its marker, ...
    cuts = sorted(rnd.sample(range(1, len(whole)), 9))
    fetches = [whole[a:b] for a, b in zip([0] + cuts, cuts + [len(whole)])]
    one, many = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        c_one = one.restore_from_topic(whole)
        c_many = many.restore_from_fetches(iter(fetches), overlap=overlap)
        assert c_one == c_many and c_one["records_aborted"] > 0
        assert one.keys.keys == many.keys.keys and len(one.keys.keys) > 500
        for k in one.keys.keys:
            assert one.get_aggregate_bytes(k) == many.get_aggregate_bytes(k)
    finally:
        one.close()
        many.close()


# ---- round-2 regressions (aggregates that first appear after recovery) ------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("overlap,consumer_threads", [(False, 1), (True, 1), (True, 2)])
def test_recovery_of_a_consumer_with_several_partitions_equals_the_literal_fold(overlap, consumer_threads):
    """restore_from_fetches(n_partitions=P): what a restore consumer with several assigned partitions receives — per fetch
    response the next bytes of every partition, framed per partition (transactions, an aborted flush, a flush that commits a
    fetch later, a batch cut by the end of a fetch) into one slab, ONE device push per fetch with four in flight, the
    resident state growing as aggregates appear — gives every aggregate the state the literal handle_event fold gives it;
    also with the pushes enqueued by a worker thread and handed to the fold without a host wait (consumer_threads=2)."""
    import random

    import kafka_wire as kw
    from surge_amd.kafka import partition_for_keys
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    model, fmt = bl.command_model(), bl.event_write_formatting()
    rng = random.Random(21)
    P, F = 6, 7
    ids = [f"agg-{i}" for i in range(400)]
    part_of = dict(zip(ids, partition_for_keys(ids, P, up_to_colon=True)))
    seq = {k: 0 for k in ids}
    expect = {}
    logs = [[] for _ in range(P)]   # per partition: the byte chunks of its log, fetch by fetch
    offs = [0] * P
    pid = 50
    for f in range(F):
        for p in range(P):
            chunk = []
            for _ in range(rng.randrange(0, 4)):
                mine = [k for k in ids if part_of[k] == p]
                events = []
                for _ in range(rng.randrange(1, 60)):
                    k = rng.choice(mine)
                    seq[k] += 1
                    events.append(rng.choice([CountIncremented(k, rng.randrange(50), seq[k]), CountDecremented(k, rng.randrange(50), seq[k]), NoOpEvent(k, seq[k])]))
                outcome = kw.COMMIT if rng.random() < 0.8 else kw.ABORT
                msgs = [fmt.write_event(e) for e in events]
                chunk.append(kw.record_batch(offs[p], [(m.key.encode(), m.value) for m in msgs], compression=rng.choice(["lz4", "none"]), transactional=True,
                                             producer_id=pid))
                offs[p] += len(msgs)
                chunk.append(kw.control_batch(offs[p], pid, outcome))
                offs[p] += 1
                pid += 1
                if outcome == kw.COMMIT:
                    for e in events:
                        expect[e.aggregateId] = model.handle_event(expect.get(e.aggregateId), e)
                else:
                    for e in events:  # an aborted flush never happened: its sequence numbers are used again
                        seq[e.aggregateId] -= 1
            logs[p].append(b"".join(chunk))
    # partition 2's third fetch ends in the middle of a batch; partition 4's commit marker of its last flush of fetch 1 arrives a fetch later
    if len(logs[2][2]) > 40:
        cut = len(logs[2][2]) - 33
        logs[2][2], logs[2][3] = logs[2][2][:cut], logs[2][2][cut:] + logs[2][3]
    if len(logs[4][1]) > 78:
        logs[4][1], logs[4][2] = logs[4][1][:-78], logs[4][1][-78:] + logs[4][2]   # (a control batch is 78 bytes on this wire)
    fetches = [[logs[p][f] or None for p in range(P)] for f in range(F)]
    store = GpuReplayStateStore(bl)
    try:
        counters = store.restore_from_fetches(fetches, n_partitions=P, framing_threads=3, overlap=overlap, consumer_threads=consumer_threads)
        assert counters["open_transactions"] == 0
        assert set(store.keys.keys) == set(expect) and counters["records_aborted"] > 0
        for k, st in expect.items():
            assert store.get_aggregate_bytes(k) == bl.aggregate_write_formatting().write_state(st).value, k
    finally:
        store.close()


# ---- the error paths of the recovery loops ---------------------------------------------------------------------
N_FETCHES, BAD_FETCH = 7, 2  # four pushes in flight: fetch 2 is refused while pushes 3 .. 5 are enqueued; seven fetches run the steady state and the drain


def _recovery_threads():
    import threading

    return [t.name for t in threading.enumerate() if t.name.startswith("surge-")]


def _fixed16_events_topic(n_partitions, ids, prior=None):
    """Seven fetch responses of Counter events as 16-byte values, about 40 records per batch (two partitions, or one partition
    with two batches per fetch): ``(good, bad, expect)`` — ``bad`` is ``good`` with one value of fetch 2 seventeen bytes long,
    ``expect`` the literal ``handle_event`` fold of the good topic onto ``prior``."""
    import random

    import kafka_wire as kw

    model = CounterBusinessLogic().command_model()
    rng = random.Random(41)
    P = max(n_partitions, 1)
    expect = dict(prior or {})
    seq = {k: st.version for k, st in expect.items()}
    offs = [0] * P
    good, bad = [], []
    for f in range(N_FETCHES):
        rows = ([], [])
        for p in range(P):
            chunks = ([], [])
            for b in range(2 if P == 1 else 1):
                recs = []
                for _ in range(rng.randrange(35, 46)):
                    k = rng.choice(ids[p::P])
                    seq[k] = seq.get(k, 0) + 1
                    e = rng.choice([CountIncremented(k, rng.randrange(50), seq[k]), CountDecremented(k, rng.randrange(50), seq[k]), NoOpEvent(k, seq[k])])
                    expect[k] = model.handle_event(expect.get(k), e)
                    recs.append((f"{k}:{seq[k]}".encode(), model.encode_events([e]).tobytes()))
                damaged = list(recs)
                if f == BAD_FETCH and p == P - 1 and b == 0:
                    damaged[len(recs) // 2] = (recs[len(recs) // 2][0], b"not sixteen bytes")
                for out, rs in zip(chunks, (recs, damaged)):
                    out.append(kw.record_batch(offs[p], rs, compression="lz4" if (f + p) % 2 else "none"))
                offs[p] += len(recs)
            for row, c in zip(rows, chunks):
                row.append(b"".join(c))
        good.append(rows[0] if n_partitions else rows[0][0])
        bad.append(rows[1] if n_partitions else rows[1][0])
    return good, bad, expect


def _counter_state_topic(n_partitions, ids):
    """Seven fetch responses of the state topic, JSON Counter states, about 40 records per batch with overwrites and tombstones:
    ``(good, bad, records, expect)`` — ``bad`` is ``good`` with the only (so winning) value of one id of fetch 2 cut short,
    ``records`` the good topic's ``(key, value | None)`` pairs, ``expect`` id -> ``State`` or ``None``."""
    import random

    import kafka_wire as kw
    from oracle import oracle

    rng = random.Random(43)
    P = max(n_partitions, 1)
    expect, version = {}, {}
    offs = [0] * P
    good, bad, records = [], [], []
    for f in range(N_FETCHES):
        rows = ([], [])
        for p in range(P):
            chunks = ([], [])
            for b in range(2 if P == 1 else 1):
                recs = []
                for _ in range(rng.randrange(35, 46)):
                    k = rng.choice(ids[p::P])
                    if expect.get(k) is not None and rng.random() < 0.15:
                        expect[k] = None
                        recs.append((k.encode(), None))
                        continue
                    version[k] = version.get(k, 0) + 1
                    expect[k] = State(k, rng.randrange(-1000, 1000), version[k])
                    recs.append((k.encode(), oracle.counter_state_json(k, expect[k].count, expect[k].version)))
                damaged = list(recs)
                if f == BAD_FETCH and p == P - 1 and b == 0:
                    expect["only-once"] = State("only-once", 5, 1)
                    recs.insert(len(recs) // 2, (b"only-once", oracle.counter_state_json("only-once", 5, 1)))
                    damaged.insert(len(damaged) // 2, (b"only-once", oracle.counter_state_json("only-once", 5, 1)[:-1]))
                records += [(k.decode(), v) for k, v in recs]
                for out, rs in zip(chunks, (recs, damaged)):
                    out.append(kw.record_batch(offs[p], rs, compression="lz4" if (f + p) % 2 else "none"))
                offs[p] += len(recs)
            for row, c in zip(rows, chunks):
                row.append(b"".join(c))
        good.append(rows[0] if n_partitions else rows[0][0])
        bad.append(rows[1] if n_partitions else rows[1][0])
    return good, bad, records, expect


def _same_as_the_literal_fold(store, bl, expect):
    assert set(store.keys.keys) == set(expect)
    for k, st in expect.items():
        assert store.get_aggregate_bytes(k) == (None if st is None else bl.aggregate_write_formatting().write_state(st).value), k


@pytest.mark.gpu
@pytest.mark.parametrize("n_partitions", [0, 2])
@pytest.mark.parametrize("overlap,consumer_threads", [(False, 1), (True, 1), (True, 2)])
def test_a_recovery_whose_middle_fetch_is_refused_raises_returns_and_the_same_store_then_recovers(overlap, consumer_threads, n_partitions):
    """restore_from_fetches over seven fetches whose third carries one 17-byte value on a topic of 16-byte events: the decoder
    refuses that push (a status, no fault) while later pushes are in flight — the call raises ``IngestError``, returns with no
    framing or push thread left, and the same store object then recovers the topic without the bad record to the literal fold."""
    from surge_amd.ingest import IngestError
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    good, bad, expect = _fixed16_events_topic(n_partitions, [f"agg-{i}" for i in range(90)])
    arm = dict(n_partitions=n_partitions, framing_threads=2, overlap=overlap, consumer_threads=consumer_threads)
    store = GpuReplayStateStore(bl)
    try:
        with pytest.raises(IngestError):
            store.restore_from_fetches(iter(bad), **arm)
        assert _recovery_threads() == []
        counters = store.restore_from_fetches(iter(good), **arm)
        assert counters["open_transactions"] == 0 and counters["records_delivered"] == counters["records_seen"] > 7 * 2 * 35
        _same_as_the_literal_fold(store, bl, expect)
    finally:
        store.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_partitions", [0, 2])
def test_a_state_topic_whose_middle_fetch_holds_a_damaged_winner_raises_returns_and_the_same_store_then_resumes(n_partitions):
    """restore_from_state_topic over seven fetches of JSON Counter states; the only value of one id, in fetch 2, does not decode:
    ``IngestError`` (CORRUPT) out of that fetch's load while later pushes are in flight, no thread left, and a second call with
    good bytes on the same store restores every id's last state (tombstones: None)."""
    from surge_amd.ingest import IngestError
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    good, bad, _, expect = _counter_state_topic(n_partitions, [f"agg-{i}" for i in range(90)])
    store = GpuReplayStateStore(bl)
    try:
        with pytest.raises(IngestError) as ei:
            store.restore_from_state_topic(iter(bad), n_partitions=n_partitions, framing_threads=2)
        assert ei.value.status == -7  # SURGE_E_CORRUPT
        assert _recovery_threads() == []
        counts = store.restore_from_state_topic(iter(good), n_partitions=n_partitions, framing_threads=2)
        assert counts["refused"] == 0 and counts["tombstones"] > 0 and counts["records_delivered"] > 7 * 2 * 35
        _same_as_the_literal_fold(store, bl, expect)
    finally:
        store.close()


@pytest.mark.gpu
def test_a_refused_fetch_in_the_tail_of_a_resume_raises_returns_and_resets_the_decode_base():
    """restore_from_state_topic(events_fetches=...): the state topic loads, the state decoder continues as the events decoder, and
    fetch 2 of the TAIL carries the 17-byte value.  ``IngestError``, no thread left; the engine's decode base is back to zeros
    (a bare ``decode_states`` leaves the bytes its template does not name zero), ``restore_from_state_records`` on the same store
    gives them the algebra's defaults as ever, and the call with the good tail resumes to the literal fold."""
    import torch

    from oracle import oracle
    from surge_amd import schema as S
    from surge_amd.encode import JsonTemplate, decode_states, key_table_utf8
    from surge_amd.ingest import IngestError
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    ids = [f"agg-{i}" for i in range(90)]
    states, _, records, snapshot = _counter_state_topic(2, ids)
    prior = {k: st for k, st in snapshot.items() if st is not None}
    tail, bad_tail, expect = _fixed16_events_topic(2, ids + [f"late-{i}" for i in range(10)], prior=prior)
    expect = {**snapshot, **expect}  # (an id deleted in the snapshot and untouched by the tail stays None)
    resume = dict(n_partitions=2, framing_threads=2, events_partitions=2)
    store = GpuReplayStateStore(bl)
    try:
        with pytest.raises(IngestError):
            store.restore_from_state_topic(iter(states), events_fetches=iter(bad_tail), **resume)
        assert _recovery_threads() == []
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        value = oracle.counter_state_json("probe", 7, 3)
        res = decode_states(store.engine, JsonTemplate.counter(), dev(np.frombuffer(value, dtype=np.uint8).copy()), dev(np.array([0, len(value)], dtype=np.int64)),
                            *(dev(x) for x in key_table_utf8(["probe"])))
        row = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)[0]
        assert res[2][0] == 1 and (int(row["count"]), int(row["version"])) == (7, 3)
        assert (int(row["min_arg"]), int(row["max_arg"])) == (0, 0)  # no base: what the template does not name is zero
        store.restore_from_state_records(records)
        _same_as_the_literal_fold(store, bl, snapshot)
        rows = store.engine.snapshot()
        present = (rows["flags"] & S.STATE_PRESENT) != 0
        assert present.sum() == len(prior) and (rows["min_arg"][present] == S.INT32_MAX).all() and (rows["max_arg"][present] == S.INT32_MIN).all()
        counts = store.restore_from_state_topic(iter(states), events_fetches=iter(tail), **resume)
        assert counts["refused"] == 0 and counts["tail_records_delivered"] > 7 * 2 * 35
        _same_as_the_literal_fold(store, bl, expect)
    finally:
        store.close()


@pytest.mark.gpu
@pytest.mark.parametrize("overlap,consumer_threads", [(False, 1), (True, 1), (True, 2)])
def test_recovery_that_folds_once_packs_the_decoded_fetches_into_the_log_the_host_pack_gives(overlap, consumer_threads):
    """restore_from_fetches(bound_log=True) — VERDICT r5 item 2: the decoded fetches of a transactional multi-partition topic
    (aborted flushes, a marker that arrives a fetch late, a batch cut by a fetch) are STAGED on the device, packed at the
    topic's end into ONE CSR log (surge_replay_pack_staged: stable sort by aggregate, topic order inside an aggregate) and
    folded once.  The packed log is byte for byte what the host pack of the SOURCE events gives (seg_off and the 16-byte
    events of every aggregate in its partition's committed order); the states are the literal fold's; the log stays bound:
    SORTED / CHUNKED / FLAT / TILED re-folds of it give the same bytes."""
    import random

    import kafka_wire as kw
    from surge_amd import schema as S
    from surge_amd.kafka import partition_for_keys
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    model, fmt = bl.command_model(), bl.event_write_formatting()
    rng = random.Random(31)
    P, F = 5, 8
    ids = [f"agg-{i}" for i in range(300)]
    part_of = dict(zip(ids, partition_for_keys(ids, P, up_to_colon=True)))
    seq = {k: 0 for k in ids}
    expect, committed = {}, {}
    logs = [[] for _ in range(P)]
    offs = [0] * P
    pid = 70
    for f in range(F):
        for p in range(P):
            chunk = []
            for _ in range(rng.randrange(0, 4)):
                mine = [k for k in ids if part_of[k] == p]
                events = []
                for _ in range(rng.randrange(1, 80)):
                    k = rng.choice(mine[: 5 + 12 * f]) if rng.random() < 0.5 else mine[0]  # one hot aggregate per partition, new ids in every fetch
                    seq[k] += 1
                    events.append(rng.choice([CountIncremented(k, rng.randrange(50), seq[k]), CountDecremented(k, rng.randrange(50), seq[k]), NoOpEvent(k, seq[k])]))
                outcome = kw.COMMIT if rng.random() < 0.8 else kw.ABORT
                msgs = [fmt.write_event(e) for e in events]
                chunk.append(kw.record_batch(offs[p], [(m.key.encode(), m.value) for m in msgs], compression=rng.choice(["lz4", "none"]), transactional=True,
                                             producer_id=pid))
                offs[p] += len(msgs)
                chunk.append(kw.control_batch(offs[p], pid, outcome))
                offs[p] += 1
                pid += 1
                if outcome == kw.COMMIT:
                    for e in events:
                        expect[e.aggregateId] = model.handle_event(expect.get(e.aggregateId), e)
                        committed.setdefault(e.aggregateId, []).append(e)
                else:
                    for e in events:
                        seq[e.aggregateId] -= 1
            logs[p].append(b"".join(chunk))
    if len(logs[1][2]) > 40:
        cut = len(logs[1][2]) - 33
        logs[1][2], logs[1][3] = logs[1][2][:cut], logs[1][2][cut:] + logs[1][3]
    if len(logs[3][1]) > 78:
        logs[3][1], logs[3][2] = logs[3][1][:-78], logs[3][1][-78:] + logs[3][2]
    fetches = [[logs[p][f] or None for p in range(P)] for f in range(F)]
    store = GpuReplayStateStore(bl)
    try:
        counters = store.restore_from_fetches(fetches, n_partitions=P, framing_threads=3, overlap=overlap, consumer_threads=consumer_threads, bound_log=True)
        assert counters["open_transactions"] == 0 and counters["records_aborted"] > 0
        assert set(store.keys.keys) == set(expect)
        for k, st in expect.items():
            assert store.get_aggregate_bytes(k) == bl.aggregate_write_formatting().write_state(st).value, k
        # the packed log against the host pack of the source events
        eng = store.engine
        so, ev = eng.bound_log()
        so, ev = so.cpu().numpy(), ev.cpu().numpy()
        keys = store.keys.keys
        assert so.shape[0] == len(keys) + 1 and so[0] == 0
        want_off = np.zeros(len(keys) + 1, np.int64)
        np.cumsum([len(committed[k]) for k in keys], out=want_off[1:])
        assert np.array_equal(so, want_off)
        want_ev = np.concatenate([model.encode_events(committed[k]) for k in keys])
        assert ev.tobytes() == want_ev.tobytes()
        assert ev.shape[0] == counters["records_delivered"]
        first = eng.snapshot().tobytes()
        for algo in (S.ALGO_SORTED, S.ALGO_CHUNKED, S.ALGO_FLAT, S.ALGO_TILED):
            eng.fold(algo)
            assert eng.snapshot().tobytes() == first, algo
    finally:
        store.close()


@pytest.mark.gpu
def test_the_packer_keeps_topic_order_inside_an_aggregate_leaves_empty_segments_and_refuses_a_bad_index():
    """surge_replay_stage_events_device / surge_replay_pack_staged alone: events staged in several calls (the staging log
    grows), ids without events (empty segments, also at both ends), a hot aggregate; the packed log = numpy's stable sort.
    An index >= n_agg fails the pack with SURGE_E_RANGE, nothing is bound and the staging log is kept: the right n_agg packs."""
    import torch

    from oracle import oracle
    from surge_amd import schema as S
    from surge_amd import synth
    from surge_amd.replay import ReplayEngine, ReplayError

    rng = np.random.default_rng(5)
    n_agg, m = 5000, 200_000
    agg = rng.integers(3, n_agg - 7, m)
    agg[rng.random(m) < 0.2] = 1234  # hot
    ev = synth.to_event_records(synth.event_words(np.arange(m, dtype=np.int64), agg, np.arange(m, dtype=np.int64), 9, synth.STRESS_MIX))
    dev = torch.device("cuda:0")
    with ReplayEngine() as eng:
        for lo in range(0, m, 37_000):
            a = torch.from_numpy(agg[lo:lo + 37_000].astype(np.int64)).to(dev)
            e = torch.from_numpy(ev[lo:lo + 37_000].view(np.int64).reshape(-1, 2)).to(dev)
            eng.stage_events(a, e)
        assert eng.staged == m
        with pytest.raises(ReplayError):
            eng.pack_staged(n_agg - 100)  # some staged index is beyond it
        assert eng.staged == m
        eng.pack_staged(n_agg)
        assert eng.staged == 0
        so, pe = eng.bound_log()
        order = np.argsort(agg, kind="stable")
        want_off = np.zeros(n_agg + 1, np.int64)
        np.cumsum(np.bincount(agg, minlength=n_agg), out=want_off[1:])
        assert np.array_equal(so.cpu().numpy(), want_off)
        assert pe.cpu().numpy().tobytes() == ev[order].tobytes()
        eng.fold()
        assert eng.snapshot().tobytes() == oracle.fold_csr(want_off, ev[order]).tobytes()


def test_pack_batch_rejects_an_over_capacity_batch_without_interning_anything():
    from surge_amd.log import KeyTable, pack_batch

    model = CounterBusinessLogic().command_model()
    keys = KeyTable()
    keys.intern("a")
    with pytest.raises(IndexError):
        pack_batch(model, [CountIncremented("a", 1, 1), CountIncremented("b", 1, 1), CountIncremented("c", 1, 1)], keys, n_agg=2)
    assert keys.keys == ["a"]  # a rejected batch leaves the key table as it was
    g, off, ev = pack_batch(model, [CountIncremented("b", 1, 1), CountIncremented("a", 2, 2)], keys, n_agg=2)
    assert list(g) == [0, 1] and keys.keys == ["a", "b"]


@pytest.mark.gpu
def test_new_aggregates_after_recovery_grow_the_resident_state():
    # restore() with the default capacity, then micro-batches that introduce new ids: the normal Surge case
    from surge_amd.snapshot import SnapshotWriter, compact
    from surge_amd.store import GpuReplayStateStore

    bl = CounterBusinessLogic()
    model = bl.command_model()
    store = GpuReplayStateStore(bl)
    try:
        first = [CountIncremented("a", 1, 1), CountIncremented("b", 2, 1), CountIncremented("a", 3, 2)]
        store.restore(first)
        assert store.engine.n_agg == 2
        expect = {}
        for e in first:
            expect[e.aggregateId] = model.handle_event(expect.get(e.aggregateId), e)
        seq = 0
        for round_ in range(4):  # each round brings ids the store has never seen (several reallocations)
            batch = []
            for i in range(50 * (round_ + 1)):
                seq += 1
                k = f"new-{round_}-{i % (20 * (round_ + 1))}"
                batch.append(CountIncremented(k, i, seq))
            batch.append(CountDecremented("a", 1, 100 + round_))
            store.apply_events(batch)
            for e in batch:
                expect[e.aggregateId] = model.handle_event(expect.get(e.aggregateId), e)
            assert store.engine.n_agg == len(store.keys) == len(expect)
        fmt = bl.aggregate_write_formatting()
        for k, st in expect.items():
            assert store.get_aggregate_bytes(k) == fmt.write_state(st).value
        table = compact(SnapshotWriter(store, n_partitions=5).full_snapshot())
        assert table == {k: fmt.write_state(st).value for k, st in expect.items()}
        # a full fold of the (now too short) bound log is refused loudly, not silently wrong
        from surge_amd.replay import ReplayError

        with pytest.raises(ReplayError):
            store.engine.fold()
    finally:
        store.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_framing", [True, False])
def test_bulk_snapshot_publish_emits_only_what_changed_as_kafka_record_batches(device_framing):
    # N2 x N3 on the device path: delta kernel -> GPU JSON encoder (filtered) -> K4 partitions -> RecordBatch v2 bytes,
    # decoded again by the product's ingest.  "Nothing published when the state did not change" (PersistentActor.scala:212,257).
    import numpy as np

    from oracle import oracle
    from surge_amd import schema as S
    from surge_amd.ingest import EventsTopicIngest
    from surge_amd.kafka import partition_for_keys
    from surge_amd.replay import ReplayEngine
    from surge_amd.snapshot import BulkSnapshotPublisher

    rng = np.random.default_rng(5)
    n, n_part = 600, 4
    keys = [f"agg-{i:04d}" for i in range(n)]
    lens = rng.integers(0, 9, size=n)
    so = np.zeros(n + 1, np.int64); np.cumsum(lens, out=so[1:])
    ne = int(so[-1])
    ev = S.make_events(rng.choice([S.EVT_INC, S.EVT_INC, S.EVT_DEC, S.EVT_NOOP, S.EVT_DELETE, S.EVT_THROW], size=ne, p=[.4, .2, .2, .1, .07, .03]),
                       rng.integers(1, 1000, size=ne), rng.integers(-50, 50, size=ne))

    def decode(batches):
        recs = {}
        for p, data in batches.items():
            with EventsTopicIngest() as g:
                g.feed(data)
                for _, _, k, v in g.drain_records():
                    assert k.decode() not in recs and partition_for_keys([k.decode()], n_part, up_to_colon=True)[0] == p
                    recs[k.decode()] = v
        return recs

    def expected(states, before):
        out = {}
        for i, k in enumerate(keys):
            st, old = states[i], before[i]
            if st["flags"] & S.STATE_POISONED or st.tobytes() == old.tobytes():
                continue
            out[k] = oracle.counter_state_json(k, int(st["count"]), int(st["version"])) if st["flags"] & S.STATE_PRESENT else None
        return out

    with ReplayEngine() as eng:
        eng.load_csr(so, ev)
        eng.fold()
        pub = BulkSnapshotPublisher(eng, keys, n_part, device_framing=device_framing)
        assert (pub.framer is not None) == device_framing
        try:
            s1 = oracle.fold_csr(so, ev)
            got = decode(pub.publish())
            assert got == expected(s1, S.empty_states(n)) and len(got) > 300
            assert all(v is not None for v in got.values())  # None aggregates were never published: no tombstone needed
            assert decode(pub.publish()) == {}               # nothing changed: nothing published
            # a micro-batch: some aggregates change, some are deleted (=> tombstones), one None aggregate materialises
            touched = rng.choice(n, size=40, replace=False)
            be = S.make_events([S.EVT_DELETE if j % 5 == 0 else S.EVT_INC for j in range(40)], rng.integers(1000, 2000, size=40), rng.integers(1, 9, size=40))
            eng.append_events(touched.astype(np.int64), be)
            full_off = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(touched, minlength=n), out=full_off[1:])
            order = np.argsort(touched, kind="stable")
            s2 = oracle.fold_csr(full_off, be[order], s1)
            got = decode(pub.publish())
            assert got == expected(s2, s1)
            assert any(v is None for v in got.values()) and 0 < len(got) <= 40
            assert pub.timings["values"] + pub.timings["tombstones"] == len(got)
            # the same publish with its framing in the background while the store keeps folding: what is published is the
            # state AT THE DELTA, the batch folded meanwhile shows up in the next snapshot — nothing lost, nothing twice
            touched2 = rng.choice(n, size=60, replace=False)
            be2 = S.make_events([S.EVT_INC] * 60, rng.integers(2000, 3000, size=60), rng.integers(1, 9, size=60))
            eng.append_events(touched2.astype(np.int64), be2)
            off2 = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(touched2, minlength=n), out=off2[1:])
            s3 = oracle.fold_csr(off2, be2[np.argsort(touched2, kind="stable")], s2)
            pending = pub.publish_async()
            touched3 = rng.choice(n, size=50, replace=False)
            be3 = S.make_events([S.EVT_DEC] * 50, rng.integers(3000, 4000, size=50), rng.integers(1, 9, size=50))
            eng.append_events(touched3.astype(np.int64), be3)  # folds while the worker thread frames
            off3 = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(touched3, minlength=n), out=off3[1:])
            s4 = oracle.fold_csr(off3, be3[np.argsort(touched3, kind="stable")], s3)
            assert decode(pending.result()) == expected(s3, s2)
            assert decode(pub.publish_async().result()) == expected(s4, s3)
            # a framing failure after the baseline was committed: the aggregates are reported again by the next publish
            touched4 = rng.choice(n, size=30, replace=False)
            be4 = S.make_events([S.EVT_INC] * 30, rng.integers(4000, 5000, size=30), rng.integers(1, 9, size=30))
            eng.append_events(touched4.astype(np.int64), be4)
            off4 = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(touched4, minlength=n), out=off4[1:])
            s5 = oracle.fold_csr(off4, be4[np.argsort(touched4, kind="stable")], s4)
            target = pub.framer if device_framing else pub.writer
            method = "frame" if device_framing else "append_indexed"
            real = getattr(target, method)
            setattr(target, method, lambda *a, **k: (_ for _ in ()).throw(MemoryError("framing failed")))
            with pytest.raises(MemoryError):
                pub.publish_async().result()
            setattr(target, method, real)
            assert decode(pub.publish()) == expected(s5, s4)
            # a deferred commit: a fold between publish(commit=False) and commit_published() is refused — the
            # commit would copy the NEWER states into the baseline and they would never be emitted — and nothing is lost:
            # the next publish reports the aggregates of both batches with their current states
            from surge_amd.replay import ReplayError

            touched5 = rng.choice(n, size=30, replace=False)
            be5 = S.make_events([S.EVT_INC] * 30, rng.integers(5000, 6000, size=30), rng.integers(1, 9, size=30))
            eng.append_events(touched5.astype(np.int64), be5)
            off5 = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(touched5, minlength=n), out=off5[1:])
            s6 = oracle.fold_csr(off5, be5[np.argsort(touched5, kind="stable")], s5)
            assert decode(pub.publish(commit=False)) == expected(s6, s5)
            touched6 = rng.choice(n, size=30, replace=False)
            be6 = S.make_events([S.EVT_INC] * 30, rng.integers(6000, 7000, size=30), rng.integers(1, 9, size=30))
            eng.append_events(touched6.astype(np.int64), be6)
            off6 = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(touched6, minlength=n), out=off6[1:])
            s7 = oracle.fold_csr(off6, be6[np.argsort(touched6, kind="stable")], s6)
            with pytest.raises(ReplayError) as ei:
                pub.commit_published()
            assert ei.value.status == -2 and "changed since" in str(ei.value)  # SURGE_E_STATE
            assert decode(pub.publish()) == expected(s7, s5)
            # and the undisturbed deferred commit still works
            eng.append_events(touched5.astype(np.int64), be5)
            s8 = oracle.fold_csr(off5, be5[np.argsort(touched5, kind="stable")], s7)
            assert decode(pub.publish(commit=False)) == expected(s8, s7)
            pub.commit_published()
            assert decode(pub.publish()) == {}
        finally:
            pub.close()
