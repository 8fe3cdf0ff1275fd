"""-m gpu: the state topic published from a store that is on the device route (``host_keys=False``) — the publisher follows the
decoder's key table and partitions the ids from their UTF-8 bytes on the GPU (``BulkSnapshotPublisher(decoder=...)``,
``GpuReplayStateStore.snapshot_publisher``), and the store stays on that route.

The expectation is the route that was there before: the same topic restored with ``host_keys=True`` and published through
``BulkSnapshotPublisher(engine, store.keys.keys, ...)`` — byte for byte; at the decoder level the test's own fold and
``kafka.partition_for_keys``."""
import ctypes

import numpy as np
import pytest
import torch

import start_offsets_gen as sgen
import state_strings_gen as gen
from fixture_models import BankAccountBusinessLogic
from state_topic_gen import compacted_batch
from surge_amd import _native
from surge_amd import schema as S
from surge_amd.encode import JsonTemplate
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest
from surge_amd.kafka import partition_for_keys, utf16_table
from surge_amd.replay import ReplayEngine, ReplayError
from surge_amd.snapshot import BulkSnapshotPublisher, StoreSnapshotPublisher
from surge_amd.store import GpuReplayStateStore
from test_store_device_reads_gpu import EndingCounterLogic, counter_topic, counting_snapshots

pytestmark = pytest.mark.gpu

BANK = JsonTemplate.bank_account()
T_INC = 1
ARMS = ({}, {"compression": "lz4", "device_compression": True}, {"compression": "lz4"}, {"device_framing": False})


def records_of(batches):
    """``{partition: [(key bytes, value bytes | None)]}`` of a publish, read back by the host framer (CRCs, LZ4, varints)."""
    out = {}
    for p, data in batches.items():
        with EventsTopicIngest() as g:
            g.feed(bytes(data))
            out[p] = [(k, v) for _, _, k, v in g.drain_records()]
    return out


def everything_again(store):
    """The next publish reports every aggregate (a resume from the state topic makes what it loaded the baseline)."""
    eng = store.engine
    ones = torch.ones(eng.n_agg, dtype=torch.uint8, device=f"cuda:{eng.device}")
    torch.cuda.synchronize()
    eng._check(_native.load().surge_replay_snapshot_invalidate(eng._h, ctypes.c_void_p(ones.data_ptr())))
    eng.synchronize()


def test_a_device_route_store_publishes_its_host_route_twins_bytes_and_stays_on_the_route():
    fetches, ids, fate = counter_topic(n_ids=300, seed=21)
    assert any(ord(ch) > 127 for k in ids for ch in k)
    a, b = GpuReplayStateStore(EndingCounterLogic()), GpuReplayStateStore(EndingCounterLogic())
    pubs = []
    try:
        mirrors = counting_snapshots(a)
        a.restore_from_fetches(fetches, host_keys=False)
        b.restore_from_fetches(fetches)
        assert a.device_route and not b.device_route
        assert type(b.snapshot_publisher(4)) is BulkSnapshotPublisher  # the host route: what callers write today
        pubs.append(b.snapshot_publisher(4))
        for arm in ARMS:
            pa, pb = a.snapshot_publisher(4, **arm), BulkSnapshotPublisher(b.engine, b.keys.keys, 4, **arm)
            pubs += [pa, pb]
            assert isinstance(pa, StoreSnapshotPublisher) and (pa.framer is None) == (pb.framer is None)
            got = {p: bytes(v) for p, v in pa.publish(commit=False, timestamp_ms=1234).items()}  # (not committed: every arm publishes everything)
            want = {p: bytes(v) for p, v in pb.publish(commit=False, timestamp_ms=1234).items()}
            assert sorted(got) == [0, 1, 2, 3] and got == want, arm
            assert a.device_route and mirrors == [] and len(a._keys) == 0
        recs = records_of(got)
        alive = {k for k in ids if not isinstance(fate[k], str)}
        assert {k.decode() for rs in recs.values() for k, v in rs if v is not None} == alive
        for p, rs in recs.items():
            assert (partition_for_keys([k.decode() for k, _ in rs], 4, up_to_colon=True) == p).all()
        assert pa.publish(timestamp_ms=1235) != {}  # committed now ...
        for _ in range(3):
            assert pa.publish(timestamp_ms=1236) == {}  # ... so a second publish has nothing to say
        assert a.device_route and mirrors == [] and len(a._keys) == 0  # any number of publishes later
        # the store leaves the route (its host table is asked for): the decoder is closed, and the publisher never touches it
        assert len(a.keys) == len(ids) and not a.device_route
        for call in (pa.publish, pa.publish_async):
            with pytest.raises(RuntimeError, match="left the device route"):
                call()
        with pytest.raises(RuntimeError, match="left the device route"):
            pubs[1].publish()  # (the first arm's)
        assert type(a.snapshot_publisher(4)) is BulkSnapshotPublisher
        pubs.append(a.snapshot_publisher(4))
        # ... and so does a store that was restored again: the publisher belongs to the recovery it was made after
        a.restore_from_fetches(fetches, host_keys=False)
        fresh = a.snapshot_publisher(4)
        pubs.append(fresh)
        with pytest.raises(RuntimeError, match="restored again"):
            pa.publish()
        fresh.publish(timestamp_ms=1237)  # (the engine's baseline outlives a restore: what it says is not this test's)
        assert a.device_route
    finally:
        for pub in pubs:
            pub.close()
        a.close()
        b.close()


def bank_topic(n_partitions=2, seed=4):
    """A BankAccount state topic over ids with colons (and without, and non-ASCII ones), each id on the partition the default
    partitioner gives it; built from ``state_strings_gen.state_text`` and ``state_topic_gen.compacted_batch``.
    -> ``(bytes per partition, {id: (owner, code, balance) | None})``."""
    rng = np.random.default_rng(seed)
    ids = [f"acct-{i}:sub" for i in range(60)] + [f"plain-{i}" for i in range(40)] + [f"é€-{i}:x:y" for i in range(20)] + [":lead", "trail:", "😀:1"]
    home = partition_for_keys(ids, n_partitions, up_to_colon=True)
    table, logs, next_off = {}, [b""] * n_partitions, [0] * n_partitions
    for round_ in range(3):
        for p in range(n_partitions):
            recs = []
            for i, k in enumerate(ids):
                if home[i] != p or (round_ and rng.random() < 0.5):
                    continue
                if table.get(k) is not None and rng.random() < 0.3:
                    table[k], value = None, None
                else:
                    table[k] = (gen.OWNERS[(i + round_) % len(gen.OWNERS)], "" if i % 5 == 0 else f"{i:04d}", float(int(rng.integers(-10 ** 6, 10 ** 6))) / 100.0 or 1.0)
                    value = gen.state_text(k, *table[k])
                recs.append((len(recs), k.encode(), value))
            data, _, next_off[p] = compacted_batch(next_off[p], recs, "lz4" if round_ % 2 else "none")
            logs[p] += data
    assert any(t is None for t in table.values()) and sum(t is not None for t in table.values()) > 80
    return logs, table


def test_a_bank_account_state_topic_with_colons_in_its_ids_is_published_with_its_kept_strings():
    logs, table = bank_topic()
    ids = list(table)
    a, b, c = (GpuReplayStateStore(BankAccountBusinessLogic()) for _ in range(3))
    pubs = []
    try:
        a.restore_from_state_topic([logs], n_partitions=2, template=BANK, host_keys=False)
        b.restore_from_state_topic([logs], n_partitions=2, template=BANK)
        assert a.device_route and a.state_strings is not None
        arm = {"compression": "lz4", "device_compression": True}
        pa = a.snapshot_publisher(2, **arm)  # template, envelope and strings are the restore's
        pb = BulkSnapshotPublisher(b.engine, b.keys.keys, 2, template=BANK, strings=b.state_string_columns(), **arm)
        pubs += [pa, pb]
        assert pa.template is BANK and pa.publish(timestamp_ms=5) == {}  # (the loaded states are the baseline)
        everything_again(a)
        everything_again(b)
        got = {p: bytes(v) for p, v in pa.publish(timestamp_ms=77).items()}
        want = {p: bytes(v) for p, v in pb.publish(timestamp_ms=77).items()}
        assert sorted(got) == [0, 1] and got == want and a.device_route
        for p, rs in records_of(got).items():
            assert (partition_for_keys([k.decode() for k, _ in rs], 2, up_to_colon=True) == p).all()
            assert all((v is None) == (table[k.decode()] is None) for k, v in rs)
            assert all(v == gen.state_text(k.decode(), *table[k.decode()]) for k, v in rs if v is not None)
        # what was published restores: rows and strings
        c.restore_from_state_topic([[got[0], got[1]]], n_partitions=2, template=BANK)
        served = b.get_aggregate_bytes_many(ids, template=BANK)
        assert c.get_aggregate_bytes_many(ids, template=BANK) == served == a.get_aggregate_bytes_many(ids, template=BANK)
        assert served == [gen.state_text(k, *t) if t else None for k, t in table.items()]
    finally:
        for pub in pubs:
            pub.close()
        for s in (a, b, c):
            s.close()


def counter_text(k, count, version):
    return b'{"aggregateId":"%s","count":%d,"version":%d}' % (k.encode(), count, version)


def push_increments(d, eng, ids, seqs, by):
    """One ``T_INC`` event per id (keys ``<id>:<seq>``), pushed, folded onto ``eng``."""
    keys = []
    for k in ids:
        raw = k if isinstance(k, bytes) else k.encode()
        seqs[raw] = seqs.get(raw, 0) + 1
        keys.append(raw + b":%d" % seqs[raw])
    d.push_records(keys, [sgen.fixed16(T_INC, seqs[k.rsplit(b":", 1)[0]], by) for k in keys])
    d.fold_into(eng)
    eng.n_agg = d.n_keys  # (grown inside fold_into)


@pytest.fixture
def folding():
    with DeviceDecoder(None) as d, ReplayEngine(EndingCounterLogic().command_model().event_algebra()) as eng:
        eng.load_csr(np.zeros(1, np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
        eng.fold()
        yield d, eng


@pytest.mark.parametrize("arm", [{}, {"device_framing": False}], ids=["device-framer", "host-writer"])
def test_a_publisher_that_follows_a_decoder_hashes_only_the_rows_that_are_new(folding, arm):
    d, eng = folding
    first = ["agg-%d" % i for i in range(200)] + ["é-ключ", "smile-😀", "x" * 200]
    later = ["born-later-%d" % i for i in range(1500)] + ["€"]
    seqs = {}
    pub = BulkSnapshotPublisher(eng, None, 4, decoder=d, **arm)
    try:
        assert pub.publish(timestamp_ms=1) == {}  # no aggregate yet
        push_increments(d, eng, first, seqs, 5)
        one = records_of(pub.publish(timestamp_ms=2))
        assert {p: sorted(rs) for p, rs in one.items()} == {
            p: sorted((k.encode(), counter_text(k, 5, 1)) for k, q in zip(first, partition_for_keys(first, 4, up_to_colon=True)) if q == p) for p in range(4)}
        hashed = []
        hash_rows = eng.partition_hash_utf8_device
        eng.partition_hash_utf8_device = lambda d_utf8, d_off, *a, **kw: (hashed.append(int(d_off.numel()) - 1), hash_rows(d_utf8, d_off, *a, **kw))[1]
        push_increments(d, eng, first[:3] + later, seqs, 2)  # the arena grows: the table's tensors move
        two = records_of(pub.publish(timestamp_ms=3))
        touched = {k: counter_text(k, 7, 2) for k in first[:3]}
        touched.update({k: counter_text(k, 2, 1) for k in later})
        want = {}
        for k, q in zip(touched, partition_for_keys(list(touched), 4, up_to_colon=True)):
            want.setdefault(int(q), []).append((k.encode(), touched[k]))
        assert {p: sorted(rs) for p, rs in two.items()} == {p: sorted(rs) for p, rs in want.items()}
        assert hashed == [len(later)]  # only the rows behind the last one hashed
        assert pub.publish(timestamp_ms=4) == {} and hashed == [len(later)]
        # today's rule stays, checked after the refresh: rows the key table has no id for are refused
        eng.grow(d.n_keys + 2)
        with pytest.raises(ValueError, match="no key for"):
            pub.publish()
    finally:
        pub.close()


def test_a_malformed_id_refuses_the_publish_before_anything_is_framed(folding):
    d, eng = folding
    good = ["agg-%d" % i for i in range(40)]
    bad = b"\xff\xfeid"
    seqs = {}
    pub = BulkSnapshotPublisher(eng, None, 4, decoder=d)
    tables_pub = None
    try:
        push_increments(d, eng, good, seqs, 1)
        assert sum(len(rs) for rs in records_of(pub.publish()).values()) == len(good)
        arrivals = [b"new-1", bad, b"new-2"]
        push_increments(d, eng, arrivals + [good[0].encode()], seqs, 3)
        offsets_before = pub.framer.next_offsets().copy()
        for _ in range(2):  # refused again as long as the id is there: its rows stay unpartitioned
            with pytest.raises(ReplayError) as ei:
                pub.publish()
            assert ei.value.status == -7 and f"row {len(good) + 1} " in str(ei.value) and repr(bad) in str(ei.value)
        assert (pub.framer.next_offsets() == offsets_before).all()  # nothing was framed
        # ... and the baseline did not move: a publisher over the same rows that is GIVEN partitions for them (the 4-tuple
        # form, whose UTF-16 table has some replacement for the malformed id) emits everything the refused publish owed
        raw = [k.encode() for k in good] + arrivals
        data = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
        off = np.concatenate(([0], np.cumsum([len(k) for k in raw]))).astype(np.int64)
        u16, o16 = utf16_table([k.decode("utf-8", "replace") for k in raw])
        tables_pub = BulkSnapshotPublisher(eng, None, 4, tables=(data, off, u16.view(np.int16), o16))
        owed = [(k, v) for rs in records_of(tables_pub.publish()).values() for k, v in rs]
        assert sorted(k for k, _ in owed) == sorted([b"new-1", bad, b"new-2", good[0].encode()]) and all(v is not None for _, v in owed)
        assert {(b"new-1", counter_text("new-1", 3, 1)), (b"new-2", counter_text("new-2", 3, 1)), (good[0].encode(), counter_text(good[0], 4, 2))} <= set(owed)
    finally:
        pub.close()
        if tables_pub is not None:
            tables_pub.close()


def test_the_following_construction_takes_neither_keys_nor_tables(folding):
    d, eng = folding
    with pytest.raises(ValueError, match="neither keys nor tables"):
        BulkSnapshotPublisher(eng, ["a"], 4, decoder=d)
