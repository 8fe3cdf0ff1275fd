"""-m gpu: a store that keeps the device decoder (``host_keys=False``) and answers ``get_aggregate_bytes`` /
``get_aggregate_bytes_many`` / ``get_aggregate`` from the device key table — a lookup, the encoders over the rows, one copy
back — and builds the host dictionary and the host mirror only when something asks for them.

The expectation is the pre-existing host route: the same topic restored with ``host_keys=True`` (the default) and read id by id
through the plugin's own formatter."""
import threading
import uuid

import numpy as np
import pytest

import kafka_wire as kw
import start_offsets_gen as sgen
import state_envelope_cases as envelope_cases
import state_strings_gen as gen
from fixture_models import (BankAccount, BankAccountBusinessLogic, BankAccountFormat, CountDecremented, CounterBusinessLogic, CounterCommandModel,
                            CountIncremented, NoOpEvent, State)
from surge_amd.encode import JsonTemplate
from surge_amd.schema import CLS_DELETE, CLS_MATERIALIZE, D_COUNT_ADD, D_COUNT_SUB, D_POISON, D_VERSION_SET, EventAlgebra
from surge_amd.store import AggregateInitializationException, GpuReplayKeyValueStore, GpuReplayStateStore

pytestmark = pytest.mark.gpu

BANK = JsonTemplate.bank_account()
T_NOOP, T_INC, T_DEC, T_THROW, T_DELETE = 0, 1, 2, 3, 4


class EndingCounterModel(CounterCommandModel):
    """The Counter fixture with one more event type: the aggregate ends (``CLS_DELETE``).  Its topic holds 16-byte events."""

    def event_algebra(self):
        return EventAlgebra(desc=(CLS_MATERIALIZE, CLS_MATERIALIZE | D_COUNT_ADD | D_VERSION_SET, CLS_MATERIALIZE | D_COUNT_SUB | D_VERSION_SET, D_POISON,
                                  CLS_DELETE), names=("no-op", "countIncremented", "countDecremented", "exception-throwing", "ended"))

    def event_json_template(self):
        return None


class EndingCounterLogic(CounterBusinessLogic):
    def __init__(self):
        super().__init__()
        self._model = EndingCounterModel()


def counter_topic(n_ids=700, seed=3):
    """-> (fetches, ids, fate): 16-byte Counter events under keys ``<id>:<seq>`` over ``n_ids`` ids in LZ4 and plain batches;
    ``fate[id]`` is ``"ended"`` (its last event is the DELETE), ``"threw"`` (it met the throwing event) or the ``State`` the
    literal fold of its events leaves."""
    rng = np.random.default_rng(seed)
    ids = ["agg-%d" % i for i in range(n_ids)] + ["a", "é-ключ", "x" * 200]
    fold = {}
    seq = {k: 0 for k in ids}
    recs = []
    for step in range(6 * len(ids)):
        k = ids[step] if step < len(ids) else ids[int(rng.integers(0, len(ids)))]  # every id once, in this order, then at random
        if fold.get(k) == "threw":
            continue
        seq[k] += 1
        u = rng.random()
        ty = T_INC if u < 0.5 else T_DEC if u < 0.8 else T_NOOP if u < 0.93 else T_DELETE if u < 0.98 else T_THROW
        by = int(rng.integers(1, 100))
        recs.append((f"{k}:{seq[k]}".encode("utf-8"), sgen.fixed16(ty, seq[k], by)))
        cur = fold.get(k)
        cur = None if cur == "ended" else cur
        if ty == T_THROW:
            fold[k] = "threw"
        elif ty == T_DELETE:
            fold[k] = "ended"
        else:
            base = cur if cur is not None else State(k, 0, 0)
            fold[k] = base if ty == T_NOOP else State(k, base.count + (by if ty == T_INC else -by), seq[k])
    blobs, at = [], 0
    while at < len(recs):
        n = int(rng.integers(1, 200))
        blobs.append(kw.record_batch(at, recs[at:at + n], compression="lz4" if len(blobs) % 3 else "none"))
        at += n
    cut = [0, len(blobs) // 3, 2 * len(blobs) // 3, len(blobs)]
    fetches = [b"".join(blobs[a:b]) for a, b in zip(cut, cut[1:])]
    assert {"ended", "threw"} <= set(v for v in fold.values() if isinstance(v, str)) and sum(isinstance(v, State) for v in fold.values()) > 0.7 * n_ids
    return fetches, ids, fold


ABSENT = ["agg-", "agg-700", "agg-1:1", "", "nobody", "x" * 199, "x" * 201]


def counting_snapshots(store):
    """Counts the host mirrors the store's engine publishes from here on."""
    calls, publish = [], store.engine.snapshot

    def snapshot():
        calls.append(1)
        return publish()

    store.engine.snapshot = snapshot
    return calls


def read(store, k):
    try:
        return store.get_aggregate_bytes(k)
    except AggregateInitializationException:
        return "raises"


@pytest.fixture(scope="module")
def counter():
    fetches, ids, fate = counter_topic()
    host, dev = GpuReplayStateStore(EndingCounterLogic()), GpuReplayStateStore(EndingCounterLogic())
    try:
        c_host = host.restore_from_fetches(fetches)
        mirrors = counting_snapshots(dev)
        c_dev = dev.restore_from_fetches(fetches, host_keys=False)
        assert c_host == c_dev
        yield host, dev, ids, fate, mirrors
    finally:
        host.close()
        dev.close()


def test_single_and_batched_reads_equal_the_host_route_and_nothing_was_built_on_the_host(counter):
    host, dev, ids, fate, mirrors = counter
    assert dev.device_route and not host.device_route
    asked = ids + ABSENT
    want = [read(host, k) for k in asked]
    # the host route against the test's own fold, so that both stores agreeing says something
    fmt = EndingCounterLogic().aggregate_write_formatting()
    for k, w in zip(ids, want):
        assert w == ("raises" if fate[k] == "threw" else None if fate[k] == "ended" else fmt.write_state(fate[k]).value), k
    assert want[len(ids):] == [None] * len(ABSENT)
    assert [read(dev, k) for k in asked] == want
    fine = [k for k, w in zip(asked, want) if w != "raises"]
    assert len(fine) > 600 and dev.get_aggregate_bytes_many(fine) == [w for w in want if w != "raises"]
    assert dev.get_aggregate_bytes_many(fine[::-1] + fine[:3]) == [w for w in want if w != "raises"][::-1] + [w for w in want if w != "raises"][:3]
    assert dev.get_aggregate_bytes_many([]) == []
    threw = next(k for k in ids if fate[k] == "threw")
    with pytest.raises(AggregateInitializationException, match=repr(threw)):
        dev.get_aggregate_bytes_many(fine[:5] + [threw] + fine[5:9])
    with pytest.raises(AggregateInitializationException):
        dev.get_aggregate(threw)
    for k in asked[:40] + asked[-12:]:
        if fate.get(k) != "threw":
            assert dev.get_aggregate(k) == host.get_aggregate(k) == (fate[k] if isinstance(fate.get(k), State) else None)
    # the device route has published no host mirror and holds no host key table
    assert dev.device_route and mirrors == [] and len(dev._keys) == 0
    with pytest.raises(ValueError, match="string column"):
        dev.get_aggregate_bytes_many(fine[:3], template=BANK)  # a template with string columns nothing restored
    # a host-keys store answers batches too: its rows from the dictionary, its key table uploaded once
    assert host.get_aggregate_bytes_many(fine) == [w for w in want if w != "raises"]
    table = host._uploaded_keys
    assert host.get_aggregate_bytes_many(fine[:7]) == [w for w in want if w != "raises"][:7] and host._uploaded_keys is table


def test_32_readers_of_one_device_route_store(counter):
    host, dev, ids, fate, _ = counter
    mine = [k for k in ids if fate[k] != "threw"][:32 * 6]
    want = {k: host.get_aggregate_bytes(k) for k in mine}
    got, errors = {}, []

    def reader(t):
        try:
            for k in mine[t::32]:
                got[k] = dev.get_aggregate_bytes(k)
            many = dev.get_aggregate_bytes_many(mine[t::32])
            assert many == [got[k] for k in mine[t::32]]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=reader, args=(t,)) for t in range(32)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got == want and dev.device_route


def test_apply_events_builds_the_host_table_and_the_two_stores_go_on_alike():
    fetches, ids, fate = counter_topic(n_ids=300, seed=8)
    host, dev = GpuReplayStateStore(EndingCounterLogic()), GpuReplayStateStore(EndingCounterLogic())
    try:
        host.restore_from_fetches(fetches)
        mirrors = counting_snapshots(dev)
        dev.restore_from_fetches(fetches, host_keys=False)
        assert dev.device_route and mirrors == []
        alive = [k for k in ids if isinstance(fate[k], State)][:20]
        ended = next(k for k in ids if fate[k] == "ended")
        new = [CountIncremented(alive[0], 5, 1000), CountDecremented(alive[1], 2, 1001), CountIncremented("born-later", 7, 1), NoOpEvent(ended, 1002),
               CountIncremented("born-later", 1, 2)]
        host.apply_events(new)
        dev.apply_events(new)
        assert not dev.device_route and len(mirrors) >= 1  # the host table and the mirror, as host_keys=True builds them
        assert dev.keys.keys == host.keys.keys and len(dev.keys) == len(ids) + 1
        assert dev.engine.snapshot().tobytes() == host.engine.snapshot().tobytes()
        for k in ids + ["born-later"] + ABSENT:
            assert read(dev, k) == read(host, k), k
        assert dev.get_aggregate("born-later") == State("born-later", 8, 2) and dev.get_aggregate(ended) == State(ended, 0, 0)
        fine = [k for k in ids + ["born-later"] if fate.get(k) != "threw"]
        assert dev.get_aggregate_bytes_many(fine) == [host.get_aggregate_bytes(k) for k in fine]
    finally:
        host.close()
        dev.close()


def test_the_key_value_store_and_the_next_restore_and_close():
    fetches, ids, fate = counter_topic(n_ids=300, seed=9)
    dev = GpuReplayStateStore(EndingCounterLogic())
    try:
        dev.restore_from_fetches(fetches, host_keys=False)
        kv = GpuReplayKeyValueStore("s", dev)
        alive = next(k for k in ids if isinstance(fate[k], State))
        assert kv.get(alive) == dev.get_aggregate_bytes(alive) and dev.device_route  # a get goes the device route
        first = dev._decoder
        dev.restore_from_fetches(fetches, host_keys=False)  # the next restore closes the decoder it replaces
        assert not first._h and dev.device_route and dev._decoder is not first
        order = sorted(ids)  # six neighbours in key order none of which threw (a range over a poisoned aggregate raises, as a get does)
        at = next(i for i in range(len(order) - 6) if all(fate[k] != "threw" for k in order[i:i + 6]) and any(isinstance(fate[k], State) for k in order[i:i + 6]))
        listed = dict(kv.range(order[at], order[at + 5]))  # a range needs the sorted host table: built now
        fmt = EndingCounterLogic().aggregate_write_formatting()
        assert not dev.device_route and listed == {k: fmt.write_state(fate[k]).value for k in order[at:at + 6] if isinstance(fate[k], State)}
        dev.restore_from_fetches(fetches, host_keys=False)
        last = dev._decoder
    finally:
        dev.close()
    assert not last._h and not dev.device_route


def test_a_bank_account_state_topic_is_served_with_owner_and_security_code():
    units, table = gen.make_topic(compression="lz4")
    fetches = [[gen.concat(gen.split(part, 3)[j])[0] or None for part in units] for j in range(3)]
    fmt = BankAccountFormat()
    text_of = lambda k, t: fmt.write_state(BankAccount(uuid.UUID(k), t[0], t[1], t[2])).value  # noqa: E731
    host, dev = GpuReplayStateStore(BankAccountBusinessLogic()), GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        host.restore_from_state_topic(fetches, n_partitions=len(units), template=BANK)
        mirrors = counting_snapshots(dev)
        counts = dev.restore_from_state_topic(fetches, n_partitions=len(units), template=BANK, host_keys=False)
        assert counts["refused"] == 0 and dev.device_route
        asked = list(table) + [str(uuid.UUID(int=99)), "", next(iter(table))[:-1]]
        want = [host.get_aggregate_bytes(k) for k in asked]
        assert want[:len(table)] == [text_of(k, t) if t else None for k, t in table.items()]  # tombstones and re-created ids as the writer left them
        assert any(t is None for t in table.values()) and any(t and t[0] and t[1] for t in table.values())
        assert dev.get_aggregate_bytes_many(asked, template=BANK) == want
        assert [dev.get_aggregate_bytes(k) for k in asked] == want  # (the single read writes the template the restore was given)
        live = next(k for k, t in table.items() if t and t[0] and t[1])
        assert dev.get_aggregate(live) == host.get_aggregate(live) == BankAccount(uuid.UUID(live), *table[live])
        assert dev.device_route and mirrors == [] and len(dev._keys) == 0
        assert sorted(dev.keys.keys) == sorted(host.keys.keys) and not dev.device_route and len(mirrors) == 1  # asked for: built
        assert [dev.get_aggregate_bytes(k) for k in asked] == want
    finally:
        host.close()
        dev.close()


@pytest.mark.parametrize("host_keys", [True, False])
def test_an_aggregate_born_after_the_resume_has_empty_restored_strings_in_a_batch(host_keys):
    """What ``get_aggregate_bytes_many`` documents: the restored string columns know nothing of an aggregate the events tail
    created — its STR parts are written empty, while the single read (the plugin's formatter over the model's own strings)
    writes them; an aggregate of the topic reads the same both ways."""
    from fixture_models import BankAccountCreated, BankAccountUpdated

    units, table = gen.make_topic(compression="none")
    fetches = [[gen.concat(part)[0] or None for part in units]]
    fmt = BankAccountFormat()
    text_of = lambda k, t: fmt.write_state(BankAccount(uuid.UUID(k), t[0], t[1], t[2])).value  # noqa: E731
    live = next(k for k, t in table.items() if t and t[0] and t[1])
    fresh = str(uuid.UUID(int=12345))
    assert fresh not in table
    tail = [BankAccountCreated(uuid.UUID(fresh), "Neu", "999", 5.0), BankAccountUpdated(uuid.UUID(live), 77.25)]
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        store.restore_from_state_topic(fetches, n_partitions=len(units), template=BANK, events_tail=tail, host_keys=host_keys)
        assert not store.device_route  # (decoded events need the host table)
        updated = text_of(live, (table[live][0], table[live][1], 77.25))
        assert store.get_aggregate_bytes(live) == updated and store.get_aggregate_bytes(fresh) == text_of(fresh, ("Neu", "999", 5.0))
        assert store.get_aggregate_bytes_many([fresh, live, "nobody"], template=BANK) == [text_of(fresh, ("", "", 5.0)), updated, None]
    finally:
        store.close()


def test_a_refused_restore_leaves_a_device_route_store_reading():
    fetches, ids, fate = counter_topic(n_ids=300, seed=9)
    alive = next(k for k in ids if isinstance(fate[k], State))
    dev = GpuReplayStateStore(EndingCounterLogic())
    try:
        dev.restore_from_fetches(fetches, host_keys=False)
        want = dev.get_aggregate_bytes(alive)
        assert want is not None
        for refused in (lambda: dev.restore_from_state_topic([b""], envelope="protobuf"),
                        lambda: dev.restore_from_state_topic([b""], events_tail=[NoOpEvent(alive, 1)], events_fetches=[b""]),
                        lambda: dev.restore_from_state_topic([b""], events_from=3)):
            with pytest.raises(ValueError):
                refused()
            assert dev.device_route and dev.get_aggregate_bytes(alive) == want
        # a restore from a state topic names what single reads write; a restore from fetches after it is back to the default
        dev.read_template, dev.read_envelope = BANK, "protobuf_state"
        dev.restore_from_fetches(fetches, host_keys=False)
        assert dev.read_template is None and dev.read_envelope == "none" and dev.get_aggregate_bytes(alive) == want
        dev.restore_from_fetches([b""], host_keys=False)  # a topic without a record: no decoder is left behind, nothing is served
        assert not dev.device_route and dev.get_aggregate_bytes(alive) is None
    finally:
        dev.close()


def test_the_sdk_sample_in_its_protobuf_envelope():
    from fixture_models import SDK_SAMPLE_MODEL, MoneyDeposited, SdkEvent, SdkSampleBusinessLogic, sdk_sample_state_bytes
    from surge_amd.snapshot import BulkSnapshotPublisher

    n = 300
    rng = np.random.default_rng(7)
    keys = [f"0c3f1d9e-7a55-4a5c-9d5e-{i:012x}" for i in range(n)]
    per_agg = [[MoneyDeposited(int(a)) for a in rng.integers(0, 2 ** 31, size=int(k))] for k in rng.integers(0, 12, size=n)]
    events = [SdkEvent(keys[a], d) for a in rng.permutation(n) for d in per_agg[a]]
    bl = SdkSampleBusinessLogic()
    writer, dev, pub = GpuReplayStateStore(bl), GpuReplayStateStore(bl), None
    try:
        writer.restore(events)
        pub = BulkSnapshotPublisher(writer.engine, writer.keys.keys, 2, template=envelope_cases.SDK, compression="lz4", device_compression=True, envelope="protobuf_state")
        topic = {p: bytes(b) for p, b in pub.publish().items()}
        dev.restore_from_state_topic([[topic.get(p) for p in range(2)]], n_partitions=2, template=envelope_cases.SDK, envelope="protobuf_state", host_keys=False)
        asked = keys + ["0c3f1d9e-7a55-4a5c-9d5e-ffffffffffff"]
        want = [writer.get_aggregate_bytes(k) for k in asked]  # the host route: the plugin's own formatter
        for a in range(0, n, 17):
            st = SDK_SAMPLE_MODEL.apply_events(None, per_agg[a])
            assert want[a] == (sdk_sample_state_bytes(keys[a], st) if st is not None else None)
        assert sum(w is None for w in want) >= 2 and sum(w is not None for w in want) > 250
        assert dev.get_aggregate_bytes_many(asked, template=envelope_cases.SDK, envelope="protobuf_state") == want
        assert [dev.get_aggregate_bytes(k) for k in asked[::9]] == want[::9] and dev.device_route
    finally:
        if pub is not None and hasattr(pub, "close"):
            pub.close()
        writer.close()
        dev.close()


def test_the_batched_read_defaults_to_the_counter_form_and_the_other_reads_to_the_restored_template():
    """The defaults differ on purpose: ``get_aggregate_bytes_many`` without a template writes ``JsonTemplate.counter()`` whatever
    the restore was given, ``get_aggregate_bytes`` and ``range_bytes`` write ``read_template`` — the restore's."""
    from surge_amd.encode import JP_I32

    short = JsonTemplate((b'{"id":', "KEY", b',"n":', (JP_I32, 0), b',"v":', (JP_I32, 4), b"}"))
    ids = ["k%d" % i for i in range(8)]
    state = {k: (3 * i - 7, i + 1) for i, k in enumerate(ids)}
    in_short = {k: b'{"id":"%s","n":%d,"v":%d}' % (k.encode(), n, v) for k, (n, v) in state.items()}
    in_counter = {k: b'{"aggregateId":"%s","count":%d,"version":%d}' % (k.encode(), n, v) for k, (n, v) in state.items()}
    wire = kw.record_batch(0, [(k.encode(), in_short[k]) for k in ids])
    store = GpuReplayStateStore(CounterBusinessLogic())
    try:
        counts = store.restore_from_state_topic([wire], template=short, host_keys=False)
        assert counts["rows_written"] == 8 and counts["refused"] == 0 and store.device_route
        assert store.read_template is short and store.read_envelope == "none"
        assert store.get_aggregate_bytes_many(ids) == [in_counter[k] for k in ids]
        assert store.get_aggregate_bytes_many(ids, template=short) == [in_short[k] for k in ids]
        assert [store.get_aggregate_bytes(k) for k in ids] == [in_short[k] for k in ids]
        assert list(store.range_bytes()) == [(k, in_short[k]) for k in sorted(ids)] and store.device_route
        assert len(store.keys) == 8 and not store.device_route  # with the host table the two defaults are the same two
        assert store.get_aggregate_bytes_many(ids) == [in_counter[k] for k in ids]
        assert list(store.range_bytes()) == [(k, in_short[k]) for k in sorted(ids)]
    finally:
        store.close()
