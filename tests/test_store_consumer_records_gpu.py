"""-m gpu: ``GpuReplayStateStore.restore_from_consumer_records`` and ``restore_from_state_consumer_records`` — a store recovered
from a consumer's polls of records instead of fetch bytes.  The pins: the same records through the wire methods
(``restore_from_fetches`` / ``restore_from_state_topic`` on ``kafka_wire`` bytes of them), and the oracle's fold of the events."""
import uuid

import numpy as np
import pytest

import kafka_wire as kw
import records_push_cases as C
import state_strings_gen as gen
from fixture_models import (BankAccountBusinessLogic, BankAccountCreated, BankAccountUpdated, CounterBusinessLogic, CountDecremented, CountIncremented,
                            MoneyDeposited, NoOpEvent, SdkEvent, SdkSampleBusinessLogic, sdk_sample_state_bytes, SdkBankAccount)
from oracle import oracle
from surge_amd.encode import JsonTemplate
from surge_amd.store import GpuReplayStateStore

pytestmark = pytest.mark.gpu

BANK = JsonTemplate.bank_account()
POLL_SIZES = (7, 500, 3000)


def polls_of(records, sizes, as_arrays=False):
    """``(offset, key, value)`` records cut into polls of ``sizes`` records, cycling; lists of ``bytes`` or arrays"""
    out, at, k = [], 0, 0
    while at < len(records):
        chunk = records[at:at + sizes[k % len(sizes)]]
        keys, values, offsets = [r[1] for r in chunk], [r[2] for r in chunk], [r[0] for r in chunk]
        out.append((C.arrays(keys), C.arrays([v or b"" for v in values]), np.asarray(offsets)) if as_arrays else (keys, values, offsets))
        at += len(chunk)
        k += 1
    return out


@pytest.fixture(scope="module")
def counter_topic():
    """6000 Counter events over 400 aggregates (transactions resolved: what a consumer hands over), the producer's flush record
    among them; the wire form of the same records; the oracle's fold of every aggregate's events."""
    rng = np.random.default_rng(11)
    bl = CounterBusinessLogic()
    model, fmt = bl.command_model(), bl.event_write_formatting()
    events = []
    for i in range(6000):
        agg = f"agg-{int(rng.integers(0, 400))}"
        events.append([CountIncremented(agg, int(rng.integers(0, 1000)), i + 1), CountDecremented(agg, int(rng.integers(0, 1000)), i + 1), NoOpEvent(agg, i + 1)][i % 3])
    msgs = [fmt.write_event(e) for e in events]
    records = [(i + i // 1000, m.key.encode(), m.value) for i, m in enumerate(msgs)]  # a gap of one offset every 1000 records (a commit marker's)
    assert (records[1999][0], records[2000][0]) == (2000, 2002)
    records.insert(2000, (2001, b"", b""))  # the flush record, in the gap
    wire = C.wire_of([r[1] for r in records], [r[2] for r in records], [r[0] for r in records], per_batch=140)
    per_agg = {}
    for e in events:
        per_agg.setdefault(e.aggregateId, []).append(e)
    want = {}
    for key, evs in per_agg.items():
        enc = model.encode_events(evs)
        want[key] = oracle.fold_csr(np.array([0, enc.shape[0]], np.int64), enc, None, model.event_algebra())[0].tobytes()
    return bl, records, wire, want, len(events)


@pytest.mark.parametrize("host_keys,bound_log,as_arrays", [(True, False, False), (False, False, True), (True, True, True), (False, True, False)])
def test_a_counter_store_from_polls_is_the_store_from_the_wire_bytes_and_the_oracles_fold(counter_topic, host_keys, bound_log, as_arrays):
    bl, records, wire, want, n_events = counter_topic
    polled, fetched = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        counters = polled.restore_from_consumer_records(iter(polls_of(records, POLL_SIZES, as_arrays)), host_keys=host_keys, bound_log=bound_log)
        wire_counters = fetched.restore_from_fetches([wire[:len(wire) // 2], wire[len(wire) // 2:]], host_keys=host_keys, bound_log=bound_log)
        assert set(counters) == set(wire_counters)  # the same dict shape
        for name in ("records_seen", "records_delivered", "flush_records_skipped", "doubles_parsed_on_host", "records_aborted", "control_batches", "open_transactions"):
            assert counters[name] == wire_counters[name], name
        assert counters["records_delivered"] == n_events and counters["flush_records_skipped"] == 1 and counters["records_decoded"] == n_events + 1
        assert counters["batches"] == len(polls_of(records, POLL_SIZES))
        assert polled.device_route == (not host_keys)
        ids = sorted(want)
        assert polled.get_aggregate_bytes_many(ids + ["no-such-id"]) == fetched.get_aggregate_bytes_many(ids + ["no-such-id"])
        for key in ids[::7]:
            assert polled.get_aggregate(key) == fetched.get_aggregate(key), key
        keys = polled.keys.keys  # (builds the host table on the device route)
        assert keys == fetched.keys.keys == list(dict.fromkeys(r[1].split(b":")[0].decode() for r in records if r[1]))
        states = polled.engine.snapshot()
        for a, key in enumerate(keys):
            assert states[a].tobytes() == want[key], key
    finally:
        polled.close()
        fetched.close()


def test_polls_of_sixteen_byte_events_and_a_topic_without_a_record():
    bl = CounterBusinessLogic()
    model = bl.command_model()
    events = [CountIncremented(f"a{i % 9}", i, i // 9 + 1) for i in range(300)]
    enc = model.encode_events(events)
    records = [(i, f"a{i % 9}:{i}".encode(), enc[i].tobytes()) for i in range(300)]
    store = GpuReplayStateStore(bl)
    try:
        counters = store.restore_from_consumer_records(polls_of(records, (64,)), depth=2)
        assert counters["records_delivered"] == 300
        states = store.engine.snapshot()
        for a, key in enumerate(store.keys.keys):
            mine = model.encode_events([e for e in events if e.aggregateId == key])
            assert states[a].tobytes() == oracle.fold_csr(np.array([0, mine.shape[0]], np.int64), mine, None, model.event_algebra())[0].tobytes()
        counters = store.restore_from_consumer_records([([], [], []), ([b""], [b""], [0])], capacity=3)  # nothing deliverable: an empty store
        assert counters["records_delivered"] == 0 and store.keys.keys == [] and store.get_aggregate("a0") is None
    finally:
        store.close()


def test_flush_records_that_lead_the_topic_are_counted_as_the_wire_route_counts_them():
    bl = CounterBusinessLogic()
    fmt = bl.event_write_formatting()
    msgs = [fmt.write_event(CountIncremented(f"agg-{i % 5}", 2, i // 5 + 1)) for i in range(60)]
    records = [(0, b"", b""), (1, b"", b"")] + [(2 + i, m.key.encode(), m.value) for i, m in enumerate(msgs)]
    wire = C.wire_of([r[1] for r in records], [r[2] for r in records], [r[0] for r in records])
    polled, fetched = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        counters = polled.restore_from_consumer_records(polls_of(records, (1, 1, 25)))  # the first two polls hold a flush record each, and nothing else
        want = fetched.restore_from_fetches([wire])
        for name in ("records_seen", "records_delivered", "flush_records_skipped", "records_decoded"):
            assert counters[name] == want[name], name
        assert counters["flush_records_skipped"] == 2 and counters["records_delivered"] == 60 and counters["records_decoded"] == 62
        assert polled.keys.keys == fetched.keys.keys and polled.engine.snapshot().tobytes() == fetched.engine.snapshot().tobytes()
    finally:
        polled.close()
        fetched.close()


def bank_tail(table):
    live = [k for k in table if table[k]]
    gone = [k for k in table if table[k] is None]
    fresh = [uuid.UUID(int=77000 + i) for i in range(40)]
    tail = [BankAccountCreated(a, f"tail \"{i}\" é", "" if i % 4 == 0 else f"t{i}", 10.0 + i) for i, a in enumerate(fresh)]
    tail += [BankAccountCreated(uuid.UUID(gone[0]), "created again", "again", 1.0), BankAccountUpdated(uuid.UUID(live[0]), 42.5),
             BankAccountCreated(uuid.UUID(live[1]), "replaced", "r", 2.0), BankAccountUpdated(fresh[3], 99.0)]
    return tail


@pytest.mark.parametrize("host_keys", [True, False])
def test_a_bank_account_state_topic_as_polls_with_an_events_tail_as_polls_and_the_strings_kept(host_keys):
    units, table = gen.make_topic(compression="none")
    state_records = [r for part in units for u in part for r in u[1]]  # partition after partition, offset order inside one
    state_fetches = [[gen.concat(part)[0] or None for part in units]]
    bl = BankAccountBusinessLogic()
    fmt = bl.event_write_formatting()
    msgs = [fmt.write_event(e) for e in bank_tail(table)]
    tail_records = [(900 + i, m.key.encode(), m.value) for i, m in enumerate(msgs)]
    tail_wire = kw.record_batch(900, [(k, v) for _, k, v in tail_records])
    polled, fetched = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        counts = polled.restore_from_state_consumer_records(polls_of(state_records, (7, 100, 333), as_arrays=not host_keys), template=BANK, host_keys=host_keys,
                                                            keep_strings=True, events_polls=iter(polls_of(tail_records, (16,))), keep_event_strings=True)
        want = fetched.restore_from_state_topic(state_fetches, n_partitions=len(units), template=BANK, events_fetches=[tail_wire], events_from=900,
                                                host_keys=host_keys, keep_event_strings=True)
        # (rows_written and tombstones count a load's winners, and six polls are six loads where one fetch is one: not comparable)
        for name in ("refused", "reparsed_on_host", "records_delivered", "tail_records_delivered", "tail_records_seen"):
            assert counts[name] == want[name], name
        assert counts["refused"] == 0 and counts["tail_records_delivered"] == len(msgs) and counts["records_delivered"] == len(state_records)
        assert polled.device_route == (not host_keys)
        ids = sorted(set(table) | {str(e.accountNumber) for e in bank_tail(table)})
        texts = fetched.get_aggregate_bytes_many(ids + ["no-such-account"], BANK)
        assert polled.get_aggregate_bytes_many(ids + ["no-such-account"], BANK) == texts and sum(t is not None for t in texts) > 100 and texts[-1] is None
        assert list(polled.all_bytes(BANK, page_rows=61)) == list(fetched.all_bytes(BANK))
        lo, hi = ids[len(ids) // 4], ids[3 * len(ids) // 4]
        assert list(polled.range_bytes(lo, hi, BANK)) == list(fetched.range_bytes(lo, hi, BANK))
        for k in ids[::5]:
            assert polled.get_aggregate(k) == fetched.get_aggregate(k), k
        mine, theirs = polled.state_strings, fetched.state_strings  # the kept columns themselves
        for a, b in zip(mine, theirs):
            assert (a is None) == (b is None)
            if a is not None:
                assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().tolist() == b[1].cpu().tolist()
    finally:
        polled.close()
        fetched.close()


def test_the_sdk_sample_with_enveloped_states_and_enveloped_events():
    from state_envelope_cases import SDK

    n = 300
    rng = np.random.default_rng(7)
    bl = SdkSampleBusinessLogic()
    fmt = bl.event_write_formatting()
    keys = [f"0c3f1d9e-7a55-4a5c-9d5e-{i:012x}" for i in range(n)]
    state_records = []
    for i, a in enumerate(rng.permutation(n)):
        balance = int(rng.integers(0, 2 ** 31))
        state_records.append((3 * i, keys[a].encode(), None if i % 17 == 3 else sdk_sample_state_bytes(keys[a], SdkBankAccount(balance))))
    tail = [SdkEvent(keys[int(a)] if i % 10 else f"new-{i}", MoneyDeposited(int(rng.integers(0, 1000)))) for i, a in enumerate(rng.integers(0, n, size=400))]
    msgs = [fmt.write_event(e) for e in tail]
    tail_records = [(i, m.key.encode(), m.value) for i, m in enumerate(msgs)]
    state_wire = C.wire_of([r[1] for r in state_records], [r[2] for r in state_records], [r[0] for r in state_records])
    tail_wire = C.wire_of([r[1] for r in tail_records], [r[2] for r in tail_records])
    polled, fetched = GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        counts = polled.restore_from_state_consumer_records(polls_of(state_records, (50, 7)), template=SDK, envelope="protobuf_state", host_keys=False,
                                                            events_polls=polls_of(tail_records, (90,), as_arrays=True))
        want = fetched.restore_from_state_topic([state_wire], template=SDK, envelope="protobuf_state", events_fetches=[tail_wire], events_from=0, host_keys=False)
        assert counts["refused"] == want["refused"] == 0 and counts["tombstones"] > 0 and counts["records_delivered"] == want["records_delivered"] == n
        assert counts["tail_records_delivered"] == want["tail_records_delivered"] == 400
        assert list(polled.all_bytes()) == list(fetched.all_bytes()) and polled.num_entries() == fetched.num_entries() > 250
        asked = keys[::3] + ["new-0", "new-10", "nobody"]
        assert polled.get_aggregate_bytes_many(asked) == fetched.get_aggregate_bytes_many(asked)
        assert [polled.get_aggregate(k) for k in asked] == [fetched.get_aggregate(k) for k in asked]
    finally:
        polled.close()
        fetched.close()


def test_a_model_without_a_template_is_refused_when_the_tail_brings_json_and_nothing_is_left_in_flight():
    class NoTemplate(type(CounterBusinessLogic().command_model())):
        def event_json_template(self):
            return None

    bl = CounterBusinessLogic()
    store = GpuReplayStateStore(bl)
    try:
        store.model = NoTemplate()
        state = [(0, b"k", oracle.counter_state_json("k", 1, 1))]
        tail = iter([([b"k:2"], [b'{"aggregateId":"k","incrementBy":1,"sequenceNumber":2}'], [0])])  # (an iterator: looked at when its turn comes)
        with pytest.raises(ValueError, match="event_json_template.*NoTemplate has none"):
            store.restore_from_state_consumer_records(polls_of(state, (1,)), events_polls=tail)
    finally:
        store.close()
