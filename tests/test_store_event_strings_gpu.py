"""``GpuReplayStateStore.restore_from_fetches(keep_strings=True)``: a BankAccount store recovered from its EVENTS topic keeps
``accountOwner`` and ``securityCode`` on the device, serves them on both read routes, publishes them as a state topic a second
store resumes from, and a resume's events tail read as bytes (``keep_event_strings=True``) goes into the restored columns.

The expectation is the host-folded model: the fixture's ``handle_event`` over the same events, written by its
``aggregate_write_formatting``.  On the parent commit the owner and the code came back ``""`` or the reads raised ``ValueError``."""
import uuid

import pytest

import kafka_wire as kw
import state_strings_gen as gen
from fixture_models import BankAccountBusinessLogic, BankAccountCreated, BankAccountUpdated, CounterBusinessLogic, CountIncremented
from surge_amd.encode import JsonTemplate
from surge_amd.kafka import partition_for_keys
from surge_amd.snapshot import BulkSnapshotPublisher
from surge_amd.store import GpuReplayStateStore

pytestmark = pytest.mark.gpu

BANK = JsonTemplate.bank_account()
N_PART = 4


def bank_events(n_accounts=300, seed=3):
    """a few hundred accounts: created (some twice, under another owner), updated; escaped and non-ASCII owners, empty codes"""
    import numpy as np

    rng = np.random.default_rng(seed)
    ids = [uuid.UUID(int=int(rng.integers(1, 2 ** 62)) * 7919 + i) for i in range(n_accounts)]
    events = []
    for i, a in enumerate(ids):
        events.append(BankAccountCreated(a, gen.OWNERS[i % len(gen.OWNERS)] + (f" {i}" if i % 3 else ""), "" if i % 5 == 0 else f"{i:04d}", float(i) + 0.25))
    for j in range(3 * n_accounts):
        i = int(rng.integers(0, n_accounts))
        if j % 11 == 0:
            events.append(BankAccountCreated(ids[i], f"second owner {j} \"é€😀\"", f"s{j}", -1.5 * j))
        else:
            events.append(BankAccountUpdated(ids[i], float(int(rng.integers(-10 ** 6, 10 ** 6))) / 100.0))
    return ids, events


def fold_on_the_host(events, into=None):
    model = BankAccountBusinessLogic().command_model()
    state = {} if into is None else into
    for e in events:
        k = str(e.accountNumber)
        state[k] = model.handle_event(state.get(k), e)
    return state


def fetches_of(events, n_fetches=3, first_offsets=None, compression="lz4"):
    """the events as their topic's consumer receives them: N_PART partitions, ``n_fetches`` fetch responses, 50-record batches"""
    fmt = BankAccountBusinessLogic().event_write_formatting()
    msgs = [fmt.write_event(e) for e in events]
    parts = partition_for_keys([m.key for m in msgs], N_PART, up_to_colon=True)
    logs = [[m for m, q in zip(msgs, parts) if q == p] for p in range(N_PART)]
    base = first_offsets or [0] * N_PART
    out = []
    for f in range(n_fetches):
        row = []
        for p in range(N_PART):
            n = len(logs[p])
            lo, hi = f * n // n_fetches, (f + 1) * n // n_fetches
            chunk = logs[p][lo:hi]
            row.append(b"".join(kw.record_batch(base[p] + lo + s, [(m.key.encode(), m.value) for m in chunk[s:s + 50]], compression=compression)
                                for s in range(0, len(chunk), 50)) or None)
        out.append(row)
    return out


def text_of(account) -> bytes:
    return BankAccountBusinessLogic().aggregate_write_formatting().write_state(account).value


@pytest.fixture(scope="module")
def case():
    ids, events = bank_events()
    want = fold_on_the_host(events)
    assert any('"' in a.accountOwner for a in want.values()) and any(ord(ch) > 0xFFFF for a in want.values() for ch in a.accountOwner)
    assert any(a.securityCode == "" for a in want.values()) and any(a.accountOwner.startswith("second owner") for a in want.values())
    return ids, events, want


def check_reads(store, want):
    for k, account in want.items():
        assert store.get_aggregate(k) == account, k
    keys = sorted(want)
    texts = {k: text_of(a) for k, a in want.items()}
    assert store.get_aggregate_bytes_many(keys + ["no-such-account"], BANK) == [texts[k] for k in keys] + [None]
    assert list(store.all_bytes(BANK, page_rows=97)) == [(k, texts[k]) for k in keys]
    lo, hi = keys[len(keys) // 4], keys[3 * len(keys) // 4]
    assert list(store.range_bytes(lo, hi, BANK)) == [(k, texts[k]) for k in keys if lo <= k <= hi]


@pytest.mark.parametrize("host_keys", [True, False])
def test_a_store_recovered_from_the_events_topic_keeps_and_serves_the_string_fields(case, host_keys):
    _, events, want = case
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        counters = store.restore_from_fetches(fetches_of(events), n_partitions=N_PART, framing_threads=2, host_keys=host_keys, keep_strings=True)
        assert counters["records_delivered"] == len(events)
        assert store.state_strings[0] is not None and store.state_strings[1] is not None and store.state_strings[2] is None
        check_reads(store, want)
    finally:
        store.close()


def test_without_keep_strings_the_recovery_is_what_it_was(case):
    _, events, want = case
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        store.restore_from_fetches(fetches_of(events), n_partitions=N_PART, framing_threads=2)
        assert not store.state_strings
        k, account = next(iter(want.items()))
        got = store.get_aggregate(k)
        assert (got.accountOwner, got.securityCode, got.balance) == ("", "", account.balance)
        with pytest.raises(ValueError, match="nothing restored it"):
            store.get_aggregate_bytes_many([k], BANK)
    finally:
        store.close()


def test_the_cycle_events_topic_to_state_topic_to_store_closes_with_equal_bytes(case):
    _, events, want = case
    texts = {k: text_of(a) for k, a in want.items()}
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        store.restore_from_fetches(fetches_of(events, compression="none"), n_partitions=N_PART, framing_threads=2, keep_strings=True)
        pub = BulkSnapshotPublisher(store.engine, store.keys.keys, N_PART, template=BANK, compression="lz4", device_compression=True, strings=store.state_string_columns())
        try:
            topic = {p: bytes(b) for p, b in pub.publish().items()}
        finally:
            pub.close()
    finally:
        store.close()
    second = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        counts = second.restore_from_state_topic([[topic.get(p) for p in range(N_PART)]], n_partitions=N_PART, template=BANK, host_keys=False)
        assert counts["refused"] == 0 and counts["rows_written"] == len(want)
        assert dict(second.all_bytes(BANK)) == texts
        for k in list(want)[:20]:
            assert second.get_aggregate(k) == want[k]
    finally:
        second.close()


@pytest.mark.parametrize("host_keys", [True, False])
def test_accounts_first_created_in_a_resumes_tail_have_the_tails_strings_on_both_read_paths(host_keys):
    units, table = gen.make_topic(compression="lz4")
    state_fetches = [[gen.concat(gen.split(part, 2)[j])[0] or None for part in units] for j in range(2)]
    live = [k for k in table if table[k]]
    gone = [k for k in table if table[k] is None]
    fresh = [uuid.UUID(int=77000 + i) for i in range(40)]
    tail = [BankAccountCreated(a, f"tail \"{i}\" é", "" if i % 4 == 0 else f"t{i}", 10.0 + i) for i, a in enumerate(fresh)]
    tail += [BankAccountCreated(uuid.UUID(gone[0]), "created again", "again", 1.0), BankAccountUpdated(uuid.UUID(live[0]), 42.5),
             BankAccountCreated(uuid.UUID(live[1]), "replaced", "r", 2.0), BankAccountUpdated(fresh[3], 99.0)]
    from fixture_models import BankAccount

    want = {k: BankAccount(uuid.UUID(k), t[0], t[1], t[2]) for k, t in table.items() if t}
    want = {k: a for k, a in fold_on_the_host(tail, into=want).items() if a is not None}
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        counts = store.restore_from_state_topic(state_fetches, n_partitions=len(units), template=BANK, events_fetches=fetches_of(tail, n_fetches=2),
                                                events_from=[0] * N_PART, events_partitions=N_PART, framing_threads=2, host_keys=host_keys, keep_event_strings=True)
        assert counts["tail_records_delivered"] == len(tail)
        check_reads(store, want)
        assert store.get_aggregate(gone[1]) is None
    finally:
        store.close()


def test_keep_strings_on_a_model_without_the_hook_is_refused_before_anything_changes():
    bl = CounterBusinessLogic()
    fmt = bl.event_write_formatting()
    msgs = [fmt.write_event(CountIncremented(f"agg-{i % 5}", 2, i // 5 + 1)) for i in range(25)]
    wire = kw.record_batch(0, [(m.key.encode(), m.value) for m in msgs], compression="lz4")
    store = GpuReplayStateStore(bl)
    try:
        store.restore_from_fetches([wire])
        before = {f"agg-{i}": store.get_aggregate(f"agg-{i}") for i in range(5)}
        assert all(v is not None for v in before.values())
        with pytest.raises(ValueError, match="event_string_fields"):
            store.restore_from_fetches([wire], keep_strings=True)
        with pytest.raises(ValueError, match="event_string_fields|keep_event_strings"):
            store.restore_from_state_topic([b""], events_fetches=[wire], keep_event_strings=True)
        assert {k: store.get_aggregate(k) for k in before} == before
    finally:
        store.close()
