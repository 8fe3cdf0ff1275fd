"""``GpuReplayStateStore.restore_from_state_topic(lenient=True)`` / ``restore_from_state_records(lenient=True)``: a store resumes
from a state topic whose values another writer of the same documents wrote — the members in another order, whitespace between
the tokens, a member the case class does not know — and folds the events tail behind it.

The expectation is the pre-existing route: the same records as compact text restored in the strict mode.  Without ``lenient`` the
rewritten topic can only be refused (CORRUPT), as on the parent commit."""
import random
import uuid

import pytest

import state_lenient_cases as L
import state_strings_gen as gen
from fixture_models import BankAccountBusinessLogic, BankAccountCreated, BankAccountUpdated
from surge_amd.ingest import IngestError
from surge_amd.replay import ReplayError
from surge_amd.store import GpuReplayStateStore
from test_store_event_strings_gpu import N_PART, fetches_of

pytestmark = pytest.mark.gpu

BANK = L.BANK
UNKNOWN = (b"openedAt", b'{"branch":{"id":7,"tags":["a}","b]\\""]},"at":1.5e9,"by":null}')  # a field a later release added: a nested object


def topic_of(parts, rewrite, seed=11, per_batch=40, compression="lz4"):
    """``parts[p]``: ``(offset, key, value | None)`` in offset order -> one fetch: per partition the records in batches of
    ``per_batch`` at their own offsets (the gaps compaction left stay), every value through ``rewrite(value, rng)``."""
    rng = random.Random(seed)
    row = []
    for recs in parts:
        data = b""
        for s in range(0, len(recs), per_batch):
            chunk = recs[s:s + per_batch]
            base = chunk[0][0]
            data += gen.compacted_batch(base, [(o - base, k, None if v is None else rewrite(v, rng)) for o, k, v in chunk], compression)[0]
        row.append(data or None)
    return [row]


def columns_of(store):
    out = []
    for col in store.state_string_columns():
        if col is None:
            out.append(None)
            continue
        data, off = col[0].cpu().numpy().tobytes(), col[1].cpu().tolist()
        out.append([data[off[a]:off[a + 1]] for a in range(len(off) - 1)])
    return out


def everything_read(store, asked, template, envelope="none"):
    keys = sorted(k for k in asked if k)
    lo, hi = keys[len(keys) // 4], keys[3 * len(keys) // 4]
    return (store.get_aggregate_bytes_many(asked, template, envelope), list(store.range_bytes(lo, hi, template, envelope)),
            dict(store.all_bytes(template, envelope)))


@pytest.fixture(scope="module")
def bank_topic():
    units, table = gen.make_topic(seed=8, n_ids=120, n_records=600, compression="none")
    parts = [gen.concat(part)[1] for part in units]
    assert any(v is None for recs in parts for _, _, v in recs)
    assert any(b"\\" in v for recs in parts for _, _, v in recs if v)  # owners with escapes
    live = [k for k in table if table[k]]
    gone = [k for k in table if table[k] is None]
    fresh = [uuid.UUID(int=88000 + i) for i in range(12)]
    tail = [BankAccountCreated(a, f"tail \"{i}\" é", "" if i % 4 == 0 else f"t{i}", 10.0 + i) for i, a in enumerate(fresh)]
    tail += [BankAccountCreated(uuid.UUID(gone[0]), "created again", "again", 1.0), BankAccountUpdated(uuid.UUID(live[0]), 42.5),
             BankAccountCreated(uuid.UUID(live[1]), "replaced", "r", 2.0), BankAccountUpdated(fresh[3], 99.0)]
    compact = topic_of(parts, lambda v, rng: v)
    rewritten = topic_of(parts, lambda v, rng: L.rewritten(v, rng, unknown=UNKNOWN))
    asked = list(table) + [str(a) for a in fresh] + [str(uuid.UUID(int=99)), ""]
    return len(units), compact, rewritten, tail, asked


def restored(n_partitions, topic, tail, host_keys, lenient):
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        kw = {"lenient": True} if lenient else {}  # (the old way: the call as it has always been made)
        counts = store.restore_from_state_topic(topic, n_partitions=n_partitions, template=BANK, events_fetches=fetches_of(tail, n_fetches=2),
                                                events_from=[0] * N_PART, events_partitions=N_PART, framing_threads=2, host_keys=host_keys,
                                                keep_event_strings=True, **kw)
    except BaseException:
        store.close()
        raise
    return store, counts


@pytest.fixture(scope="module")
def bank_reference(bank_topic):
    """the compact topic restored the old way, once: (counts, reads, string columns, rows)"""
    n_partitions, compact, _, tail, asked = bank_topic
    store, counts = restored(n_partitions, compact, tail, True, False)
    try:
        return counts, everything_read(store, asked, BANK), columns_of(store), {k: store.get_aggregate(k) for k in asked if k}
    finally:
        store.close()


@pytest.mark.parametrize("host_keys", [True, False])
def test_a_rewritten_bank_account_topic_restores_to_what_the_compact_topic_restores(bank_topic, bank_reference, host_keys):
    n_partitions, _, rewritten, tail, asked = bank_topic
    want_counts, want_reads, want_columns, want_accounts = bank_reference
    store, counts = restored(n_partitions, rewritten, tail, host_keys, True)
    try:
        assert counts["refused"] == 0 and counts["rows_written"] == want_counts["rows_written"] > 50 and counts["tombstones"] == want_counts["tombstones"]
        assert counts["tail_records_delivered"] == len(tail)
        assert store.device_route == (not host_keys)
        assert not store.engine._reading_leniently  # the mode went back to strict
        assert everything_read(store, asked, BANK) == want_reads
        assert sum(b is not None for b in want_reads[0]) > 60 and len(want_reads[1]) > 20
        assert columns_of(store) == want_columns and want_columns[0] and any(b'"' in s for s in want_columns[0])
        for k in asked[::7]:
            if k:
                assert store.get_aggregate(k) == want_accounts[k], k
    finally:
        store.close()


@pytest.mark.parametrize("host_keys", [True, False])
def test_the_same_topic_without_the_option_is_refused_as_corrupt(bank_topic, host_keys):
    n_partitions, _, rewritten, tail, _ = bank_topic
    with pytest.raises((IngestError, ReplayError)) as ei:
        restored(n_partitions, rewritten, tail, host_keys, False)[0].close()
    assert ei.value.status == -7  # SURGE_E_CORRUPT


def test_rewritten_records_restore_through_restore_from_state_records(bank_topic):
    units, table = gen.make_topic(seed=8, n_ids=120, n_records=600, compression="none")
    records = sorted((r for part in units for r in gen.concat(part)[1]), key=lambda r: r[0])
    rng = random.Random(5)
    compact = [(k.decode(), v) for _, k, v in records]
    rewritten = [(k, None if v is None else L.rewritten(v, rng, unknown=UNKNOWN)) for k, v in compact]
    tail = [BankAccountUpdated(uuid.UUID(next(k for k in table if table[k])), 42.5)]
    a, b = GpuReplayStateStore(BankAccountBusinessLogic()), GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        want = a.restore_from_state_records(compact, events_tail=tail, template=BANK)
        assert b.restore_from_state_records(rewritten, events_tail=tail, template=BANK, lenient=True) == want and want["refused"] == 0
        asked = list(table)
        assert b.get_aggregate_bytes_many(asked, BANK) == a.get_aggregate_bytes_many(asked, BANK)
        assert columns_of(b) == columns_of(a)
        with pytest.raises(ReplayError) as ei:
            b.restore_from_state_records(rewritten, template=BANK)
        assert ei.value.status == -7
    finally:
        a.close()
        b.close()


# ---- the SDK sample: the same inside the protobuf envelope --------------------------------------------------------------------------
@pytest.mark.parametrize("host_keys", [True, False])
def test_a_rewritten_sdk_sample_topic_restores_inside_its_envelope(host_keys):
    from fixture_models import MoneyDeposited, SdkEvent, SdkSampleBusinessLogic

    n = 400
    rng = random.Random(7)
    keys = [f"0c3f1d9e-7a55-4a5c-9d5e-{i:012x}" for i in range(n)]
    parts = [[], []]
    for step in range(3 * n):
        i = step if step < n else rng.randrange(n)
        gone = step >= n and rng.random() < 0.15
        parts[i % 2].append((1000 + 2 * step, keys[i].encode(), None if gone else b'{"balance":%d}' % rng.randrange(0, 2 ** 31)))
    tail = [SdkEvent(keys[i], MoneyDeposited(rng.randrange(1, 1000))) for i in (3, 3, 50, n - 1)] + [SdkEvent("0c3f1d9e-7a55-4a5c-9d5e-ffffffffffff", MoneyDeposited(5))]
    wrap = lambda recs, rewrite: [[(o, k, None if v is None else L.wrap(k, rewrite(v))) for o, k, v in part] for part in recs]  # noqa: E731
    other = random.Random(8)
    compact = topic_of(wrap(parts, lambda v: v), lambda v, _: v)
    rewritten = topic_of(wrap(parts, lambda v: L.rewritten(v, other, unknown=(b"owner", b'{"name":"x","since":[2020,{"m":1}]}'))), lambda v, _: v)
    asked = keys + ["0c3f1d9e-7a55-4a5c-9d5e-ffffffffffff", "nobody"]
    bl = SdkSampleBusinessLogic()
    old, new, strict = GpuReplayStateStore(bl), GpuReplayStateStore(bl), GpuReplayStateStore(bl)
    try:
        want_counts = old.restore_from_state_topic(compact, n_partitions=2, template=L.SDK, envelope="protobuf_state", events_tail=tail)
        with pytest.raises((IngestError, ReplayError)) as ei:
            strict.restore_from_state_topic(rewritten, n_partitions=2, template=L.SDK, envelope="protobuf_state", events_tail=tail, host_keys=host_keys)
        assert ei.value.status == -7  # SURGE_E_CORRUPT
        counts = new.restore_from_state_topic(rewritten, n_partitions=2, template=L.SDK, envelope="protobuf_state", events_tail=tail, host_keys=host_keys, lenient=True)
        assert counts["refused"] == 0 and (counts["rows_written"], counts["tombstones"]) == (want_counts["rows_written"], want_counts["tombstones"])
        assert counts["tombstones"] > 5
        want = old.get_aggregate_bytes_many(asked, L.SDK, "protobuf_state")
        assert new.get_aggregate_bytes_many(asked, L.SDK, "protobuf_state") == want and sum(w is not None for w in want) > 300 and want[-1] is None
        lo, hi = keys[100], keys[300]
        assert list(new.range_bytes(lo, hi, L.SDK, "protobuf_state")) == list(old.range_bytes(lo, hi, L.SDK, "protobuf_state"))
        for k in asked[::13]:
            assert new.get_aggregate(k) == old.get_aggregate(k), k
    finally:
        old.close()
        new.close()
        strict.close()
