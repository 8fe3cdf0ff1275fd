"""-m gpu: ``GpuReplayStateStore`` recovered from snappy topics — a Counter events topic with transactions
(``restore_from_fetches``) and a BankAccount state topic with a snappy events tail (``restore_from_state_topic``) — gives the
rows, the reads and the kept strings of the same topics written as lz4, and the oracle's fold.  The snappy topics are the
uncompressed ones re-written batch by batch (tests/snappy_cases.py ``transcode``: what a broker or mirror configured for the
codec does), in kafka-clients' framing; nothing here needs a snappy library."""
import uuid

import numpy as np
import pytest

import kafka_wire as kw
import snappy_cases as sc
import state_strings_gen as gen
from fixture_models import (BankAccount, BankAccountBusinessLogic, BankAccountCreated, BankAccountUpdated, CounterBusinessLogic, CountDecremented,
                            CountIncremented)
from oracle import oracle
from surge_amd.encode import JsonTemplate
from surge_amd.kafka import partition_for_keys
from surge_amd.store import GpuReplayStateStore

pytestmark = pytest.mark.gpu

BANK = JsonTemplate.bank_account()
N_PART = 4


def written_as(fetches, codec):
    """The fetches' partitions (uncompressed bytes or None) re-written with ``codec``: 2 snappy (1 KiB chunks: several per batch,
    the last one short), 3 lz4."""
    writer = (lambda s: sc.compress_section(s, chunk=1024)) if codec == 2 else None
    return [[None if part is None else sc.transcode(part, codec, writer) for part in row] for row in fetches]


def routes(store):
    s = store._decoder.route_stats()
    return s["snappy_device_chunks"], s["snappy_host_sections"]


# ---- a Counter events topic with transactions ---------------------------------------------------------------------------------------
def counter_topic(n_events=3000, n_fetches=3, per_batch=70):
    """(fetches of uncompressed bytes, the events a read_committed consumer is delivered): 4 partitions; every third batch of a
    partition is a transaction of its own, closed by a COMMIT marker — the fifth by an ABORT: its events never happened."""
    bl = CounterBusinessLogic()
    fmt = bl.event_write_formatting()
    events = [(CountIncremented if i % 3 else CountDecremented)(f"agg-{i % 61}", i % 11, i // 61 + 1) for i in range(n_events)]
    msgs = [fmt.write_event(e) for e in events]
    parts = partition_for_keys([m.key for m in msgs], N_PART, up_to_colon=True)
    delivered = [True] * n_events
    fetches = [[b"" for _ in range(N_PART)] for _ in range(n_fetches)]
    for p in range(N_PART):
        mine = [i for i, q in enumerate(parts) if q == p]
        off = 0
        for b, s in enumerate(range(0, len(mine), per_batch)):
            idx = mine[s:s + per_batch]
            recs = [(msgs[i].key.encode(), msgs[i].value) for i in idx]
            tx = b % 3 == 2
            aborted = b == 5
            data = kw.record_batch(off, recs, **(dict(transactional=True, producer_id=100 + p, base_sequence=0) if tx else {}))
            off += len(recs)
            if tx:
                data += kw.control_batch(off, 100 + p, 0 if aborted else 1)
                off += 1
            if aborted:
                for i in idx:
                    delivered[i] = False
            fetches[min(n_fetches - 1, s * n_fetches // len(mine))][p] += data
    return [[part or None for part in row] for row in fetches], [e for e, d in zip(events, delivered) if d]


def test_a_counter_events_topic_with_transactions_written_as_snappy_restores_what_the_lz4_topic_and_the_oracle_give():
    fetches, events = counter_topic()
    bl = CounterBusinessLogic()
    model = bl.command_model()
    got = {}
    for name, codec in (("lz4", 3), ("snappy", 2)):
        store = GpuReplayStateStore(bl)
        try:
            counters = store.restore_from_fetches(written_as(fetches, codec), n_partitions=N_PART, framing_threads=2, host_keys=False)
            assert counters["records_delivered"] == len(events) and counters["records_aborted"] > 0, counters
            chunks, host = routes(store)
            assert (chunks > 4 * 9, host) == (codec == 2, 0), (name, chunks, host)
            keys = sorted({e.aggregateId for e in events})
            got[name] = {k: store.get_aggregate(k) for k in keys}
        finally:
            store.close()
    assert got["snappy"] == got["lz4"]
    for key, state in got["snappy"].items():
        enc = model.encode_events([e for e in events if e.aggregateId == key])
        want = oracle.fold_csr(np.array([0, enc.shape[0]], np.int64), enc, None, model.event_algebra())[0]
        assert state == model.state_from_fixed(key, want), key


# ---- a BankAccount state topic, and a snappy tail -------------------------------------------------------------------------------------
def bank_tail(table):
    live = [k for k in table if table[k]]
    gone = [k for k in table if table[k] is None]
    fresh = [uuid.UUID(int=88000 + i) for i in range(60)]
    tail = [BankAccountCreated(a, f"tail \"{i}\" é", "" if i % 4 == 0 else f"t{i}", 10.0 + i) for i, a in enumerate(fresh)]
    tail += [BankAccountCreated(uuid.UUID(gone[0]), "created again", "again", 1.0), BankAccountUpdated(uuid.UUID(live[0]), 42.5),
             BankAccountCreated(uuid.UUID(live[1]), "replaced", "r", 2.0), BankAccountUpdated(fresh[3], 99.0)]
    return tail, gone


def tail_fetches(events, n_fetches=2):
    fmt = BankAccountBusinessLogic().event_write_formatting()
    msgs = [fmt.write_event(e) for e in events]
    parts = partition_for_keys([m.key for m in msgs], N_PART, up_to_colon=True)
    logs = [[m for m, q in zip(msgs, parts) if q == p] for p in range(N_PART)]
    out = []
    for f in range(n_fetches):
        row = []
        for p in range(N_PART):
            n = len(logs[p])
            lo, hi = f * n // n_fetches, (f + 1) * n // n_fetches
            row.append(b"".join(kw.record_batch(lo + s, [(m.key.encode(), m.value) for m in logs[p][lo:hi][s:s + 20]]) for s in range(0, hi - lo, 20)) or None)
        out.append(row)
    return out


def fold_on_the_host(events, into):
    model = BankAccountBusinessLogic().command_model()
    for e in events:
        k = str(e.accountNumber)
        into[k] = model.handle_event(into.get(k), e)
    return into


def test_a_bank_account_state_topic_and_its_events_tail_written_as_snappy_resume_to_what_the_lz4_topics_give():
    units, table = gen.make_topic(compression="none")
    state = [[gen.concat(gen.split(part, 2)[j])[0] or None for part in units] for j in range(2)]
    tail, gone = bank_tail(table)
    want = {k: BankAccount(uuid.UUID(k), t[0], t[1], t[2]) for k, t in table.items() if t}
    want = {k: a for k, a in fold_on_the_host(tail, want).items() if a is not None}
    texts = {k: BankAccountBusinessLogic().aggregate_write_formatting().write_state(a).value for k, a in want.items()}
    got = {}
    for name, codec in (("lz4", 3), ("snappy", 2)):
        store = GpuReplayStateStore(BankAccountBusinessLogic())
        try:
            counts = store.restore_from_state_topic(written_as(state, codec), n_partitions=len(units), template=BANK, events_fetches=written_as(tail_fetches(tail), codec),
                                                    events_from=[0] * N_PART, events_partitions=N_PART, framing_threads=2, host_keys=False, keep_event_strings=True)
            assert counts["tail_records_delivered"] == len(tail) and counts["refused"] == 0, counts
            chunks, host = routes(store)
            assert (chunks > 20, host) == (codec == 2, 0), (name, chunks, host)
            keys = sorted(want)
            got[name] = (dict(store.all_bytes(BANK, page_rows=97)), store.get_aggregate_bytes_many(keys + ["no-such-account"], BANK),
                         list(store.range_bytes(keys[len(keys) // 4], keys[3 * len(keys) // 4], BANK)), {k: store.get_aggregate(k) for k in keys[:40]},
                         store.get_aggregate(gone[1]))
        finally:
            store.close()
    assert got["snappy"] == got["lz4"]
    rows, many, ranged, some, deleted = got["snappy"]
    keys = sorted(want)
    assert rows == texts and many == [texts[k] for k in keys] + [None] and deleted is None
    assert ranged == [(k, texts[k]) for k in keys if keys[len(keys) // 4] <= k <= keys[3 * len(keys) // 4]]
    assert some == {k: want[k] for k in keys[:40]}
