"""What keeping the events' string fields costs a recovery from the events topic: the same restore with and without ``keep_strings``.

    python scripts/event_strings_bench.py [n_accounts=1000000] [pairs=5] > profiles/event_strings.json

The shape of ``bench.py --workload e2e --e2e-topic mixed`` at a size that runs in under a minute: n BankAccount accounts (UUID
keys, Double balances as play-json text), Zipf(1..4096) event counts (seed 3) cut to <= 8 — the first event of an account is its
``BankAccountCreated`` with ``accountOwner`` / ``securityCode``, the others ``BankAccountUpdated`` — published in rounds (a fetch
touches as many accounts as it has records) as LZ4 record batches on 8 partitions, fetches of 250,000 records (the records by
``tests/native/topic_gen.c``, framed by the product's ``RecordBatchWriter``; no record headers, no transactions).  Then
``GpuReplayStateStore.restore_from_fetches(host_keys=False)`` runs ``pairs`` times with ``keep_strings=True`` and ``pairs`` times
without, alternating in one process after a warm-up of both: framing, pushes, interning, fold and — with ``keep_strings`` — the
select / spans / gather passes of every push, the merges and the clone of the columns at the end.  The kept columns are checked
against the owners and codes the generator wrote.  The merge is timed alone too: an armed ``DeviceDecoder`` takes the whole topic
with the pending bound out of reach, then ``state_strings()`` — one merge per column over everything pending — is timed as wall
time of the synchronous call.  Recorded, not held to a bar; a cost is a cost only where it exceeds both spreads."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("", "examples", "tests"):
    sys.path.insert(0, os.path.join(ROOT, sub))

N_PART = 8
FETCH_RECORDS = 250_000
CAP = 8


def make_topic(n):
    """-> (fetches: per fetch one ``bytes`` or ``None`` per partition, records in all)"""
    import topic_gen
    from surge_amd import synth
    from surge_amd.snapshot import RecordBatchWriter

    ids = np.arange(n, dtype=np.int64)
    counts = np.minimum(synth.zipf_lengths(ids, 3), CAP).astype(np.int64)
    rng = np.random.default_rng(3)
    agg, seq = [], []
    for j in range(1, CAP + 1):  # round j: the j-th event of every account that has one, in a fixed pseudo-random order
        a = ids[counts >= j]
        agg.append(a[rng.permutation(a.shape[0])])
        seq.append(np.full(a.shape[0], j, dtype=np.int32))
    agg, seq = np.concatenate(agg), np.concatenate(seq)
    cents = 1 + (agg * 8192 + seq) % 999_999_998
    fetches = []
    with RecordBatchWriter(N_PART, compression="lz4") as w:
        for lo in range(0, agg.shape[0], FETCH_RECORDS):
            a, j = agg[lo:lo + FETCH_RECORDS], seq[lo:lo + FETCH_RECORDS]
            keys, ko, vals, vo = topic_gen.bank_records(a, j, cents[lo:lo + FETCH_RECORDS])
            fetches.append([None if b is None else bytes(b) for b in topic_gen.frame_partitions(w, (a % N_PART).astype(np.int32), keys, ko, vals, vo)])
    return fetches, int(agg.shape[0])


def recover(fetches, n, keep, look=None):
    """one recovery on the device route -> seconds (``look(store)`` runs before the store is closed, untimed)"""
    import torch

    from fixture_models import BankAccountBusinessLogic
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.restore_from_fetches(fetches, n_partitions=N_PART, framing_threads=4, capacity=n, host_keys=False, keep_strings=keep)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, (look(store) if look is not None else None)
    finally:
        store.close()


def columns_are_the_generators(store):
    """owner ``Owner <id % 1000>`` and code ``<id % 10000, four digits>`` for every account, under the decoder's key order"""
    keys = store._decoder.keys()
    ids = np.array([int(k[-12:], 16) for k in keys], dtype=np.int64)
    ok = True
    for col, want in ((store.state_strings[0], [b"Owner %d" % (i % 1000) for i in ids]), (store.state_strings[1], [b"%04d" % (i % 10000) for i in ids])):
        data, off = col[0].cpu().numpy().tobytes(), col[1].cpu().numpy()
        ok = ok and data == b"".join(want) and (np.diff(off) == [len(w) for w in want]).all()
    return bool(ok)


def merge_alone(fetches):
    """the whole topic through an armed decoder with the bound out of reach, then the merges of both columns, timed on their own"""
    import torch

    from fixture_models import BankAccountBusinessLogic
    from surge_amd.ingest import DeviceDecoder, PartitionedFramedFetches

    model = BankAccountBusinessLogic().command_model()
    os.environ["SURGE_INGEST_EVENT_STRINGS_PENDING"] = str(1 << 40)
    try:
        with DeviceDecoder(model.event_json_template(), event_strings=model.event_string_fields()) as d:
            with PartitionedFramedFetches(fetches, N_PART, threads=4, hold=4, overlap=True) as framed:
                for item in framed:
                    parts = [(sec, arena) for sec, arena in (item if isinstance(item, list) else [item]) if sec.shape[0]]
                    if parts:
                        d.push_async(parts)
                        d.finish()
            pend = d.event_strings_pending()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cols = d.state_strings()
            dt = time.perf_counter() - t0
            return {"pending_records": pend["records"], "pending_value_bytes": pend["bytes"], "aggregates": d.n_keys, "seconds_both_columns": dt,
                    "column_bytes": [int(c[0].numel()) for c in cols[:2]]}
    finally:
        del os.environ["SURGE_INGEST_EVENT_STRINGS_PENDING"]


def run(n, pairs):
    fetches, n_records = make_topic(n)
    out = {"accounts": n, "records": n_records, "partitions": N_PART, "fetches": len(fetches), "topic_bytes": sum(len(b) for f in fetches for b in f if b), "pairs": pairs}
    small = make_topic(20000)[0]
    for keep in (True, False):  # warm-up of both (code objects, pinned slabs' first touch, Python imports)
        recover(small, 20000, keep)
    out["kept_columns_equal_the_generators"] = recover(fetches, n, True, look=columns_are_the_generators)[1]
    runs = {"keep_strings": [], "plain": []}
    for _ in range(pairs):
        runs["keep_strings"].append(recover(fetches, n, True)[0])
        runs["plain"].append(recover(fetches, n, False)[0])
    for name, ts in runs.items():
        out[name] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts), "events_per_s": n_records / float(np.median(ts))}
    out["keep_over_plain_median"] = out["keep_strings"]["median_s"] / out["plain"]["median_s"]
    out["keep_minus_plain_median_s"] = out["keep_strings"]["median_s"] - out["plain"]["median_s"]
    out["cost_exceeds_both_spreads"] = bool(out["keep_minus_plain_median_s"] > max(out["keep_strings"]["spread_s"], out["plain"]["spread_s"]))
    out["merge_alone"] = merge_alone(fetches)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    print(json.dumps(run(int(args[0]) if args else 1_000_000, int(args[1]) if len(args) > 1 else 5)))
