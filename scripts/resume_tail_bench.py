"""Resuming a store from snapshot BYTES and then TAIL bytes: the tail decoded on the device against the tail decoded on the host,
in one process.

    python scripts/resume_tail_bench.py [n_aggregates=200000] [tail_events=200000] [pairs=5] > profiles/resume_tail.json

n Counter aggregates are folded and published as the state topic (LZ4, 4 partitions, the device framer); the events behind
that snapshot are written as an events topic of 4 partitions whose first batches straddle the positions committed with the
snapshot (ten records of each lie below).  Two routes from those bytes to the same resident states alternate, ``pairs`` times
each after a warm-up of both:

* ``host_tail`` (what there was): ``restore_from_state_topic(..., events_tail=...)`` — the state topic on the device, the tail
  decoded on the host (``EventsTopicIngest(start_offset=...)``, the plugin's event reader per record) and folded by
  ``apply_events``;
* ``device_tail``: ``restore_from_state_topic(..., events_fetches=..., events_from=...)`` — the state decoder continues as the
  events decoder, the framers start at the positions, records below them are dropped where records are parsed.

Both end in the same 64-byte rows per key (checked).  One JSON line: the seconds of every repeat, medians, spreads, and the
ratio of the medians.  Recorded, not held to a bar."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_PART = 4
BELOW = 10  # records of each partition's first batch that lie below its start


def publish_states(n):
    from surge_amd import schema as S
    from surge_amd.replay import ReplayEngine
    from surge_amd.snapshot import BulkSnapshotPublisher

    rng = np.random.default_rng(1)
    keys = [f"agg-{i:08d}" for i in range(n)]
    ev = S.make_events(np.full(n, S.EVT_INC), rng.integers(1, 10**5, size=n), rng.integers(-10**6, 10**6, size=n))
    with ReplayEngine() as eng:
        eng.load_csr(np.arange(n + 1, dtype=np.int64), ev)
        eng.fold()
        pub = BulkSnapshotPublisher(eng, keys, N_PART, compression="lz4", device_compression=True)
        try:
            return keys, {p: bytes(b) for p, b in pub.publish().items()}
        finally:
            pub.close()


def events_topic(keys, m, batch=500):
    """-> (per partition the topic's bytes from the batch that contains its start on, the starts)"""
    import kafka_wire as kw
    from fixture_models import CounterBusinessLogic, CountIncremented
    from surge_amd import _native
    from surge_amd.kafka import partition_for_keys

    lib = _native.load()
    kw.crc32c = lambda data: int(lib.surge_crc32c(data, len(data))) & 0xFFFFFFFF  # (the writer's own table walk takes a second per megabyte)
    rng = np.random.default_rng(2)
    fmt = CounterBusinessLogic().event_write_formatting()
    ids = keys + [f"new-{i:08d}" for i in range(len(keys) // 10)]  # one event in eleven names an aggregate the snapshot has not seen
    history = [CountIncremented(ids[int(a)], int(b), int(s)) for a, b, s in zip(rng.integers(0, len(ids), size=m), rng.integers(-50, 50, size=m), rng.integers(1, 10**6, size=m))]
    msgs = [fmt.write_event(e) for e in history]
    parts = partition_for_keys([x.key for x in msgs], N_PART, up_to_colon=True)
    wires, starts = [], []
    for p in range(N_PART):
        base = 1000 * (p + 1)  # the partition's first batch: ten records the snapshot already holds, then the tail
        mine = [(x.key.encode(), x.value) for x, q in zip(msgs, parts) if q == p]
        mine = mine[:BELOW] + mine
        wires.append(b"".join(kw.record_batch(base + s, mine[s:s + batch]) for s in range(0, len(mine), batch)))
        starts.append(base + BELOW)
    return wires, starts


def host_tail_route(bl, states, wires, starts):
    from surge_amd.core import SerializedMessage
    from surge_amd.ingest import EventsTopicIngest
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(bl)
    reader = bl.event_write_formatting()
    t0 = time.perf_counter()
    tail = []
    for wire, start in zip(wires, starts):
        with EventsTopicIngest(start_offset=start) as g:
            g.feed(wire)
            tail.extend(reader.read_event(SerializedMessage(k.decode("utf-8"), v)) for _, _, k, v in g.drain_records())
    counts = store.restore_from_state_topic([[states.get(p) for p in range(N_PART)]], n_partitions=N_PART, events_tail=tail)
    return time.perf_counter() - t0, store, counts


def device_tail_route(bl, states, wires, starts):
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(bl)
    t0 = time.perf_counter()
    counts = store.restore_from_state_topic([[states.get(p) for p in range(N_PART)]], n_partitions=N_PART, events_fetches=[list(wires)], events_from=starts,
                                            events_partitions=N_PART)
    return time.perf_counter() - t0, store, counts


def rows_by_key(store):
    snap = store.engine.snapshot()
    order = np.argsort(np.array(store.keys.keys))
    return np.array(store.keys.keys)[order], snap[order]


def run(n, m, pairs):
    from fixture_models import CounterBusinessLogic

    bl = CounterBusinessLogic()
    keys, states = publish_states(n)
    wires, starts = events_topic(keys, m)
    out = {"aggregates": n, "tail_events": m, "partitions": N_PART, "state_topic_bytes": sum(len(b) for b in states.values()), "tail_bytes": sum(len(w) for w in wires),
           "records_below_the_starts": BELOW * N_PART, "pairs": pairs}
    small_keys, small_states = publish_states(5000)
    small = events_topic(small_keys, 5000)
    for route in (host_tail_route, device_tail_route):  # warm-up of both (code objects, pinned slabs' first touch, Python imports)
        route(bl, small_states, small[0], small[1])[1].close()
    runs = {"host_tail": [], "device_tail": []}
    for i in range(pairs):
        th, sh, _ = host_tail_route(bl, states, wires, starts)
        td, sd, counts = device_tail_route(bl, states, wires, starts)
        if i == 0:
            kh, rh = rows_by_key(sh)
            kd, rd = rows_by_key(sd)
            out["rows_equal_between_the_routes"] = bool(len(kh) == len(kd) and (kh == kd).all() and rh.tobytes() == rd.tobytes())
            out["device_tail_counts"] = {k: v for k, v in counts.items() if k.startswith("tail_")}
        sh.close()
        sd.close()
        runs["host_tail"].append(th)
        runs["device_tail"].append(td)
    for route, ts in runs.items():
        out[route] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts)}
    spread = max(out["host_tail"]["spread_s"], out["device_tail"]["spread_s"])
    out["device_tail_wins_every_pair_by_more_than_both_spreads"] = all(h - d > spread for h, d in zip(runs["host_tail"], runs["device_tail"]))
    out["host_tail_over_device_tail_median"] = out["host_tail"]["median_s"] / out["device_tail"]["median_s"]
    return out


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    print(json.dumps(run(args[0] if args else 200_000, args[1] if len(args) > 1 else 200_000, args[2] if len(args) > 2 else 5)))
