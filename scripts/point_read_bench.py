"""What serving reads from the device key table costs and saves, against the host dictionary and host mirror.

    python scripts/point_read_bench.py [n_aggregates=2000000] [pairs=5] [out=profiles/point_reads.json]

n Counter aggregates (UUID-like keys) are published as the state topic — LZ4 record batches on 4 partitions, framed by the device
framer (``BulkSnapshotPublisher``) — and a store is restored from those bytes once per route: ``host_keys=False`` (the decoder
stays, nothing is built on the host) and ``host_keys=True`` (every id downloaded and interned, the states mirrored).  Then, in
``pairs`` alternating pairs in one process after a warm-up of both:

* reads: ``get_aggregate_bytes_many`` of m ids on the device route against a loop of ``get_aggregate_bytes`` on the host-keys
  store, m = 1, 10^3, 10^6 (capped at n), one id in eight a miss; both must return the same bytes;
* the restore itself, ``host_keys=False`` against ``host_keys=True``, a fresh store each time.

Medians and spreads (max - min) as the other pair benches report them; ``device_won_by_more_than_both_spreads`` per pair of
series.  A single read (m = 1) pays a launch chain and two copies on the device route against a dictionary lookup and a
formatter call on the host, and IS slower there: 0.30 ms against 14 us in the run committed as ``profiles/point_reads.json``
(2 M aggregates), where 10^3 ids took 0.49 ms against 5.01 ms, 10^6 ids 0.44 s against 5.76 s and the restore 108 ms against
824 ms.  Nothing here is held to a bar."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

N_PART = 4


def publish_topic(n):
    """-> ({partition: bytes}, keys): n Counter states, every sixteenth aggregate None (never published)"""
    from surge_amd import schema as S
    from surge_amd.encode import JsonTemplate
    from surge_amd.replay import ReplayEngine
    from surge_amd.snapshot import BulkSnapshotPublisher

    rng = np.random.default_rng(1)
    keys = [f"{i:08x}-0000-4000-8000-{(i * 2654435761) % (1 << 48):012x}" for i in range(n)]
    prior = np.zeros(n, dtype=S.STATE_DTYPE)
    prior["count"] = rng.integers(-10**6, 10**6, size=n)
    prior["version"] = rng.integers(1, 10**4, size=n)
    prior["flags"] = np.where(np.arange(n) % 16 == 5, 0, S.STATE_PRESENT)
    with ReplayEngine() as eng:
        eng.load_csr(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE), prior)
        eng.fold()
        pub = BulkSnapshotPublisher(eng, keys, N_PART, template=JsonTemplate.counter(), compression="lz4", device_compression=True)
        try:
            out = {p: bytes(b) for p, b in pub.publish().items()}
        finally:
            pub.close()
    return out, keys


def restored(topic, host_keys):
    """-> (store, seconds of the restore)"""
    import torch

    from fixture_models import CounterBusinessLogic
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(CounterBusinessLogic())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store.restore_from_state_topic([[topic.get(p) for p in range(N_PART)]], n_partitions=N_PART, host_keys=host_keys)
    torch.cuda.synchronize()
    return store, time.perf_counter() - t0


def series(ts, n=None):
    out = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts)}
    if n:
        out["per_second"] = n / out["median_s"]
    return out


def won(device, host):
    return bool(host["median_s"] - device["median_s"] > max(device["spread_s"], host["spread_s"]))


def run(n, pairs):
    topic, keys = publish_topic(n)
    out = {"aggregates": n, "partitions": N_PART, "topic_bytes": sum(len(b) for b in topic.values()), "pairs": pairs}
    small = publish_topic(20000)[0]
    for host_keys in (False, True):  # warm-up of both routes (code objects, pinned slabs' first touch, Python imports)
        s, _ = restored(small, host_keys)
        s.get_aggregate_bytes_many(["nobody"])
        s.close()
    dev, _ = restored(topic, False)
    host, _ = restored(topic, True)
    try:
        rng = np.random.default_rng(2)
        out["reads"] = []
        for m in (1, 1000, 1000000):
            m = min(m, n)
            ids = [keys[i] if q % 8 != 7 else "absent-%d" % i for q, i in enumerate(rng.integers(0, n, size=m).tolist())]
            if m == 1:
                ids = [keys[n // 2]]
            same = dev.get_aggregate_bytes_many(ids) == [host.get_aggregate_bytes(k) for k in ids]  # (and the warm-up at this size)
            runs = {"device_many": [], "host_loop": []}
            for _ in range(pairs):
                t0 = time.perf_counter()
                dev.get_aggregate_bytes_many(ids)
                runs["device_many"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for k in ids:
                    host.get_aggregate_bytes(k)
                runs["host_loop"].append(time.perf_counter() - t0)
            row = {"ids": m, "same_bytes": bool(same), "device_route_kept": dev.device_route}
            row.update({name: series(ts, m) for name, ts in runs.items()})
            row["host_over_device_median"] = row["host_loop"]["median_s"] / row["device_many"]["median_s"]
            row["device_won_by_more_than_both_spreads"] = won(row["device_many"], row["host_loop"])
            out["reads"].append(row)
    finally:
        dev.close()
        host.close()
    runs = {"host_keys_false": [], "host_keys_true": []}
    for _ in range(pairs):
        for name, host_keys in (("host_keys_false", False), ("host_keys_true", True)):
            s, dt = restored(topic, host_keys)
            s.close()
            runs[name].append(dt)
    out["restore"] = {name: series(ts, n) for name, ts in runs.items()}
    out["restore"]["true_over_false_median"] = out["restore"]["host_keys_true"]["median_s"] / out["restore"]["host_keys_false"]["median_s"]
    out["restore"]["device_won_by_more_than_both_spreads"] = won(out["restore"]["host_keys_false"], out["restore"]["host_keys_true"])
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = run(int(args[0]) if args else 2_000_000, int(args[1]) if len(args) > 1 else 5)
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "point_reads.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
