"""What publishing the state topic from a device-route store costs, against the route callers had before.

    python scripts/device_publish_bench.py [n_aggregates=2000000] [pairs=5] [out=profiles/device_route_publish.json]

n Counter aggregates (UUID-like keys) are published as the state topic (LZ4 record batches on 4 partitions) and a store is
restored from those bytes with ``host_keys=False``: no id on the host.  Then, in ``pairs`` alternating pairs in one process
after a warm-up of both, a FIRST FULL publish of that store (LZ4, compressed on the device; the baseline the resume left is
invalidated first, outside the timing):

* ``follow``: ``store.snapshot_publisher(...)`` + ``publish()`` — the publisher follows the decoder's key table, the ids are
  partitioned from their UTF-8 bytes on the device (``partition_hash_utf8_kernel``); the store stays on the device route and is
  used again by the next pair;
* ``host_table``: ``BulkSnapshotPublisher(store.engine, store.keys.keys, ...)`` + ``publish()`` — every id downloaded, the host
  dictionary and mirror built, the UTF-8 and UTF-16 tables built from Python strings, K4; the store has left the device route, so
  every pair restores a fresh one (outside the timing).

Both must give the same bytes.  Beside that the shard map alone over the same ids, synchronised calls: the UTF-8 kernel over the
decoder's key table against K4 over a UTF-16 table built beforehand (building it is not timed).  Medians and spreads (max - min);
``follow_won_in_every_pair_by_more_than_both_spreads`` is the only claim the numbers make.  Nothing here is held to a bar."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from point_read_bench import N_PART, publish_topic, restored, series  # noqa: E402

ARM = {"compression": "lz4", "device_compression": True}


def everything_again(store):
    """The next publish reports every aggregate (a resume from the state topic makes what it loaded the baseline)."""
    import torch

    from surge_amd import _native

    eng = store.engine
    ones = torch.ones(eng.n_agg, dtype=torch.uint8, device=f"cuda:{eng.device}")
    torch.cuda.synchronize()
    eng._check(_native.load().surge_replay_snapshot_invalidate(eng._h, ctypes.c_void_p(ones.data_ptr())))
    eng.synchronize()


def follow(store):
    """-> (seconds, {partition: bytes}) of construct + first full publish on the device route"""
    import torch

    everything_again(store)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pub = store.snapshot_publisher(N_PART, **ARM)
    out = pub.publish(timestamp_ms=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {p: bytes(b) for p, b in out.items()}
    pub.close()
    assert store.device_route
    return dt, out


def host_table(store):
    """-> (seconds, {partition: bytes}) of the route callers had: the host key table, then the publisher over its strings"""
    import torch

    from surge_amd.snapshot import BulkSnapshotPublisher

    everything_again(store)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pub = BulkSnapshotPublisher(store.engine, store.keys.keys, N_PART, **ARM)
    out = pub.publish(timestamp_ms=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {p: bytes(b) for p, b in out.items()}
    pub.close()
    assert not store.device_route
    return dt, out


def won_every_pair(new, old):
    bar = max(new["spread_s"], old["spread_s"])
    return bool(all(o - n > bar for n, o in zip(new["seconds"], old["seconds"])))


def kernels_alone(store, pairs):
    """The shard map alone, both kernels over the same ids: the UTF-8 one over the decoder's key table, K4 over a UTF-16 table
    built beforehand.  Each call is timed until its result is complete (the UTF-8 form returns then; K4 is synchronised)."""
    import torch

    from surge_amd.kafka import utf16_table

    eng, d = store.engine, store._decoder
    d_keys, d_key_off = d.device_key_table()
    n = int(d_key_off.numel()) - 1
    u16, o16 = utf16_table(d.keys())  # (the same rows, in the decoder's order)
    d_u16, d_o16 = torch.from_numpy(u16.view(np.int16)).cuda(), torch.from_numpy(o16).cuda()
    out8, out16 = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    runs = {"utf8_kernel": [], "k4_utf16": []}
    for i in range(pairs + 1):  # (the first pair warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.partition_hash_utf8_device(d_keys, d_key_off, N_PART, out8, up_to_colon=True)
        t1 = time.perf_counter()
        eng.partition_hash_device(d_u16, d_o16, N_PART, out16, up_to_colon=True)
        eng.synchronize()
        t2 = time.perf_counter()
        if i:
            runs["utf8_kernel"].append(t1 - t0)
            runs["k4_utf16"].append(t2 - t1)
    row = {name: series(ts, n) for name, ts in runs.items()}
    row.update({"ids": n, "same_partitions": bool(torch.equal(out8, out16)), "utf8_bytes": int(d_keys.numel()), "utf16_bytes": int(u16.nbytes),
                "utf8_won_in_every_pair_by_more_than_both_spreads": won_every_pair(row["utf8_kernel"], row["k4_utf16"])})
    return row


def run(n, pairs):
    topic, _ = publish_topic(n)
    out = {"aggregates": n, "partitions": N_PART, "topic_bytes": sum(len(b) for b in topic.values()), "pairs": pairs, "compression": "lz4, on the device"}
    small = publish_topic(20000)[0]
    for fn in (follow, host_table):  # warm-up of both routes
        s, _ = restored(small, False)
        fn(s)
        s.close()
    dev, _ = restored(topic, False)
    runs, same = {"follow": [], "host_table": []}, True
    try:
        for _ in range(pairs):
            dt, got = follow(dev)
            runs["follow"].append(dt)
            old, _ = restored(topic, False)  # the old route drops the decoder: a fresh restore per pair, not timed
            try:
                dt, want = host_table(old)
            finally:
                old.close()
            runs["host_table"].append(dt)
            same = same and got == want
        out["publish"] = {name: series(ts, n) for name, ts in runs.items()}
        out["publish"].update({"same_bytes": bool(same), "record_batch_bytes": sum(len(b) for b in got.values()), "device_route_kept": dev.device_route,
                               "host_table_over_follow_median": out["publish"]["host_table"]["median_s"] / out["publish"]["follow"]["median_s"],
                               "follow_won_in_every_pair_by_more_than_both_spreads": won_every_pair(out["publish"]["follow"], out["publish"]["host_table"])})
        out["shard_map_alone"] = kernels_alone(dev, pairs)
    finally:
        dev.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = run(int(args[0]) if args else 2_000_000, int(args[1]) if len(args) > 1 else 5)
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "device_route_publish.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
