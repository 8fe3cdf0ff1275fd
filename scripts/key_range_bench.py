"""What ordered reads — range, all, substates — cost from the device key order, against the host table built on demand.

    python scripts/key_range_bench.py [n_aggregates=2000000] [pairs=5] [out=profiles/key_range_reads.json]

n Counter aggregates (UUID-like keys) are published as the state topic (``point_read_bench.publish_topic``) and restored with
``host_keys=False``.  The device route reads through ``GpuReplayStateStore.range_bytes`` / ``all_bytes`` /
``substates_for_aggregate`` (the decoder's key order, the row encoders, the ids gathered on the device); the host route is what
such a store did before: ``GpuReplayKeyValueStore.range`` / ``all``, which download every id, build the host table and the
mirror on first use, sort the ids on every call and format one key at a time.  In ``pairs`` alternating pairs, after a warm-up
of both routes on a small topic:

* first: a range of about 10^3 keys on a store nothing has read yet — the device route's includes the build of the key order,
  the host route's the host table (a fresh restore per measurement, not timed);
* warm: the same stores again — a range of 10 and of about 10^3 keys, and the substates of one id;
* all: ``all_bytes()`` / ``all()`` consumed to the end.

``order_build`` times ``DeviceDecoder.key_order()`` alone on fresh restores and records its passes.  Medians and spreads
(max - min); ``device_won_every_pair_by_more_than_both_spreads`` is the bar the README's word "faster" is held to.  Nothing
here is held to a bar of its own."""
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


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return got, time.perf_counter() - t0


def compared(runs, n=None):
    """The two series of one measurement with the verdicts on them."""
    dev, host = runs["device"], runs["host"]
    row = {"device": series(dev, n), "host": series(host, n)}
    row["host_over_device_median"] = row["host"]["median_s"] / row["device"]["median_s"]
    margin = max(row["device"]["spread_s"], row["host"]["spread_s"])
    row["device_won_every_pair_by_more_than_both_spreads"] = bool(all(h - d > margin for d, h in zip(dev, host)))
    row["host_won_every_pair_by_more_than_both_spreads"] = bool(all(d - h > margin for d, h in zip(dev, host)))
    return row


def run(n, pairs):
    from surge_amd.store import GpuReplayKeyValueStore

    topic, keys = publish_topic(n)
    order = sorted(keys)
    out = {"aggregates": n, "partitions": N_PART, "topic_bytes": sum(len(b) for b in topic.values()), "pairs": pairs}
    small, small_keys = publish_topic(20000)
    for device in (True, False):  # warm-up of both routes (code objects, rocPRIM's kernels, Python imports)
        s, _ = restored(small, False)
        a, b = sorted(small_keys)[100], sorted(small_keys)[1100]
        list(s.range_bytes(a, b)) if device else list(GpuReplayKeyValueStore("w", s).range(a, b))
        s.close()
    at = n // 3
    wide = (order[at], order[min(at + 999, n - 1)])
    narrow = (order[at], order[min(at + 9, n - 1)])
    out["range_keys"] = {"wide": min(1000, n - at), "narrow": min(10, n - at)}

    # first: nothing has read the store yet
    runs = {"device": [], "host": []}
    stores = []
    same = True
    for _ in range(pairs):
        dev, _ = restored(topic, False)
        host, _ = restored(topic, False)
        kv = GpuReplayKeyValueStore("s", host)
        got_d, dt = timed(lambda: list(dev.range_bytes(*wide)))
        runs["device"].append(dt)
        got_h, dt = timed(lambda: list(kv.range(*wide)))
        runs["host"].append(dt)
        same = same and got_d == got_h and dev.device_route and not host.device_route
        for s in stores:
            s.close()
        stores = [dev, host]
    out["first_range"] = compared(runs)
    dev._decoder.key_order()  # (built by the range above: this only reads what that build took)
    out["first_range"].update({"same_results": bool(same), "values": len(got_d), "order_passes": dev._decoder.order_passes})
    dev, host = stores
    kv = GpuReplayKeyValueStore("s", host)
    try:
        # warm: the key order is built, the host table and mirror are there
        out["warm"] = {}
        for name, fn_d, fn_h in (("range_10", lambda: list(dev.range_bytes(*narrow)), lambda: list(kv.range(*narrow))),
                                 ("range_1000", lambda: list(dev.range_bytes(*wide)), lambda: list(kv.range(*wide))),
                                 ("substates", lambda: dev.substates_for_aggregate(order[at]),
                                  lambda: [(k, v) for k, v in kv.range(order[at], order[at] + ":~") if k.split(":", 1)[0] == order[at]])):
            runs = {"device": [], "host": []}
            same = fn_d() == fn_h()
            for _ in range(pairs):
                runs["device"].append(timed(fn_d)[1])
                runs["host"].append(timed(fn_h)[1])
            out["warm"][name] = compared(runs)
            out["warm"][name]["same_results"] = bool(same)
        # all, consumed to the end
        runs = {"device": [], "host": []}
        same, values = True, 0
        for _ in range(pairs):
            got_d, dt = timed(lambda: list(dev.all_bytes()))
            runs["device"].append(dt)
            got_h, dt = timed(lambda: list(kv.all()))
            runs["host"].append(dt)
            same, values = same and got_d == got_h, len(got_d)
            del got_d, got_h
        out["all"] = compared(runs, values)
        out["all"].update({"same_results": bool(same), "values": values, "device_route_kept": dev.device_route})
        _, dt = timed(dev.num_entries)
        out["num_entries_s"] = dt
    finally:
        dev.close()
        host.close()

    # the build of the key order alone
    build, passes = [], 0
    for _ in range(pairs):
        s, _ = restored(topic, False)
        _, dt = timed(s._decoder.key_order)
        build.append(dt)
        passes = s._decoder.order_passes
        s.close()
    out["order_build"] = series(build, n)
    out["order_build"]["passes"] = passes
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = run(int(args[0]) if args else 2_000_000, int(args[1]) if len(args) > 1 else 5)
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "key_range_reads.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
