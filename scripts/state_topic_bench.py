"""Restoring the aggregate store from the state topic's BYTES: the device route against the host route, in one process.

    python scripts/state_topic_bench.py [n_aggregates=2000000] [pairs=5] > profiles/state_topic_restore.json
    python scripts/state_topic_bench.py --envelope protobuf_state [n_aggregates] [pairs] > profiles/state_topic_restore_protobuf.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/state_topic_bench.py --one-push [n_aggregates]
    python scripts/state_topic_bench.py --kernel-split DIR profiles/state_topic_restore.json   # folds the trace's stats into the JSON
    python scripts/state_topic_bench.py --lenient [n_aggregates] [pairs] > profiles/state_decode_lenient.json

n Counter aggregates are folded into an engine and published as the state topic — LZ4 record batches on 4 partitions,
framed and compressed by the device framer (``BulkSnapshotPublisher``).  Then two routes from those bytes to the same
resident states alternate, ``pairs`` times each after a warm-up of both:

* ``device``: ``GpuReplayStateStore.restore_from_state_topic`` — framing on the host, records found / ids interned / values
  gathered by the state-mode device decoder, ``surge_device_decoder_load_states``; the host key table from ``d.keys()``;
* ``host``: the only route there was before — ``EventsTopicIngest`` host decode, ``drain_records``, then
  ``restore_from_state_records`` (ids interned per record in Python, values joined on the host, one copy, device decode).

Both end in the same 64-byte rows (checked).  ``device_core`` times the device route without the store around it (framing,
pushes, loads; no key table to the host).  One JSON line: the seconds of every repeat, medians, spreads, aggregates/s, and
whether the device route wins every pair by more than both spreads.  ``--one-push`` runs one push + load of the whole topic
(for a kernel trace); ``--kernel-split`` reads that trace's kernel stats: per kernel of the push its time, and for the value
gather its time against the bytes it moves (read + written) as a fraction of 8 TB/s — recorded, not held to a bar.
``--envelope protobuf_state`` (in front of the other arguments) publishes the same aggregates as a multilanguage (SDK)
application stores them — ``encode_states(envelope="protobuf_state")`` behind the same device framer — and restores them
through the envelope route of every call above.
``--lenient`` (likewise in front) measures what the lenient reading mode costs on text that does not need it: the same compact
topic — both modes accept it — restored in the strict and in the lenient mode, ``pairs`` alternating pairs in one process after
a warm-up of both, for ``device_core`` and for the whole ``restore_from_state_topic``.  One JSON line: every repeat's seconds,
medians, spreads, the rows compared, and whether the medians differ by more than the larger spread.
``--strict-leg LABEL [n_aggregates] [pairs]`` prints the strict route alone as one JSON line — for comparing this tree with another
one in separate processes (A / B / A); ``SURGE_BENCH_ROOT`` names the tree whose ``surge_amd`` is measured (default: this
script's).  ``--merge-aba A1 B A2 JSON`` folds three such lines (this tree, the parent, this tree) into the JSON under
``strict_route_aba``."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SURGE_BENCH_ROOT", HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "examples"))

N_PART = 4
PEAK_BYTES_PER_S = 8e12
ENVELOPE = "none"  # --envelope: how the topic's values are written and read


def publish_topic(n):
    """-> (keys, {partition: bytes}, value bytes in the topic)"""
    from surge_amd import schema as S
    from surge_amd.replay import ReplayEngine
    from surge_amd.snapshot import BulkSnapshotPublisher

    rng = np.random.default_rng(1)
    keys = [f"agg-{i:08d}" for i in range(n)]
    so = np.arange(n + 1, dtype=np.int64)
    ev = S.make_events(np.full(n, S.EVT_INC), rng.integers(1, 10**5, size=n), rng.integers(-10**6, 10**6, size=n))
    with ReplayEngine() as eng:
        eng.load_csr(so, ev)
        eng.fold()
        pub = BulkSnapshotPublisher(eng, keys, N_PART, compression="lz4", device_compression=True, envelope=ENVELOPE)
        try:
            out = {p: bytes(b) for p, b in pub.publish().items()}
            text = int(pub.timings["text_bytes"])
        finally:
            pub.close()
    return keys, out, text


def device_route(bl, topic, lenient=False):
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(bl)
    mode = {"lenient": True} if lenient else {}
    t0 = time.perf_counter()
    counts = store.restore_from_state_topic([[topic.get(p) for p in range(N_PART)]], n_partitions=N_PART, envelope=ENVELOPE, **mode)
    return time.perf_counter() - t0, store, counts


def host_route(bl, topic):
    from surge_amd.ingest import EventsTopicIngest
    from surge_amd.store import GpuReplayStateStore

    store = GpuReplayStateStore(bl)
    t0 = time.perf_counter()
    records = []
    for p in sorted(topic):
        with EventsTopicIngest() as g:
            g.feed(topic[p])
            records.extend((k.decode("utf-8"), v) for _, _, k, v in g.drain_records())
    store.restore_from_state_records(records, envelope=ENVELOPE)
    return time.perf_counter() - t0, store, None


def device_core(topic, template, lenient=False):
    """framing + push + load, no store: seconds, and the engine / decoder for whoever wants to look"""
    import torch

    from surge_amd import schema as S
    from surge_amd.ingest import DeviceDecoder, PartitionedFramedFetches
    from surge_amd.replay import ReplayEngine

    eng = ReplayEngine()
    eng.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    eng.fold()
    d = DeviceDecoder(states=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with PartitionedFramedFetches([[topic.get(p) for p in range(N_PART)]], N_PART, threads=4, hold=4, overlap=True, device_crc=True, in_place=True) as framed:
        for item in framed:
            parts = [(sec, arena) for sec, arena in (item if isinstance(item, list) else [item]) if sec.shape[0]]
            d.push_async(parts)
            d.finish()
            counts = d.load_states_into(eng, template, envelope=ENVELOPE, **({"lenient": True} if lenient else {}))
    dt = time.perf_counter() - t0
    d.close()
    eng.close()
    return dt, counts


def rows_by_key(store):
    snap = store.engine.snapshot()
    order = np.argsort(np.array(store.keys.keys))
    return np.array(store.keys.keys)[order], snap[order]


def run(n, pairs):
    from fixture_models import CounterBusinessLogic
    from surge_amd.encode import JsonTemplate

    bl = CounterBusinessLogic()
    keys, topic, text_bytes = publish_topic(n)
    out = {"aggregates": n, "envelope": ENVELOPE, "partitions": N_PART, "topic_bytes": sum(len(b) for b in topic.values()), "value_bytes": text_bytes, "pairs": pairs}
    small = {p: b for p, b in publish_topic(20000)[1].items()}
    for route in (device_route, host_route):  # warm-up of both (code objects, pinned slabs' first touch, Python imports)
        route(bl, small)[1].close()
    runs = {"device": [], "host": [], "device_core": []}
    same = True
    for i in range(pairs):
        td, sd, counts = device_route(bl, topic)
        th, sh, _ = host_route(bl, topic)
        if i == 0:
            kd, rd = rows_by_key(sd)
            kh, rh = rows_by_key(sh)
            same = bool((kd == kh).all() and rd.tobytes() == rh.tobytes() and len(kd) == n)
            out["device_counts"] = counts
        sd.close()
        sh.close()
        runs["device"].append(td)
        runs["host"].append(th)
        runs["device_core"].append(device_core(topic, JsonTemplate.counter())[0])
    out["rows_equal_between_the_routes"] = same
    for route, ts in runs.items():
        out[route] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts), "aggregates_per_s": n / float(np.median(ts))}
    spread = max(out["device"]["spread_s"], out["host"]["spread_s"])
    out["device_wins_every_pair_by_more_than_both_spreads"] = all(h - d > spread for h, d in zip(runs["host"], runs["device"]))
    out["host_over_device_median"] = out["host"]["median_s"] / out["device"]["median_s"]
    return out


def run_lenient(n, pairs):
    """the strict and the lenient mode over the same compact topic, alternating"""
    from fixture_models import CounterBusinessLogic
    from surge_amd.encode import JsonTemplate

    bl = CounterBusinessLogic()
    _, topic, text_bytes = publish_topic(n)
    out = {"aggregates": n, "envelope": ENVELOPE, "partitions": N_PART, "topic_bytes": sum(len(b) for b in topic.values()), "value_bytes": text_bytes, "pairs": pairs}
    small = {p: b for p, b in publish_topic(20000)[1].items()}
    for lenient in (False, True):  # warm-up of both (code objects, pinned slabs' first touch, Python imports)
        device_route(bl, small, lenient)[1].close()
        device_core(small, JsonTemplate.counter(), lenient)
    names = {False: "strict", True: "lenient"}
    runs = {f"{what}_{mode}": [] for what in ("restore", "device_core") for mode in names.values()}
    same = True
    for i in range(pairs):
        rows = {}
        for lenient in ((False, True) if i % 2 == 0 else (True, False)):  # the order within a pair alternates too
            t, store, counts = device_route(bl, topic, lenient)
            if i == 0:
                rows[lenient] = rows_by_key(store)
                out[f"{names[lenient]}_counts"] = counts
            store.close()
            runs[f"restore_{names[lenient]}"].append(t)
            runs[f"device_core_{names[lenient]}"].append(device_core(topic, JsonTemplate.counter(), lenient)[0])
        if i == 0:
            same = bool((rows[False][0] == rows[True][0]).all() and rows[False][1].tobytes() == rows[True][1].tobytes() and len(rows[True][0]) == n)
    out["rows_equal_between_the_modes"] = same
    for name, ts in runs.items():
        out[name] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts), "aggregates_per_s": n / float(np.median(ts))}
    for what in ("restore", "device_core"):
        a, b = out[f"{what}_strict"], out[f"{what}_lenient"]
        spread = max(a["spread_s"], b["spread_s"])
        out[f"{what}_lenient_over_strict_median"] = b["median_s"] / a["median_s"]
        out[f"{what}_difference_exceeds_the_pairs_spread"] = bool(abs(b["median_s"] - a["median_s"]) > spread)
    return out


def run_strict_leg(label, n, pairs):
    """the strict route of one tree: ``pairs`` repeats of the whole restore and of device_core after a warm-up"""
    from fixture_models import CounterBusinessLogic
    from surge_amd.encode import JsonTemplate

    bl = CounterBusinessLogic()
    _, topic, _ = publish_topic(n)
    small = {p: b for p, b in publish_topic(20000)[1].items()}
    device_route(bl, small)[1].close()
    device_core(small, JsonTemplate.counter())
    runs = {"restore": [], "device_core": []}
    for _ in range(pairs):
        t, store, _ = device_route(bl, topic)
        store.close()
        runs["restore"].append(t)
        runs["device_core"].append(device_core(topic, JsonTemplate.counter())[0])
    out = {"label": label, "root": os.path.basename(os.path.abspath(ROOT)), "aggregates": n, "pairs": pairs}
    for name, ts in runs.items():
        out[name] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts)}
    return out


def merge_aba(a1, b, a2, json_path):
    legs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in (a1, b, a2)]
    doc = json.load(open(json_path)) if os.path.exists(json_path) else {}
    aba = {"legs": legs}
    for what in ("restore", "device_core"):
        this = [legs[0][what]["median_s"], legs[2][what]["median_s"]]
        parent = legs[1][what]["median_s"]
        spread = max(leg[what]["spread_s"] for leg in legs)
        aba[what] = {"this_tree_median_s": this, "parent_median_s": parent, "largest_spread_s": spread,
                     "difference_inside_the_spread": bool(abs(sum(this) / 2 - parent) <= max(spread, abs(this[0] - this[1])))}
    doc["strict_route_aba"] = aba
    json.dump(doc, open(json_path, "w"))
    print(json.dumps(aba))


def kernel_split(trace_dir, json_path):
    """rocprofv3's kernel stats of a --one-push run -> {"kernels": {name: {"calls", "total_us"}}, "value_gather": {...}} merged into json_path"""
    stats = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        raise SystemExit(f"no *kernel_stats.csv under {trace_dir}")
    kernels = {}
    for row in csv.DictReader(open(stats[-1])):
        name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if any(w in name for w in ("section_kernel", "lz4_", "crc", "probe_kernel", "flag_kernel", "assign_kernel", "finalize_kernel", "value_", "state_decode", "scan", "table_")):
            k = kernels.setdefault(name[:96], {"calls": 0, "total_us": 0.0})
            k["calls"] += int(row["Calls"])
            k["total_us"] += float(row["TotalDurationNs"]) / 1e3
    doc = json.load(open(json_path))
    doc["one_push_kernels"] = kernels
    gather_us = sum(v["total_us"] for k, v in kernels.items() if "value_gather" in k)
    moved = 2 * doc["value_bytes"]  # every value byte is read once and written once
    doc["value_gather"] = {"total_us": gather_us, "bytes_moved": moved,
                           "fraction_of_8TBps": (moved / (gather_us * 1e-6)) / PEAK_BYTES_PER_S if gather_us else None}
    json.dump(doc, open(json_path, "w"))
    print(json.dumps(doc["value_gather"]))


if __name__ == "__main__":
    args = sys.argv[1:]
    lenient_run = bool(args) and args[0] == "--lenient"
    if lenient_run:
        args = args[1:]
    if args and args[0] == "--envelope":
        ENVELOPE = args[1]
        if ENVELOPE not in ("none", "protobuf_state"):
            raise SystemExit(f"unknown envelope {ENVELOPE!r}")
        args = args[2:]
    if args and args[0] == "--kernel-split":
        kernel_split(args[1], args[2])
    elif args and args[0] == "--merge-aba":
        merge_aba(*args[1:5])
    elif args and args[0] == "--strict-leg":
        print(json.dumps(run_strict_leg(args[1], int(args[2]) if len(args) > 2 else 2_000_000, int(args[3]) if len(args) > 3 else 5)))
    elif args and args[0] == "--one-push":
        from surge_amd.encode import JsonTemplate

        n = int(args[1]) if len(args) > 1 else 2_000_000
        _, topic, _ = publish_topic(n)
        print(json.dumps({"one_push_seconds": device_core(topic, JsonTemplate.counter())[0]}))
    else:
        n = int(args[0]) if args else 2_000_000
        pairs = int(args[1]) if len(args) > 1 else 5
        print(json.dumps(run_lenient(n, pairs) if lenient_run else run(n, pairs)))
