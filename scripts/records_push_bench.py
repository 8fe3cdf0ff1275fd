#!/usr/bin/env python3
"""The framed-records route of the device decoder (``push_records`` / ``push_records_async``), measured.   (needs a GPU)

    python scripts/records_push_bench.py [records] --part pipelining|kernel|store|all [--label NAME] [--out FILE]
    python scripts/records_push_bench.py --merge FILE [FILE ...] --out profiles/records_push.json      (no GPU: joins the parts)

Two topics, handed over as arrays ``(data_uint8, off_int64)``: scripts/ingest_gpu_bench.py's play-json Counter topic (16 generated
batches of 140 events, repeated; default 4 * 10^6 records) and a BankAccount topic in the shape of ``bench.py --e2e-topic mixed``
(UUID keys, Double balances as text; 10^6 records).

pipelining  polls of 500, 10^4 and 10^6 records pushed as a loop of synchronous ``push_records`` and as ``push_records_async`` at
            depth 4 with ``finish(wait=False)``: five alternating pairs in one process, the key table warm; median, spread
            (max - min) and records/s per poll size.
kernel      one warm synchronous push of a whole topic (copy + record stage + interning), five times behind a warm-up that runs
            until the times are stationary, per topic; and the wire
            route's push of the same Counter records (uncompressed batches) for scale.  Run once per library build (--label;
            ``SURGE_REPLAY_LIB`` names another build): A / B / A in three processes is how two builds are compared.
store       ``restore_from_consumer_records`` against ``restore_from_fetches`` on the first 10^6 Counter records, the rows compared.
Each part prints one JSON line (and appends it to --out when given)."""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

ap = argparse.ArgumentParser()
ap.add_argument("records", nargs="?", type=int, default=4_000_000)
ap.add_argument("--mixed-records", type=int, default=1_000_000)
ap.add_argument("--part", default="all", choices=["pipelining", "kernel", "store", "all"])
ap.add_argument("--label", default="this tree")
ap.add_argument("--build", default="this tree", help="kernel: what the library named by SURGE_REPLAY_LIB was built from (recorded as it is given)")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--merge", nargs="+", default=None)
args = ap.parse_args()

if args.merge:
    parts = [json.loads(line) for path in args.merge for line in open(path) if line.strip().startswith("{")]
    doc = {"what": "scripts/records_push_bench.py on one MI355X", "kernel": [p for p in parts if p["part"] == "kernel"],
           "pipelining": [p for p in parts if p["part"] == "pipelining"], "store": [p for p in parts if p["part"] == "store"]}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sys.exit(0)

import numpy as np
import torch

import kafka_wire as kw
import topic_gen
from fixture_models import BankAccountBusinessLogic, CounterBusinessLogic, CountDecremented, CountIncremented, NoOpEvent
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest
from surge_amd.store import GpuReplayStateStore

PER = 140  # play-json Counter events the reference's producer packs into a 16 KiB batch (scripts/ingest_gpu_bench.py)


def tiled(keys, values, n):
    """``len(keys)`` generated records repeated up to ``n``: ``((key data, key off), (value data, value off))``"""
    def side(items):
        lens = np.array([len(x) for x in items], dtype=np.int64)
        reps = -(-n // len(items))
        data = np.tile(np.frombuffer(b"".join(items), dtype=np.uint8), reps)
        off = np.zeros(reps * len(items) + 1, dtype=np.int64)
        np.cumsum(np.tile(lens, reps), out=off[1:])
        return np.ascontiguousarray(data[: off[n]]), np.ascontiguousarray(off[: n + 1])

    return side(keys), side(values)


def counter_topic(n, seed=1):
    """ingest_gpu_bench.py's topic("json", ...): the same generator, the same seed -> arrays, and the uncompressed wire bytes"""
    rng = np.random.default_rng(seed)
    fmt = CounterBusinessLogic().event_write_formatting()
    keys, values, protos = [], [], []
    for b in range(16):
        recs = []
        for i in range(PER):
            agg = f"acct-{int(rng.integers(0, 100000)):08d}"
            e = [CountIncremented(agg, int(rng.integers(0, 1000)), i + 1), CountDecremented(agg, int(rng.integers(0, 1000)), i + 1), NoOpEvent(agg, i + 1)][i % 3]
            m = fmt.write_event(e)
            recs.append((m.key.encode(), m.value))
        keys += [k for k, _ in recs]
        values += [v for _, v in recs]
        protos.append(bytearray(kw.record_batch(0, recs)))
    n -= n % (16 * PER)
    wire = []
    for b in range(n // PER):
        p = bytearray(protos[b % 16])
        struct.pack_into(">q", p, 0, b * PER)
        wire.append(bytes(p))
    return tiled(keys, values, n), b"".join(wire), n, [len(w) for w in wire]


def mixed_topic(n, accounts=100_000, seed=2):
    """BankAccount events in the shape of bench.py's --e2e-topic mixed: the key is the account's UUID alone, every account is
    created once and updated from then on, the balances are Doubles as play-json writes them (tests/native/topic_gen.c)"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    k, ko, v, vo = topic_gen.bank_records(i % accounts, (1 + i // accounts).astype(np.int32), rng.integers(1, 10 ** 9, size=n))
    return (np.array(k, dtype=np.uint8), np.array(ko, dtype=np.int64)), (np.array(v, dtype=np.uint8), np.array(vo, dtype=np.int64))


def window(side, lo, hi):
    return side[0], side[1][lo:hi + 1]  # (offsets that do not start at 0 are the library's to rebase)


def stats(seconds, n):
    t = sorted(seconds)
    return {"seconds": seconds, "median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1], "spread_s": t[-1] - t[0], "records_per_sec_at_median": n / t[len(t) // 2]}


def emit(doc):
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def sync_loop(d, keys, values, n, poll):
    t0 = time.perf_counter()
    for lo in range(0, n, poll):
        hi = min(n, lo + poll)
        d.push_records(window(keys, lo, hi), window(values, lo, hi))
        d.clear()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def async_loop(d, keys, values, n, poll, depth=4):
    t0 = time.perf_counter()
    pending = 0
    for lo in range(0, n, poll):
        if pending == depth:
            d.finish(wait=False)
            d.clear()
            pending -= 1
        hi = min(n, lo + poll)
        d.push_records_async(window(keys, lo, hi), window(values, lo, hi))
        pending += 1
    while pending:
        d.finish(wait=False)
        d.clear()
        pending -= 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def part_pipelining(keys, values, n, template):
    out = {"part": "pipelining", "label": args.label, "topic": "counter", "depth": 4, "pairs": args.pairs, "polls": {}}
    with DeviceDecoder(template) as d:
        sync_loop(d, keys, values, n, 1_000_000)  # the key table and every buffer warm
        for poll in (500, 10_000, 1_000_000):
            m = min(n, 1_000_000) if poll == 500 else n  # (2000 polls of 500 are enough to say what a launch chain costs)
            async_loop(d, keys, values, m, poll)  # the slots' buffers sized for this poll size
            runs = {"sync": [], "async": []}
            for _ in range(args.pairs):
                runs["sync"].append(sync_loop(d, keys, values, m, poll))
                runs["async"].append(async_loop(d, keys, values, m, poll))
            s, a = stats(runs["sync"], m), stats(runs["async"], m)
            out["polls"][str(poll)] = {"records": m, "sync": s, "async": a, "async_faster_in_every_pair": all(x < y for x, y in zip(runs["async"], runs["sync"])),
                                       "median_gain_s": s["median_s"] - a["median_s"], "gain_beyond_both_spreads": s["median_s"] - a["median_s"] > max(s["spread_s"], a["spread_s"])}
    emit(out)


def warm_push(template, keys, values, n, runs=5, warm_min=8, warm_max=20):
    """Untimed pushes until the time is stationary — at least ``warm_min``, until two in a row differ by less than 5 %, at most
    ``warm_max`` (a process's first pushes of a size take about twice as long as its later ones) — then ``runs`` timed ones."""
    def once(d):
        d.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.push_records(window(keys, 0, n), window(values, 0, n))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with DeviceDecoder(template) as d:
        warm = [once(d)]
        while len(warm) < warm_max and (len(warm) < warm_min or abs(warm[-1] - warm[-2]) > 0.05 * warm[-1]):
            warm.append(once(d))
        return {"warm_up_s": warm, **stats([once(d) for _ in range(runs)], n)}


def warm_wire_push(template, wire, n, runs=5):
    with EventsTopicIngest(frames=True, device_lz4=True) as g, DeviceDecoder(template) as d:
        secs = []
        for r in range(runs + 2):
            d.clear()
            g.feed(wire)
            sections, arena = g.drain_sections()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.push(sections, arena)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return stats(secs[2:], n)


def part_kernel(counter, wire, n, mixed, n_mixed):
    emit({"part": "kernel", "label": args.label, "library": os.path.basename(os.environ.get("SURGE_REPLAY_LIB", "libsurge_replay.so")),
          "build": args.build, "what": "seconds of one warm synchronous push of the whole topic (copy + record stage + interning), five runs behind the warm-up",
          "counter": {"records": n, **warm_push(COUNTER_TEMPLATE, *counter, n)}, "mixed": {"records": n_mixed, **warm_push(BANK_TEMPLATE, *mixed, n_mixed)},
          "counter_wire_route_uncompressed": {"records": n, **warm_wire_push(COUNTER_TEMPLATE, wire, n)}})


def part_store(counter, wire, n, batch_lens):
    n = min(n, 1_000_000)
    n -= n % (16 * PER)
    keys, values = counter
    offsets = np.arange(n, dtype=np.int64)
    bl = CounterBusinessLogic()
    polls = [(window(keys, lo, min(n, lo + 10_000)), window(values, lo, min(n, lo + 10_000)), offsets[lo:lo + 10_000]) for lo in range(0, n, 10_000)]
    ends = np.concatenate([[0], np.cumsum(batch_lens)])
    cut = [int(ends[min(n // PER, b)]) for b in range(0, n // PER + 72, 72)]  # fetches of 72 batches: 10 080 records, about what a poll holds
    out = {"part": "store", "label": args.label, "records": n, "poll_records": 10_000}
    rows = {}
    for name in ("consumer_records", "fetches", "consumer_records", "fetches"):
        store = GpuReplayStateStore(bl)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "consumer_records":
                store.restore_from_consumer_records(polls, host_keys=False)
            else:
                store.restore_from_fetches([wire[a:b] for a, b in zip(cut, cut[1:]) if b > a], host_keys=False)
            torch.cuda.synchronize()
            out.setdefault(name + "_s", []).append(time.perf_counter() - t0)
            ids = store.keys.keys
            rows[name] = (ids, store.engine.snapshot().tobytes())
        finally:
            store.close()
    assert rows["consumer_records"] == rows["fetches"], "the two recoveries differ"
    out["rows_equal"], out["aggregates"] = True, len(rows["fetches"][0])
    for name in ("consumer_records", "fetches"):
        out[name + "_records_per_sec_second_run"] = n / out[name + "_s"][1]
    emit(out)


COUNTER_TEMPLATE = CounterBusinessLogic().command_model().event_json_template()
BANK_TEMPLATE = BankAccountBusinessLogic().command_model().event_json_template()
counter, wire, n, batch_lens = counter_topic(args.records)
if args.part in ("pipelining", "all"):
    part_pipelining(*counter, n, COUNTER_TEMPLATE)
if args.part in ("kernel", "all"):
    part_kernel(counter, wire, n, mixed_topic(args.mixed_records), args.mixed_records)
if args.part in ("store", "all"):
    part_store(counter, wire, n, batch_lens)
