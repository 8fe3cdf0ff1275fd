#!/usr/bin/env python3
"""The device decoder on the same play-json Counter events written once as lz4 and once as snappy: host framing (compressed
sections left as they are on the wire) + one warm device push of the whole topic, in alternating pairs; medians and spreads
(max - min) go to profiles/snappy_ingest.json.   python scripts/snappy_ingest_bench.py [records]   (needs a GPU and pyarrow)

The topic is scripts/ingest_gpu_bench.py's: 4 * 10^6 events in batches of 140 (about 15.7 KB of records: what the reference's
producer packs into one batch).  The snappy topic holds raw blocks from pyarrow's bundled snappy inside the framing
kafka-clients writes (snappy-java's SnappyOutputStream), 32 KiB chunks — one chunk per batch at this batch size.

--leg lz4 --label NAME: the lz4 leg alone, printed as one JSON line — for comparing this tree with another one in separate
processes (A / B / A); SURGE_BENCH_ROOT names the tree whose surge_amd is measured (default: this script's).  --merge-aba A1 B A2
writes three such lines into the output file."""
import argparse
import json
import os
import struct
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SURGE_BENCH_ROOT", HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.join(HERE, "examples"))

ap = argparse.ArgumentParser()
ap.add_argument("records", nargs="?", type=int, default=4_000_000)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--leg", choices=["both", "lz4"], default="both")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "snappy_ingest.json"))
ap.add_argument("--merge-aba", nargs=3, metavar=("A1", "B", "A2"), help="files holding one --leg lz4 line each: this tree, the parent, this tree")
args = ap.parse_args()

if args.merge_aba:
    runs = [json.loads(open(p).read().strip().splitlines()[-1]) for p in args.merge_aba]
    a1, b, a2 = (r["lz4"]["median_s"] for r in runs)
    spread = max(r["lz4"]["max_s"] - r["lz4"]["min_s"] for r in runs)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["lz4_leg_this_tree_parent_this_tree"] = {
        "what": "median seconds of the warm lz4 push in three processes on one box: this tree, the parent commit, this tree",
        "a1_median_s": a1, "b_parent_median_s": b, "a2_median_s": a2, "larger_spread_s": spread,
        "a_runs_bracket_b": min(a1, a2) <= b <= max(a1, a2), "b_within_the_larger_spread_of_both": abs(b - a1) < spread and abs(b - a2) < spread,
        "runs": runs}
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out["lz4_leg_this_tree_parent_this_tree"]))
    sys.exit(0)

import numpy as np
import torch

import kafka_wire as kw
from fixture_models import CounterBusinessLogic, CountDecremented, CountIncremented, NoOpEvent
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest

PER = 140
bl = CounterBusinessLogic()
model, fmt = bl.command_model(), bl.event_write_formatting()
tmpl = model.event_json_template()


def snappy_section(recs: bytes, chunk: int = 32768) -> bytes:
    import pyarrow as pa

    codec = pa.Codec("snappy")
    blocks = [codec.compress(recs[s:s + chunk], asbytes=True) for s in range(0, len(recs), chunk)]
    return bytes([0x82, 0x53, 0x4E, 0x41, 0x50, 0x50, 0x59, 0x00]) + struct.pack(">ii", 1, 1) + b"".join(struct.pack(">i", len(b)) + b for b in blocks)


def topic(codec, seed=1):
    """(wire bytes, records, records-section bytes per batch): 16 generated batches repeated; the same events for both codecs"""
    rng = np.random.default_rng(seed)
    n_batches = args.records // PER
    protos, section_bytes = [], 0
    for b in range(16):
        recs = []
        for i in range(PER):
            agg = f"acct-{int(rng.integers(0, 100000)):08d}"
            e = [CountIncremented(agg, int(rng.integers(0, 1000)), i + 1), CountDecremented(agg, int(rng.integers(0, 1000)), i + 1), NoOpEvent(agg, i + 1)][i % 3]
            m = fmt.write_event(e)
            recs.append((m.key.encode(), m.value))
        section_bytes += len(b"".join(kw.record(i, k, v) for i, (k, v) in enumerate(recs)))
        if codec == "snappy":
            protos.append(bytearray(kw.record_batch(0, recs, compression="lz4", codec_override=2, compressor=snappy_section)))
        else:
            protos.append(bytearray(kw.record_batch(0, recs, compression="lz4")))
    parts = []
    for b in range(n_batches):
        p = bytearray(protos[b % len(protos)])
        struct.pack_into(">q", p, 0, b * PER)  # baseOffset is outside the CRC
        parts.append(bytes(p))
    return b"".join(parts), n_batches * PER, section_bytes / 16


def warm_push_seconds(wire, passes=3):
    """Host framing + one device push of the whole topic, `passes` times on one decoder; the last pass (warm buffers, a populated key
    table) is what counts: (framing seconds, push seconds to the device's synchronise, the decoder's stats)."""
    with EventsTopicIngest(frames=True, device_lz4=True) as g, DeviceDecoder(tmpl) as d:
        for _ in range(passes):
            d.clear()
            t0 = time.perf_counter()
            g.feed(wire)
            sections, arena = g.drain_sections()
            t1 = time.perf_counter()
            d.push(sections, arena)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        n, stats = d.result()[0].shape[0], (d.route_stats() if hasattr(d, "route_stats") else {})
    return t1 - t0, t2 - t1, n, stats


legs = ["lz4"] + (["snappy"] if args.leg == "both" else [])
wires = {c: topic(c) for c in legs}
runs = {c: {"framing_s": [], "push_s": []} for c in legs}
last = {}
for _ in range(args.pairs):
    for c in legs:  # alternating: one after the other inside every pair
        f, p, n, stats = warm_push_seconds(wires[c][0])
        assert n == wires[c][1], (c, n, wires[c][1])
        runs[c]["framing_s"].append(f)
        runs[c]["push_s"].append(p)
        last[c] = stats
out = {"records": wires["lz4"][1], "batch_records": PER, "records_section_bytes_per_batch": wires["lz4"][2], "pairs": args.pairs, "label": args.label,
       "what": "host framing (sections left compressed) + the warm device push (copy, decompression, records, interning) of the whole topic; seconds",
       "device": torch.cuda.get_device_name(0)}
for c in legs:
    t, fr = sorted(runs[c]["push_s"]), sorted(runs[c]["framing_s"])
    out[c] = {"wire_bytes": len(wires[c][0]), "push_s": runs[c]["push_s"], "median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1], "spread_s": t[-1] - t[0],
              "framing_median_s": fr[len(fr) // 2], "framing_spread_s": fr[-1] - fr[0], "records_per_sec_at_median": wires[c][1] / t[len(t) // 2]}
if "snappy" in legs:
    # (three passes per run on one decoder, of which the counters see all: chunks per pass = a third)
    out["snappy"]["device_chunks_per_push"] = last["snappy"].get("snappy_device_chunks", 0) // 3
    out["snappy"]["host_sections"] = last["snappy"].get("snappy_host_sections", 0)
    out["snappy_over_lz4_push_seconds_at_medians"] = out["snappy"]["median_s"] / out["lz4"]["median_s"]
    keep = json.load(open(args.out)).get("lz4_leg_this_tree_parent_this_tree") if os.path.exists(args.out) else None
    if keep:
        out["lz4_leg_this_tree_parent_this_tree"] = keep
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))
