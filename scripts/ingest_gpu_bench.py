#!/usr/bin/env python3
"""Events-topic bytes -> (aggregate index, 16-byte event) arrays: the host decoder (one partition thread) against host framing
+ the device decoder, on the same wire bytes.  Counter fixture events as play-json text, and the same records with 16-byte
values; uncompressed and LZ4 batches of 16 KiB (the reference producer's batch size).   python scripts/ingest_gpu_bench.py [records]   (needs a GPU)
--envelope adds the case "json_envelope": the same generated events, each inside the protobuf message Event{aggregateId, payload}
a multilanguage application writes (EventJsonTemplate(envelope="protobuf_event")).  --pairs N: instead of the table, the device
decoder alone on the bare JSON topic and (with --envelope) on the enveloped one, N alternating pairs, medians and spreads of
the warm push."""
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np
import torch

import kafka_wire as kw
from fixture_models import CounterBusinessLogic, CountDecremented, CountIncremented, NoOpEvent
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest

import argparse

ap = argparse.ArgumentParser()
ap.add_argument("records", nargs="?", type=int, default=4_000_000)
ap.add_argument("--envelope", action="store_true", help="also the JSON events inside the protobuf Event envelope")
ap.add_argument("--pairs", type=int, default=0, help="alternating bare / enveloped device-decoder runs instead of the table")
ap.add_argument("--envelope-batch-records", type=int, default=122, help="enveloped events per batch (122: the bytes of 140 bare ones)")
ap.add_argument("--codec", default="lz4", choices=["none", "lz4"], help="--pairs: the batches' compression")
args = ap.parse_args()
n_records = args.records
# records per batch: what the reference's producer packs into one batch — it closes a batch at 16 KiB of records
# (kafka.publisher.batch-size = 16384, reference.conf:115): ~140 play-json Counter events, ~400 16-byte ones
# (the envelope adds 17 bytes to each of these values: 122 enveloped events fill the 15.7 KB that 140 bare ones do.  With 140 per batch a
# records section is 18.1 KB: beyond the record stage's 16.25 KiB LDS class and its 17.75 KiB limit for chaining a batch by a whole wave —
# --envelope-batch-records 140 measures that shape)
PER_BY_MODE = {"json": 140, "fixed16": 400, "json_envelope": args.envelope_batch_records}
bl = CounterBusinessLogic()
model, fmt = bl.command_model(), bl.event_write_formatting()
tmpl = model.event_json_template()
TEMPLATES = {"json": tmpl, "fixed16": None}
if args.envelope:
    from fixture_models import protobuf_varint
    from surge_amd.ingest import EventJsonTemplate

    TEMPLATES["json_envelope"] = EventJsonTemplate(tmpl.discriminator, tmpl.types, envelope="protobuf_event")


def enveloped(aggregate_id: str, payload: bytes) -> bytes:
    key = aggregate_id.encode()
    return b"\x0a" + protobuf_varint(len(key)) + key + b"\x12" + protobuf_varint(len(payload)) + payload


def topic(mode, codec, seed=1):
    """(wire bytes, records): 16 generated batches repeated; the same events for every mode of one seed"""
    rng = np.random.default_rng(seed)
    PER = PER_BY_MODE[mode]
    n_batches = n_records // PER
    protos = []
    for b in range(16):
        recs = []
        for i in range(PER):
            agg = f"acct-{int(rng.integers(0, 100000)):08d}"
            e = [CountIncremented(agg, int(rng.integers(0, 1000)), i + 1), CountDecremented(agg, int(rng.integers(0, 1000)), i + 1), NoOpEvent(agg, i + 1)][i % 3]
            m = fmt.write_event(e)
            recs.append((m.key.encode(), m.value if mode == "json" else enveloped(e.aggregateId, m.value) if mode == "json_envelope" else model.encode_events([e]).tobytes()))
        protos.append(bytearray(kw.record_batch(0, recs, compression=codec)))
    parts = []
    for b in range(n_batches):
        p = bytearray(protos[b % len(protos)])
        struct.pack_into(">q", p, 0, b * PER)  # baseOffset is outside the CRC
        parts.append(bytes(p))
    return b"".join(parts), n_batches * PER


def warm_push_seconds(wire, template, passes=3):
    """Host framing + one device push of the whole topic, `passes` times on one decoder; the last pass (warm buffers, a populated key
    table) is what counts: (framing seconds, push seconds to the device's synchronise)."""
    with EventsTopicIngest(frames=True, device_lz4=True) as g, DeviceDecoder(template) as d:
        for _ in range(passes):
            d.clear()
            t0 = time.perf_counter()
            g.feed(wire)
            sections, arena = g.drain_sections()
            t1 = time.perf_counter()
            d.push(sections, arena)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
    return t1 - t0, t2 - t1


if args.pairs:
    modes = ["json"] + (["json_envelope"] if args.envelope else [])
    wires = {m: topic(m, args.codec) for m in modes}
    runs = {m: [] for m in modes}
    for _ in range(args.pairs):
        for m in modes:  # alternating: one after the other inside every pair
            runs[m].append(warm_push_seconds(wires[m][0], TEMPLATES[m])[1])
    out = {"records": {m: wires[m][1] for m in modes}, "batch_records": {m: PER_BY_MODE[m] for m in modes}, "codec": args.codec, "pairs": args.pairs, "what": "seconds of the warm device push (copy, LZ4, records, interning) of the whole topic"}
    for m in modes:
        t = sorted(runs[m])
        out[m] = {"wire_bytes": len(wires[m][0]), "push_s": runs[m], "median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1],
                  "records_per_sec_at_median": wires[m][1] / t[len(t) // 2]}
    if args.envelope:
        out["envelope_over_bare_seconds_per_record_at_medians"] = (out["json_envelope"]["median_s"] / wires["json_envelope"][1]) / (out["json"]["median_s"] / wires["json"][1])
    print(json.dumps(out))
    sys.exit(0)

res = {"records_per_case": n_records, "batch_records": PER_BY_MODE}
for mode in ["json", "fixed16"] + (["json_envelope"] if args.envelope else []):
    PER = PER_BY_MODE[mode]
    n_batches = n_records // PER
    for codec in ("none", "lz4"):
        wire, n = topic(mode, codec)
        with EventsTopicIngest() as g:
            t0 = time.perf_counter()
            g.feed(wire)
            t1 = time.perf_counter()
            h_agg, h_ev, h_off = g.drain_json(TEMPLATES[mode]) if mode != "fixed16" else g.drain_fixed16()
            t2 = time.perf_counter()
        r = {"wire_bytes": len(wire), "host_decoder": {"feed_s": t1 - t0, "drain_s": t2 - t1, "records_per_sec": n / (t2 - t0)}}
        variants = [("framing_plus_device_decoder", False)] + ([("framing_plus_device_decoder_lz4_on_device", True)] if codec == "lz4" else [])
        for label, device_lz4 in variants:
          with EventsTopicIngest(frames=True, device_lz4=device_lz4) as g, DeviceDecoder(TEMPLATES[mode]) as d:
            for rep in range(3):  # the last pass runs with warm buffers (both of the framer's arenas) and a populated key table
                d.clear()
                t0 = time.perf_counter()
                g.feed(wire)
                t1 = time.perf_counter()
                sections, arena = g.drain_sections()
                t2 = time.perf_counter()
                d.push(sections, arena)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
            agg, ev, off, n_keys = d.result()
            same = bool((agg.cpu().numpy() == h_agg).all() and (ev.cpu().numpy().view(h_ev.dtype).reshape(-1) == h_ev).all() and (off.cpu().numpy() == h_off).all())
          r[label] = {"host_framing_s": t1 - t0, "drain_sections_s": t2 - t1, "device_push_s": t3 - t2,
                      "records_per_sec": n / (t3 - t0), "device_push_records_per_sec": n / (t3 - t2), "equal_to_host_decoder": same, "keys": n_keys}
        r["speedup_one_host_thread"] = max(r[l]["records_per_sec"] for l, _ in variants) / r["host_decoder"]["records_per_sec"]
        res[f"{mode}/{codec}"] = r
print(json.dumps(res))
