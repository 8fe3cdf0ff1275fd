"""What keeping the string fields costs a resume from the state topic: the same restore with and without ``keep_strings``.

    python scripts/state_strings_bench.py [n_aggregates=2000000] [pairs=5] > profiles/state_strings.json

n BankAccount aggregates (UUID keys, a Double, ``accountOwner`` / ``securityCode`` from side string columns — every eighth
owner with escapes and non-ASCII) are published as the state topic: LZ4 record batches on 4 partitions, framed and
compressed by the device framer (``BulkSnapshotPublisher``).  Then the device route from those bytes to resident states —
framing, one push of the state-mode ``DeviceDecoder``, ``load_states_into`` — runs ``pairs`` times with ``keep_strings`` and
``pairs`` times without, alternating in one process after a warm-up of both; the kept columns are checked against the
columns that were published.  One more load is taken apart: ``decode_states(want_spans=True)`` over the decoder's arrays,
then ``merge_state_strings`` per column, timed on its own (wall time of the synchronous call, kernels and its three host
waits).  Bytes moved by a merge: both passes read the load's values (staged per workgroup), the spans and the statuses,
the second writes the column — ``2 x (values + 65 B per record) + column + 8 B per aggregate x 3``; reported against
8 TB/s — recorded, not held to a bar.  What to look at: ``keep_over_plain_median``, the added cost on the same box."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

N_PART = 4
PEAK_BYTES_PER_S = 8e12


def csr_column(strings):
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return np.frombuffer(b"".join(strings), dtype=np.uint8).copy(), off


def publish_topic(n):
    """-> ({partition: bytes}, keys, owners, codes, value bytes in the topic)"""
    import torch

    from surge_amd import schema as S
    from surge_amd.encode import JsonTemplate
    from surge_amd.replay import ReplayEngine
    from surge_amd.snapshot import BulkSnapshotPublisher

    rng = np.random.default_rng(1)
    keys = [f"{i:08x}-0000-4000-8000-{(i * 2654435761) % (1 << 48):012x}" for i in range(n)]
    owners = [(f'Owner "{i}" \\ Zoë €'.encode() if i % 8 == 0 else b"Account Owner %d" % i) for i in range(n)]
    codes = [b"" if i % 5 == 0 else b"%04d" % (i % 10000) for i in range(n)]
    prior = np.zeros(n, dtype=S.STATE_DTYPE)
    prior["balance"] = rng.integers(-10**8, 10**8, size=n) / 100.0
    prior["flags"] = S.STATE_PRESENT
    to_dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    with ReplayEngine() as eng:
        eng.load_csr(np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE), prior)
        eng.fold()
        cols = tuple((to_dev(d), to_dev(o)) for d, o in (csr_column(owners), csr_column(codes)))
        pub = BulkSnapshotPublisher(eng, keys, N_PART, template=JsonTemplate.bank_account(), compression="lz4", device_compression=True, strings=cols)
        try:
            out = {p: bytes(b) for p, b in pub.publish().items()}
            text = int(pub.timings["text_bytes"])
        finally:
            pub.close()
    return out, keys, owners, codes, text


def restore(topic, keep, look=None):
    """framing + one push + load; -> seconds (``look(decoder, engine)`` runs before the two are closed, untimed)"""
    import torch

    from surge_amd import schema as S
    from surge_amd.encode import JsonTemplate
    from surge_amd.ingest import DeviceDecoder, PartitionedFramedFetches
    from surge_amd.replay import ReplayEngine

    eng = ReplayEngine()
    eng.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    eng.fold()
    d = DeviceDecoder(states=True, keep_strings=keep)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with PartitionedFramedFetches([[topic.get(p) for p in range(N_PART)]], N_PART, threads=4, hold=4, overlap=True, device_crc=True, in_place=True) as framed:
            for item in framed:
                parts = [(sec, arena) for sec, arena in (item if isinstance(item, list) else [item]) if sec.shape[0]]
                d.push_async(parts)
                d.finish()
                if look is None:
                    d.load_states_into(eng, JsonTemplate.bank_account())
        dt = time.perf_counter() - t0
        return dt, (look(d, eng) if look is not None else None)
    finally:
        d.close()
        eng.close()


def merge_alone(d, eng):
    """the decoder's delivered records -> decode with spans -> the two merges, each timed on its own"""
    import torch

    from surge_amd.encode import JsonTemplate, decode_states, merge_state_strings

    agg, values, value_off, _, n_keys = d.state_result()
    eng.grow(n_keys)
    res = decode_states(eng, JsonTemplate.bank_account(), values, value_off, d_agg_idx=agg, out=eng.device_state(), want_spans=True)
    out = {"records": int(agg.numel()), "aggregates": int(n_keys), "value_bytes": int(values.numel()), "columns": []}
    for c in (0, 1):
        merge_state_strings(eng, c, values, value_off, agg, res[1], res.spans, n_agg=n_keys)  # (first call: scratch sized)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col = merge_state_strings(eng, c, values, value_off, agg, res[1], res.spans, n_agg=n_keys)
        dt = time.perf_counter() - t0
        moved = 2 * (out["value_bytes"] + 65 * out["records"]) + int(col[0].numel()) + 24 * out["aggregates"]
        out["columns"].append({"column": c, "seconds": dt, "column_bytes": int(col[0].numel()), "bytes_moved": moved,
                               "fraction_of_8TBps": moved / dt / PEAK_BYTES_PER_S})
    return out


def run(n, pairs):
    topic, keys, owners, codes, text_bytes = publish_topic(n)
    out = {"aggregates": n, "partitions": N_PART, "topic_bytes": sum(len(b) for b in topic.values()), "value_bytes": text_bytes, "pairs": pairs}
    small = publish_topic(20000)[0]
    for keep in (True, False):  # warm-up of both (code objects, pinned slabs' first touch, Python imports)
        restore(small, keep)

    def check(d, eng):  # the kept columns are the published ones, under the decoder's key order
        from surge_amd.encode import JsonTemplate

        d.load_states_into(eng, JsonTemplate.bank_account())
        index = {k: i for i, k in enumerate(keys)}
        order = [index[k] for k in d.keys()]
        cols = d.state_strings()
        ok = True
        for col, want in ((cols[0], owners), (cols[1], codes)):
            data, off = col[0].cpu().numpy().tobytes(), col[1].cpu().numpy()
            ok = ok and len(order) == n and data == b"".join(want[i] for i in order) and (np.diff(off) == [len(want[i]) for i in order]).all()
        return bool(ok)

    out["kept_columns_equal_the_published_ones"] = restore(topic, True, look=check)[1]
    runs = {"keep_strings": [], "plain": []}
    for _ in range(pairs):
        runs["keep_strings"].append(restore(topic, True)[0])
        runs["plain"].append(restore(topic, False)[0])
    for name, ts in runs.items():
        out[name] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts), "aggregates_per_s": n / float(np.median(ts))}
    out["keep_over_plain_median"] = out["keep_strings"]["median_s"] / out["plain"]["median_s"]
    out["keep_minus_plain_median_s"] = out["keep_strings"]["median_s"] - out["plain"]["median_s"]
    out["merge_alone"] = restore(topic, True, look=merge_alone)[1]
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    print(json.dumps(run(int(args[0]) if args else 2_000_000, int(args[1]) if len(args) > 1 else 5)))
