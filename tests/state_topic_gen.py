"""State-topic partitions as a consumer receives them after log compaction, for the state-mode device decoder's tests.

Built from ``kafka_wire.record`` / ``crc32c`` / ``lz4_frame`` and NOT through ``kafka_wire.record_batch``: a compacted batch
keeps its ``baseOffset`` and ``lastOffsetDelta`` while fewer records remain, so the ``offsetDelta``s of what is left are
non-contiguous — gaps.  A partition is a list of UNITS, each ``(bytes, delivered)``: whole batches in which every transaction
that opens also closes, and the ``(offset, key, value | None)`` records a ``read_committed`` consumer gets out of them, in
offset order.  Units can be concatenated and split freely (``concat``): what a fetch delivers is the concatenation of its
units' lists."""
import struct

import numpy as np

from kafka_wire import ABORT, COMMIT, control_batch, crc32c, lz4_frame, record
from oracle import oracle


def batch(base_offset, raw_records, last_offset_delta, compression="none", transactional=False, producer_id=-1, base_timestamp=0):
    """One RecordBatch v2 around already encoded records (``kafka_wire.record``): ``lastOffsetDelta`` is what the producer
    wrote, however many records compaction left."""
    recs = b"".join(raw_records)
    codec = {"none": 0, "lz4": 3}[compression]
    payload = lz4_frame(recs) if compression == "lz4" else recs
    attrs = codec | (0x10 if transactional else 0)
    after_crc = struct.pack(">hiqqqhii", attrs, last_offset_delta, base_timestamp, base_timestamp, producer_id, 0, 0 if transactional else -1,
                            len(raw_records)) + payload
    body = struct.pack(">ib", 0, 2) + struct.pack(">I", crc32c(after_crc)) + after_crc
    return struct.pack(">qi", base_offset, len(body)) + body


def compacted_batch(base_offset, kept, compression="none", **kw):
    """``kept``: ``(offset_delta, key, value | None[, headers])`` in ascending delta order -> (bytes, delivered records,
    the next batch's base offset).  The batch spans a few offsets beyond its last kept record, as one whose tail was compacted
    away does."""
    raws = [record(r[0], r[1], r[2], r[3] if len(r) > 3 else ()) for r in kept]
    last = (kept[-1][0] if kept else 0) + kw.pop("tail_gap", 0)
    data = batch(base_offset, raws, last, compression, **kw)
    return data, [(base_offset + r[0], r[1], r[2]) for r in kept], base_offset + last + 1


HEADERS = ((b"surge-state-version", b"1"), (b"traceparent", None))  # stateHeaders: two per record, one with a null value


def ids_of(n_ids):
    """Aggregate ids with what the state topic's whole-key rule has to survive: ``a`` next to ``a:b`` (the events topic would
    cut both to ``a``), ids with several colons, ids that need JSON escaping."""
    ids = []
    for i in range(n_ids):
        if i == 0:
            ids.append("a")
        elif i == 1:
            ids.append("a:b")
        elif i % 13 == 2:
            ids.append(f"ns:{i}:x")
        elif i % 17 == 3:
            ids.append(f'q"{i}\\t\x05ü')
        else:
            ids.append(f"agg-{i:04d}")
    return ids


def make_topic(seed=11, n_ids=300, n_records=2000, n_partitions=2, compression="lz4"):
    """-> ``units[p]`` = list of ``(bytes, delivered)``.  The same seed gives the same records whatever the compression.
    Per id the values count versions up; a live id is deleted with probability 1/4 (a tombstone, null value) and may come
    back later.  An id lives in one partition."""
    rng = np.random.default_rng(seed)
    ids = ids_of(n_ids)
    version = [0] * n_ids
    alive = [False] * n_ids
    units = [[] for _ in range(n_partitions)]
    next_off = [int(rng.integers(0, 1000)) for _ in range(n_partitions)]
    made = 0
    first = True

    def draw(p, n):
        """n data records for partition p: (key, value, headers)"""
        out = []
        for _ in range(n):
            i = int(rng.integers(0, n_ids // n_partitions)) * n_partitions + p
            if i >= n_ids:
                i = p
            if alive[i] and rng.random() < 0.25:
                alive[i] = False
                value = None
            else:
                alive[i] = True
                version[i] += 1
                value = oracle.counter_state_json(ids[i], int(rng.integers(-1000, 1000)), version[i])
            out.append((ids[i].encode("utf-8"), value, HEADERS if rng.random() < 0.2 else ()))
        return out

    def gapped(recs):
        """offset deltas with gaps: each record is followed by 0 .. 2 compacted-away offsets"""
        kept, delta = [], int(rng.integers(0, 3))
        for k, v, h in recs:
            kept.append((delta, k, v, h))
            delta += 1 + int(rng.integers(0, 3)) * (rng.random() < 0.3)
        return kept

    while made < n_records:
        p = int(rng.integers(0, n_partitions))
        kind = rng.choice(["plain", "txn", "txn2", "mixed"], p=[0.4, 0.3, 0.1, 0.2])
        data, delivered = b"", []

        def add(recs, keep=True, **kw):
            nonlocal data, delivered
            b, d, nxt = compacted_batch(next_off[p], gapped(recs), compression, tail_gap=int(rng.integers(0, 3)), **kw)
            next_off[p] = nxt
            data += b
            if keep:
                delivered += d

        def marker(pid, what):
            nonlocal data
            data += control_batch(next_off[p], pid, what)
            next_off[p] += 1

        n = int(rng.integers(1, 40))
        if first:  # the producer's flush record leads the topic (KafkaProducerActorImpl.scala:322-329): in a batch of its own transaction
            first = False
            b, _, nxt = compacted_batch(next_off[p], [(0, b"", b"")], compression, transactional=True, producer_id=7)
            next_off[p] = nxt
            data += b
            marker(7, COMMIT)
        if kind == "plain":
            add(draw(p, n))
        elif kind == "txn":
            add(draw(p, n), transactional=True, producer_id=7)
            marker(7, COMMIT)
        elif kind == "txn2":  # two batches of one transaction
            add(draw(p, n), transactional=True, producer_id=7)
            add(draw(p, max(1, n // 2)), transactional=True, producer_id=7)
            marker(7, COMMIT)
        else:  # a committed and an aborted transaction interleaved with a plain batch: the aborted records never appear
            add(draw(p, n), transactional=True, producer_id=7)
            saved = (list(version), list(alive))
            add(draw(p, max(1, n // 3)), keep=False, transactional=True, producer_id=9)
            version[:], alive[:] = saved  # (what was aborted never happened)
            add(draw(p, max(1, n // 2)))
            marker(7, COMMIT)
            marker(9, ABORT)
        made += len(delivered)
        units[p].append((data, delivered))
    return units


def concat(units):
    """-> (bytes, delivered) of consecutive units of one partition"""
    return b"".join(u[0] for u in units), [r for u in units for r in u[1]]


def split(units, k):
    """k consecutive slices of a partition's units (the fetches of a consumer)"""
    cut = [len(units) * j // k for j in range(k + 1)]
    return [units[cut[j]:cut[j + 1]] for j in range(k)]
