"""TEST INFRASTRUCTURE: small events topics for the start-offset tests, with the record list the writer itself keeps.

``Topic`` writes message-format-v2 batches through ``tests/kafka_wire.py`` — with compaction gaps (a batch that keeps its
``lastOffsetDelta`` while records are gone), transactions that commit or abort, control markers and flush records — and
remembers every record it wrote with its offset, so what a consumer that starts at offset ``s`` must be handed is the writer's
own list filtered by ``offset >= s``: nothing is derived from the code under test.
"""
import struct

import kafka_wire as kw


def data_batch(base_offset, recs, last_delta, *, compression="none", transactional=False, producer_id=-1):
    """``recs``: ``(offset_delta, key, value)``; ``last_delta``: the header's lastOffsetDelta (compaction keeps the written one)."""
    body = b"".join(kw.record(d, k, v) for d, k, v in recs)
    payload = kw.lz4_frame(body) if compression == "lz4" else body
    attrs = (3 if compression == "lz4" else 0) | (0x10 if transactional else 0)
    after_crc = struct.pack(">hiqqqhii", attrs, last_delta, 0, 0, producer_id, 0, -1, len(recs)) + payload
    out = struct.pack(">ib", 0, 2) + struct.pack(">I", kw.crc32c(after_crc)) + after_crc
    return struct.pack(">qi", base_offset, len(out)) + out


class Topic:
    """One partition.  ``batches``: per batch ``dict(bytes, base, last, kind, pid, records)`` in offset order; ``records`` of a
    data batch are ``(offset, key, value)``."""

    def __init__(self, compression="none"):
        self.compression = compression
        self.batches = []
        self.next_offset = 0

    def data(self, recs, *, pid=None, gone=(), written=None):
        """``recs``: ``(key, value)`` at consecutive offsets; ``gone``: the deltas compaction has removed; ``written``: how many
        records the batch was written with (default: all of ``recs``)."""
        base = self.next_offset
        n = written if written is not None else len(recs)
        kept = [(d, k, v) for d, (k, v) in enumerate(recs) if d not in gone]
        raw = data_batch(base, kept, n - 1, compression=self.compression, transactional=pid is not None, producer_id=-1 if pid is None else pid)
        self.batches.append(dict(bytes=raw, base=base, last=base + n - 1, kind="data", pid=pid, records=[(base + d, k, v) for d, k, v in kept]))
        self.next_offset = base + n
        return self

    def marker(self, pid, kind):
        raw = kw.control_batch(self.next_offset, pid, kind)
        self.batches.append(dict(bytes=raw, base=self.next_offset, last=self.next_offset, kind="commit" if kind == kw.COMMIT else "abort", pid=pid, records=[]))
        self.next_offset += 1
        return self

    @property
    def bytes(self):
        return b"".join(b["bytes"] for b in self.batches)

    def committed(self, upto=None):
        """Indices of the data batches a read_committed consumer of batches ``[0, upto)`` delivers, in offset order (the last
        stable offset: nothing behind a transaction that is still open at ``upto``)."""
        bs = self.batches[:upto]
        fate = {}
        for i, b in enumerate(bs):
            if b["kind"] == "data" and b["pid"] is not None:
                end = next((m["kind"] for m in bs[i + 1:] if m["kind"] != "data" and m["pid"] == b["pid"]), None)
                fate[i] = end
        out = []
        for i, b in enumerate(bs):
            if b["kind"] != "data":
                continue
            if b["pid"] is None or fate[i] == "commit":
                out.append(i)
            elif fate[i] is None:
                break  # an open transaction: nothing behind it is stable
        return out

    def delivered(self, start=0, upto=None):
        """``(offset, key, value)`` of what is delivered from offset ``start`` on: committed, no flush record."""
        return [r for i in self.committed(upto) for r in self.batches[i]["records"] if r[0] >= start and not (r[1] == b"" and r[2] == b"")]

    def position(self, upto):
        """Where a consumer of batches ``[0, upto)`` resumes: in front of its oldest open transaction, else behind the last batch."""
        bs = self.batches[:upto]
        for i, b in enumerate(bs):
            if b["kind"] == "data" and b["pid"] is not None and not any(m["kind"] != "data" and m["pid"] == b["pid"] for m in bs[i + 1:]):
                return b["base"]
        return bs[-1]["last"] + 1 if bs else 0

    def tail_bytes(self, start):
        """What a consumer that seeks to ``start`` is sent: the topic from the batch that contains ``start`` on."""
        return b"".join(b["bytes"] for b in self.batches if b["last"] >= start)


def fixed16(etype, seq, payload):
    return struct.pack("<IIq", etype, seq, payload)


def standard_topic(compression, value_of=None):
    """Batches of 1, 2, 7 and 64 records; a flush record; a compacted batch with a gap in the middle and one at its end; a
    committed and an aborted transaction of two batches each; keys ``<id>:<seq>`` over a dozen ids."""
    value_of = value_of or (lambda n: fixed16(1, n, n * 3 + 1))
    t = Topic(compression)
    n = [0]

    def recs(count):
        out = []
        for _ in range(count):
            out.append((b"agg-%d:%d" % (n[0] % 13, n[0]), value_of(n[0])))
            n[0] += 1
        return out

    t.data(recs(1))
    t.data(recs(2))
    seven = recs(7)
    seven[2] = (b"", b"")  # the producer's flush record, offset 5
    t.data(seven)
    t.data(recs(64), gone=set(range(20, 30)) | {63})  # offsets 10 .. 73: 30 .. 39 and 73 are gone
    t.data(recs(7), pid=7).data(recs(2), pid=7).marker(7, kw.COMMIT)  # 74 .. 82, marker at 83
    t.data(recs(7), pid=8).data(recs(1), pid=8).marker(8, kw.ABORT)   # 84 .. 91, marker at 92
    t.data(recs(64))  # 93 .. 156
    t.data(recs(2))   # 157, 158
    return t


def interesting_starts(t):
    """Every start the cases name: each batch's first offset, first + 1, last, last + 1; inside the gaps; the markers; inside
    both transactions; beyond the end; 0 and -1."""
    s = {0, -1, t.next_offset, t.next_offset + 341}
    for b in t.batches:
        s |= {b["base"], b["base"] + 1, b["last"], b["last"] + 1}
    s |= {30, 35, 39, 40, 73, 78, 81, 82, 88, 91}
    return sorted(s)
