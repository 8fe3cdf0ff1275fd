"""TEST INFRASTRUCTURE: a deterministic trace of the host framer (surge_amd/csrc/ingest.cpp, ingest_group.cpp) through its C ABI.

    python tests/ingest_trace.py LIB SEED

LIB is a host-only build of the library (g++ -O2 -shared -fPIC of ingest.cpp, ingest_group.cpp, crc32c.cpp, event_decode.cpp,
f64_text.cpp, lz4_frame.cpp and snapshot_writer.cpp: build_host_library below).  A seeded corpus is driven through single framers and partition groups, and
every call prints one line: what was called, the status, what was consumed, the last-error text and a digest of everything the
call handed back (records and the arena bytes they span, events and offsets, sections with their offsets and codec bits and the
bytes they span, the counters, the key table, the group's slab bytes, positions, floors and what lies below a start offset).  Two builds of the framer that behave alike print the same
trace; tests/test_ingest_trace.py holds the trace to be reproducible and to reach every message the framer can return."""
import ctypes
import hashlib
import os
import random
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kafka_wire as kw  # noqa: E402
import start_offsets_gen as gen  # noqa: E402

HOST_SOURCES = ("ingest.cpp", "ingest_group.cpp", "crc32c.cpp", "event_decode.cpp", "f64_text.cpp", "lz4_frame.cpp", "snapshot_writer.cpp")
FRAMES, DEVICE_LZ4, DEVICE_CRC = 0x100, 0x200, 0x400
vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32


def build_host_library(out_path, csrc=os.path.join(ROOT, "surge_amd", "csrc"), include=os.path.join(ROOT, "include")):
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + include] + [os.path.join(csrc, f) for f in HOST_SOURCES]
                   + ["-o", out_path, "-lpthread"], check=True, capture_output=True)
    return out_path


class Rec(ctypes.Structure):  # surge_ingest_record
    _fields_ = [("offset", i64), ("agg_idx", i64), ("key_off", i64), ("key_len", i32), ("value_len", i32), ("value_off", i64)]


class Section(ctypes.Structure):  # surge_batch_section
    _fields_ = [("byte_off", i64), ("byte_len", i64), ("base_offset", i64), ("n_records", i32), ("codec", i32)]


class Floor(ctypes.Structure):  # surge_section_floor
    _fields_ = [("part", i32), ("reserved", i32), ("section", i64), ("first_offset", i64)]


class EvType(ctypes.Structure):  # surge_event_json_type
    _fields_ = [("name", ctypes.c_char * 64), ("event_type", ctypes.c_uint32), ("arg_kind", ctypes.c_uint32), ("seq_field", ctypes.c_char * 64),
                ("arg_field", ctypes.c_char * 64)]


class EvTemplate(ctypes.Structure):  # surge_event_json_template
    _fields_ = [("n_types", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("discriminator", ctypes.c_char * 64), ("types", EvType * 16)]


def counter_template(n_types=2):
    t = EvTemplate()
    t.n_types, t.discriminator = n_types, b"_type"
    for k, (name, ty, kind, seq, arg) in enumerate([(b"countIncremented", 1, 1, b"sequenceNumber", b"incrementBy"), (b"no-op", 0, 0, b"sequenceNumber", b"")]):
        t.types[k].name, t.types[k].event_type, t.types[k].arg_kind, t.types[k].seq_field, t.types[k].arg_field = name, ty, kind, seq, arg
    return t


def load(path):
    lib = ctypes.CDLL(path)
    P = ctypes.POINTER
    for name, args, res in [
        ("surge_ingest_create", [i32, P(vp)], i32), ("surge_ingest_destroy", [vp], i32), ("surge_ingest_last_error", [vp], ctypes.c_char_p),
        ("surge_ingest_feed", [vp, vp, i64, P(i64)], i32), ("surge_ingest_set_threads", [vp, i32], i32), ("surge_ingest_ready", [vp], i64),
        ("surge_ingest_drain", [vp, i64, vp, P(i64)], i32), ("surge_ingest_arena", [vp], vp),
        ("surge_ingest_drain_fixed16", [vp, i64, vp, vp, vp, P(i64)], i32), ("surge_ingest_drain_json", [vp, i64, vp, vp, vp, vp, P(i64)], i32),
        ("surge_ingest_drain_sections", [vp, i64, vp, P(i64)], i32), ("surge_ingest_set_allocator", [vp, vp, vp], i32),
        ("surge_ingest_key_count", [vp], i64), ("surge_ingest_key", [vp, i64, P(vp), P(i64)], i32), ("surge_ingest_counters", [vp, P(i64 * 8)], i32),
        ("surge_ingest_group_create", [i32, i32, P(vp)], i32), ("surge_ingest_group_destroy", [vp], i32),
        ("surge_ingest_group_last_error", [vp], ctypes.c_char_p), ("surge_ingest_group_feed", [vp, vp, vp, i32, vp, i64, vp, P(i64), P(vp)], i32),
        ("surge_ingest_group_receive_buffer", [vp, i64, P(vp)], i32), ("surge_ingest_group_receive_copy", [vp, vp, vp, i32, vp], i32),
        ("surge_ingest_group_slab_bytes", [vp, P(i64), P(i32)], i32), ("surge_ingest_group_queued_sections", [vp], i64),
        ("surge_ingest_group_counters", [vp, P(i64 * 8)], i32), ("surge_ingest_group_set_allocator", [vp, vp, vp], i32),
        ("surge_ingest_set_start_offset", [vp, i64], i32), ("surge_ingest_take_floors", [vp, i64, vp, P(i64)], i32),
        ("surge_ingest_position", [vp], i64), ("surge_ingest_below_start", [vp, P(i64 * 2)], i32),
        ("surge_ingest_group_set_start_offsets", [vp, vp], i32), ("surge_ingest_group_take_floors", [vp, i64, vp, P(i64)], i32),
        ("surge_ingest_group_positions", [vp, vp], i32), ("surge_ingest_group_below_start", [vp, P(i64 * 2)], i32),
        ("surge_crc32c", [vp, i64], ctypes.c_uint32),
    ]:
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    return lib


# ---------------------------------------------------------------------------------------------------------------- the wire
def raw_batch(base_offset, count, payload, attrs=0, producer_id=-1, magic=2):
    """A v2 batch around an arbitrary records section (kw.record_batch only writes well-formed records)."""
    after_crc = struct.pack(">hiqqqhii", attrs, max(count - 1, 0), 0, 0, producer_id, 0, -1, count) + payload
    body = struct.pack(">ib", 0, magic) + struct.pack(">I", kw.crc32c(after_crc)) + after_crc
    return struct.pack(">qi", base_offset, len(body)) + body


def reseal(batch):
    """The batch with its CRC field recomputed: a mutation behind it then gets past the CRC check."""
    return batch[:17] + struct.pack(">I", kw.crc32c(batch[21:])) + batch[21:]


def patch(batch, at, data, seal=True):
    out = batch[:at] + data + batch[at + len(data):]
    return reseal(out) if seal else out


def record_body(*fields):
    body = b"\x00" + kw.varint(0) + kw.varint(0) + b"".join(fields)
    return kw.varint(len(body)) + body


class Corpus:
    def __init__(self, seed):
        self.rng = random.Random(seed)

    def records(self, n, fixed16=False):
        rng, recs = self.rng, []
        for i in range(n):
            key = f"agg-{rng.randrange(40)}:{i}".encode()[: rng.randrange(1, 20)]
            if fixed16:
                recs.append((key, rng.randbytes(16)))
                continue
            r = rng.random()
            if r < 0.08:
                recs.append((b"", b""))  # the producer's flush record
            elif r < 0.12:
                recs.append((None, rng.randbytes(5)))
            elif r < 0.16:
                recs.append((key, None))
            else:
                hdrs = [(b"h" * rng.randrange(0, 5), None if rng.random() < 0.3 else b"v" * rng.randrange(0, 9))] if rng.random() < 0.3 else []
                recs.append((key, rng.choice([b"", rng.randbytes(16), rng.randbytes(rng.randrange(1, 300)), b"ab" * rng.randrange(1, 400)]), hdrs))
        return recs

    def topic(self, n_batches, base=None, fixed16=False, codecs=("none", "lz4"), late_marker=True):
        """(batches, next offset): plain and lz4 batches, transactions of two producers that commit, abort, or stay open until a
        marker that comes `late` (the caller appends it to a later feed: the second return value's third entry)."""
        rng = self.rng
        off = rng.randrange(0, 1 << 40) if base is None else base
        out, late = [], []
        for _ in range(n_batches):
            n = rng.randrange(1, 30)
            tx = rng.random() < 0.4
            pid = rng.choice([7, 9])
            out.append(kw.record_batch(off, self.records(n, fixed16), compression=rng.choice(codecs), transactional=tx, producer_id=pid if tx else -1))
            off += n
            if tx:
                r = rng.random()
                if r < 0.7:
                    out.append(kw.control_batch(off, pid, kw.COMMIT if r < 0.45 else kw.ABORT))
                    off += 1
                elif late_marker:
                    late.append(pid)
        for pid in late:
            out.append(kw.control_batch(off, pid, rng.choice([kw.COMMIT, kw.ABORT])))
            off += 1
        return out, off


def big_lz4_batch(lib):
    """An lz4 batch whose frame announces 512 MiB + 1 of content and delivers more: the host decoder's 2 GiB guard.  One block:
    64 KiB of literals, then matches of 65535 bytes at distance 65535 (a memcpy each), 260 bytes of input per match."""
    def ext(n):
        return b"\xff" * (n // 255) + bytes([n % 255])
    want = (1 << 29) + 1
    block = b"\xff" + ext(65536 - 15) + bytes(65536) + struct.pack("<H", 65535) + ext(65535 - 4 - 15)
    n_more = (want + 65536) // 65535 + 1
    block += (b"\x0f" + struct.pack("<H", 65535) + ext(65535 - 4 - 15)) * n_more + b"\x00"
    desc = bytes([0x68, 0x40]) + struct.pack("<Q", want)
    frame = struct.pack("<I", 0x184D2204) + desc + bytes([kw.header_checksum(desc)]) + struct.pack("<I", len(block)) + block + struct.pack("<I", 0)
    after_crc = struct.pack(">hiqqqhii", 3, 0, 0, 0, -1, 0, -1, 1) + frame
    crc = lib.surge_crc32c(after_crc, len(after_crc))  # (2.4 MB: the table walk in Python takes seconds)
    body = struct.pack(">ib", 0, 2) + struct.pack(">I", crc) + after_crc
    return struct.pack(">qi", 0, len(body)) + body


# ---------------------------------------------------------------------------------------------------------------- the trace
class Trace:
    def __init__(self, lib, out=sys.stdout):
        self.lib, self.out, self.n = lib, out, 0

    def line(self, what, rc, consumed, err, *returned):
        h = hashlib.sha1()
        for r in returned:
            h.update(repr(r).encode() if not isinstance(r, (bytes, bytearray)) else bytes(r))
            h.update(b"|")
        self.n += 1
        self.out.write(f"{self.n:05d} {what} rc={rc} consumed={consumed} err={err!r} {h.hexdigest()[:20]}\n")


class Framer:
    """One surge_ingest handle; every call is a trace line that also carries the counters and the key table."""

    def __init__(self, tr, flags, tag):
        self.tr, self.lib, self.tag, self.flags = tr, tr.lib, tag, flags
        self.h = vp()
        rc = self.lib.surge_ingest_create(flags, ctypes.byref(self.h))
        tr.line(f"{tag} create({flags:#x})", rc, 0, self.err(None) if rc else "")

    def err(self, h="self"):
        return (self.lib.surge_ingest_last_error(self.h if h == "self" else h) or b"").decode()

    def state(self):
        c = (i64 * 8)()
        self.lib.surge_ingest_counters(self.h, ctypes.byref(c))
        keys = []
        for k in range(self.lib.surge_ingest_key_count(self.h)):
            p, n = vp(), i64()
            assert self.lib.surge_ingest_key(self.h, k, ctypes.byref(p), ctypes.byref(n)) == 0
            keys.append(ctypes.string_at(p.value, n.value))
        return list(c), keys, self.lib.surge_ingest_ready(self.h)

    def arena(self, off, n):
        base = self.lib.surge_ingest_arena(self.h)
        return ctypes.string_at(base + off, n) if n > 0 else b""

    def feed(self, data):
        buf = ctypes.create_string_buffer(data, len(data))
        consumed = i64(-1)
        rc = self.lib.surge_ingest_feed(self.h, buf, len(data), ctypes.byref(consumed))
        self.tr.line(f"{self.tag} feed({len(data)})", rc, consumed.value, self.err(), self.state())
        return rc, consumed.value

    def feed_cut(self, wire, rng, drain):
        """The wire in pieces cut at random byte positions; what a feed does not consume is fed again in front of the next piece."""
        pending, pos = b"", 0
        while pos < len(wire) or pending:
            step = rng.randrange(1, 2500)
            pending += wire[pos:pos + step]
            pos += step
            rc, consumed = self.feed(pending)
            if rc != 0:
                return rc
            pending = pending[consumed:]
            if pos >= len(wire) and consumed == 0:
                break
            if rng.random() < 0.7:
                drain(rng.choice([3, 50, 100000]))
        drain(100000)
        return 0

    def drain(self, max_n):
        recs, got = (Rec * max(max_n, 1))(), i64(-1)
        rc = self.lib.surge_ingest_drain(self.h, max_n, recs, ctypes.byref(got))
        rows = [(r.offset, r.agg_idx, r.key_len, r.value_len, self.arena(r.key_off, r.key_len), self.arena(r.value_off, r.value_len))
                for r in recs[: max(got.value, 0)]] if rc == 0 else []
        self.tr.line(f"{self.tag} drain({max_n})", rc, got.value, self.err(), rows, self.state())
        return rc, got.value

    def drain_fixed16(self, max_n, json_template=None):
        idx, ev, off, got = (i64 * max(max_n, 1))(), (ctypes.c_uint8 * (16 * max(max_n, 1)))(), (i64 * max(max_n, 1))(), i64(-1)
        if json_template is None:
            what, rc = "drain_fixed16", self.lib.surge_ingest_drain_fixed16(self.h, max_n, idx, ev, off, ctypes.byref(got))
        else:
            what, rc = "drain_json", self.lib.surge_ingest_drain_json(self.h, max_n, ctypes.byref(json_template), idx, ev, off, ctypes.byref(got))
        n = max(got.value, 0) if rc == 0 else 0
        self.tr.line(f"{self.tag} {what}({max_n})", rc, got.value, self.err(), list(idx[:n]), bytes(ev[: 16 * n]), list(off[:n]), self.state())
        return rc, got.value

    def drain_sections(self, max_n):
        secs, got = (Section * max(max_n, 1))(), i64(-1)
        rc = self.lib.surge_ingest_drain_sections(self.h, max_n, secs, ctypes.byref(got))
        rows = []
        for s in secs[: max(got.value, 0)] if rc == 0 else []:
            pre = 8 if s.codec & 0x100 else 44 if s.codec & 0x200 else 0
            rows.append((s.byte_off, s.byte_len, s.base_offset, s.n_records, s.codec, self.arena(s.byte_off - pre, s.byte_len + pre)))
        self.tr.line(f"{self.tag} drain_sections({max_n})", rc, got.value, self.err(), rows, self.state())
        return rc, got.value

    def set_start(self, first):
        rc = self.lib.surge_ingest_set_start_offset(self.h, first)
        self.tr.line(f"{self.tag} set_start_offset({first})", rc, 0, self.err(), self.where())

    def where(self):
        """(position, batches discarded and records dropped below the start, counters, keys, ready)"""
        below = (i64 * 2)(-1, -1)
        rc = self.lib.surge_ingest_below_start(self.h, ctypes.byref(below))
        return self.lib.surge_ingest_position(self.h), rc, list(below), self.state()

    def report(self):
        self.tr.line(f"{self.tag} position / below_start", 0, 0, self.err(), self.where())

    def take_floors(self, max_n):
        floors, got = (Floor * max(max_n, 1))(), i64(-1)
        rc = self.lib.surge_ingest_take_floors(self.h, max_n, floors if max_n > 0 else None, ctypes.byref(got))
        rows = [(f.part, f.reserved, f.section, f.first_offset) for f in floors[: max(got.value, 0)]] if rc == 0 else []
        self.tr.line(f"{self.tag} take_floors({max_n})", rc, got.value, self.err(), rows, self.where())

    def any_drain(self, max_n):
        return self.drain_sections(min(max_n, 4096)) if self.flags & ~1 else self.drain(min(max_n, 4096))

    def close(self):
        self.lib.surge_ingest_destroy(self.h)


ALL_FLAGS = [iso | fr | lz | crc for iso in (0, 1) for fr in (0, FRAMES) for lz in (0, DEVICE_LZ4) for crc in (0, DEVICE_CRC)]


def mutated_batches(c):
    """name -> a damaged batch (each is fed behind one good batch)."""
    rng = c.rng
    good = kw.record_batch(500, c.records(12))
    lz = kw.record_batch(500, [(b"k:%d" % i, b"value " * 30) for i in range(12)], compression="lz4")
    key, val = kw.varint(1) + b"k", kw.varint(1) + b"v"
    return {
        "bad-crc": patch(good, len(good) - 3, b"\xa5", seal=False),
        "bad-crc-field": patch(good, 17, b"\x01\x02\x03\x04", seal=False),
        "magic-1": patch(good, 16, b"\x01", seal=False),
        "length-48": good[:8] + struct.pack(">i", 48) + good[12:],
        "length-negative": good[:8] + struct.pack(">i", -5) + good[12:],
        "codec-gzip": kw.record_batch(500, c.records(3), codec_override=1),
        "codec-zstd-control": raw_batch(500, 1, record_body(kw.varint(4) + struct.pack(">hh", 0, 1), kw.varint(-1), kw.varint(0)), attrs=0x34, producer_id=7),
        "lz4-damaged": patch(lz, 61 + 9 + rng.randrange(0, 20), b"\xff\xff"),
        "lz4-bad-magic": patch(lz, 61, b"\x05"),
        "lz4-header-checksum": patch(lz, 61 + 6, bytes([lz[61 + 6] ^ 0x10])),
        "count-impossible": patch(good, 57, struct.pack(">i", 1 << 30)),
        "count-impossible-lz4": patch(lz, 57, struct.pack(">i", 1 << 30)),
        "count-negative": patch(good, 57, struct.pack(">i", -2)),
        "count-too-many": patch(good, 57, struct.pack(">i", 13)),
        "record-length": raw_batch(500, 1, kw.varint(100) + b"\x00\x00\x00"),
        "record-key": raw_batch(500, 1, record_body(kw.varint(50) + b"ab")),
        "record-key-length": raw_batch(500, 1, record_body(kw.varint(-2))),
        "record-value": raw_batch(500, 1, record_body(key, kw.varint(50) + b"ab")),
        "header-count": raw_batch(500, 1, record_body(key, val, kw.varint(-1))),
        "header-key": raw_batch(500, 1, record_body(key, val, kw.varint(1), kw.varint(50) + b"h")),
        "header-value": raw_batch(500, 1, record_body(key, val, kw.varint(1), kw.varint(1) + b"h", kw.varint(50) + b"v")),
        "varint-endless": raw_batch(500, 1, b"\xff" * 12),
    }


def single_framers(tr, c):
    lib, rng = tr.lib, c.rng
    # the calls that fail before they look at a framer
    tr.line("create(out NULL)", lib.surge_ingest_create(1, None), 0, (lib.surge_ingest_last_error(None) or b"").decode())
    Framer(tr, 7, "iso7")
    tr.line("feed(handle NULL)", lib.surge_ingest_feed(None, b"", 0, None), 0, (lib.surge_ingest_last_error(None) or b"").decode())
    f = Framer(tr, 1, "args")
    tr.line("args feed(len -1)", lib.surge_ingest_feed(f.h, b"x", -1, None), 0, f.err())
    tr.line("args feed(data NULL)", lib.surge_ingest_feed(f.h, None, 4, None), 0, f.err())
    one = kw.record_batch(0, [(b"a", b"b")])
    tr.line("args feed(no consumed_out)", lib.surge_ingest_feed(f.h, one, len(one), None), 0, f.err(), f.state())
    for t in (0, 65, 3):
        tr.line(f"args set_threads({t})", lib.surge_ingest_set_threads(f.h, t), 0, f.err())
    got = i64()
    tr.line("args drain(out NULL)", lib.surge_ingest_drain(f.h, 4, None, ctypes.byref(got)), 0, f.err())
    tr.line("args drain_fixed16(out NULL)", lib.surge_ingest_drain_fixed16(f.h, 4, None, None, None, ctypes.byref(got)), 0, f.err())
    tr.line("args drain_json(template NULL)", lib.surge_ingest_drain_json(f.h, 4, None, None, None, None, ctypes.byref(got)), 0, f.err())
    tr.line("args drain_sections(n_out NULL)", lib.surge_ingest_drain_sections(f.h, 4, None, None), 0, f.err())
    f.drain_sections(4)
    f.drain_fixed16(4, json_template=counter_template(0))
    f.drain(4)
    libc = ctypes.CDLL(None)
    malloc, free = ctypes.cast(libc.malloc, vp), ctypes.cast(libc.free, vp)
    tr.line("args set_allocator(alloc only)", lib.surge_ingest_set_allocator(f.h, malloc, None), 0, f.err())
    tr.line("args set_allocator(late)", lib.surge_ingest_set_allocator(f.h, malloc, free), 0, f.err())
    f.close()
    f = Framer(tr, 1 | FRAMES, "args-frames")
    tr.line("args-frames set_allocator", lib.surge_ingest_set_allocator(f.h, malloc, free), 0, f.err())
    f.feed(kw.record_batch(0, [(b"a", b"b")]))
    f.drain(4)
    f.drain_fixed16(4)
    f.drain_fixed16(4, json_template=counter_template())
    f.drain_sections(0)
    f.drain_sections(4)
    f.close()

    # every flag combination in both isolation levels: a topic with transactions (commit, abort, a late marker), flush records and
    # null keys / values, plain and lz4, cut at random byte positions; then the damaged batches, each behind a good one
    damaged = mutated_batches(c)
    for flags in ALL_FLAGS:
        f = Framer(tr, flags, f"f{flags:#05x}")
        batches, _ = c.topic(14)
        f.feed_cut(b"".join(batches), rng, f.any_drain)
        # several feeds without a drain between them, then more feeds than there are arenas
        batches, off = c.topic(10, late_marker=False, codecs=("none",) if flags & DEVICE_CRC and not flags & DEVICE_LZ4 else ("none", "lz4"))
        for b in batches[:5]:
            f.feed(b)
        f.any_drain(2)
        for b in batches[5:]:
            f.feed(b)
            f.any_drain(rng.choice([1, 100]))
        f.any_drain(100000)
        f.close()
        for name, bad in damaged.items():
            f = Framer(tr, flags, f"f{flags:#05x} {name}")
            f.feed(kw.record_batch(400, c.records(5)) + bad + kw.record_batch(600, c.records(2)))
            f.any_drain(100)
            f.close()

    # CRC threads: a feed above 1 MiB whose batches are verified up front, with a cut batch at its end / a bad CRC / another
    # magic in the middle (the walk reports what the one-thread walk reports)
    proto = kw.record_batch(0, [(b"key-%d:x" % i, rng.randbytes(200)) for i in range(90)])
    n_copies = (1 << 20) // len(proto) + 8
    copies = [struct.pack(">q", k * 90) + proto[8:] for k in range(n_copies)]
    for name, mutate in [("whole", lambda x: x), ("cut", lambda x: x[:-1] + [x[-1][:100]]),
                         ("bad-crc", lambda x: x[:30] + [patch(x[30], 200, b"\x00\x01", seal=False)] + x[31:]),
                         ("magic-1", lambda x: x[:40] + [patch(x[40], 16, b"\x01", seal=False)] + x[41:]),
                         ("length-48", lambda x: x[:20] + [x[20][:8] + struct.pack(">i", 48) + x[20][12:]] + x[21:])]:
        for flags, threads in ((1, 1), (1, 4), (1 | FRAMES, 3), (1 | FRAMES | DEVICE_CRC, 4)):
            f = Framer(tr, flags, f"mt-{name}-{flags:#x}-{threads}")
            tr.line(f"{f.tag} set_threads", lib.surge_ingest_set_threads(f.h, threads), 0, f.err())
            f.feed(b"".join(mutate(list(copies))))
            f.any_drain(4096)
            f.close()

    # the all-or-nothing drains: a value that is refused pops nothing — the drain that follows delivers everything
    tmpl = counter_template()
    for iso in (0, 1):
        f = Framer(tr, iso, f"fixed16-{iso}")
        batches, off = c.topic(6, base=1000, fixed16=True)
        f.feed(b"".join(batches))
        f.drain_fixed16(7)
        f.feed(kw.record_batch(off, [(b"a:1", rng.randbytes(16)), (b"b:1", rng.randbytes(15)), (b"c:1", rng.randbytes(16))]))
        f.drain_fixed16(1)       # stops in front of the refused value
        f.drain_fixed16(100000)  # reaches it
        f.drain(3)
        f.feed(kw.record_batch(off + 3, [(None, rng.randbytes(16))]))
        f.drain_fixed16(100000)
        f.drain(100000)
        f.drain_fixed16(100000)
        f.close()
        f = Framer(tr, iso, f"json-{iso}")
        vals = [b'{"aggregateId":"a","incrementBy":%d,"sequenceNumber":%d,"_type":"countIncremented"}' % (rng.randrange(-99, 99), k + 1) for k in range(9)]
        vals[4] = b'{"_type":"no-op","aggregateId":"x","sequenceNumber":7}'
        f.feed(kw.record_batch(0, [(b"agg-%d" % (k % 3), v) for k, v in enumerate(vals)], compression="lz4"))
        f.drain_fixed16(4, json_template=tmpl)
        f.feed(kw.record_batch(9, [(b"agg-5", vals[0]), (b"agg-6", b'{"_type":"countIncremented","incrementBy":'), (b"agg-7", vals[1])]))
        f.drain_fixed16(100, json_template=tmpl)
        f.drain_fixed16(6, json_template=tmpl)  # the five left of the first batch and the one in front of the refused value
        f.drain_fixed16(100, json_template=tmpl)
        f.drain(1)
        f.drain_fixed16(100, json_template=tmpl)
        f.feed(kw.record_batch(12, [(b"agg-8", None)]) + kw.record_batch(13, [(None, vals[2])]))
        f.drain_fixed16(100, json_template=tmpl)
        f.drain(1)
        f.drain_fixed16(100, json_template=tmpl)
        f.drain(100)
        f.close()

    # the host decoder's 2 GiB guard
    big = big_lz4_batch(lib)
    f = Framer(tr, 1, "lz4-2gib")
    f.feed(kw.record_batch(0, [(b"a", b"b")]) + big)
    f.drain(10)
    f.close()


# ---------------------------------------------------------------------------------------------------------------- groups
class Group:
    def __init__(self, tr, n, flags, tag):
        self.tr, self.lib, self.n, self.tag = tr, tr.lib, n, tag
        self.g = vp()
        rc = self.lib.surge_ingest_group_create(n, flags, ctypes.byref(self.g))
        tr.line(f"{tag} group_create({n}, {flags:#x})", rc, 0, (self.lib.surge_ingest_last_error(None) or b"").decode() if rc else "")

    def err(self):
        return (self.lib.surge_ingest_group_last_error(self.g) or b"").decode()

    def state(self):
        c, b, custom = (i64 * 8)(), i64(), i32()
        self.lib.surge_ingest_group_counters(self.g, ctypes.byref(c))
        self.lib.surge_ingest_group_slab_bytes(self.g, ctypes.byref(b), ctypes.byref(custom))
        return list(c), b.value, custom.value, self.lib.surge_ingest_group_queued_sections(self.g)

    def feed(self, parts, threads, inplace, max_sections=None):
        """parts[p]: bytes or None.  Returns (rc, consumed per partition, sections the feed wants room for)."""
        n = self.n
        bufs = [ctypes.create_string_buffer(w, len(w)) if w else None for w in parts]
        lens = (i64 * n)(*[len(w) if w else 0 for w in parts])
        data = (vp * n)(*[ctypes.addressof(b) if b is not None else None for b in bufs])
        what = "by copy"
        if inplace:
            placed = (vp * n)()
            rc = self.lib.surge_ingest_group_receive_copy(self.g, data, lens, threads, placed)
            self.tr.line(f"{self.tag} receive_copy({sum(lens)}, threads {threads})", rc, 0, self.err(), self.state())
            if rc != 0:
                return rc, [0] * n, 0
            data, what = placed, "in place"
        cap = sum(lens) // 61 + self.lib.surge_ingest_group_queued_sections(self.g) + 4 if max_sections is None else max_sections
        secs, n_sec, slab, consumed = (Section * max(cap, 1))(), i64(-1), vp(), (i64 * n)(*[-1] * n)
        rc = self.lib.surge_ingest_group_feed(self.g, data, lens, threads, consumed, cap, secs, ctypes.byref(n_sec), ctypes.byref(slab))
        rows = []
        for s in secs[: max(n_sec.value, 0)] if rc == 0 else []:
            pre = 8 if s.codec & 0x100 else 44 if s.codec & 0x200 else 0
            rows.append((s.byte_off, s.byte_len, s.base_offset, s.n_records, s.codec, ctypes.string_at(slab.value + s.byte_off - pre, s.byte_len + pre)))
        self.tr.line(f"{self.tag} group_feed({what}, threads {threads}, room {cap})", rc, list(consumed), self.err(), n_sec.value, slab.value is None, rows, self.state())
        return rc, list(consumed), n_sec.value

    def thread_err(self):
        return (self.lib.surge_ingest_group_last_error(None) or b"").decode()

    def where(self):
        """(status and positions, status and what lies below the starts, the thread's last error, counters / slabs / queued sections)"""
        pos, below = (i64 * self.n)(*[-1] * self.n), (i64 * 2)(-1, -1)
        rc = self.lib.surge_ingest_group_positions(self.g, pos)
        rc2 = self.lib.surge_ingest_group_below_start(self.g, ctypes.byref(below))
        return rc, list(pos), rc2, list(below), self.thread_err(), self.state()

    def set_starts(self, starts):
        rc = self.lib.surge_ingest_group_set_start_offsets(self.g, (i64 * self.n)(*starts) if starts is not None else None)
        self.tr.line(f"{self.tag} group_set_start_offsets({starts})", rc, 0, self.err(), self.where())

    def report(self):
        self.tr.line(f"{self.tag} group_positions / group_below_start", 0, 0, self.err(), self.where())

    def take_floors(self, max_n):
        floors, got = (Floor * max(max_n, 1))(), i64(-1)
        rc = self.lib.surge_ingest_group_take_floors(self.g, max_n, floors if max_n > 0 else None, ctypes.byref(got))
        rows = [(f.part, f.reserved, f.section, f.first_offset) for f in floors[: max(got.value, 0)]] if rc == 0 else []
        self.tr.line(f"{self.tag} group_take_floors({max_n})", rc, got.value, self.err(), rows, self.where())

    def close(self):
        self.lib.surge_ingest_group_destroy(self.g)


def groups(tr, c):
    lib, rng = tr.lib, c.rng
    tr.line("group_create(out NULL)", lib.surge_ingest_group_create(4, 1, None), 0, (lib.surge_ingest_last_error(None) or b"").decode())
    Group(tr, 0, 1, "g-none")
    Group(tr, 2, 9, "g-iso9")
    g = Group(tr, 2, 1, "g-args")
    tr.line("g-args group_feed(data NULL)", lib.surge_ingest_group_feed(g.g, None, None, 1, None, 0, None, None, None), 0, (lib.surge_ingest_group_last_error(None) or b"").decode())
    tr.line("g-args receive_copy(data NULL)", lib.surge_ingest_group_receive_copy(g.g, None, None, 1, None), 0, (lib.surge_ingest_group_last_error(None) or b"").decode())
    tr.line("g-args receive_buffer(-1)", lib.surge_ingest_group_receive_buffer(g.g, -1, None), 0, (lib.surge_ingest_group_last_error(None) or b"").decode())
    lens, data, n_sec, slab = (i64 * 2)(4, -1), (vp * 2)(), i64(), vp()
    tr.line("g-args group_feed(len -1)", lib.surge_ingest_group_feed(g.g, data, lens, 1, None, 0, None, ctypes.byref(n_sec), ctypes.byref(slab)), 0, g.err())
    tr.line("g-args receive_copy(len -1)", lib.surge_ingest_group_receive_copy(g.g, data, lens, 1, (vp * 2)()), 0, g.err())
    libc = ctypes.CDLL(None)
    malloc, free = ctypes.cast(libc.malloc, vp), ctypes.cast(libc.free, vp)
    tr.line("g-args set_allocator(alloc only)", lib.surge_ingest_group_set_allocator(g.g, malloc, None), 0, g.err())
    tr.line("g-args set_allocator", lib.surge_ingest_group_set_allocator(g.g, malloc, free), 0, g.err(), g.state())
    g.feed([kw.record_batch(0, [(b"a", b"b")]), None], 1, False)
    tr.line("g-args set_allocator(late)", lib.surge_ingest_group_set_allocator(g.g, malloc, free), 0, g.err(), g.state())
    g.close()

    for n in (1, 8, 9, 19):
        for flags in (0, 1, 1 | DEVICE_LZ4, 1 | DEVICE_LZ4 | DEVICE_CRC, DEVICE_CRC):
            for inplace in (False, True):
                threads = rng.randrange(1, 5)
                g = Group(tr, n, flags, f"g{n}-{flags:#x}-{'inplace' if inplace else 'copy'}")
                codecs = ("none", "lz4") if (flags & DEVICE_LZ4 or not flags & DEVICE_CRC) and (flags & DEVICE_LZ4 or not inplace) else ("none",)
                # every partition's log, dealt out over the fetches; a marker that belongs to an earlier fetch's transaction
                # arrives with a later one, and a fetch may end inside a batch (what is not consumed is fed again)
                logs = [b"".join(c.topic(rng.randrange(2, 9), codecs=codecs)[0]) if rng.random() < 0.85 else b"" for _ in range(n)]
                pos = [0] * n
                for fetch in range(8):
                    parts = []
                    for p in range(n):
                        take = len(logs[p]) - pos[p] if fetch == 7 else rng.randrange(0, max(len(logs[p]) // 3, 1))
                        parts.append(logs[p][pos[p]:pos[p] + take] or None)
                    rc, consumed, _ = g.feed(parts, threads, inplace)
                    if rc != 0:
                        break
                    pos = [a + b for a, b in zip(pos, consumed)]
                g.close()

    # host-side lz4 that outgrows the partition's slice: the feed is undone and run again with more room (and the next feed starts
    # from the factor this one needed)
    squeezed = [kw.record_batch(k * 50, [(b"key-%d:%d" % (k, i), bytes(3000)) for i in range(50)], compression="lz4") for k in range(6)]
    for n, threads in ((1, 1), (9, 3)):
        g = Group(tr, n, 1, f"g{n}-expand")
        for fetch in range(3):
            g.feed([squeezed[(p + fetch) % 6] + squeezed[(p + fetch + 1) % 6] if p % 4 != 3 else None for p in range(n)], threads, False)
        g.close()

    # a failing partition undoes the whole feed — the group is what it was: the same fetch without that partition's bytes delivers
    # everything else, carried transactions included; then a section table that is too small, and the same feed with room
    damaged = mutated_batches(c)
    for n, threads, flags, inplace in ((8, 2, 1, False), (9, 4, 1 | DEVICE_LZ4 | DEVICE_CRC, True), (19, 3, 1 | DEVICE_LZ4, False), (19, 2, 1 | DEVICE_LZ4, True)):
        g = Group(tr, n, flags, f"g{n}-{flags:#x}-undo-{'inplace' if inplace else 'copy'}")
        open_tx = [kw.record_batch(p * 1000, c.records(4), transactional=True, producer_id=7) for p in range(n)]
        g.feed(open_tx, threads, inplace)
        for name in ("bad-crc", "magic-1", "length-48", "codec-gzip", "count-impossible", "lz4-damaged", "record-key"):
            parts = [kw.control_batch(p * 1000 + 4, 7, kw.COMMIT) + kw.record_batch(p * 1000 + 5, c.records(3)) for p in range(n)]
            bad_at = rng.randrange(n)
            parts[bad_at] = parts[bad_at] + damaged[name]
            rc, consumed, _ = g.feed(parts, threads, inplace)
            if rc != 0:
                g.feed([None if p == bad_at else w for p, w in enumerate(parts)], threads, inplace)
        parts = [kw.record_batch(p * 1000 + 8, c.records(2)) + kw.record_batch(p * 1000 + 10, c.records(2)) for p in range(n)]
        rc, _, need = g.feed(parts, threads, inplace, max_sections=n)
        g.feed(parts, threads, inplace, max_sections=need)
        g.feed([None] * n, threads, inplace, max_sections=0)
        g.close()

    # in place, an lz4 batch and no SURGE_INGEST_DEVICE_LZ4
    g = Group(tr, 2, 1, "g2-inplace-lz4")
    g.feed([kw.record_batch(0, [(b"a", b"b")]), squeezed[0]], 2, True)
    g.close()


# ---------------------------------------------------------------------------------------------------------------- start offsets
START = 5


def straddling_topic(codec, value_of=lambda n: gen.fixed16(1, n, n * 3 + 1)):
    """With START = 5: a batch below the start as a whole (0 .. 1); the batch that straddles it (2 .. 6), with a flush record at
    offset 3, below the start; a committed transaction with a flush record above the start (7 .. 9, marker at 10); 11 .. 12, which
    straddles a start of 12."""
    v = value_of
    t = gen.Topic(codec)
    t.data([(b"a:0", v(0)), (b"b:1", v(1))])
    t.data([(b"a:2", v(2)), (b"", b""), (b"c:4", v(4)), (b"c:5", v(5)), (b"d:6", v(6))])
    t.data([(b"e:7", v(7)), (b"", b""), (b"a:9", v(9))], pid=5).marker(5, kw.COMMIT)
    t.data([(b"f:11", v(11)), (b"f:12", v(12))])
    return t


def start_offsets(tr):
    """The start-offset, floors and position calls (include/surge_ingest.h, "start offsets and positions") through single framers
    — the three host drains and the FRAMES drain — and through groups.  Nothing here is drawn at random."""
    lib = tr.lib
    thread_err = lambda: (lib.surge_ingest_last_error(None) or b"").decode()  # noqa: E731
    tr.line("set_start_offset(handle NULL)", lib.surge_ingest_set_start_offset(None, START), 0, thread_err())
    tr.line("position(handle NULL)", 0, 0, thread_err(), lib.surge_ingest_position(None))
    tr.line("below_start(handle NULL)", lib.surge_ingest_below_start(None, None), 0, thread_err())
    tr.line("take_floors(handle NULL)", lib.surge_ingest_take_floors(None, 0, None, None), 0, thread_err())
    tmpl = counter_template()
    json_value = lambda n: b'{"aggregateId":"a","incrementBy":%d,"sequenceNumber":%d,"_type":"countIncremented"}' % (n % 7 - 3, n + 1)  # noqa: E731
    for codec in ("none", "lz4"):
        t = straddling_topic(codec)
        cut = len(t.batches[0]["bytes"]) + len(t.batches[1]["bytes"]) // 2  # inside the straddling batch: what a feed does not consume is fed again
        # the host drains: records below the start are passed over one by one, the flush record among them
        for name, drain, topic in (("drain", lambda f, n: f.drain(n), t), ("fixed16", lambda f, n: f.drain_fixed16(n), t),
                                   ("json", lambda f, n: f.drain_fixed16(n, json_template=tmpl), straddling_topic(codec, json_value))):
            for iso in (0, 1):
                f = Framer(tr, iso, f"start-{codec}-{name}-{iso}")
                f.set_start(START)
                _, consumed = f.feed(topic.bytes[:cut])
                f.set_start(START + 1)  # refused: the first feed has been
                drain(f, 1)
                f.report()
                f.feed(topic.bytes[consumed:])
                f.report()
                drain(f, 1)  # the first record at the start: in front of it a whole batch and three records are passed over
                f.report()
                f.take_floors(0)  # (a host drain floors nothing)
                drain(f, 2)
                f.report()
                drain(f, 100000)
                f.report()
                f.close()
        f = Framer(tr, 1, f"start-{codec}-none")  # a start <= 0 is no start
        f.set_start(-3)
        f.feed(t.bytes)
        f.drain(100000)
        f.report()
        f.close()
        # the FRAMES drain: the batch below the start is discarded, the straddling one handed out floored and named in the floors list
        for flags in (1 | FRAMES, FRAMES | DEVICE_LZ4, 1 | FRAMES | DEVICE_LZ4 | DEVICE_CRC):
            for start in (START, 12, 2, 40):
                f = Framer(tr, flags, f"start-{codec}-{flags:#x}-at{start}")
                f.set_start(start)
                f.take_floors(0)
                _, consumed = f.feed(t.bytes[:cut])
                f.drain_sections(4)
                f.take_floors(4)
                f.report()
                f.feed(t.bytes[consumed:])
                f.set_start(start)
                f.report()
                f.drain_sections(1)
                f.take_floors(0)  # too small when the section is floored
                tr.line(f"{f.tag} take_floors(-1)", lib.surge_ingest_take_floors(f.h, -1, None, ctypes.byref(i64())), 0, f.err())
                f.take_floors(4)
                f.report()
                f.drain_sections(100)
                f.take_floors(4)
                f.report()
                f.close()

    # groups: partition 0 starts at START, partition 1 has no start, partition 2 starts at 12.  The first feed hands out partition 0's
    # straddling batch (a floor); the second, with partition 2's, is undone for want of room in sections_out and fed again
    for flags, inplace, codec, threads in ((1, False, "none", 1), (1, False, "lz4", 2), (1 | DEVICE_LZ4, True, "lz4", 2), (1 | DEVICE_LZ4 | DEVICE_CRC, True, "none", 3),
                                           (DEVICE_LZ4 | DEVICE_CRC, False, "lz4", 1)):
        t = straddling_topic(codec)
        g = Group(tr, 3, flags, f"g3-start-{flags:#x}-{codec}-{'inplace' if inplace else 'copy'}")
        tr.line(f"{g.tag} group_set_start_offsets(NULL)", lib.surge_ingest_group_set_start_offsets(g.g, None), 0, g.err(), g.thread_err())
        tr.line(f"{g.tag} group_take_floors(n_out NULL)", lib.surge_ingest_group_take_floors(g.g, 0, None, None), 0, g.err(), g.thread_err())
        tr.line(f"{g.tag} group_positions(out NULL)", lib.surge_ingest_group_positions(g.g, None), 0, g.err(), g.thread_err())
        tr.line(f"{g.tag} group_below_start(out NULL)", lib.surge_ingest_group_below_start(g.g, None), 0, g.err(), g.thread_err())
        g.set_starts([START, -1, 12])
        g.take_floors(0)
        first = b"".join(b["bytes"] for b in t.batches[:3])  # ... and the open transaction behind the straddling batch
        g.feed([first, t.bytes, None], threads, inplace)
        g.take_floors(0)  # too small
        g.take_floors(8)
        g.report()
        g.set_starts([START, -1, 12])  # refused: the first feed has been
        parts = [t.bytes[len(first):], None, t.bytes]
        rc, _, need = g.feed(parts, threads, inplace, max_sections=1)  # undone
        g.take_floors(8)
        g.report()
        g.feed(parts, threads, inplace, max_sections=need)
        g.take_floors(0)
        g.take_floors(8)
        g.report()
        g.feed([None, None, None], threads, inplace)
        g.take_floors(8)
        g.report()
        g.close()


def run(lib_path, seed, out=sys.stdout):
    tr = Trace(load(lib_path), out)
    single_framers(tr, Corpus(seed))
    groups(tr, Corpus(seed + 1000003))
    start_offsets(tr)
    return tr.n


if __name__ == "__main__":
    run(sys.argv[1], int(sys.argv[2]))
