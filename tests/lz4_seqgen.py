"""TEST INFRASTRUCTURE: a sequence-level LZ4 block writer, and the inputs of tests/test_lz4_seqgen.py (CPU) and
tests/test_ingest_stage_edges_gpu.py (GPU).

The device decoder's LZ4 stage (surge_amd/csrc/ingest_lz4.hip) branches on the SEQUENCE stream of a block — literal run
lengths, match lengths, offsets, where a header lies in the compressed bytes — not on the text.  The greedy encoders the other
tests use (kafka_wire.lz4_block_compress, liblz4) reach most of those branches by luck only; this writer takes the parse as
its input: a random valid parse of the text (``random_parse_frame``), or one the caller states (``encode_sequences``,
``Script``), an all-literal block, and a block padded to a compressed size of exactly 64 KiB (``padded_plan``).

A sequence is ``(literal length, offset, match length)``; a block's closing literal run is ``(literals, 0, 0)``.
"""
import random
import struct

import numpy as np

import kafka_wire as kw

BLOCK = 65536
PERIODS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 255, 256, 300)
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_.~"  # no ':' (the id ends at the key's first colon)
CLASS_CAPS = (8192, 16384, 24576, 32768, 49152, 65536)  # kLz4ClassCap
PARSE_LDS = (6656, 16448)                               # parse_caps of launch_lz4: skew + n_in + 48 on either side of these
EVENT_DTYPE = np.dtype([("type", "<i4"), ("seq", "<i4"), ("raw", "<u8")])  # surge_event16


# ---- the block writer ----------------------------------------------------------------------------------------------------
def _length_bytes(rest):
    """The bytes that continue a length whose nibble is 15 (``rest`` = length - 15)."""
    out = bytearray()
    while rest >= 255:
        out.append(255)
        rest -= 255
    out.append(rest)
    return bytes(out)


def encode_sequences(raw, plan, empty_last=True):
    """The block that decodes to ``raw`` through exactly the sequences of ``plan`` ([(literal length, offset, match length)],
    the closing literal run is whatever is left).  Asserts that the plan reproduces ``raw``.  Returns (block, sequences).
    A parse whose last match runs to the end of ``raw`` closes with the empty sequence (token 0x00)."""
    out = bytearray()
    pos, n = 0, len(raw)
    seqs = []
    for lit, off, ml in plan:
        start = pos + lit
        assert lit >= 0 and ml >= 4 and 1 <= off <= 65535 and off <= start and start + ml <= n, (lit, off, ml, pos, n)
        assert raw[start:start + ml] == raw[start - off:start - off + ml], f"no match of {ml} bytes at {start} with offset {off}"
        out.append((min(lit, 15) << 4) | min(ml - 4, 15))
        if lit >= 15:
            out += _length_bytes(lit - 15)
        out += raw[pos:start]
        out += struct.pack("<H", off)
        if ml - 4 >= 15:
            out += _length_bytes(ml - 4 - 15)
        seqs.append((lit, off, ml))
        pos = start + ml
    lit = n - pos
    if lit > 0 or empty_last:
        out.append(min(lit, 15) << 4)
        if lit >= 15:
            out += _length_bytes(lit - 15)
        out += raw[pos:]
        seqs.append((lit, 0, 0))
    return bytes(out), seqs


def plan_from_matches(matches):
    """[(start, offset, match length)] in the decoded text -> the plan (literal runs fill the gaps)."""
    plan, pos = [], 0
    for start, off, ml in sorted(matches):
        assert start >= pos, (start, pos)
        plan.append((start - pos, off, ml))
        pos = start + ml
    return plan


def frame_of_blocks(blocks):
    """A kafka-shaped LZ4 frame (FLG 0x60: version 01, independent blocks; BD 0x40: 64 KiB) of [(body, stored)]."""
    out = bytearray(struct.pack("<I", 0x184D2204)) + bytes([0x60, 0x40, kw.header_checksum(bytes([0x60, 0x40]))])
    for body, stored in blocks:
        assert 0 < len(body) <= BLOCK
        out += struct.pack("<I", len(body) | (0x80000000 if stored else 0)) + body
    return bytes(out + struct.pack("<I", 0))


def _common_prefix(raw, a, b, limit):
    k = 0
    while k < limit:
        s = min(256, limit - k)
        if raw[a + k:a + k + s] != raw[b + k:b + k + s]:
            break
        k += s
    while k < limit and raw[a + k] == raw[b + k]:
        k += 1
    return k


def _draw_literal_run(rng):
    r = rng.random()
    if r < 0.30:
        return 0
    if r < 0.40:
        return 12
    if r < 0.50:
        return 13
    if r < 0.57:
        return 15
    if r < 0.62:
        return 270 + rng.randrange(40)
    if r < 0.85:
        return rng.randrange(1, 12)
    return rng.randrange(14, 60)


_LENGTHS = (18, 19, 20, 63, 64, 65, 256, 256, 256, 257, 257, 257, 258, 269, 270, 273, 273, 273, 274, 400, 524, 528, 529)


def _draw_match_length(rng, longest):
    r = rng.random()
    if r < 0.30:
        return rng.randrange(4, min(longest, 24) + 1)
    if r < 0.65:
        fits = [m for m in _LENGTHS if m <= longest]
        return rng.choice(fits) if fits else longest
    if r < 0.80:
        return longest
    return rng.randrange(4, longest + 1)


def random_parse(raw, rng, mapped=False):
    """A random valid parse of one block: every earlier position of a 4-gram is a candidate (not only the nearest), the
    length is drawn between 4 and the longest possible; liblz4's end rules hold (the last 5 bytes are literals, no match
    starts within the last 12 bytes).  ``mapped``: only what lz4_exec_kernel's mapped route takes — matches that do not
    overlap, of at most 256 bytes, short enough that 64 sequences span less than 2048 bytes (the shape of compressed text:
    the route nearly every block of a real topic goes, and a parse drawn freely almost never does)."""
    n = len(raw)
    plan = []
    table = {}
    anchor = i = known = 0
    draw_run = (lambda: rng.choice((0, 0, 0, 1, 2, 3, 5, 12, 13))) if mapped else (lambda: _draw_literal_run(rng))
    want = draw_run()
    while i <= n - 12 - 4:
        while known < i:
            table.setdefault(raw[known:known + 4], []).append(known)
            known += 1
        cands = table.get(raw[i:i + 4]) if i - anchor >= want else None
        if cands and mapped:
            cands = [c for c in cands[-64:] if i - c >= 4]
        if not cands:
            i += 1
            continue
        c = cands[-1] if rng.random() < 0.4 else rng.choice(cands)
        longest = _common_prefix(raw, c, i, n - 5 - i)
        if mapped:
            ml = rng.randrange(4, min(longest, i - c, rng.choice((8, 16, 40, 256))) + 1)
        else:
            ml = _draw_match_length(rng, longest)
        plan.append((i - anchor, i - c, ml))
        i += ml
        anchor = i
        want = draw_run()
    return plan


def random_parse_frame(raw, rng, mapped=False):
    """(frame, sequences): ``raw`` in independent 64 KiB blocks, each a random valid parse (``random_parse``); a block that
    does not shrink is stored, as every writer of the format does.  The sequences of all compressed blocks, in order."""
    blocks, seqs = [], []
    for s in range(0, len(raw), BLOCK):
        chunk = raw[s:s + BLOCK]
        body, sq = encode_sequences(chunk, random_parse(chunk, rng, mapped), empty_last=False)
        if len(body) >= len(chunk):
            blocks.append((chunk, True))
        else:
            blocks.append((body, False))
            seqs += sq
    return frame_of_blocks(blocks), seqs


def groups_of(seqs):
    """[(first output byte, end, mapped)] of every group of 64 table entries of lz4_exec_kernel, block after block (a block's
    sequences end with its closing literal run; an empty one has no entry): mapped = the group spans at most 2048 bytes and
    holds no overlapping match and none above 256 bytes."""
    out, ents, pos = [], [], 0
    for lit, off, ml in seqs:
        if lit or ml:
            ents.append((pos, pos + lit + ml, off, ml))
        pos += lit + ml
        if ml == 0:
            for g in range(0, len(ents), 64):
                grp = ents[g:g + 64]
                out.append((grp[0][0], grp[-1][1], grp[-1][1] - grp[0][0] <= 2048 and not any(m and (o < m or m > 256) for _, _, o, m in grp)))
            ents, pos = [], 0
    return out


def padded_plan(raw, stop):
    """A parse of raw[:stop] out of sequences of 15 literals + a 4-byte match (19 bytes in, 19 out) and of 270 literals + a
    4-byte match (275 in, 274 out): a block that does not shrink, for a compressed size of exactly 64 KiB."""
    table, plan = {}, []
    pos = known = 0
    while True:
        for lit in (15, 270):
            at = pos + lit
            if at + 4 > stop:
                continue
            while known < at:
                table.setdefault(raw[known:known + 4], []).append(known)
                known += 1
            cands = table.get(raw[at:at + 4])
            if cands:
                plan.append((lit, at - cands[-1], 4))
                pos = at + 4
                break
        else:
            return plan


# ---- content: records whose decoded bytes are observable ----------------------------------------------------------------------
def event(ty, seq, arg, raw=None):
    e = np.zeros(1, dtype=EVENT_DTYPE)
    e["type"], e["seq"], e["raw"] = ty, seq, np.uint64(np.uint32(np.int32(arg))) if raw is None else np.uint64(raw)
    return e.tobytes()


def letters(rng, n):
    return bytes(rng.choice(ALPHABET) for _ in range(n))


def periodic_id(rng, length=None, period=None):
    period = period or rng.choice(PERIODS)
    length = length or rng.randrange(1, 801)
    return (letters(rng, period) * (length // period + 1))[:length]


class Script:
    """An id written the way a decoder reads it: literal runs and matches.  The text follows from the matches, so the
    stated parse is valid by construction (``encode_sequences`` checks it again)."""

    def __init__(self, rng):
        self.rng, self.buf, self.matches = rng, bytearray(), []

    def lit(self, k):
        self.buf += letters(self.rng, k)
        return self

    def match(self, off, ml):
        start = len(self.buf)
        assert 1 <= off <= start
        for i in range(ml):
            self.buf.append(self.buf[start - off + i])
        self.matches.append((start, off, ml))
        return self


class Topic:
    """The test's own source list — ids, 16-byte events, offsets — and the wire bytes written from it, batch by batch."""

    def __init__(self):
        self.ids, self.events, self.batches, self.names = [], [], [], []
        self.frames = []     # (name, frame, raw, sequences, obeys liblz4's end rules) of every LZ4 batch
        self.sequences = []  # of every compressed block, in order

    @property
    def n(self):
        return len(self.ids)

    @property
    def wire(self):
        return b"".join(self.batches)

    def keys(self):
        return [i.decode() for i in dict.fromkeys(self.ids)]

    def agg(self):
        index = {k: a for a, k in enumerate(dict.fromkeys(self.ids))}
        return np.array([index[i] for i in self.ids], np.int64)

    def event_bytes(self):
        return b"".join(self.events)

    def records(self, recs, skip=0):
        """[(id, event, headers)] -> kafka_wire records with keys <id>:<offset>"""
        return [(i + b":%d" % (self.n + skip + j), v, h) for j, (i, v, h) in enumerate(recs)]

    def section(self, recs, skip=0):
        """The records section ``recs`` would make as the next batch (from its ``skip``-th record on)."""
        return b"".join(kw.record(skip + j, *r) for j, r in enumerate(self.records(recs, skip)))

    def add(self, name, recs, writer=None, end_rules=True):
        """One batch of ``recs``.  ``writer``: None = uncompressed, else raw -> (frame, sequences)."""
        def compressor(raw):
            frame, seqs = writer(raw)
            self.frames.append((name, frame, raw, seqs, end_rules))
            self.sequences += seqs
            return frame

        self.batches.append(kw.record_batch(self.n, self.records(recs), compression="lz4" if writer else "none", compressor=compressor if writer else None))
        self.names += [name] * len(recs)
        self.ids += [i for i, _, _ in recs]
        self.events += [v for _, v, _ in recs]


def random_records(rng, n_bytes, repeat=0.3):
    """About ``n_bytes`` of records: ids of 1 .. 800 bytes with the designed periods (some ids come back), random events."""
    recs, ids, size = [], [], 0
    while size < n_bytes:
        i = rng.choice(ids) if ids and rng.random() < repeat else periodic_id(rng)
        ids.append(i)
        recs.append((i, event(rng.choice([0, 1, 2]), rng.randrange(1 << 31), rng.randrange(-1000, 1000)), []))
        size += len(i) + 35
    return recs


def sized_records(rng, size, topic, tail=None, skip=0):
    """Records whose section is exactly ``size`` bytes long: a header value of random bytes in the last but ``len(tail)``
    records is tuned, as tests/test_ingest_gpu.py tunes its 65536-byte section."""
    recs = random_records(rng, size - 1500) if size > 2200 else []
    tail = tail or []
    hv_len = max(0, size - len(topic.section(recs + [(b"pad", event(1, 1, 1), [(b"h", b"")])] + tail, skip)))
    for _ in range(8):
        pad = (b"pad", event(1, 7, 7), [(b"h", rng.randbytes(hv_len))])
        got = len(topic.section(recs + [pad] + tail, skip))
        if got == size:
            return recs + [pad] + tail
        hv_len += size - got
        assert hv_len >= 0, (size, got)
    raise AssertionError(f"no section of {size} bytes")


# ---- a: random parses ------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = (1, 2, 3)
MAPPED_SEEDS = (11, 12)


def fuzz_topic(seed, mapped=False):
    """About 150 KB of records in batches of 1 .. 400 records, every batch one frame of random parses."""
    rng = random.Random(seed)
    t = Topic()
    recs = random_records(rng, 150_000)
    at = 0
    sizes = [1, 200, 3, 40, 400]  # (about 350 records in all: one, a frame of two blocks, small ones, and the rest)
    while at < len(recs):
        n = sizes[len(t.batches) % 5]
        t.add(f"fuzz {seed} batch at {at}", recs[at:at + n], lambda raw: random_parse_frame(raw, rng, mapped))
        at += n
    return t


def stated(plan_of):
    """A writer of ONE block with the parse ``plan_of(raw)`` states."""
    def write(raw):
        assert len(raw) <= BLOCK
        body, seqs = encode_sequences(raw, plan_of(raw))
        return frame_of_blocks([(body, False)]), seqs
    return write


def scripted(script):
    """... with the matches of ``script``, whose text is the id of the batch's first record."""
    def plan_of(raw):
        at = raw.index(bytes(script.buf))
        return plan_from_matches([(at + s, o, m) for s, o, m in script.matches])
    return stated(plan_of)


def _one(topic, rng, name, script):
    topic.add(name, [(bytes(script.buf), event(rng.choice([0, 1, 2]), rng.randrange(1 << 31), rng.randrange(-1000, 1000)), [])], scripted(script))


# ---- b: forced sequence edges ------------------------------------------------------------------------------------------------
def tile_plan(raw, rng, spans, per_group=64):
    """A parse whose k-th group of ``per_group`` sequences spans exactly spans[k] bytes of output, out of matches that
    lz4_exec_kernel's mapped route takes (offset >= length, length <= 256)."""
    table, plan = {}, []
    pos = known = 0

    def candidates(at):
        nonlocal known
        while known < at:
            table.setdefault(raw[known:known + 4], []).append(known)
            known += 1
        return table.get(raw[at:at + 4], [])

    for span in spans:
        end = pos + span
        for left in range(per_group, 0, -1):
            want = end - pos if left == 1 else max(4, (end - pos) // left)
            placed = False
            for size in ([want] if left == 1 else range(want, end - pos + 1)):
                if end - (pos + size) < 4 * (left - 1):
                    break
                for ml in sorted(range(4, min(size, 256) + 1), key=lambda m: rng.random()):
                    at = pos + size - ml
                    fit = [c for c in candidates(at) if at - c >= ml and raw[c:c + ml] == raw[at:at + ml]]
                    if fit:
                        plan.append((size - ml, at - rng.choice(fit), ml))
                        pos += size
                        placed = True
                        break
                if placed:
                    break
            assert placed, (span, left, pos)
        assert pos == end
    return plan


def forced_topics():
    """{name: Topic}: one frame per case, the cases of one kind in one topic (one push)."""
    rng = random.Random(77)
    out = {}
    # literal runs 11 .. 16 in front of a match (12 | 13: the last run a "simple header" of pass 1 holds)
    t = out["literal runs"] = Topic()
    for k in (11, 12, 13, 14, 15, 16):
        for ml in (8, 40):  # offset k + 8: not overlapping, overlapping
            _one(t, rng, f"literal run {k}, match {ml}", Script(rng).lit(4).match(4, 4).lit(k).match(k + 8, ml).lit(9))
    # match lengths around one and two extension bytes (19 = 15 + 4: the first with an extension byte; 274 = 19 + 255, 529 = 19 + 2 x 255)
    t = out["match lengths"] = Topic()
    for ml in (18, 19, 20, 269, 270, 273, 274, 524, 528, 529):
        _one(t, rng, f"match {ml}, offset 13", Script(rng).lit(4).match(4, 4).lit(5).match(13, ml).lit(7))
        far = ml + 3 if ml < 300 else 262  # (an id is at most 800 bytes: the longest do overlap)
        _one(t, rng, f"match {ml}, offset {far}", Script(rng).lit(far).match(far, ml).lit(7))
    # a sequence whose header starts at bytes 60 .. 63 of a 64-byte window of the compressed block: chains of short
    # sequences (3 + literals bytes each) walk the parse up to it, window after window
    t = out["window ends"] = Topic()
    for lane in (60, 61, 62, 63):
        for kinds in (((0, 4), (12, 4), (13, 4), (5, 19)), ((12, 4), (0, 18), (15, 4), (1, 300))):
            s = Script(rng).lit(4)
            # the first sequence: the record's first 7 bytes and these 4 as literals, then 4 matched bytes: 11 + 3 bytes in
            s.match(4, 4)
            at = 14
            for w, (lit, ml) in enumerate(kinds):
                target = 64 * (w + 1) + lane
                while target - at > 18:
                    s.lit(5).match(rng.randrange(4, 9), 4)
                    at += 8
                for size in ([target - at] if target - at <= 15 else [9, target - at - 9]):
                    s.lit(size - 3).match(rng.randrange(4, 9), 4)
                    at += size
                s.lit(lit).match(4 if ml < 100 else 9, ml)
                at += 3 + lit + (1 if lit >= 15 else 0) + (1 if ml >= 19 else 0) + (1 if ml >= 274 else 0)
            _one(t, rng, f"headers at byte {lane} of a window, {kinds}", s.lit(6))
    # matches of 256 and of 257 bytes at offset >= 257 (the longest the map takes | the first that goes sequence by sequence)
    t = out["256 and 257"] = Topic()
    for ml in (256, 257):
        for off in (257, 300, 500):
            _one(t, rng, f"match {ml}, offset {off}", Script(rng).lit(off).match(off, ml).lit(3))
    # chains: k back-to-back matches of 4 .. 8 bytes at offsets 4 .. 12 that do not overlap
    t = out["chains"] = Topic()
    for k in list(range(1, 13)) + [40, 90]:
        s = Script(rng).lit(12)
        for _ in range(k):
            ml = rng.randrange(4, 9)
            s.match(rng.randrange(max(ml, 4), 13), ml)
        _one(t, rng, f"chain of {k}", s.lit(2))
    # overlapping matches of every designed period: 1 .. 63 through src[i % O], 64 and above through the chunked copy
    for name, periods in (("overlaps below 64", PERIODS[:11]), ("overlaps from 64", PERIODS[11:])):
        t = out[name] = Topic()
        for p in periods:
            for ml in sorted({max(p + 1, 4), 63, 64, 65, 300, 2000}):
                if ml > p:  # (the 2000-byte runs need ids longer than the 800 bytes of the other inputs)
                    _one(t, rng, f"period {p}, match {ml}", Script(rng).lit(p).match(p, ml).lit(5))
    # the last match's header starts 16 .. 20 bytes before the block's end (16: the 16-byte window a lane of pass 1 loads ends
    # exactly there): the match is the first half of the event, which the record before carries too; 9 literals close the block
    t = out["block ends"] = Topic()
    for j in range(5):
        same = event(1, 1000 + j, j)
        s = Script(rng).lit(9).match(5, 5).lit(j)
        recs = [(letters(rng, 20), same, []), (bytes(s.buf), same, [])]

        def plan_of(raw, s=s, same=same):
            at, value = raw.index(bytes(s.buf)), len(raw) - 17
            return plan_from_matches([(at + a, o, m) for a, o, m in s.matches] + [(value, value - raw.index(same), 8)])

        t.add(f"last header {16 + j} bytes before the end", recs, stated(plan_of))
    # 64 consecutive sequences whose output spans exactly 2048 bytes (the map's size) | 2049; the group behind them then
    # lies across a multiple of 2048: the map wraps
    t = out["group spans"] = Topic()
    for spans in ((2048, 2048), (2049, 2047), (1500, 2048), (2048 - 7, 2049)):
        same = letters(rng, 300)
        recs = [(letters(rng, 3) + same + same, event(1, j, j), []) for j in range(8)]
        t.add(f"groups of 64 sequences spanning {spans}", recs, stated(lambda raw, spans=spans: tile_plan(raw, rng, spans)))
    return out


def matches_of(plan):
    out, pos = [], 0
    for lit, off, ml in plan:
        out.append((pos + lit, off, ml))
        pos += lit + ml
    return out


def full_block_topics():
    """Blocks of exactly 65536 decoded bytes whose last match ends at the block's end (an empty closing sequence: liblz4 writes
    no such block and refuses it; the project's host decoder takes it), one of them with the largest offset a 64 KiB block can
    reach: 65532 (a match is at least 4 bytes long and the block holds 65536, so 65535 is out of reach)."""
    out = {}
    for name in ("match to the end", "offset 65532"):
        rng = random.Random(78)
        t = out[name] = Topic()
        if name == "offset 65532":
            first = [(b"a", event(1, 5, 5), [])]
            assert t.section(first)[:4] == bytes([50, 0, 0, 0])  # the record's length (zig-zag 25), attributes, two deltas
            last = (periodic_id(rng, 40, 7), event(2, 9, 0, raw=(50 << 40) | 77), [])  # the section ends 32 00 00 | 00 (no headers)
            closing = (BLOCK - 4, BLOCK - 4, 4)
        else:
            first = [(periodic_id(rng, 90, 3), event(0, 3, 0, raw=0x1122334455667788), [])]
            last = (periodic_id(rng, 33, 2), event(2, 4, 0, raw=0x1122334455667788), [])  # the same 8 bytes and the empty header list
            closing = (BLOCK - 9, BLOCK - len(t.section(first)), 9)
        recs = first + sized_records(rng, BLOCK - len(t.section(first)), t, tail=[last], skip=1)
        assert len(t.section(recs)) == BLOCK

        def plan_of(raw, closing=closing, rng=rng):
            return plan_from_matches(matches_of(random_parse(raw[:BLOCK - 64], rng)) + [closing])

        t.add(name, recs, stated(plan_of), end_rules=False)
    return out


# ---- c: size classes -----------------------------------------------------------------------------------------------------
# C and C + 1 of every class, and C + 2: a section ends with its last record's 16-byte event and the one byte of its empty
# header list, which no decoder output shows — at C + 1 the event ends with the class's last byte, at C + 2 it lies across the
# capacity.  65537 / 65538 / 65545: two blocks, the second holding that byte alone / behind 1 / behind 8 bytes of the event.
SIZES = tuple(s for c in CLASS_CAPS[:-1] for s in (c, c + 1, c + 2)) + (65535, 65536, 65537, 65538, 65545)


def size_class_topic():
    """One frame of random parses per size.  The section's LAST record has no headers (its event lies at the block's end:
    the bytes a wrong size class or a short copy-out loses); the header value tuned to reach the size lies in front of it."""
    rng = random.Random(79)
    t = Topic()
    for size in SIZES:
        last = (periodic_id(rng, rng.randrange(30, 60)), event(rng.choice([0, 1, 2]), rng.randrange(1 << 31), 0, raw=rng.getrandbits(64)), [])
        t.add(f"decoded size {size}", sized_records(rng, size, t, tail=[last]), lambda raw: random_parse_frame(raw, rng))
    return t


# ---- d: LDS classes of pass 1 ----------------------------------------------------------------------------------------------
def records_of_length(rng, topic, length, ident=b"k"):
    """Records (one; two where a varint's step leaves no single record of that size) whose uncompressed section is exactly
    ``length`` bytes: a header value of random bytes, and the id's length for the smallest."""
    def ev():
        return event(rng.choice([0, 1, 2]), rng.randrange(1 << 31), rng.randrange(-1000, 1000))

    for extra in range(0, 6):
        rec = (ident + letters(rng, extra), ev(), [])
        base = len(topic.section([rec]))
        if base == length:
            return [rec]
        hv_len = length - base - 3
        for _ in range(4):
            if hv_len < 0:
                break
            got = len(topic.section([rec[:2] + ([(b"h", bytes(hv_len))],)]))
            if got == length:
                return [rec[:2] + ([(b"h", rng.randbytes(hv_len))],)]
            hv_len += length - got
    second = (ident, ev(), [])
    for hv_len in range(max(0, length - 80), length):
        recs = [(ident, ev(), [(b"h", rng.randbytes(hv_len))]), second]
        if len(topic.section(recs)) == length:
            return recs
    raise AssertionError(f"no section of {length} bytes")


def smallest_record(topic):
    return len(topic.section([(b"k", event(0, 0, 0), [])]))


def literal_block_writer(n_in):
    """One block of compressed size exactly ``n_in``: all literals (one closing sequence: len(raw) + 1 + extension bytes) —
    or, where the extension bytes step over n_in, literals around one 4-byte match."""
    def write(raw):
        body, seqs = encode_sequences(raw, [])
        if len(body) != n_in:
            at = raw.index(b"\x01\x02\x03\x04\x01\x02\x03\x04") + 4
            body, seqs = encode_sequences(raw, [(at, 4, 4)])
        assert len(body) == n_in, (len(body), n_in)
        return frame_of_blocks([(body, False)]), seqs
    return write


def lds_class_topic():
    """Blocks of random bytes with skew + n_in + 48 equal to the LDS of a launch of pass 1 and one above it, for every skew
    0 .. 15 (n_in = cap - 48 - skew and one more: [cap - 63, cap - 47]), in ONE push: a filler batch in front of each puts the block's
    first byte at the skew it is meant for (sections lie back to back in the arena; a block starts 11 bytes into its frame)."""
    rng = random.Random(80)
    t = Topic()
    at = 0  # where the next section starts
    expect = []  # (skew, n_in) of every block
    for cap in PARSE_LDS:
        for skew in range(16):
            for n_in in (cap - 48 - skew, cap - 48 - skew + 1):
                fill = smallest_record(t) + (skew - 11 - at - smallest_record(t)) % 16
                t.add("filler", records_of_length(rng, t, fill))
                at += fill
                # the record whose all-literal block is n_in bytes long
                rec = None
                last = (b"end", event(2, n_in, 0, raw=rng.getrandbits(64)), [])  # (no headers: the block ends with an event)
                for form in (b"", b"\x01\x02\x03\x04\x01\x02\x03\x04"):
                    hv_len = n_in - 100
                    for _ in range(8):
                        cand = (b"lds", event(1, skew, n_in), [(b"h", form + rng.randbytes(hv_len))])
                        raw = t.section([cand, last])
                        got = len(encode_sequences(raw, [(raw.index(form) + 4, 4, 4)] if form else [])[0])
                        if got == n_in:
                            rec = cand
                            break
                        hv_len += n_in - got
                    if rec:
                        break
                assert rec, n_in
                t.add(f"skew {skew}, n_in {n_in}", [rec, last], literal_block_writer(n_in))
                expect.append((skew, n_in, at))
                at += n_in + 15  # frame header, size word, block, EndMark
    t.expect = expect
    return t


# ---- e: the compressed path of lz4_block_kernel -------------------------------------------------------------------------------
def padded_blocks(raw, stored_first):
    head, chunk = (raw[:BLOCK], raw[BLOCK:]) if stored_first else (b"", raw)
    stop = chunk.index(b"pad:")  # the last two records are the closing literal run
    body, seqs = encode_sequences(chunk, padded_plan(chunk, stop - 8))
    return ([(head, True)] if stored_first else []) + [(body, False)], seqs


def padded_writer(stored_first):
    def write(raw):
        blocks, seqs = padded_blocks(raw, stored_first)
        return frame_of_blocks(blocks), seqs
    return write


def padded_topics():
    """A frame whose only block has a COMPRESSED size of exactly 65536, and one whose first block is stored and full and whose
    second is such a block: lz4_plan_section hands a block of 65536 bytes or more to lz4_block_kernel."""
    out = {}
    for name, stored_first in (("one padded block", False), ("stored block, padded block", True)):
        rng = random.Random(81 + stored_first)
        t = out[name] = Topic()
        head = []
        if stored_first:
            while len(t.section(head)) < BLOCK + 100:
                head.append((periodic_id(rng, rng.randrange(1, 60)), event(1, len(head), 3), [(b"h", rng.randbytes(rng.randrange(3000)))]))
        body = [(periodic_id(rng, rng.randrange(600, 801), rng.choice(PERIODS[:6])), event(rng.choice([0, 1, 2]), rng.randrange(1 << 31), 5), []) for _ in range(76)]
        write = padded_writer(stored_first)
        last = (periodic_id(rng, 50, 5), event(1, 4, 0, raw=rng.getrandbits(64)), [])  # (no headers: the block ends with an event)
        hv_len = 2000
        for _ in range(12):
            recs = head + body + [(b"pad", event(2, 2, 2), [(b"h", rng.randbytes(hv_len))]), last]
            got = len(padded_blocks(t.section(recs), stored_first)[0][-1][0])
            if got == BLOCK:
                break
            hv_len += BLOCK - got
        assert got == BLOCK, got
        t.add(name, recs, write)
    return out


# ---- f: CRC-32C length and alignment sweep ---------------------------------------------------------------------------------
CRC_TILE = 4096
CRC_REMAINDERS = tuple(range(0, 9)) + tuple(range(60, 69)) + tuple(range(4088, 4096))


def crc_lengths(covered_header, smallest):
    """The section lengths of the sweep: every length from the smallest record to 160, then, for 1, 2 and 3 tiles, every
    length whose remainder mod 4096 — counted over what the device runs the CRC over: the section, and in WIRE mode the 40
    covered header bytes in front of it — is in CRC_REMAINDERS."""
    out = set(range(smallest, 161))
    for tiles in (1, 2, 3):
        for rem in CRC_REMAINDERS:
            span = (tiles - 1) * CRC_TILE + (rem or CRC_TILE)
            if span - covered_header >= smallest:
                out.add(span - covered_header)
    return sorted(out)


def crc_topic(covered_header, shift):
    """One uncompressed one-record batch per length of the sweep, behind a filler batch that is ``shift`` bytes longer than
    the smallest batch: 0 .. 3 put every section at each of the four alignments."""
    rng = random.Random(82 + covered_header)  # (the same records whatever the shift)
    t = Topic()
    small = smallest_record(t)
    t.add("filler", records_of_length(random.Random(shift), t, small + shift, ident=b"f"))
    t.lengths = crc_lengths(covered_header, small)
    for length in t.lengths:
        t.add(f"section of {length} bytes", records_of_length(rng, t, length))
    return t
