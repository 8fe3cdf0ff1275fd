"""TEST INFRASTRUCTURE: inputs for the WRITING side of the device's LZ4 path (surge_amd/csrc/frame_lz4.hip:
frame_lz4_block_kernel, frame_lz4_pack_kernel and the uncompressed framer under them), built on the CPU, next to
tests/lz4_seqgen.py, which does the same for the reading side.

What is here:
  * section() / value_for_section_size() / value_for_layout(): framer inputs whose records sections, with ONE RECORD PER
    BATCH, are ``head + value + 0x00`` -- so an LZ4 block's content is the test's own bytes apart from a short head and one
    trailing byte, and a value beyond 64 KiB gives middle blocks that are payload only;
  * the named cases of tests/test_lz4_blockgen.py (CPU: every case reaches the edge it is named for) and
    tests/test_frame_lz4_edges_gpu.py (GPU: the device's output for the same inputs): CASES;
  * wave_compress(): the scheme of frame_lz4_block_kernel's header comment restated on the CPU -- a MODEL, not an oracle;
  * the walkers of LZ4 frames and blocks, a plain block decoder, and check_against_uncompressed(), the routine every GPU
    test of the LZ4 mode rests on (moved here from tests/test_frame_lz4_gpu.py, which imports them).
"""
import functools
import struct

import numpy as np

import kafka_wire as kw

FRAME_HEAD = bytes([0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82])
BLOCK = 65536
SMALL = 4096                      # blocks up to this size are compressed with the small hash table
HASH_LOG_SMALL, HASH_LOG = 11, 13


def hash_log_for(n):
    return HASH_LOG_SMALL if n <= SMALL else HASH_LOG


def pa_lz4():
    """pyarrow when it is there and bundles liblz4's frame codec, else None."""
    try:
        import pyarrow as pa
    except ImportError:
        return None
    return pa if pa.Codec.is_available("lz4") else None


# ---- inputs ---------------------------------------------------------------------------------------------------------
def build_input(records):
    """The framer input ``(kind, part, keys, key_off, vals, val_off)`` of ``[(kind, partition, key, value)]``, kind 0 = a
    skipped aggregate (it keeps its key, and shifts every offset behind it), 1 = a value, 2 = a tombstone."""
    n = len(records)
    kind = np.array([r[0] for r in records], np.uint8)
    part = np.array([r[1] for r in records], np.int32)
    keys = [r[2] for r in records]
    values = [r[3] if r[0] == 1 else b"" for r in records]
    key_off = np.zeros(n + 1, np.int64); np.cumsum([len(k) for k in keys], out=key_off[1:])
    val_off = np.zeros(n + 1, np.int64); np.cumsum([len(v) for v in values], out=val_off[1:])
    kb = np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy()
    vb = np.frombuffer(b"".join(values) or b"\0", np.uint8).copy()
    return kind, part, kb, key_off, vb, val_off


def host_frames(writer, inp, ts):
    """``{partition: bytes}`` of one publish through a RecordBatchWriter."""
    writer.reset()
    writer.append(*inp, ts)
    out = {}
    for p in range(writer.n_partitions):
        data, nrec, _ = writer.partition_bytes(p)
        if nrec:
            out[p] = data
    return out


def device_frames(framer, inp, ts):
    """``{partition: bytes}`` of one publish through a DeviceFramer on cuda:0."""
    import torch

    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a).to(dev) for a in inp]
    torch.cuda.synchronize(dev)
    return {p: bytes(v) for p, v in framer.frame(*t, timestamp_ms=ts).items()}


def section(values, key=b"k", part=None, n_part=1):
    """``(inp, sections)``: the framer input ``(kind, part, keys, key_off, vals, val_off)`` for the given values (bytes
    each; None = a tombstone) and the records sections the host writer produces for them with max_records_per_batch = 1:
    ``kafka_wire.record(0, key, value)`` each.  ``key``: one for all, or one per value; ``part``: a partition per value
    (default: all in partition 0)."""
    n = len(values)
    keys = [key] * n if isinstance(key, (bytes, bytearray)) else list(key)
    assert len(keys) == n
    part = [0] * n if part is None else [int(p) for p in part]
    assert len(part) == n and all(0 <= p < n_part for p in part)
    inp = build_input([(2 if v is None else 1, p, k, v) for p, k, v in zip(part, keys, values)])
    return inp, [kw.record(0, k, v) for k, v in zip(keys, values)]


def value_for_layout(n, layout, key=b"k"):
    """A value whose one-record section is exactly ``n`` bytes long: ``layout(h)`` gives the n - 1 - h bytes that follow a
    head of h bytes (the section's last byte is the record's empty header list, 0x00).  The length prefixes grow at 64 /
    8192 / 2^20, so h is solved for; raises ValueError where no value length gives n with this key (the section grows by
    two bytes where a prefix grows)."""
    for h in range(6 + len(key), 14 + len(key)):
        if n - 1 - h < 0:
            break
        v = layout(h)
        assert len(v) == n - 1 - h, (len(v), n, h)
        if len(kw.record(0, key, v)) == n:
            return v
    raise ValueError(f"no value gives a section of {n} bytes with a key of {len(key)} bytes")


def value_for_section_size(n, fill, key=b"k"):
    """``fill(L)`` gives a value of L bytes; the L for which the one-record section is exactly ``n`` bytes long."""
    return value_for_layout(n, lambda h: fill(n - 1 - h), key)


def record_for_section_size(n, fill):
    """``(key, value)``: value_for_section_size with the first key of b"k", b"kk", b"kkk" that can reach n."""
    for key in (b"k", b"kk", b"kkk"):
        try:
            return key, value_for_section_size(n, fill, key)
        except ValueError:
            pass
    raise ValueError(n)


def blocks_of(sec):
    return [sec[i:i + BLOCK] for i in range(0, len(sec), BLOCK)]


def rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def zeros(n):
    return bytes(n)


PERIOD7 = bytes(range(0xF1, 0xF8))


def periodic(pattern):
    return lambda n: (pattern * (n // len(pattern) + 1))[:n]


# ---- the named cases: each returns [(key, value)], one record per batch, one partition -------------------------------
# (no ONE record has a section of 65 bytes: a body of 63 bytes gives 64, a body of 64 takes a second length byte and gives
# 66.  65 is the two-record batch of pair_for_section_size.)
PAIR_SIZES = [65]
BLOCK_SIZES = [n for n in list(range(8, 81)) + list(range(4090, 4101)) + list(range(65530, 65541)) + list(range(131070, 131075))
               if n not in PAIR_SIZES]


def case_block_sizes(fill):
    """Sections of every size in BLOCK_SIZES of one fill: blocks of 12 bytes and fewer, last windows with only some
    lanes active, both sides of the size-class split, 65536 / 65537 (a next block of one byte), two and three blocks."""
    return [record_for_section_size(n, fill) for n in BLOCK_SIZES]


def pair_for_section_size(n, fill):
    """``(records, section)``: two records of ONE batch (max_records_per_batch = 2) whose records section is n bytes: an
    8-byte record without a value, then the fill."""
    first = kw.record(0, b"k", b"")
    for L in range(n):
        sec = first + kw.record(1, b"k", fill(L))
        if len(sec) == n:
            return [(b"k", b""), (b"k", fill(L))], sec
    raise ValueError(n)


LITERAL_LENGTHS = list(range(0, 41)) + list(range(240, 301)) + list(range(16320 - 96, 16320 + 96))
PRIMED_LITERAL_LENGTHS = list(range(0, 41)) + list(range(250, 290)) + list(range(16335 - 32, 16335 + 32))


def case_literal_runs(seed=11):
    """L random bytes, then 3000 zeros.  The zeros begin inside a window of new content, so the first match starts at the
    next window: the literal run is the next multiple of 64 (hence a sweep, not a hand-placed length).  16320 has 64
    length bytes, 16384 has 65.  The 'primed' records put 100 zeros in front: the table then knows the zeros, the match
    begins with them, and the literal run is L itself -- both sides of 15, 270 and 16335 exactly."""
    rng = np.random.default_rng(seed)
    out = [(b"k", rnd(rng, L) + zeros(3000)) for L in LITERAL_LENGTHS]
    out += [(b"k", zeros(100) + rnd(rng, L) + zeros(3000)) for L in PRIMED_LITERAL_LENGTHS]
    return out


MATCH_LENGTHS = list(range(4, 41)) + list(range(270, 341)) + list(range(16340 - 64, 16340 + 128))


def case_match_lengths(pattern, seed=12):
    """16 random bytes, the pattern repeated to m bytes, 16 random bytes: matches of every length class (no length byte,
    one, two, 64 and 65: 16339 is the first match with 65), as overlapping copies at offset len(pattern).  The match
    begins at the window after the one the run begins in, some 40 bytes into the run (with a period of 64, a window later
    still): hence 270 .. 340 for the step from one length byte to two at 274, and 192 values from 16276 on for the step
    from 64 to 65."""
    rng = np.random.default_rng(seed + len(pattern))
    fill = periodic(pattern)
    return [(b"k", rnd(rng, 16) + fill(m) + rnd(rng, 16)) for m in MATCH_LENGTHS]


def case_whole_blocks():
    """Values of three blocks and a little of 0x00 and of 0xFF: the middle blocks are 65536 equal bytes, one match with
    257 length bytes."""
    return [(b"k", zeros(3 * BLOCK + 100)), (b"k", b"\xff" * (3 * BLOCK + 100))]


END_SIZES = [204, 235, 202]  # n - 11 positions may start a match: 64 k + 1, + 32, + 63 of them: the last window's lanes


def case_block_ends(seed=13):
    """Per n of END_SIZES (the last window has 1, 32 and 63 active lanes): random sections whose ONLY repeat, 7 bytes of
    window 0, begins at n - 12 (the last place a match may start: compressed, 2 bytes saved), at n - 11 (none may: stored)
    and at n - 13; and random + zeros to the end, whose last match is cut at n - 5."""
    rng = np.random.default_rng(seed)
    out = []
    for n in END_SIZES:
        for back in (12, 11, 13):
            def layout(h, n=n, back=back):
                body = bytearray(rnd(rng, n - 1 - h))
                s = n - back - h  # index in the value of section position n - back
                body[s:s + 7] = body[10:17]
                return bytes(body)
            out.append((b"k", value_for_layout(n, layout)))
        for tail in (40, 100):
            out.append((b"k", value_for_layout(n, lambda h, n=n, tail=tail: rnd(rng, n - 1 - h - tail) + zeros(tail))))
    return out


FAR_SIZES = [4096, 4097, 65536]


def case_far_offsets(seed=14):
    """Per n of FAR_SIZES (both hash tables): R + zeros + R with R = 64 random bytes; and sections whose LAST bytes are a
    copy of the section's FIRST bytes, record head included -- the candidate is position 0, which the zero-initialised table
    holds without anybody having inserted it: the last 64 bytes (offset n - 64), and 12 bytes at n - 12, the largest offset
    a block can have (65524 at 64 KiB)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in FAR_SIZES:
        R = rnd(rng, 64)
        out.append((b"k", value_for_layout(n, lambda h: R + zeros(n - 1 - h - 128) + R)))
        for copy in (64, 12):
            def layout(h, n=n, copy=copy):
                front = bytearray(rnd(rng, 64))
                front[copy - 1 - h] = 0  # section[copy - 1] is what the section's last byte, 0x00, is a copy of
                probe = bytes(front) + zeros(n - 1 - h - len(front))
                head = kw.record(0, b"k", probe)[:h]  # the head depends on the value's length alone
                tail = (head + bytes(front))[:copy - 1]
                return bytes(front) + zeros(n - 1 - h - len(front) - len(tail)) + tail
            out.append((b"k", value_for_layout(n, layout)))
    return out


STORED_K = list(range(4, 41))
# A literal run of 60000 bytes has 236 length bytes, which a repeat of 40 bytes never pays for -- and 60000 insertions
# into a table of 8192 entries leave nothing of r's first bytes for the repeat to be found by.  The sweep of r = 60000
# therefore goes on with repeats of what lies 512 bytes back, over the k at which the output (n - k + 242) crosses n.
STORED_K_RECENT = list(range(225, 261))


def case_stored_decision(r_len, seed=15):
    """r + r[:k] + 30 random bytes, r random: the one match of k bytes pays for the length bytes of the literal run in
    front of it only from some k on, so the sweep crosses ``op + need >= n`` byte by byte."""
    rng = np.random.default_rng(seed + r_len)
    out = []
    for k in STORED_K:
        r = rnd(rng, r_len)
        out.append((b"k", r + r[:k] + rnd(rng, 30)))
    if r_len >= 60000:
        for k in STORED_K_RECENT:
            r = rnd(rng, r_len)
            out.append((b"k", r + r[r_len - 512:r_len - 512 + k] + rnd(rng, 30)))
    return out


def protobuf_state(aggregate_id, payload):
    """The multilanguage module's State{aggregateId = 1, payload = 2} as surge_amd/encode.py's "protobuf_state" envelope
    writes it: two length-delimited fields."""
    def uvarint(x):
        out = bytearray()
        while x >= 0x80:
            out.append(x & 0x7F | 0x80)
            x >>= 7
        out.append(x)
        return bytes(out)
    return b"\x0a" + uvarint(len(aggregate_id)) + aggregate_id + b"\x12" + uvarint(len(payload)) + payload


def case_binary(seed=16):
    """All 256 byte values, in runs and in repeats, 0x80 .. 0xFF alone, and protobuf-like states."""
    rng = np.random.default_rng(seed)
    every = bytes(range(256))
    high = bytes(range(0x80, 0x100))
    out = [
        (b"k", every * 20),                                                   # repeats at offset 256
        (b"k", b"".join(bytes([b]) * 37 for b in range(256))),                # runs of every byte value
        (b"k", high * 9 + high[::-1] * 9),
        (b"k", b"".join(bytes([b]) * int(rng.integers(1, 90)) for b in rng.integers(0x80, 0x100, 300))),
        (b"\xff\x00\x80k", bytes(rng.integers(0x80, 0x100, 5000, dtype=np.uint8).tobytes()) + high * 40),
        (b"k", (b"\xff\xfe" * 40000)),                                        # two blocks of a period-2 fill
    ]
    for i in range(40):
        payload = struct.pack("<qdI", -i * 7919, i * 1e300, 0xFFFFFFFF - i) * int(rng.integers(1, 30)) + bytes([0xFF] * int(rng.integers(0, 70)))
        out.append((b"acct-%d" % i, protobuf_state(b"acct-%d" % i, payload)))
    return out


MIXED_LENGTHS = list(range(1000, 1016))


def mixed_value(rng_blocks, t, n_blocks=6, last=30000):
    """One value whose section is ``n_blocks`` blocks: even blocks random (stored), odd blocks a period-5 fill then ``t + k``
    random bytes (one long match from the block's start, then one literal run: t + k bytes and a constant, so the
    compressed size moves byte by byte with t -- random bytes IN FRONT would move it in steps of 64), the last block
    ``last`` bytes long."""
    fill = periodic(b"\x80\x01\xfe\x7f\x00")
    total = (n_blocks - 1) * BLOCK + last

    def layout(h):
        parts = []
        for k in range(n_blocks):
            size = BLOCK if k < n_blocks - 1 else last
            parts.append(rng_blocks[k] if k % 2 == 0 else fill(size - t - k) + rng_blocks[k][:t + k])
            parts[-1] = parts[-1][:size]
        return b"".join(parts)[h:total - 1]
    return value_for_layout(total, layout)


def case_mixed_frames(seed=17):
    """16 values of 6 blocks, stored and compressed blocks alternating; the incompressible tail of the compressed blocks grows byte by byte over
    the 16, so compressed blocks of every size modulo 8 sit behind stored ones (the pack kernel's 8-byte copy and its tail,
    at every alignment).  The random blocks are the same in all 16."""
    rng = np.random.default_rng(seed)
    rb = [rnd(rng, BLOCK) for _ in range(6)]
    return [(b"k", mixed_value(rb, t)) for t in MIXED_LENGTHS]


def case_many_partitions(seed=18, n_part=64):
    """``(records, partitions)``: 64 partitions, every third holding one record of about 300 KiB (5 blocks, mixed), the
    others one 8-byte record: both size classes, two launches, in one block table."""
    rng = np.random.default_rng(seed)
    rb = [rnd(rng, BLOCK) for _ in range(5)]
    big = [mixed_value(rb, 500 + 3 * j, n_blocks=5, last=300 * 1024 - 4 * BLOCK) for j in range(4)]
    recs = [(b"k", big[p % 4] if p % 3 == 0 else b"") for p in range(n_part)]
    return recs, list(range(n_part))


CASES = {
    "block_sizes_zeros": lambda: case_block_sizes(zeros),
    "block_sizes_period7": lambda: case_block_sizes(periodic(PERIOD7)),
    "literal_runs": case_literal_runs,
    "match_lengths_byte": lambda: case_match_lengths(b"\xc3"),
    "match_lengths_period3": lambda: case_match_lengths(b"\x01\xfe\x80"),
    "match_lengths_period64": lambda: case_match_lengths(bytes(range(0xA0, 0xE0))),
    "whole_blocks": case_whole_blocks,
    "block_ends": case_block_ends,
    "far_offsets": case_far_offsets,
    "stored_decision_300": lambda: case_stored_decision(300),
    "stored_decision_2000": lambda: case_stored_decision(2000),
    "stored_decision_60000": lambda: case_stored_decision(60000),
    "binary": case_binary,
    "mixed_frames": case_mixed_frames,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """``(records, inp, sections)`` of a named case, built once."""
    records = CASES[name]()
    inp, sections = section([v for _, v in records], [k for k, _ in records])
    return records, inp, sections


# ---- the model ------------------------------------------------------------------------------------------------------
def _len_bytes(x):
    return (x - 15) // 255 + 1 if x >= 15 else 0


def _put_len(out, x):
    v = x - 15
    out += b"\xff" * (v // 255) + bytes([v % 255])


def _common_prefix(src, a, b, limit):
    """Number of equal bytes of src[a:] and src[b:] before position ``limit`` of the first (a > b)."""
    done, step = 0, 64
    while a + done < limit:
        m = min(step, limit - a - done)
        x, y = src[a + done:a + done + m], src[b + done:b + done + m]
        diff = np.flatnonzero(x != y)
        if diff.size:
            return done + int(diff[0])
        done += m
        step *= 2
    return done


def wave_compress(block, hash_log=None):
    """The scheme of frame_lz4_block_kernel's header comment, restated from that comment: one LZ4 block, or None where
    the kernel gives the block up as stored.

      * windows of 64 positions from ``ip``; every position up to n - 12 hashes its 4 bytes (Knuth's multiplier, the top
        ``hash_log`` bits), reads its candidate from a table of positions that starts as all zeros, and tests it: the
        candidate must lie strictly before the position and hold the same 4 bytes;
      * in a block's LAST window (ip + 64 > n - 12), when the table gave no hit, every position takes the nearest earlier
        position of the window with the same 4 bytes as its candidate;
      * the lowest position that hit wins; only the positions up to and including it insert themselves into the table
        (all 64 when nothing hit); the match is extended up to n - 5, the sequence emitted, and the next window begins
        behind the match; with no hit the window moves on by 64;
      * a sequence, the last run of literals included, is emitted only if the output stays below n bytes with it:
        otherwise the block is stored.

    This is NOT an oracle of the device's bytes: two positions of one window that hash alike leave the table entry to
    the hardware (here: to the higher position), and the device's offsets and cuts may then differ.  Its purpose is to
    prove on the CPU that a case reaches the edge it is named for, and that the scheme's output is a valid block."""
    return _wave_compress(bytes(block), hash_log_for(len(block)) if hash_log is None else hash_log)


@functools.lru_cache(maxsize=None)
def _wave_compress(block, hash_log):
    n = len(block)
    mflimit, matchlimit = n - 12, n - 5
    src = np.frombuffer(block, np.uint8)
    out = bytearray()
    ip = anchor = 0
    if mflimit >= 0:
        a = src.astype(np.uint32)
        v = a[:n - 3] | a[1:n - 2] << 8 | a[2:n - 1] << 16 | a[3:] << 24
        h = ((v.astype(np.uint64) * 2654435761 & 0xFFFFFFFF) >> (32 - hash_log)).astype(np.int64)
        table = np.zeros(1 << hash_log, np.int64)
    while ip <= mflimit:
        hi = min(ip + 64, mflimit + 1)
        pos = np.arange(ip, hi)
        hh, vv = h[ip:hi], v[ip:hi]
        cand = table[hh]
        hit = (cand < pos) & (v[cand] == vv)
        if ip + 64 > mflimit and not hit.any():
            cand = cand.copy()
            for lane in range(1, hi - ip):
                same = np.flatnonzero(vv[:lane] == vv[lane])
                if same.size:
                    hit[lane], cand[lane] = True, ip + same[-1]
        hits = np.flatnonzero(hit)
        f = int(hits[0]) if hits.size else 63
        table[hh[:f + 1]] = pos[:f + 1]
        if not hits.size:
            ip += 64
            continue
        mpos = ip + f
        off = mpos - int(cand[f])
        length = 4 + _common_prefix(src, mpos + 4, mpos + 4 - off, matchlimit)
        lit, ml = mpos - anchor, length - 4
        need = 1 + _len_bytes(lit) + lit + 2 + _len_bytes(ml)
        if len(out) + need >= n:
            return None
        out.append(min(lit, 15) << 4 | min(ml, 15))
        if lit >= 15:
            _put_len(out, lit)
        out += block[anchor:mpos]
        out += struct.pack("<H", off)
        if ml >= 15:
            _put_len(out, ml)
        ip = anchor = mpos + length
    lit = n - anchor
    if len(out) + 1 + _len_bytes(lit) + lit >= n:
        return None
    out.append(min(lit, 15) << 4)
    if lit >= 15:
        _put_len(out, lit)
    out += block[anchor:]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def host_compress(block):
    """kafka_wire.lz4_block_compress, remembered per block (the mixed cases repeat their random blocks)."""
    return kw.lz4_block_compress(block)


# ---- test-side walkers ----------------------------------------------------------------------------------------------
def walk_batches(data):
    """[(61-byte header, records section)] of back-to-back RecordBatch v2 bytes."""
    out, pos = [], 0
    while pos < len(data):
        assert len(data) - pos >= 61
        (length,) = struct.unpack_from(">i", data, pos + 8)
        assert length >= 49 and pos + 12 + length <= len(data)
        out.append((data[pos:pos + 61], data[pos + 61:pos + 12 + length]))
        pos += 12 + length
    return out


def walk_frame(frame):
    """[(stored, block bytes)] of one LZ4 frame as kafka-clients writes it; its size words must tile it exactly."""
    assert frame[:7] == FRAME_HEAD, frame[:7].hex()
    assert frame[-4:] == b"\0\0\0\0"
    blocks, pos = [], 7
    while True:
        (word,) = struct.unpack_from("<I", frame, pos)
        pos += 4
        if word == 0:
            break
        size = word & 0x7FFFFFFF
        assert 0 < size <= BLOCK and pos + size + 4 <= len(frame)
        blocks.append((bool(word >> 31), frame[pos:pos + size]))
        pos += size
    assert pos == len(frame)
    return blocks


def walk_block(b):
    """One compressed LZ4 block: (decoded size, [(start, length) of every match], literals of the last sequence); the
    offsets are checked on the way."""
    i = out = 0
    matches = []
    while True:
        tok = b[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                x = b[i]; i += 1
                lit += x
                if x != 255:
                    break
        i += lit
        out += lit
        assert i <= len(b)
        if i == len(b):
            assert tok & 15 == 0  # the last sequence is literals only
            return out, matches, lit
        off = b[i] | b[i + 1] << 8
        i += 2
        assert 1 <= off <= 65535 and off <= out, (off, out)  # never before the block's start: blocks are independent
        ml = tok & 15
        if ml == 15:
            while True:
                x = b[i]; i += 1
                ml += x
                if x != 255:
                    break
        ml += 4
        matches.append((out, ml))
        out += ml


def _sequences(b):
    """(first literal, literals, offset, match length, length bytes of the literal run, length bytes of the match) per
    sequence of one compressed block; the last sequence has offset 0 and match length 0."""
    def extended(x, i):
        nb = 0
        if x == 15:
            while True:
                y = b[i]; i += 1
                x += y; nb += 1
                if y != 255:
                    break
        return x, nb, i
    i = 0
    while True:
        tok = b[i]
        lit, lit_lb, start = extended(tok >> 4, i + 1)
        i = start + lit
        assert i <= len(b)
        if i == len(b):
            yield start, lit, 0, 0, lit_lb, 0
            return
        off = b[i] | b[i + 1] << 8
        ml, ml_lb, i = extended(tok & 15, i + 2)
        yield start, lit, off, ml + 4, lit_lb, ml_lb


def walk_sequences(b):
    """[(literals, offset, match length, length bytes of the literal run, length bytes of the match)] of one compressed
    block; the last sequence has offset 0 and match length 0."""
    return [q[1:] for q in _sequences(b)]


def block_decode(b):
    """A plain decoder of one LZ4 block (no end rules asked: those are walk_block's and the tests')."""
    out = bytearray()
    for start, lit, off, ml, _, _ in _sequences(b):
        out += b[start:start + lit]
        if not ml:
            return bytes(out)
        assert 1 <= off <= len(out), (off, len(out))
        first = len(out) - off
        if off >= ml:
            out += out[first:first + ml]
        else:  # an overlapping copy repeats the last ``off`` bytes
            out += (bytes(out[first:]) * (ml // off + 1))[:ml]


def frame_of_blocks(blocks):
    """An LZ4 frame (kafka-clients' header) of the given ``(stored, body)`` blocks: what liblz4 is handed on the CPU."""
    out = bytearray(FRAME_HEAD)
    for stored, body in blocks:
        out += struct.pack("<I", len(body) | (0x80000000 if stored else 0)) + body
    return bytes(out + b"\0\0\0\0")


def lz4_decompress(frame, size):
    return pa_lz4().Codec("lz4").decompress(frame, decompressed_size=size).to_pybytes()


def check_against_uncompressed(got, exp):
    """Same batches, same records, block rules, for one publish: got = device LZ4 output, exp = the host writer's uncompressed output.
    Returns (compressed blocks, stored blocks) seen."""
    assert sorted(got) == sorted(exp)
    n_comp = n_stored = 0
    for p in exp:
        gb, eb = walk_batches(got[p]), walk_batches(exp[p])
        assert len(gb) == len(eb), (p, len(gb), len(eb))
        pos = 0
        for (gh, frame), (eh, records) in zip(gb, eb):
            assert gh[0:8] == eh[0:8] and gh[12:17] == eh[12:17] and gh[23:61] == eh[23:61]  # all but batchLength, crc, attributes
            assert struct.unpack(">h", gh[21:23])[0] == 3
            assert struct.unpack(">i", gh[8:12])[0] == 49 + len(frame)
            batch = got[p][pos:pos + 61 + len(frame)]
            assert struct.unpack(">I", gh[17:21])[0] == kw.crc32c(batch[21:])
            pos += len(batch)
            blocks = walk_frame(frame)
            assert len(blocks) == (len(records) + BLOCK - 1) // BLOCK
            for k, (stored, body) in enumerate(blocks):
                want = BLOCK if k < len(blocks) - 1 else len(records) - BLOCK * (len(blocks) - 1)
                if stored:
                    assert len(body) == want
                    n_stored += 1
                    continue
                n_comp += 1
                size, matches, last_lit = walk_block(body)
                assert size == want
                assert len(body) < size               # a block that does not shrink is stored
                assert last_lit >= 5                  # the last 5 bytes are literals
                assert all(start <= size - 12 for start, _ in matches)  # no match starts within the last 12 bytes
            assert lz4_decompress(frame, len(records)) == records  # liblz4 is the pin
    return n_comp, n_stored
