"""Case builders and references for the device state encoder and the snapshot delta (no GPU, no torch).

Shared by tests/test_state_out_cases.py (which holds every builder to the property it names), tests/test_encode_edges_gpu.py
and tests/test_snapshot_delta_gpu.py.  Nothing here comes from surge_amd/csrc: the constants below restate
include/surge_replay.h and the comments of state_kernels.hip, and the CPU test pins them on the package's own.

States are ``uint8[n, 64]`` rows: the flags word is the little-endian u32 at byte 36 (PRESENT = 1, POISONED = 2), a v1 state
keeps bytes 40..63 zero, a v2 slot schema may use all 64.  Keys and strings are ``bytes`` (UTF-8)."""
import math
import struct
from dataclasses import dataclass, field

import numpy as np

JP_LITERAL, JP_KEY, JP_I32, JP_U32, JP_I64, JP_F64, JP_STR = 0, 1, 2, 3, 4, 5, 6
PRESENT, POISONED = 1, 2
SKIP, VALUE, TOMBSTONE = 0, 1, 2
FLAGS_AT = 36

ENCODE_BLOCK = 256        # aggregates whose text one block of the write pass composes
STAGE_BYTES = 32 * 1024   # a block stages its text in LDS when (end - base) + shift <= STAGE_BYTES
SCAN_BLOCK = 1024         # lengths per block of the scan; the totals kernel has 1024 threads
DELTA_TRIP = 8192 * 64    # aggregates one trip of the delta's grid-stride loop covers (8192 blocks x 256 lanes / 4)

COUNTER = (b'{"aggregateId":', "KEY", b',"count":', (JP_I32, 0), b',"version":', (JP_I32, 4), b"}")
BANK_ACCOUNT = (b'{"accountNumber":', "KEY", b',"accountOwner":', (JP_STR, 0), b',"securityCode":', (JP_STR, 1),
                b',"balance":', (JP_F64, 16), b"}")
I32_ONLY = ((JP_I32, 0),)


# ---- rows ---------------------------------------------------------------------------------------------------------------
def rows(n):
    return np.zeros((n, 64), dtype=np.uint8)


def put(st, off, values, dtype):
    """Column ``values`` (little-endian ``dtype``) at byte ``off`` of every row."""
    v = np.ascontiguousarray(np.asarray(values).astype(dtype))
    st[:, off:off + v.dtype.itemsize] = v.view(np.uint8).reshape(st.shape[0], v.dtype.itemsize)


def flags_of(st):
    return np.ascontiguousarray(st[:, FLAGS_AT:FLAGS_AT + 4]).view("<u4").reshape(-1)


# ---- the snapshot delta ---------------------------------------------------------------------------------------------------
def delta_kinds(now, base, full64):
    """``(kind[n], n_values, n_tombstones)`` of ``now`` relative to the baseline ``base`` (include/surge_replay.h): SKIP when
    the compared bytes are equal (0..39 for v1, all 64 for a v2 slot schema) or ``now`` is POISONED, else VALUE when
    PRESENT, else TOMBSTONE."""
    span = 64 if full64 else 40
    differs = (now[:, :span] != base[:, :span]).any(axis=1)
    fl = flags_of(now)
    kind = np.where(differs & ((fl & POISONED) == 0), np.where((fl & PRESENT) != 0, VALUE, TOMBSTONE), SKIP).astype(np.uint8)
    return kind, int((kind == VALUE).sum()), int((kind == TOMBSTONE).sum())


def committed(baseline, states, kind):
    """The baseline after a commit of ``kind``: the reported aggregates' current states, the others as they were."""
    return np.where((kind != SKIP)[:, None], states, baseline)


def invalidated(baseline, kind):
    """The baseline after an invalidate of ``kind``: all ones for the reported aggregates (no fold produces that)."""
    return np.where((kind != SKIP)[:, None], np.uint8(0xFF), baseline)


def random_rows(n, rng, full64, p_none=0.1, p_poisoned=0.05):
    """Random states: every compared byte random, flags PRESENT for most, None (fields kept) and POISONED for some."""
    st = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    if not full64:
        st[:, 40:] = 0
    u = rng.random(n)
    fl = np.where(u < p_none, 0, np.where(u < p_none + p_poisoned, PRESENT | POISONED, PRESENT))
    put(st, FLAGS_AT, fl, "<u4")
    return st


def mutate(st, idx, rng, full64):
    """A copy of ``st`` whose rows ``idx`` have one random bit of the compared span flipped (never PRESENT / POISONED)."""
    out = st.copy()
    span = 64 if full64 else 40
    byte = rng.integers(0, span, size=len(idx))
    bit = rng.integers(0, 8, size=len(idx))
    bit = np.where(byte == FLAGS_AT, 2 + bit % 6, bit)
    out[idx, byte] ^= (1 << bit).astype(np.uint8)
    return out


def delta_cases(full64, rng):
    """``(base, now, labels)`` of the transition table.  The expected kinds are ``delta_kinds`` over the baseline the first
    load's commit leaves (a POISONED row is never committed: ``committed`` says so), whatever a label promises."""
    words = 16 if full64 else 10
    base, now, labels = [], [], []

    def some(poisoned=False):
        r = random_rows(1, rng, full64, 0.0, 0.0)[0]
        r[FLAGS_AT:FLAGS_AT + 4] = np.frombuffer(struct.pack("<I", PRESENT | (POISONED if poisoned else 0)), np.uint8)
        return r

    def none_nonzero():
        r = some()
        r[FLAGS_AT:FLAGS_AT + 4] = 0
        return r

    # one aggregate per 4-byte word: a single bit of that word differs, in a random byte, byte 0, byte 3 and a middle byte
    for where in ("any", 0, 3, "middle"):
        for w in range(words):
            b = some()
            byte = int(rng.integers(0, 4)) if where == "any" else int(rng.integers(1, 3)) if where == "middle" else where
            at = 4 * w + byte
            bit = int(rng.integers(2, 8)) if at == FLAGS_AT else int(rng.integers(0, 8))  # both stay PRESENT, not POISONED
            n = b.copy()
            n[at] ^= np.uint8(1 << bit)
            base.append(b), now.append(n), labels.append(f"bit word {w} byte {byte}")
    # every ordered pair of the four conditions, as baseline and as now; now with equal and with different field bytes
    make = {"never": lambda: np.zeros(64, np.uint8), "none": none_nonzero, "some": some, "poisoned": lambda: some(True)}
    for x in make:
        for y in make:
            for same in (True, False):
                b = make[x]()
                n = make[y]()
                if same and y != "never" and x != "never":
                    fl = n[FLAGS_AT:FLAGS_AT + 4].copy()
                    n = b.copy()
                    n[FLAGS_AT:FLAGS_AT + 4] = fl
                base.append(b), now.append(n), labels.append(f"{x} -> {y} {'equal' if same else 'different'} bytes")
    return np.stack(base), np.stack(now), labels


# ---- the encoder's reference ------------------------------------------------------------------------------------------------
def _jackson_table():
    t = [bytes([c]) for c in range(256)]
    for c in range(0x20):
        t[c] = b"\\u00" + b"0123456789ABCDEF"[c >> 4:(c >> 4) + 1] + b"0123456789ABCDEF"[c & 15:(c & 15) + 1]
    for c, e in ((0x22, b'\\"'), (0x5C, b"\\\\"), (0x08, b"\\b"), (0x0C, b"\\f"), (0x0A, b"\\n"), (0x0D, b"\\r"), (0x09, b"\\t")):
        t[c] = e
    return t


JACKSON = _jackson_table()  # Jackson's default escaping: seven short escapes, other controls \u00XX upper-case, rest verbatim


def quote(b):
    return b'"' + b"".join(JACKSON[c] for c in b) + b'"'


_STATE_CLASS = None


def protobuf_state_class():
    """message State { string aggregateId = 1; bytes payload = 2; } (multilanguage-protocol.proto:7-10), built with
    the real protobuf runtime so the expected bytes come from Google's encoder, not from a restatement."""
    global _STATE_CLASS
    if _STATE_CLASS is None:
        from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

        fd = descriptor_pb2.FileDescriptorProto(name="surge_multilanguage_state.proto", syntax="proto3")
        m = fd.message_type.add(name="State")
        F = descriptor_pb2.FieldDescriptorProto
        m.field.add(name="aggregateId", number=1, type=F.TYPE_STRING, label=F.LABEL_OPTIONAL)
        m.field.add(name="payload", number=2, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
        pool = descriptor_pool.DescriptorPool()
        pool.Add(fd)
        _STATE_CLASS = message_factory.GetMessageClass(pool.FindMessageTypeByName("State"))
    return _STATE_CLASS


def _part_text(part, row, key, strings, a):
    """The text of one template part, or ``None`` for a Double that is not a JSON number."""
    if isinstance(part, bytes):
        return part
    if part == "KEY":
        return quote(key)
    kind, off = part
    if kind == JP_STR:
        return quote(strings[off][a])
    if kind == JP_I32:
        return str(int.from_bytes(row[off:off + 4], "little", signed=True)).encode()
    if kind == JP_U32:
        return str(int.from_bytes(row[off:off + 4], "little", signed=False)).encode()
    if kind == JP_I64:
        return str(int.from_bytes(row[off:off + 8], "little", signed=True)).encode()
    if kind == JP_F64:
        from oracle import oracle

        x = struct.unpack("<d", row[off:off + 8])[0]
        return oracle.play_json_double_text(x).encode() if math.isfinite(x) else None
    raise ValueError(f"unknown part {part!r}")


def encode_reference(template, states, keys, strings=(), filter=None, envelope=False):
    """``(bytes, offsets[n + 1], n_not_a_number)`` of the encoder, from the contract: an aggregate emits when it is PRESENT,
    not POISONED, the filter (if any) says VALUE and every Double part is finite; one the filter lets through that holds a
    non-finite Double emits nothing and counts once."""
    n = states.shape[0]
    fl = flags_of(states)
    out, off, nan = [], np.zeros(n + 1, dtype=np.int64), 0
    State = protobuf_state_class() if envelope else None
    for a in range(n):
        text = b""
        if (fl[a] & PRESENT) and not (fl[a] & POISONED) and (filter is None or filter[a] == VALUE):
            row = states[a].tobytes()
            parts = [_part_text(p, row, keys[a], strings, a) for p in template]
            if any(p is None for p in parts):
                nan += 1
            else:
                text = b"".join(parts)
                if envelope:
                    text = State(aggregateId=keys[a].decode("utf-8"), payload=text).SerializeToString()
        out.append(text)
        off[a + 1] = off[a] + len(text)
    return b"".join(out), off, nan


def i32_only_reference(states):
    """``(bytes, offsets)`` of the ``I32_ONLY`` template, vectorised: offsets from a cumsum of digit counts, bytes from
    one join of ``str(int)`` — two routes that must agree on the total."""
    v = np.ascontiguousarray(states[:, 0:4]).view("<i4").reshape(-1).astype(np.int64)
    fl = flags_of(states)
    emit = ((fl & PRESENT) != 0) & ((fl & POISONED) == 0)
    digits = np.searchsorted(10 ** np.arange(1, 11, dtype=np.int64), np.abs(v), side="right") + 1
    off = np.zeros(v.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.where(emit, digits + (v < 0), 0), out=off[1:])
    text = "".join(map(str, v[emit].tolist())).encode()
    assert len(text) == off[-1]
    return text, off


def block_spans(offsets, lead=0):
    """Per block of the write pass: ``(base, end, shift)`` with shift = position of the block's first byte in its 16-byte
    word when the output starts ``lead`` bytes behind a 16-byte boundary."""
    n = len(offsets) - 1
    return [(int(offsets[a0]), int(offsets[min(a0 + ENCODE_BLOCK, n)]), (lead + int(offsets[a0])) % 16) for a0 in range(0, n, ENCODE_BLOCK)]


def copy_shape(base, end, shift):
    """``(staged, body_lo, body_hi)`` of a block as the write pass lays it out (frame: 16-byte word of the first byte)."""
    lo, hi = shift, shift + (end - base)
    return (end - base) + shift <= STAGE_BYTES, (lo + 15) & ~15, hi & ~15


@dataclass
class EncodeCase:
    name: str
    template: tuple
    states: np.ndarray
    keys: list
    strings: tuple = ()
    envelope: bool = False
    prop: dict = field(default_factory=dict)

    def reference(self, filter=None):
        return encode_reference(self.template, self.states, self.keys, self.strings, filter, self.envelope)


def _counter_states(n, rng, p_absent=0.125):
    st = rows(n)
    mag = 10 ** rng.integers(0, 10, size=n)
    put(st, 0, rng.integers(-mag, mag + 1), "<i4")
    put(st, 4, rng.integers(0, 1 << 20, size=n), "<i4")
    u = rng.random(n)
    put(st, FLAGS_AT, np.where(u < p_absent, 0, np.where(u < p_absent + 0.02, PRESENT | POISONED, PRESENT)), "<u4")
    return st


def _pad_key0(template, st, keys, residue):
    """Lengthen key 0 (PRESENT) so that block 0's text is ``residue`` (mod 16)."""
    put(st[:1], FLAGS_AT, [PRESENT], "<u4")
    t0 = int(encode_reference(template, st[:ENCODE_BLOCK], keys[:ENCODE_BLOCK])[1][-1])
    keys[0] = keys[0] + b"x" * ((residue - t0) % 16)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def shift_cases():
    """16 logs of 512 Counter aggregates; block 0's text is r (mod 16), so block 1 starts at every residue."""
    out = []
    for r in range(16):
        rng = np.random.default_rng(100 + r)
        st = _counter_states(512, rng)
        keys = [b"k%03d" % i for i in range(512)]
        _pad_key0(COUNTER, st, keys, r)
        out.append(EncodeCase(f"shift{r}", COUNTER, st, keys, prop={"residue": r}))
    return out


# 2 ---------------------------------------------------------------------------------------------------------------------------
def _i32_of_length(length):
    return 7 if length == 1 else 10 ** (length - 1) + 7 if length <= 10 else -1234567890


def _tiny(name, start, texts, at=None, **prop):
    """Three blocks of ``I32_ONLY``: block 0 emits ``start`` (mod 16) bytes, block 1 the given values only, block 2 emits."""
    st = rows(3 * ENCODE_BLOCK)
    v = np.full(3 * ENCODE_BLOCK, 7, dtype=np.int64)
    fl = np.full(3 * ENCODE_BLOCK, PRESENT, dtype=np.int64)
    v[:start] = 42                                # start two-digit texts among one-digit ones: 256 + start bytes
    fl[ENCODE_BLOCK:2 * ENCODE_BLOCK] = 0
    v[ENCODE_BLOCK:2 * ENCODE_BLOCK] = 987654321  # None with fields set: nothing may be emitted for them
    at = at if at is not None else [(17 * start + 5 * sum(texts)) % ENCODE_BLOCK]
    for i, length in zip(at, texts):
        v[ENCODE_BLOCK + i], fl[ENCODE_BLOCK + i] = _i32_of_length(length), PRESENT
    v[2 * ENCODE_BLOCK:] = np.arange(ENCODE_BLOCK) - 100
    put(st, 0, v, "<i4")
    put(st, FLAGS_AT, fl, "<u4")
    return EncodeCase(name, I32_ONLY, st, [b""] * (3 * ENCODE_BLOCK), prop=dict(start=start, total=sum(texts), **prop))


def tiny_block_cases():
    """Blocks whose whole text is shorter than a 16-byte word, at every start residue; a word-straddling one; a block of
    exactly 16 aligned bytes; a block that emits nothing between two that do."""
    out = []
    for s in range(16):
        for length in sorted({1, min(11, 16 - s)}):
            out.append(_tiny(f"tiny_s{s}_l{length}", s, [length], inside_one_word=True))
    for s, length in ((12, 8), (15, 11), (9, 11), (15, 2)):
        out.append(_tiny(f"straddle_s{s}_l{length}", s, [length], inside_one_word=False))
    out.append(_tiny("exact_word", 0, [11, 5], at=[3, 250], inside_one_word=True))
    out.append(_tiny("aligned_17", 0, [11, 6], at=[0, 255], inside_one_word=False))
    for s in (0, 5):
        out.append(_tiny(f"silent_block_s{s}", s, [], at=[], inside_one_word=True))
    return out


# 3 ---------------------------------------------------------------------------------------------------------------------------
STAGE_SUMS = (STAGE_BYTES - 1, STAGE_BYTES, STAGE_BYTES + 1, STAGE_BYTES + 4096)


def stage_threshold_cases():
    """One long key in block 1 puts (end - base) + shift on either side of the staging threshold, at shift 0 and 15; the
    key mixes plain bytes, two-byte and six-byte escapes; blocks 0 and 2 are ordinary staged ones."""
    unit = b'ab"\x01\\\ncd\x1f'  # 22 bytes once escaped
    assert sum(len(JACKSON[c]) for c in unit) == 22
    out = []
    for shift in (0, 15):
        for want in STAGE_SUMS:
            rng = np.random.default_rng(want + shift)
            n, long_at = 3 * ENCODE_BLOCK, ENCODE_BLOCK + 44
            st = _counter_states(n, rng)
            put(st[long_at:long_at + 1], FLAGS_AT, [PRESENT], "<u4")
            keys = [b"a%03d" % i for i in range(n)]
            keys[long_at] = b""
            _pad_key0(COUNTER, st, keys, shift)
            off = encode_reference(COUNTER, st, keys)[1]
            extra = (want - shift) - int(off[2 * ENCODE_BLOCK] - off[ENCODE_BLOCK])
            m = (extra - 50) // 22
            keys[long_at] = unit * m + b"z" * (extra - 22 * m)
            out.append(EncodeCase(f"stage_{want}_shift{shift}", COUNTER, st, keys, prop={"sum": want, "shift": shift, "long_at": long_at}))
    return out


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _edge_values(lo, hi):
    """0, +-1, +-9, +-10, +-99, +-100, ... every power of ten and its predecessor inside [lo, hi], and lo and hi."""
    vals = {0, lo, hi}
    p = 1
    while p <= max(hi, -lo):
        vals.update(x for x in (p, p - 1, -p, -(p - 1)) if lo <= x <= hi)
        p *= 10
    return sorted(vals)


I32_VALUES = _edge_values(-2 ** 31, 2 ** 31 - 1)
U32_VALUES = _edge_values(0, 2 ** 32 - 1) + [2 ** 31 - 1, 2 ** 31]
I64_VALUES = _edge_values(-2 ** 63, 2 ** 63 - 1)


def integer_cases():
    """I32 at every aligned offset 0..36, U32 at 32 (the same bytes read as I32 beside it), I64 at 8; the values are
    ``_edge_values``, the whole list at every offset.  The word at 36 is the flags word: there every value comes with its
    two low bits replaced by PRESENT set and POISONED clear (nothing else can be emitted from that word)."""
    n = len(I32_VALUES)
    st = rows(n)
    parts = []
    for j, off in enumerate(range(0, 32, 4)):
        put(st, off, np.roll(np.array(I32_VALUES, dtype=np.int64), 7 * j), "<i4")
        parts += [b","] * (j > 0) + [(JP_I32, off)]
    put(st, FLAGS_AT, [PRESENT] * n, "<u4")
    a = EncodeCase("i32_offsets_0_28", tuple(parts), st, [b""] * n, prop={"kinds": {JP_I32}, "offsets": list(range(0, 32, 4))})
    n = len(I64_VALUES)
    st = rows(n)
    put(st, 8, np.array(I64_VALUES, dtype=object).astype(np.int64), "<i8")
    put(st, 32, np.resize(np.array(U32_VALUES, dtype=np.int64), n), "<u4")
    put(st, FLAGS_AT, (np.resize(np.array(I32_VALUES, dtype=np.int64), n) & ~np.int64(3) | PRESENT) & 0xFFFFFFFF, "<u4")
    tmpl = ((JP_I32, 32), b",", (JP_I32, 36), b",", (JP_U32, 32), b",", (JP_I64, 8))
    b = EncodeCase("i32_32_36_u32_32_i64_8", tmpl, st, [b""] * n, prop={"kinds": {JP_I32, JP_U32, JP_I64}, "offsets": [32, 36, 8]})
    n = len(I32_VALUES)
    st = rows(n)
    put(st, 32, I32_VALUES, "<i4")
    put(st, FLAGS_AT, (np.roll(np.array(I32_VALUES, dtype=np.int64), 11) & ~np.int64(3) | PRESENT) & 0xFFFFFFFF, "<u4")
    tmpl = ((JP_I32, 32), b",", (JP_I32, 36), b",", (JP_U32, 32))
    d = EncodeCase("i32_32_36_full_list", tmpl, st, [b""] * n, prop={"kinds": {JP_I32, JP_U32}, "offsets": [32, 36]})
    return [a, b, d]


# 5 ---------------------------------------------------------------------------------------------------------------------------
def escape_cases():
    """BankAccount rows: every byte 0x00..0x7F once as a key character and once in a string column; two-, three- and
    four-byte UTF-8; an empty key, empty strings, a key of six-byte escapes only.  A Double sits behind the strings."""
    keys = [b"k" + bytes([c]) for c in range(0x80)]
    owners = [bytes([c]) + b"o" if c % 2 else b"" for c in range(0x80)]
    codes = [b"" if c % 2 else b"c" + bytes([c]) + b"c" for c in range(0x80)]
    for k, o, c in ((b"", b"empty key", b"0000"), (b"empty strings", b"", b""), (b"\x01\x02\x1f\x00\x0b", b"controls", b"\x1e"),
                    ("\u043a\u043b\u044e\u0447-\u00e9".encode(), "\u00fcn\u00ef \u2713 \u20ac".encode(), "\U0001d11e\U00010348".encode()),
                    ("\U0001d11e".encode(), b'"\\', b"\t\n\r\b\f"), (b"\x7f", b"\x7f\x7f", "\u0080\u07ff\u0800\uffff".encode())):
        keys.append(k), owners.append(o), codes.append(c)
    n = len(keys)
    rng = np.random.default_rng(5)
    st = rows(n)
    bal = np.round(rng.random(n) * 1e7) / 100
    bal[:12] = [0.0, -0.0, 100.0, 1e20, 1e21, 1e-7, 5e-324, 1.7976931348623157e308, 0.1 + 0.2, -2.5, 1e-10, 123456789012345680.0]
    put(st, 16, bal, "<f8")
    put(st, FLAGS_AT, [PRESENT] * n, "<u4")
    return [EncodeCase("escapes", BANK_ACCOUNT, st, keys, (owners, codes), prop={"bytes": set(range(0x80))})]


# 6 ---------------------------------------------------------------------------------------------------------------------------
ENVELOPE_LENGTHS = (0, 127, 128, 16383, 16384)


def _id_of(length):
    return ("\u00e9" * min(2, length // 2)).encode() + b"k" * (length - 2 * min(2, length // 2))


def envelope_cases():
    """protobuf State{aggregateId, payload}: id length and payload length on either side of the 1 / 2 / 3-byte varint steps,
    set independently (the template's text does not hold the key).  One measured aggregate per block."""
    out = []
    digits = 5  # every "v" has five digits: the payload length is the template's alone
    for want in (127, 128):
        n = len(ENVELOPE_LENGTHS) * ENCODE_BLOCK
        rng = np.random.default_rng(want)
        st = rows(n)
        put(st, 8, rng.integers(10000, 100000, size=n), "<i8")
        put(st, FLAGS_AT, np.where(rng.random(n) < 0.05, PRESENT, 0), "<u4")
        keys = [b"id%d" % i for i in range(n)]
        at = [j * ENCODE_BLOCK + 17 * j + 3 for j in range(len(ENVELOPE_LENGTHS))]
        for a, idlen in zip(at, ENVELOPE_LENGTHS):
            keys[a] = _id_of(idlen)
            put(st[a:a + 1], FLAGS_AT, [PRESENT], "<u4")
        tmpl = (b'{"v":', (JP_I64, 8), b',"p":"' + b"p" * (want - 13 - digits) + b'"}')
        out.append(EncodeCase(f"envelope_payload{want}", tmpl, st, keys, envelope=True,
                              prop={"at": at, "ids": list(ENVELOPE_LENGTHS), "payloads": [want] * len(at)}))
    n = 2 * len(ENVELOPE_LENGTHS) * ENCODE_BLOCK
    rng = np.random.default_rng(16383)
    st = rows(n)
    put(st, 8, rng.integers(10000, 100000, size=n), "<i8")
    put(st, FLAGS_AT, np.where(rng.random(n) < 0.05, PRESENT, 0), "<u4")
    keys = [b"id%d" % i for i in range(n)]
    col = [b"s%d" % (i % 7) for i in range(n)]
    at, ids, payloads = [], [], []
    for j, (want, idlen) in enumerate((w, i) for w in (16383, 16384) for i in ENVELOPE_LENGTHS):
        a = j * ENCODE_BLOCK + 23 * j + 1
        keys[a], col[a] = _id_of(idlen), b"q" * (want - 13 - digits)
        put(st[a:a + 1], FLAGS_AT, [PRESENT], "<u4")
        at.append(a), ids.append(idlen), payloads.append(want)
    tmpl = (b'{"v":', (JP_I64, 8), b',"p":', (JP_STR, 0), b"}")
    out.append(EncodeCase("envelope_payload16383_16384", tmpl, st, keys, (col,), envelope=True, prop={"at": at, "ids": ids, "payloads": payloads}))
    return out


# 7 ---------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (1023, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, 1024 * 1024 + 1025)


def scan_case(n):
    """``n`` aggregates of ``I32_ONLY`` with empty keys, about a quarter of them absent (use ``i32_only_reference``)."""
    rng = np.random.default_rng(n)
    st = rows(n)
    mag = 10 ** rng.integers(0, 10, size=n)
    put(st, 0, rng.integers(-mag, mag + 1), "<i4")
    put(st, FLAGS_AT, np.where(rng.random(n) < 0.25, 0, PRESENT), "<u4")
    nb = -(-n // SCAN_BLOCK)
    return EncodeCase(f"scan{n}", I32_ONLY, st, None, prop={"n": n, "nb": nb, "per": -(-nb // 1024)})


def scan_cases():
    return [scan_case(n) for n in SCAN_SIZES]
