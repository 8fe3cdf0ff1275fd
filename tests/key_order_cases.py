"""What the key-order tests share: the key corpus, its expectation — Python's ``sorted`` / ``bisect`` over ``bytes``, which
compare unsigned bytes and put a proper prefix first — and a plain-Python restatement of the device's pass rule
(ingest_order.hip), which the CPU test holds to ``sorted`` so that the corpus is shown to reach the passes it is there for."""
import bisect
import random

STEM_LENGTHS = (3, 4, 5, 7, 8, 9)
DECIDING = (0x00, 0x01, 0x7F, 0x80, 0xFF)
LONG = b"L" * 253  # 255-byte ids that differ only in byte 253: decided in pass 63, the last one ceil(255 / 4) allows


def corpus():
    """Unique keys, in an order that is not theirs: proper prefixes down to the empty id; stems of exactly 3 .. 9 shared bytes
    with 0x00 / 0x7f / 0x80 / 0xff deciding behind them (a signed compare puts 0x80 in front of 0x7f; a compare without the
    bytes-left component makes ``a`` and ``a\\0`` one key); 255-byte ids that differ in byte 253; a 200-byte id among short
    ones, and its 196-byte prefix; ids with ``:`` and the neighbours of ``id:~``."""
    keys = [b"", b"a", b"a\0", b"a\0\0", b"a\0\0\0", b"a\0\0\0\0", b"a\x01", b"a\0\x01", b"b"]
    for n in STEM_LENGTHS:
        stem = bytes([0x50 + n]) + b"q" * (n - 1)
        keys += [stem] + [stem + bytes([c]) for c in DECIDING] + [stem + b"\x7f\0", stem + b"\x80\x80\x80\x80\x80"]
    keys += [LONG + bytes([c]) + b"z" for c in (0x01, 0x7F, 0x80, 0xFF)]
    keys += [b"M" * 200, b"M" * 196, b"M", b"N"]
    keys += [b"id", b"id!x", b"id:", b"id:~", b"id:\x7f", b"idx", b"id:1", b"id:~z", b"ie"]
    assert len(set(keys)) == len(keys)
    random.Random(4).shuffle(keys)
    return keys


def random_keys(n, seed):
    """``n`` unique keys of 0 .. 13 bytes over six byte values: ties in every chunk, many proper prefixes."""
    rng = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        k = bytes(rng.choice((0x00, 0x3A, 0x61, 0x7F, 0x80, 0xFF)) for _ in range(rng.randrange(0, 14)))
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def expected_order(keys):
    """The dense indices (positions in ``keys``, the delivery order) in key order."""
    return sorted(range(len(keys)), key=lambda i: keys[i])


def expected_range(keys, lo, hi):
    """The rows of ``lo <= key <= hi`` ascending; ``None``: unbounded."""
    order = expected_order(keys)
    srt = [keys[i] for i in order]
    a = 0 if lo is None else bisect.bisect_left(srt, lo)
    b = len(srt) if hi is None else bisect.bisect_right(srt, hi)
    return order[a:b] if a < b else []


def order_by_passes(keys, max_passes=None):
    """The pass rule, restated: pass p sorts the positions stably by (group, bytes [4p, 4p + 4) big-endian and zero-padded, bytes
    left from 4p on clipped to 0 .. 4); a position whose triple differs from its predecessor's opens a group; it ends when every
    group is one key or no key had a byte.  -> (order, passes, groups)."""
    n = len(keys)
    idx, grp, passes, groups = list(range(n)), [0] * n, 0, min(n, 1)
    while groups < n and (max_passes is None or passes < max_passes):
        at = 4 * passes
        triple = []
        for j in range(n):
            k = keys[idx[j]]
            left = min(max(len(k) - at, 0), 4)
            triple.append((grp[j], int.from_bytes(k[at:at + 4].ljust(4, b"\0"), "big"), left))
        perm = sorted(range(n), key=lambda j: triple[j])  # (stable)
        idx = [idx[j] for j in perm]
        triple = [triple[j] for j in perm]
        grp = [0] * n
        for j in range(1, n):
            grp[j] = grp[j - 1] + (triple[j] != triple[j - 1])
        groups = grp[-1] + 1
        passes += 1
        if not any(t[2] for t in triple):
            break
    return idx, passes, groups
