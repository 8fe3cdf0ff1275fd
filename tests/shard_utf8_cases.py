"""The corpus of the UTF-8 shard map (``surge_replay_partition_hash_utf8[_device]``), plain Python: ids as bytes, each with a
name, in one fixed order — the CPU tests, the sanitizer program and the GPU tests all walk this list.

What an id must give is decided here and nowhere else: if its hashed span (the whole id, or what lies in front of its first
``:``) decodes as strict UTF-8, the partition is ``kafka.partition_for_keys([text], n)`` — the UTF-16 route, pinned against the
reference long ago — else ``-1``."""
import random

import numpy as np

from surge_amd import kafka

N_PARTITIONS = (1, 2, 7, 64, 2**31 - 1)

TWO_BYTE = ("\u0080", "\u00e9", "\u07ff")
THREE_BYTE = ("\u0800", "\ud7ff", "\ue000", "\ufffd", "\uffff")
FOUR_BYTE = ("\U00010000", "\U0001f600", "\U0010ffff")

#: one input per class of malformed id (the lead byte table of include/surge_replay.h, every way out of it)
MALFORMED = (
    ("lone continuation byte", b"ab\x80cd"),
    ("continuation byte first", b"\xbfid"),
    ("over-long two-byte form C0", b"\xc0\xafid"),
    ("over-long two-byte form C1", b"id\xc1\xbf"),
    ("over-long three-byte form", b"\xe0\x9f\xbf"),
    ("over-long three-byte form of NUL", b"x\xe0\x80\x80"),
    ("over-long four-byte form", b"\xf0\x8f\xbf\xbf"),
    ("encoded high surrogate", b"\xed\xa0\x80"),
    ("encoded low surrogate", b"id-\xed\xbf\xbf"),
    ("encoded surrogate pair", b"\xed\xa0\xbd\xed\xb8\x80"),
    ("above U+10FFFF", b"\xf4\x90\x80\x80"),
    ("lead byte F5", b"\xf5\x80\x80\x80"),
    ("lead byte F8", b"\xf8\x88\x80\x80\x80"),
    ("byte FE", b"id\xfe"),
    ("byte FF", b"\xff\xfeid"),
    ("two-byte sequence cut by the end", b"ab\xc3"),
    ("three-byte sequence cut by the end after one byte", b"ab\xe2"),
    ("three-byte sequence cut by the end after two bytes", b"ab\xe2\x82"),
    ("four-byte sequence cut by the end after three bytes", b"\xf0\x9f\x98"),
    ("second byte not a continuation", b"\xe2\x28\xa1"),
    ("third byte not a continuation", b"\xe2\x82\x28"),
    ("fourth byte not a continuation", b"\xf0\x9f\x98\x41"),
    ("second byte is the next lead", b"\xc3\xc3\xa9"),
    ("malformed in front of a colon", b"\xff:id"),
    ("sequence cut by a colon", b"\xe2\x82:x"),
)

#: neighbours in the arena: each is malformed, and read across their boundary they would be "€"
NEIGHBOURS = (("neighbour: E2 82", b"\xe2\x82"), ("neighbour: AC", b"\xac"))

#: malformed only behind the cut: good with up_to_colon, bad without
BEHIND_THE_COLON = (("malformed byte behind a colon", b"id:\xff"), ("cut sequence behind a colon", b"\xc3\xa9:\xe2\x82"),
                    ("over-long form behind two colons", b"a:b:\xc0\x80"))


def good_ids():
    """``(name, bytes)``: well-formed ids (under either span)."""
    out = [("empty", b"")]
    out += [(f"ascii {n} units", "abcdefghi"[:n].encode()) for n in range(1, 10)]
    for ch in TWO_BYTE + THREE_BYTE + FOUR_BYTE:
        cp = f"U+{ord(ch):04X}"
        out += [(f"{cp} alone", ch.encode()),
                (f"{cp} at an even unit", (ch + "x").encode()),       # a surrogate pair fills one murmur pair
                (f"{cp} at an odd unit", ("a" + ch + "x").encode()),  # ... and straddles two
                (f"{cp} last, even", ("ab" + ch).encode()),
                (f"{cp} last, odd", ("a" + ch).encode()),
                (f"{cp} twice", (ch + ch).encode())]
    out += [("colon first", b":abc"), ("colon last", b"abc:"), ("colon in the middle", b"ab:cd"), ("two colons", b"a:b:c"),
            ("colon only", b":"), ("colon behind a two-byte character", "\u00e9:x".encode()),
            ("colon behind a four-byte character", "id\U0001f600:7".encode()), ("no colon", b"abcd"),
            ("uuid", b"123e4567-e89b-12d3-a456-426614174000"), ("mixed", "agg-\u00e9\u20ac\U0001f600-7".encode())]
    stem = ("k\u00e9" * 84 + "\u00e9").encode()  # 254 bytes: the last byte of the id follows a two-byte character
    assert len(stem) == 254 and stem.decode()
    out += [("255 bytes ending in a", stem + b"a"), ("255 bytes ending in b", stem + b"b")]
    return out


def mutations(per_id=3, seed=20240917):
    """Seeded single-byte mutations of the good ids: ``(name, bytes)``.  Some stay well-formed, some do not."""
    rng = random.Random(seed)
    out = []
    for name, raw in good_ids():
        for _ in range(per_id if raw else 0):
            at = rng.randrange(len(raw))
            new = rng.choice([b for b in range(256) if b != raw[at]])
            out.append((f"{name}: byte {at} -> {new:02X}", raw[:at] + bytes([new]) + raw[at + 1:]))
    return out


def corpus():
    """Every case, ``(name, bytes)``; the neighbours are adjacent."""
    return good_ids() + list(MALFORMED) + list(NEIGHBOURS) + list(BEHIND_THE_COLON) + mutations()


def span_of(raw: bytes, up_to_colon: bool) -> bytes:
    return raw.split(b":", 1)[0] if up_to_colon else raw


def is_well_formed(raw: bytes, up_to_colon: bool) -> bool:
    try:
        span_of(raw, up_to_colon).decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def expected(ids, n_partitions: int, up_to_colon: bool) -> np.ndarray:
    """``int32[len(ids)]``: the pinned UTF-16 route over the spans that decode, ``-1`` for the others."""
    out = np.full(len(ids), -1, dtype=np.int32)
    good = [i for i, raw in enumerate(ids) if is_well_formed(raw, up_to_colon)]
    if good:
        texts = [span_of(ids[i], up_to_colon).decode("utf-8") for i in good]
        out[good] = kafka.partition_for_keys(texts, n_partitions, up_to_colon=up_to_colon)
    return out


def table(ids, lead: bytes = b""):
    """``(uint8 data, int64 offsets)``: the ids back to back behind ``lead`` (``offsets[0] == len(lead)``), no byte of slack."""
    off = np.zeros(len(ids) + 1, dtype=np.int64)
    off[0] = len(lead)
    if ids:
        off[1:] = len(lead) + np.cumsum([len(k) for k in ids])
    return np.frombuffer(lead + b"".join(ids), dtype=np.uint8).copy(), off
