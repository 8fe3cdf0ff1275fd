"""The corpus of the state decoder's lenient reading mode (no test functions; shared by tests/test_state_lenient.py and the
GPU tests): state values as ``Json.parse(bytes).asOpt[State]`` takes them — members in any order, whitespace between the
tokens, members the case class does not know — over the Counter, BankAccount and SDK-sample templates, and one named input
per refusal.  Everything is built from a fixed seed.

The reference for an accepted value is ``json.loads`` (``document`` / ``expected_row`` below): the expected row and strings
are derived from the parsed document and the template's own parts, nothing of the library is in the expectation."""
import itertools
import json
import random
import struct
from dataclasses import dataclass
from typing import Optional

from fixture_models import protobuf_varint
from surge_amd.encode import JP_F64, JP_I32, JP_I64, JP_KEY, JP_STR, JP_U32, JsonTemplate

COUNTER, BANK = JsonTemplate.counter(), JsonTemplate.bank_account()
SDK = JsonTemplate((b'{"balance":', (JP_I32, 0), b"}"))  # json4s write(BankAccount(balance)) of the SDK sample (Main.scala:19, 41-60)
WS = (b" ", b"\t", b"\n", b"\r")
OK, STRING, ESCAPE, KEY_MISMATCH, INT, RANGE, NUMBER, TRAILING, SURROGATE, ENVELOPE, SYNTAX, MISSING = 0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13
MUTATED, REFUSED = -1, -2
SEED = 20251


@dataclass
class Case:
    name: str
    template: JsonTemplate
    value: bytes
    key: Optional[bytes]   # the id a KEY member must equal (None: not compared)
    status: int = OK       # MUTATED: whatever the parser says; REFUSED: any status but OK
    envelope: bool = False
    payload_at: int = 0    # envelope cases: where the JSON text lies in the value


def fields_of(template):
    """``[(name, kind, field_offset)]`` from the template's parts alone: a literal ``{"name":`` / ``,"name":`` and the part behind it."""
    out = []
    parts = list(template.parts)
    for lit, val in zip(parts[0::2], parts[1::2]):
        assert isinstance(lit, bytes) and lit[:2] in (b'{"', b',"') and lit.endswith(b'":')
        kind, off = (JP_KEY, 0) if val == "KEY" else (int(val[0]), int(val[1]))
        out.append((lit[2:-2], kind, off))
    assert parts[-1] == b"}"
    return out


# ---- the reference: json.loads --------------------------------------------------------------------------------------------
class _Int(int):
    def __new__(cls, text):
        self = int.__new__(cls, text)
        self.text = text
        return self


class _Float(float):
    def __new__(cls, text):
        self = float.__new__(cls, text)
        self.text = text
        return self


class _Object(list):
    """an object's ``(name, value)`` members in text order"""


def _no_constants(word):
    raise ValueError(f"{word} is not JSON")


def document(text: bytes):
    """The top-level members ``[(name, value)]`` in text order as ``json.loads`` reads them (duplicates kept), or raises.
    Bytes that are not UTF-8 pass through strings unchanged (surrogateescape: the decoder does not check them either);
    numbers keep their text."""
    doc = json.loads(text.decode("utf-8", "surrogateescape"), parse_constant=_no_constants, parse_int=_Int, parse_float=_Float,
                     object_pairs_hook=lambda pairs: _Object(k for k in pairs))
    if not isinstance(doc, _Object):
        raise ValueError("the top level is not an object")
    return doc


def _bytes_of(s: str) -> bytes:
    return s.encode("utf-8", "surrogateescape")


def expected_row(template, members, key):
    """``(row bytes, {column: string bytes})`` of a document every field of which occurs with a value of its own type and
    range, by the LAST occurrence of each name; ``None`` when a field is absent or is not such a value."""
    row = bytearray(64)
    strings = {}
    last = {}
    for name, value in members:
        last[_bytes_of(name)] = value
    for name, kind, off in fields_of(template):
        if name not in last:
            return None
        v = last[name]
        if kind in (JP_KEY, JP_STR):
            if not isinstance(v, str):
                return None
            if kind == JP_KEY and key is not None and _bytes_of(v) != key:
                return None
            if kind == JP_STR:
                strings[off] = _bytes_of(v)
        elif kind == JP_F64:
            if not isinstance(v, (_Int, _Float)):
                return None
            struct.pack_into("<d", row, off, float(v.text))
        else:
            lo, hi, fmt = {JP_I32: (-2 ** 31, 2 ** 31 - 1, "<i"), JP_U32: (0, 2 ** 32 - 1, "<I"), JP_I64: (-2 ** 63, 2 ** 63 - 1, "<q")}[kind]
            if not isinstance(v, _Int) or not lo <= v <= hi:
                return None
            struct.pack_into(fmt, row, off, int(v))
    struct.pack_into("<I", row, 36, 1)  # SURGE_STATE_PRESENT
    return bytes(row), strings


# ---- builders ---------------------------------------------------------------------------------------------------------------
COUNTER_KEY, BANK_KEY, SDK_KEY = b"agg-1", "acct-\u00e9-1".encode("utf-8"), b"k1"
BASE = {
    id(COUNTER): (COUNTER_KEY, [(b"aggregateId", b'"agg-1"'), (b"count", b"-17"), (b"version", b"42")]),
    id(BANK): (BANK_KEY, [(b"accountNumber", b'"acct-\xc3\xa9-1"'), (b"accountOwner", b'"J \\"q\\" \\/ \\u20ac"'), (b"securityCode", b'"0042"'),
                          (b"balance", b"-1.25E+3")]),
    id(SDK): (SDK_KEY, [(b"balance", b"77")]),
}


def text_of(members, gaps=None):
    """``members``: ``(raw name, raw value text)`` -> the object; ``gaps``: callable giving the whitespace of the next token gap."""
    g = gaps or (lambda: b"")
    out = g() + b"{"
    for i, (name, value) in enumerate(members):
        out += g() + (b"," + g() if i else b"") + b'"' + name + b'"' + g() + b":" + g() + value
    return out + g() + b"}" + g()


def base_case(template, name, members=None, status=OK, key="base", gaps=None):
    bkey, bmembers = BASE[id(template)]
    return Case(name, template, text_of(bmembers if members is None else members, gaps), bkey if key == "base" else key, status)


def field_order_cases():
    out = [base_case(t, f"compact {n}") for t, n in ((COUNTER, "counter"), (BANK, "bank"), (SDK, "sdk"))]
    for perm in itertools.permutations(BASE[id(COUNTER)][1]):
        out.append(base_case(COUNTER, "counter order " + b",".join(m[0] for m in perm).decode(), list(perm)))
    rng = random.Random(SEED)
    perms = list(itertools.permutations(BASE[id(BANK)][1]))  # four fields: 24 orders, every one of them, in a seeded sequence
    rng.shuffle(perms)
    for i, perm in enumerate(perms):
        perm = list(perm)
        out.append(base_case(BANK, f"bank order {i} " + b",".join(m[0][:3] for m in perm).decode(), perm))
    return out


def whitespace_cases():
    out = []
    calls = itertools.count()
    base_case(COUNTER, "", gaps=lambda: b"" if next(calls) >= 0 else b"")
    n_gaps = next(calls)  # in front of {, around every name, colon, value and comma, in front of } and behind it
    assert n_gaps == 14
    for w in WS:
        for at in range(n_gaps + 1):
            counter = itertools.count()
            out.append(base_case(COUNTER, f"ws {w!r} at gap {at}", gaps=lambda: w if next(counter) == at else b""))
    assert len({c.value for c in out}) == 4 * n_gaps + 1  # (the last `at` is beyond the gaps: the compact text, once)
    rng = random.Random(SEED + 1)
    for t, n in ((COUNTER, "counter"), (BANK, "bank"), (SDK, "sdk")):
        out.append(base_case(t, f"ws everywhere {n}", gaps=lambda: b"".join(rng.choice(WS) for _ in range(rng.randint(1, 3)))))
    return out


def nested(depth, obj=False, mixed=False):
    text = b"1"
    for d in range(depth):
        text = b'{"a":' + text + b"}" if (obj or (mixed and d % 2)) else b"[" + text + b"]"
    return text


UNKNOWN_VALUES = [
    ("string", b'"x"'), ("empty string", b'""'), ("zero", b"0"), ("negative zero", b"-0"), ("fraction", b"-12.5"), ("exponent", b"1E5"),
    ("signed exponent", b"-0.5e+10"), ("negative exponent", b"2e-3"), ("true", b"true"), ("false", b"false"), ("null", b"null"),
    ("empty object", b"{}"), ("empty array", b"[]"), ("spaced empties", b"{ } "), ("array", b'[1,"a",null,true,[],{}]'),
    ("object", b'{"k":1,"l":{"m":[false]},"n":"s"}'), ("spaced nest", b'[ 1 , { "a" : [ ] , "b" : { } } ]'),
    ("string with }", b'"a}b"'), ("string with ]", b'"a]b"'), ("string with quote", b'"a\\"b"'), ("string ending in backslash", b'"ab\\\\"'),
    ("surrogate pair", b'"\\uD83D\\uDE00"'), ("lone surrogate", b'"\\uDC00"'), ("every escape", b'"\\"\\\\\\/\\b\\f\\n\\r\\t\\u00e9"'),
    ("raw utf-8", "\"\u00e9\u6f22\U0001F600\"".encode("utf-8")), ("a known name inside", b'{"count":"no","balance":null}'),
    ("depth 1", nested(1)), ("depth 31", nested(31)), ("depth 32", nested(32)), ("object depth 32", nested(32, obj=True)), ("mixed depth 32", nested(32, mixed=True)),
]


def unknown_field_cases():
    out = []
    for t, n in ((COUNTER, "counter"), (BANK, "bank")):
        members = BASE[id(t)][1]
        for at in range(len(members) + 1):
            for what, text in UNKNOWN_VALUES if t is COUNTER or at == 1 else UNKNOWN_VALUES[:3]:
                out.append(base_case(t, f"{n} unknown {what} at {at}", members[:at] + [(b"extra", text)] + members[at:]))
    out.append(base_case(SDK, "sdk unknown in front", [(b"owner", b'"o"')] + BASE[id(SDK)][1]))
    out.append(base_case(SDK, "sdk unknown behind", BASE[id(SDK)][1] + [(b"owner", b'{"a":[1]}')]))
    m = BASE[id(COUNTER)][1]
    for what, text in (("depth 33", nested(33)), ("object depth 33", nested(33, obj=True)), ("mixed depth 33", nested(33, mixed=True))):
        out.append(base_case(COUNTER, "unknown " + what, m[:1] + [(b"extra", text)] + m[1:], SYNTAX))
    out.append(base_case(COUNTER, "40 KB of unknown string", m[:2] + [(b"blob", b'"' + b"x}]\\\"" * 8192 + b'"')] + m[2:]))
    return out


def name_cases():
    m = BASE[id(COUNTER)][1]
    return [
        base_case(COUNTER, "escaped first letter", [m[0], (b"\\u0063ount", m[1][1]), m[2]]),
        base_case(COUNTER, "escaped inner letter", [m[0], (b"c\\u006funt", m[1][1]), (b"versio\\u006E", m[2][1])]),
        base_case(COUNTER, "escaped solidus in an unknown name", m + [(b"a\\/b", b"1")]),
        base_case(COUNTER, "a proper prefix of a name", [m[0], (b"coun", b'"skipped"'), m[1], m[2]]),
        base_case(COUNTER, "a name one longer", [m[0], (b"counter", b"[0]"), m[1], m[2]]),
        base_case(COUNTER, "an empty name", [(b"", b"null")] + m),
        base_case(COUNTER, "only the prefix", [m[0], (b"coun", m[1][1]), m[2]], MISSING),
        base_case(COUNTER, "only the longer name", [m[0], (b"counter", m[1][1]), m[2]], MISSING),
        base_case(COUNTER, "another letter case", [m[0], (b"Count", m[1][1]), m[2]], MISSING),
        base_case(COUNTER, "a surrogate escape in a name", m + [(b"\\uD83D", b"1")], SURROGATE),
        base_case(COUNTER, "an unknown escape in a name", m + [(b"\\x", b"1")], ESCAPE),
        base_case(COUNTER, "a raw control byte in a name", m + [(b"a\x1fb", b"1")], STRING),
    ]


def duplicate_cases():
    c, b = BASE[id(COUNTER)][1], BASE[id(BANK)][1]
    return [
        base_case(COUNTER, "a number twice", [c[0], (b"count", b"5"), c[2], c[1]]),
        base_case(COUNTER, "a number twice, adjacent", [c[0], (b"count", b"5"), c[1], c[2]]),
        base_case(COUNTER, "the KEY twice", [c[0], c[1], c[0], c[2]]),
        base_case(BANK, "a STR twice", [b[0], (b"accountOwner", b'"first \\n owner"'), b[2], b[3], b[1]]),
        base_case(BANK, "a Double twice", [b[0], b[1], (b"balance", b"7"), b[2], b[3]]),
        base_case(COUNTER, "the KEY twice, the last one wrong", [c[0], c[1], c[2], (b"aggregateId", b'"agg-2"')], KEY_MISMATCH),
        base_case(COUNTER, "the KEY twice, the first one wrong", [(b"aggregateId", b'"agg-2"'), c[1], c[2], c[0]], KEY_MISMATCH),
        base_case(COUNTER, "a bad earlier number", [c[0], (b"count", b"null"), c[1], c[2]], INT),
        base_case(COUNTER, "an earlier number out of range", [c[0], (b"count", b"2147483648"), c[1], c[2]], RANGE),
        base_case(BANK, "a bad earlier string", [b[0], (b"accountOwner", b'"\\uD800"'), b[1], b[2], b[3]], SURROGATE),
    ]


LONG = (b' {"extra":[1,{"a":"b\\"}"}],\n"version" : 42 ,"aggregateId":"agg-1","x":-0.5e+10,"n":null,"t":true,"f":false,"\\u0063ount":-17,"s":"\\u00e9\\\\"}')


def refusal_cases():
    c, b = BASE[id(COUNTER)][1], BASE[id(BANK)][1]
    raw = lambda name, text, status, t=COUNTER, key="base": Case(name, t, text, BASE[id(t)][0] if key == "base" else key, status)  # noqa: E731
    out = [raw("an empty object", b"{}", MISSING), raw("an empty object, spaced", b" { } ", MISSING), raw("an empty object for the sdk sample", b"{}", MISSING, SDK)]
    for t, n in ((COUNTER, "counter"), (BANK, "bank")):
        m = BASE[id(t)][1]
        for i in range(len(m)):
            out.append(base_case(t, f"{n} without {m[i][0].decode()}", m[:i] + m[i + 1:], MISSING))
    comma = text_of(c)
    out += [
        raw("a top-level array", b"[" + text_of(c) + b"]", SYNTAX), raw("a top-level number", b"17", SYNTAX), raw("a top-level string", b'"count"', SYNTAX),
        raw("a top-level null", b"null", SYNTAX), raw("nothing but whitespace", b" \t\n\r", SYNTAX), raw("nothing", b" ", SYNTAX),
        raw("an object that never closes", comma[:-1], SYNTAX), raw("an object that closes with ]", comma[:-1] + b"]", SYNTAX),
        raw("a trailing comma", comma[:-1] + b",}", SYNTAX), raw("a leading comma", b"{," + comma[1:], SYNTAX),
        raw("two commas", comma.replace(b',"count"', b',,"count"'), SYNTAX),
        raw("a missing colon", comma.replace(b'"count":', b'"count"'), SYNTAX), raw("a missing comma", comma.replace(b',"version"', b' "version"'), SYNTAX),
        raw("a name without quotes", comma.replace(b'"count"', b"count"), SYNTAX), raw("a single-quoted name", comma.replace(b'"count"', b"'count'"), SYNTAX),
        raw("a known number followed by junk", comma.replace(b"-17", b"-17x"), SYNTAX),
        raw("bytes behind the closing brace", comma + b"x", TRAILING), raw("a second object", comma + b" {}", TRAILING),
        raw("a NUL behind the closing brace", comma + b"\x00", TRAILING), raw("a comma behind the closing brace", comma + b"\n,", TRAILING),
        raw("a form feed is no whitespace", b"\x0c" + comma, SYNTAX), raw("a byte order mark", b"\xef\xbb\xbf" + comma, SYNTAX),
        raw("null for an Int", comma.replace(b"-17", b"null"), INT), raw("a fraction for an Int", comma.replace(b"-17", b"1.0"), INT),
        raw("an exponent for an Int", comma.replace(b"-17", b"1e2"), INT), raw("a string for an Int", comma.replace(b"-17", b'"1"'), INT),
        raw("an Int out of range", comma.replace(b"-17", b"-2147483649"), RANGE),
        raw("null for the KEY", comma.replace(b'"agg-1"', b"null"), STRING), raw("a number for the KEY", comma.replace(b'"agg-1"', b"1"), STRING),
        raw("another id", comma.replace(b'"agg-1"', b'"agg-2"'), KEY_MISMATCH),
        raw("null for a STR", text_of([b[0], (b"accountOwner", b"null"), b[2], b[3]]), STRING, BANK),
        raw("null for a Double", text_of(b[:3] + [(b"balance", b"null")]), NUMBER, BANK),
        raw("a string for a Double", text_of(b[:3] + [(b"balance", b'"1"')]), NUMBER, BANK),
        raw("a word for a Double", text_of(b[:3] + [(b"balance", b"true")]), NUMBER, BANK),
        raw("a Double that ends in its exponent", text_of(b[:3] + [(b"balance", b"1e")]), NUMBER, BANK),
        raw("a surrogate in a STR", text_of([b[0], (b"accountOwner", b'"\\uD83D\\uDE00"'), b[2], b[3]]), SURROGATE, BANK),
    ]
    for what, text in (("01", b"01"), ("1.", b"1."), (".5", b".5"), ("1e", b"1e"), ("1e+", b"1e+"), ("-", b"-"), ("-a", b"-a"), ("+1", b"+1"), ("0x10", b"0x10"), ("1.e5", b"1.e5"),
                       ("tru", b"tru"), ("truE", b"truE"), ("nul", b"nul"), ("fals", b"fals"), ("True", b"True"), ("NaN", b"NaN"), ("Infinity", b"Infinity"),
                       ("a raw 0x1f in a string", b'"a\x1fb"'), ("a raw newline in a string", b'"a\nb"'), ("\\u12G4", b'"\\u12G4"'), ("\\u12", b'"\\u12"'), ("\\x", b'"\\x41"'),
                       ("a string that never ends", b'"abc'), ("[1,]", b"[1,]"), ("[,1]", b"[,1]"), ("[1 2]", b"[1 2]"), ('{"a"}', b'{"a"}'), ('{"a":}', b'{"a":}'),
                       ("{1:2}", b"{1:2}"), ('{"a":1,}', b'{"a":1,}'), ("[1}", b"[1}"), ('{"a":1]', b'{"a":1]'), ("[", b"["), ("nothing", b""), ("a comment", b"/**/1")):
        out.append(base_case(COUNTER, "skipped value " + what, c[:1] + [(b"extra", text)] + c[1:], SYNTAX))
        out.append(base_case(COUNTER, "skipped value " + what + ", last", c + [(b"extra", text)], SYNTAX))
    assert document(LONG)
    for cut in range(len(LONG)):
        out.append(raw(f"the long case cut at {cut}", LONG[:cut], REFUSED))  # (SYNTAX, STRING or INT by where the cut falls: never OK)
    out.append(raw("the long case", LONG, OK))
    return out


def wrap(key: bytes, payload: bytes) -> bytes:
    """``State{aggregateId = key, payload}`` as scalapb writes it: proto3 omits an empty field."""
    return (b"\x0a" + protobuf_varint(len(key)) + key if key else b"") + (b"\x12" + protobuf_varint(len(payload)) + payload if payload else b"")


def enveloped(case: Case, key=None) -> Case:
    key = case.key if key is None else key
    value = wrap(key or b"", case.value)
    return Case(case.name + " enveloped", case.template, value, key, case.status, True, len(value) - len(case.value))


def envelope_cases():
    plain = field_order_cases()[:12] + whitespace_cases()[-3:] + name_cases() + duplicate_cases() + unknown_field_cases()[:40]
    plain += [c for c in refusal_cases() if c.status >= 0][:60]
    out = [enveloped(c) for c in plain if len(c.value) < 4000]
    m = BASE[id(COUNTER)][1]
    for paylen in (127, 128, 16383, 16384):  # the payload length's varint steps, reached with an unknown string
        frame = len(text_of(m[:1] + [(b"pad", b'""')] + m[1:]))
        c = base_case(COUNTER, f"payload of {paylen} bytes", m[:1] + [(b"pad", b'"' + b"p" * (paylen - frame) + b'"')] + m[1:])
        assert len(c.value) == paylen
        out.append(enveloped(c))
    for idlen in (0, 127, 128):
        key = b"k" * idlen
        out.append(enveloped(base_case(SDK, f"sdk id of {idlen} bytes", [(b"x", b"[]")] + BASE[id(SDK)][1], key=key)))
    good = enveloped(base_case(SDK, "sdk"))
    out += [Case("unknown tag behind field 2", SDK, good.value + b"\x1a\x00", SDK_KEY, ENVELOPE, True),
            Case("field 2 before field 1", SDK, good.value[4:] + good.value[:4], SDK_KEY, ENVELOPE, True),
            Case("another id in field 1", SDK, good.value, b"k2", KEY_MISMATCH, True),
            Case("an absent payload", SDK, b"\x0a\x02k1", SDK_KEY, SYNTAX, True),
            Case("a payload of one space", SDK, wrap(SDK_KEY, b" "), SDK_KEY, SYNTAX, True)]
    return out


def corpus():
    """Every unmutated bare case."""
    return field_order_cases() + whitespace_cases() + unknown_field_cases() + name_cases() + duplicate_cases() + refusal_cases()


_ALPHABET = b'"\\u/bfnrt0123456789aAfF-+.eE{}[]:, \t\n\x01\x1f\x7f\xc3\xff'


def mutations(cases, per_case, seed=SEED + 7):
    """Seeded one-byte mutations: a byte replaced by, or inserted from, the bytes the parser branches on; a byte erased; a
    random byte.  Long values are mutated near their head and tail."""
    rng = random.Random(seed)
    out = []
    for c in cases:
        if not c.value:
            continue
        for _ in range(per_case):
            m = bytearray(c.value)
            at = rng.randrange(len(m)) if len(m) < 256 else rng.choice([rng.randrange(0, 100), len(m) - 1 - rng.randrange(0, 100)])
            op = rng.randrange(4)
            if op == 0:
                m[at] = rng.choice(_ALPHABET)
            elif op == 1:
                m.insert(at, rng.choice(_ALPHABET))
            elif op == 2:
                del m[at]
            else:
                m[at] = rng.randrange(256)
            out.append(Case(c.name + " mutated", c.template, bytes(m), c.key, MUTATED, c.envelope, c.payload_at))
    return out


# ---- compact text, rewritten: what the topic tests feed ---------------------------------------------------------------------
def members_of(text: bytes):
    """The ``(raw name, raw value text)`` members of a COMPACT object whose values are strings and numbers (what the encoders write)."""
    assert text[:1] == b"{" and text[-1:] == b"}"
    out, i = [], 1
    while i < len(text) - 1:
        tokens = []
        for _ in range(2):  # the name, then the value
            j = i
            if text[i:i + 1] == b'"':
                j += 1
                while text[j:j + 1] != b'"':
                    j += 2 if text[j:j + 1] == b"\\" else 1
                j += 1
            else:
                while text[j:j + 1] not in (b",", b"}"):
                    j += 1
            tokens.append(text[i:j])
            i = j + 1  # behind the colon / the comma / the closing brace
        out.append((tokens[0][1:-1], tokens[1]))
    assert text_of(out) == text
    return out


def rewritten(text: bytes, rng: random.Random, unknown=(b"addedLater", b'{"since":[2,{"x":null}],"note":"a}\\"]"}')) -> bytes:
    """A compact value as another writer of the same document might have written it: the members in a seeded order, seeded
    whitespace in the gaps, and one member the template does not name."""
    members = members_of(text)
    rng.shuffle(members)
    members.insert(rng.randrange(len(members) + 1), unknown)
    return text_of(members, gaps=lambda: b"".join(rng.choice(WS) for _ in range(rng.choice((0, 0, 1, 2)))))
