"""The corpus of event values for the string fields of events (``surge_event_json_string_spans``, ``include/surge_ingest.h``)
and its references (no test functions; shared by tests/test_event_strings.py and tests/test_event_strings_gpu.py).

A case's ``want`` has one entry per string column: the expected string (``str``: what ``json.loads`` reads out of the value, or,
where the rule differs from a dict on purpose — a duplicate, an escaped name, position 25 — what the case was built to give),
``None`` for a column the record's class does not name, or an ``int``: the refusal."""
import json
from dataclasses import dataclass
from typing import List

import numpy as np

import event_envelope_cases as eec
from surge_amd.encode import DECODE_ESCAPE, DECODE_STRING, DECODE_SURROGATE
from surge_amd.ingest import ARG_F64, ARG_I32, ARG_NONE, EVENT_STRING_MISSING, EVENT_STRING_RECORD, EventJsonTemplate, EventStrings

CREATED, UPDATED = "docs.command.BankAccountCreated", "docs.command.BankAccountUpdated"
_BANK_TYPES = [(CREATED, 0, "", "balance", ARG_F64), (UPDATED, 1, "", "newBalance", ARG_F64)]
BANK = EventJsonTemplate("_type", _BANK_TYPES)
BANK_ENV = EventJsonTemplate("_type", _BANK_TYPES, envelope="protobuf_event")
BANK_STRINGS = EventStrings([(CREATED, "accountOwner", 0), (CREATED, "securityCode", 1)])
# the synthetic two-class case: two classes name column 0 through different fields, one of them column 2 as well, one nothing
TWO = EventJsonTemplate("k", [("a", 0, "", "n", ARG_I32), ("b", 1, "", "n", ARG_I32), ("c", 2, "", "", ARG_NONE)])
TWO_STRINGS = EventStrings([("a", "owner", 0), ("b", "label", 0), ("b", "tag", 2)])
SHORT = EventJsonTemplate("", [("", 0, "", "", ARG_NONE)])  # no discriminator: every value is the one class
SHORT_STRINGS = EventStrings([("", "o", 3)])
RULES = {"bank": (BANK, BANK_STRINGS), "bank_env": (BANK_ENV, BANK_STRINGS), "two": (TWO, TWO_STRINGS), "short": (SHORT, SHORT_STRINGS)}

SINGLE = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]
BOUNDARIES = [b"\\u007f", b"\\u0080", b"\\u07ff", b"\\u07FF", b"\\u0800", b"\\uffff", b"\\ud7ff", b"\\ue000", b"\\u0000", b"\\u001f"]
RAW_UTF8 = ["\x7f".encode(), "\u0080".encode(), "\u07ff".encode(), "\u0800".encode(), "\uffff".encode(), "\U00010000".encode(), "\U0010ffff".encode()]  # 1, 2, 2, 3, 3, 4, 4 bytes


@dataclass
class Case:
    name: str
    rule: str          # a key of RULES
    value: bytes
    want: List         # per column: str, None (ABSENT) or int (the refusal)
    key: bytes = b""   # the record's key on a topic (the GPU tests give one to the cases they push)

    @property
    def refused(self) -> bool:
        return any(isinstance(w, int) for w in self.want)


def created(owner_raw: bytes, code_raw: bytes = b"0042", account: bytes = b"acc", balance: bytes = b"1.5") -> bytes:
    """a BankAccountCreated value with the given still-escaped strings, in the writer's field order"""
    return (b'{"accountNumber":"' + account + b'","accountOwner":"' + owner_raw + b'","securityCode":"' + code_raw + b'","balance":' + balance +
            b',"_type":"' + CREATED.encode() + b'"}')


def updated(account: bytes = b"acc", balance: bytes = b"2.5") -> bytes:
    return b'{"accountNumber":"' + account + b'","newBalance":' + balance + b',"_type":"' + UPDATED.encode() + b'"}'


def obj(fields) -> bytes:
    """``(raw name, raw value text)`` pairs -> the object, compact"""
    return b"{" + b",".join(b'"' + n + b'":' + v for n, v in fields) + b"}"


def _by_json(name, value, rule="bank", payload=None) -> Case:
    """an accepted BankAccountCreated value: the expectation is json.loads of its text"""
    o = json.loads(value if payload is None else payload)
    return Case(name, rule, value, [o["accountOwner"], o["securityCode"], None, None])


def escape_cases() -> List[Case]:
    out = []
    for i, raw in enumerate(SINGLE + BOUNDARIES + RAW_UTF8):
        for j, text in enumerate((raw, raw + b"tail", b"head" + raw, b"a" + raw + b"b", raw * 3)):
            out.append(_by_json(f"escape {i}.{j}", created(text, code_raw=text[::-1] if b"\\" not in text and max(text) < 0x80 else raw)))
    return out


def dumped_cases(n=120, seed=11) -> List[Case]:
    """values written by json.dumps, both ways of writing non-ASCII"""
    rng = np.random.default_rng(seed)
    alphabet = list("abc xyz019\"\\/\b\f\n\r\t\x00\x01\x1f\x7f") + ["é", "ß", "\u07ff", "\u0800", "€", "漢", "\uffff", "😀", "\U0010ffff"]
    out = []
    for it in range(n):
        owner = "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), size=int(rng.integers(0, 40))))
        code = "".join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), size=int(rng.integers(0, 6))))
        ascii_only = bool(it % 2) and all(ord(ch) < 0x10000 for ch in owner + code)  # (json.dumps writes a surrogate pair beyond the BMP: refused, see the named inputs)
        o = {"accountNumber": f"acc{it}", "accountOwner": owner, "securityCode": code, "balance": it + 0.5, "_type": CREATED}
        value = json.dumps(o, ensure_ascii=ascii_only, separators=(",", ":") if it % 3 else (", ", " : ")).encode("utf-8")
        out.append(Case(f"dumped {it}", "bank", value, [owner, code, None, None]))
    return out


def _filler(n, first=0):
    return [(b"f%d" % (first + i), [b"1", b'"s"', b"[1,{\"accountOwner\":\"no\"}]", b"null", b"true", b'{"a":"}"}'][i % 6]) for i in range(n)]


def position_cases() -> List[Case]:
    t, code, bal = (b"_type", b'"' + CREATED.encode() + b'"'), (b"securityCode", b'"c"'), (b"balance", b"7")
    owner = (b"accountOwner", b'"O"')
    good = ["O", "c", None, None]
    return [
        Case("owner first", "bank", obj([owner, t, code, bal] + _filler(3)), good),
        Case("owner last", "bank", obj([t, code, bal] + _filler(3) + [owner]), good),
        Case("owner behind 23 other fields", "bank", obj([t, code, bal] + _filler(20) + [owner]), good),
        Case("owner at position 25 does not count", "bank", obj([t, code, bal] + _filler(21) + [owner]), [EVENT_STRING_MISSING, "c", None, None]),
        Case("owner at position 25 behind an escaped name, which takes no position", "bank", obj([t, code, bal] + _filler(10) + [(b"f\\u0058", b"1")] + _filler(10, 10) + [owner]), good),
        Case("escaped name does not count, the plain one behind it does", "bank", obj([t, (b"account\\u004fwner", b'"escaped"'), owner, code, bal]), good),
        Case("only an escaped name", "bank", obj([t, (b"account\\u004fwner", b'"escaped"'), code, bal]), [EVENT_STRING_MISSING, "c", None, None]),
        Case("a numeric field of the same name in front", "bank", obj([t, (b"accountOwner", b"5"), owner, code, bal]), good),
        Case("an object, null and true of the same name in front", "bank", obj([t, (b"accountOwner", b'{"accountOwner":"in"}'), (b"accountOwner", b"null"), (b"accountOwner", b"true"), owner, code, bal]), good),
        Case("a duplicate field: the first wins", "bank", obj([t, owner, (b"accountOwner", b'"second"'), code, (b"securityCode", b'"d"'), bal]), good),
        Case("the first is refused though a good one follows", "bank", obj([t, (b"accountOwner", b'"\\q"'), owner, code, bal]), [DECODE_ESCAPE, "c", None, None]),
        Case("empty strings", "bank", created(b"", b""), ["", "", None, None]),
        Case("white space everywhere", "bank", b' { "_type" : "' + CREATED.encode() + b'" ,\n"accountOwner"\t:\r"O" , "securityCode":"c","balance" : 1 } \n', good),
        Case("an updated event names nothing", "bank", updated(), [None] * 4),
        Case("an updated event with the fields of a created one", "bank", obj([(b"_type", b'"' + UPDATED.encode() + b'"'), owner, code, (b"newBalance", b"1")]), [None] * 4),
        Case("the last discriminator decides", "bank", obj([(b"_type", b'"' + UPDATED.encode() + b'"'), owner, code, bal, t]), good),
        Case("a 16-byte value", "short", b'{"k":"a","o":""}', [None, None, None, ""]),
        Case("no discriminator: the one class", "short", b'{"o":"x\\u00e9"}', [None, None, None, "x\u00e9"]),
        Case("class a: owner", "two", b'{"k":"a","n":1,"owner":"Ann","label":"not mine","tag":"nor this"}', ["Ann", None, None, None]),
        Case("class b: label and tag", "two", b'{"owner":"not mine","label":"L\\n","tag":"","n":2,"k":"b"}', ["L\n", None, "", None]),
        Case("class c names nothing", "two", b'{"k":"c","owner":"x"}', [None] * 4),
        Case("class b without its tag", "two", b'{"k":"b","n":1,"label":"L"}', ["L", None, EVENT_STRING_MISSING, None]),
    ]


def envelope_cases() -> List[Case]:
    out = []
    for n in eec.ID_LENGTHS:
        aid = eec.id_of(n)
        payload = created(b"own\\u00e9r %d" % n, b"c%d" % n)
        out.append(_by_json(f"enveloped id{n}", eec.wrap(aid, payload), "bank_env", payload))
        out[-1].key = aid
    for n in (126, 127, 128, 129, 16383, 16384):  # payload lengths on both sides of the varint steps
        base = len(created(b"", b"\\t"))
        payload = created(b"p" * (n - base), b"\\t")
        assert len(payload) == n
        out.append(_by_json(f"enveloped payload{n}", eec.wrap(b"pay%d" % n, payload), "bank_env", payload))
        out[-1].key = b"pay%d" % n
    out.append(Case("enveloped updated", "bank_env", eec.wrap(b"u", updated()), [None] * 4, b"u"))
    return out


def refused_cases() -> List[Case]:
    rec = [EVENT_STRING_RECORD] * 4
    return [
        Case("no such field", "bank", obj([(b"_type", b'"' + CREATED.encode() + b'"'), (b"securityCode", b'"c"'), (b"balance", b"1")]), [EVENT_STRING_MISSING, "c", None, None]),
        Case("neither field", "bank", obj([(b"_type", b'"' + CREATED.encode() + b'"'), (b"balance", b"1")]), [EVENT_STRING_MISSING, EVENT_STRING_MISSING, None, None]),
        Case("the field is a number", "bank", obj([(b"_type", b'"' + CREATED.encode() + b'"'), (b"accountOwner", b"12"), (b"securityCode", b'"c"'), (b"balance", b"1")]),
             [EVENT_STRING_MISSING, "c", None, None]),
        Case("a raw control byte", "bank", created(b"ab\x1fcd"), [DECODE_STRING, "0042", None, None]),
        Case("an unknown escape", "bank", created(b"ab\\qcd"), [DECODE_ESCAPE, "0042", None, None]),
        Case("not a hex digit", "bank", created(b"\\u00g1"), [DECODE_ESCAPE, "0042", None, None]),
        Case("a surrogate", "bank", created(b"\\ud83d\\ude00"), [DECODE_SURROGATE, "0042", None, None]),
        Case("a low surrogate in the code", "bank", created(b"ok", b"x\\uDFFFy"), ["ok", DECODE_SURROGATE, None, None]),
        Case("the string ends inside \\u12", "bank", created(b"abc\\u12"), [DECODE_STRING, "0042", None, None]),
        Case("not an object", "bank", b'["accountOwner"]', rec),
        Case("an empty value", "bank", b"", rec),
        Case("an unknown class", "bank", created(b"x").replace(b"Created", b"Closed"), rec),
        Case("no discriminator field", "bank", obj([(b"accountOwner", b'"x"'), (b"securityCode", b'"c"')]), rec),
        Case("the discriminator is a number", "bank", obj([(b"_type", b"1"), (b"accountOwner", b'"x"')]), rec),
        Case("the discriminator is escaped", "bank", created(b"x").replace(b"docs.command", b"docs\\u002ecommand"), rec),
        Case("trailing bytes", "bank", created(b"x") + b"x", rec),
        Case("cut inside the owner", "bank", created(b"x" * 10)[:40], rec),
        Case("bare JSON where an envelope is named", "bank_env", created(b"x"), rec),
        Case("an envelope with a third field", "bank_env", eec.wrap(b"a", created(b"x")) + b"\x1a\x00", rec),
        Case("an enveloped empty payload", "bank_env", eec.wrap(b"a", b""), rec),
        Case("an enveloped refusal", "bank_env", eec.wrap(b"a", created(b"\\q")), [DECODE_ESCAPE, "0042", None, None], b"a"),
    ]


def accepted_cases() -> List[Case]:
    return [c for c in escape_cases() + dumped_cases() + position_cases() + envelope_cases() if not c.refused]


def all_cases() -> List[Case]:
    return escape_cases() + dumped_cases() + position_cases() + envelope_cases() + refused_cases()


_ALPHABET = b'"\\u/bfnrt0123456789aAfFdD8 {}[]:,\x01\x1f\x7f\xc3\xff\x0a\x12'


def mutations(cases, per_case=6, seed=2026) -> List[Case]:
    """Seeded byte mutations of the cases' values over the bytes the walk branches on; ``want`` is not known (``["?"]``)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in cases:
        for _ in range(per_case):
            m = bytearray(c.value) or bytearray(b"{")
            for _ in range(1 + int(rng.integers(3))):
                at = int(rng.integers(len(m))) if len(m) < 200 or rng.random() < 0.3 else int(rng.choice([rng.integers(0, 60), len(m) - 1 - rng.integers(0, 60)]))
                op = int(rng.integers(4))
                if op == 0:
                    m[at] = _ALPHABET[int(rng.integers(len(_ALPHABET)))]
                elif op == 1:
                    m.insert(at, _ALPHABET[int(rng.integers(len(_ALPHABET)))])
                elif op == 2:
                    del m[at:at + 1 + int(rng.integers(3))]
                else:
                    m[at] = int(rng.integers(256))
                if not m:
                    m = bytearray(b"\\")
            if rng.random() < 0.25:
                del m[int(rng.integers(len(m) + 1)):]
            out.append(Case(c.name + " mutated", c.rule, bytes(m), ["?"], c.key))
    return out
