"""The corpus of protobuf ``State{aggregateId, payload}`` values for the envelope route of the state decoder, and its
references (no test functions; shared by tests/test_state_envelope.py and tests/test_state_envelope_gpu.py).

The reference for a value's id and payload is the protobuf runtime (``State.FromString``, the class of
``state_out_cases.protobuf_state_class``); for the payload's fields it is ``decode_state_host(envelope="none")`` — the bare
route, pinned by tests/test_state_decode.py — or ``json.loads``.  Accepted values are built by the runtime's own encoder;
only the over-long varints and the refusals are spelled by hand, byte by byte."""
import json
from dataclasses import dataclass

import numpy as np

import state_out_cases as soc
from fixture_models import SdkBankAccount, protobuf_varint, sdk_sample_state_bytes
from surge_amd.encode import (DECODE_ENVELOPE, DECODE_KEY_MISMATCH, DECODE_LITERAL, DECODE_OK, DECODE_TRAILING, JP_F64, JP_I32, JsonTemplate,
                              decode_state_host)

SDK = JsonTemplate((b'{"balance":', (JP_I32, 0), b"}"))  # json4s write(BankAccount(balance)) of the SDK sample (Main.scala:19, 41-60)
COUNTER, BANK = JsonTemplate.counter(), JsonTemplate.bank_account()
F64_ONLY = JsonTemplate((b'{"balance":', (JP_F64, 16), b"}"))
ID_LENGTHS = (0, 1, 127, 128, 16383, 16384)
# the three Doubles of tests/test_state_decode.py:125-126 that Eisel-Lemire cannot decide
AMBIGUOUS_DOUBLES = ("0.1000000000000000055511151231257827021181583404541015625", "9007199254740993.00000000000000000001",
                     "123456789012345678901234567890")
BANK_KEY = "acct-é-1"
BANK_PAYLOAD = ('{"accountNumber":"acct-é-1","accountOwner":"J \\"q\\" \\/ \\u20ac","securityCode":"","balance":-1.25E+3}').encode("utf-8")


def State():
    return soc.protobuf_state_class()


def wrap(key, payload: bytes) -> bytes:
    """The protobuf runtime's bytes of ``State(aggregateId=key, payload=payload)``; ``key``: ``str`` or UTF-8 ``bytes``."""
    key = key.decode("utf-8") if isinstance(key, bytes) else key
    return State()(aggregateId=key, payload=payload).SerializeToString()


def runtime_fields(value: bytes):
    """``(id bytes, payload)`` as the protobuf runtime parses ``value``, or ``None`` when it rejects it."""
    try:
        m = State().FromString(value)
    except Exception:
        return None
    return m.aggregateId.encode("utf-8"), bytes(m.payload)


@dataclass
class Case:
    name: str
    template: JsonTemplate
    value: bytes
    key: bytes          # the id the value was built around (what a key table holds for its aggregate)
    status: int = DECODE_OK


def id_of(length: int) -> bytes:
    return soc._id_of(length)


def counter_payload(key: bytes, count: int, version: int) -> bytes:
    return b'{"aggregateId":' + soc.quote(key) + b',"count":%d,"version":%d}' % (count, version)


def accepted_cases():
    out = []
    for n in ID_LENGTHS:  # (length 0: the runtime leaves field 1 out)
        key = id_of(n)
        out.append(Case(f"sdk id{n}", SDK, wrap(key, b'{"balance":%d}' % (n - 7)), key))
        out.append(Case(f"counter id{n}", COUNTER, wrap(key, counter_payload(key, n, -n)), key))
    for key in ("ünï-✓-ключ", "\U0001d11e\U00010348", 'we"ird\\id', '"', "tab\there\nnl"):
        kb = key.encode("utf-8")
        out.append(Case(f"sdk {key!r}", SDK, wrap(kb, b'{"balance":2147483647}'), kb))
        out.append(Case(f"counter {key!r}", COUNTER, wrap(kb, counter_payload(kb, -2**31, 7)), kb))  # raw in field 1, escaped in the KEY
    out.append(Case("bank account", BANK, wrap(BANK_KEY, BANK_PAYLOAD), BANK_KEY.encode("utf-8")))
    # payload lengths on both sides of 127 / 128 and 16383 / 16384: what the encoder's envelope cases emit, decoded back
    for case in soc.envelope_cases():
        data, off, _ = case.reference()
        for a, idlen, paylen in zip(case.prop["at"], case.prop["ids"], case.prop["payloads"]):
            value = data[off[a]:off[a + 1]]
            assert len(runtime_fields(value)[1]) == paylen and len(case.keys[a]) == idlen
            out.append(Case(f"{case.name} id{idlen} payload{paylen}", JsonTemplate(case.template), value, case.keys[a]))
    return out


def overlong_cases():
    """Non-minimal length varints the runtime accepts: ``0x85 0x00`` and a 5-byte spelling, both for length 5 — and for the
    payload's 15."""
    pay = b'{"balance":-12}'
    five = bytes([0x85, 0x80, 0x80, 0x80, 0x00])
    return [Case("2-byte varint for 5", SDK, b"\x0a\x85\x00hello\x12" + protobuf_varint(len(pay)) + pay, b"hello"),
            Case("5-byte varint for 5", SDK, b"\x0a" + five + b"hello\x12" + protobuf_varint(len(pay)) + pay, b"hello"),
            Case("over-long payload length", SDK, b"\x0a\x05hello\x12\x8f\x80\x00" + pay, b"hello"),
            Case("over-long, no id", SDK, b"\x12\x8f\x00" + pay, b"")]


def refused_cases():
    pay = b'{"balance":1}'
    good = sdk_sample_state_bytes("k1", SdkBankAccount(1))
    f1, f2 = b"\x0a\x02k1", b"\x12" + protobuf_varint(len(pay)) + pay
    assert good == f1 + f2
    E = DECODE_ENVELOPE
    return [
        Case("unknown tag 0x1A", SDK, good[:4] + b"\x1a\x01x" + good[4:], b"k1", E),
        Case("unknown tag 0x1A behind field 2", SDK, good + b"\x1a\x00", b"k1", E),
        Case("wrong wire type 0x08", SDK, b"\x08\x02k1" + f2, b"k1", E),
        Case("wrong wire type 0x10", SDK, f1 + b"\x10" + f2[1:], b"k1", E),
        Case("field 1 twice", SDK, f1 + f1 + f2, b"k1", E),
        Case("field 2 twice", SDK, f1 + f2 + f2, b"k1", E),
        Case("field 2 before field 1", SDK, f2 + f1, b"k1", E),
        Case("id length beyond the end", SDK, b"\x0a\x7fk1", b"k1", E),
        Case("payload length beyond the end", SDK, f1 + b"\x12" + protobuf_varint(len(pay) + 1) + pay, b"k1", E),
        Case("payload length one short of the end", SDK, f1 + b"\x12" + protobuf_varint(len(pay) - 1) + pay, b"k1", E),
        Case("a 6-byte varint", SDK, b"\x0a\x82\x80\x80\x80\x80\x00k1" + f2, b"k1", E),
        Case("a length of 2^31", SDK, b"\x0a\x80\x80\x80\x80\x08k1" + f2, b"k1", E),
        Case("ends inside a varint", SDK, f1 + b"\x12\x8d", b"k1", E),
        Case("ends behind a tag", SDK, f1 + b"\x12", b"k1", E),
    ]


def other_status_cases():
    good = sdk_sample_state_bytes("k1", SdkBankAccount(1))
    return [
        Case("one flipped id byte", SDK, good[:3] + bytes([good[3] ^ 1]) + good[4:], b"k1", DECODE_KEY_MISMATCH),
        Case("absent id where the key is not empty", SDK, good[4:], b"k1", DECODE_KEY_MISMATCH),
        Case("the key inside the payload differs", COUNTER, wrap(b"k1", counter_payload(b"k2", 1, 1)), b"k1", DECODE_KEY_MISMATCH),
        Case("absent payload", SDK, b"\x0a\x02k1", b"k1", DECODE_LITERAL),
        Case("empty payload spelled out", SDK, b"\x0a\x02k1\x12\x00", b"k1", DECODE_LITERAL),
        Case("payload text longer than the template", SDK, wrap(b"k1", b'{"balance":1} '), b"k1", DECODE_TRAILING),
    ]


def ambiguous_cases():
    return [Case(f"ambiguous {text[:12]}", F64_ONLY, wrap(f"d{i}", b'{"balance":' + text.encode() + b"}"), b"d%d" % i) for i, text in enumerate(AMBIGUOUS_DOUBLES)]


def corpus():
    """Every unmutated case: accepted, over-long, refused, other statuses, ambiguous Doubles."""
    return accepted_cases() + overlong_cases() + refused_cases() + other_status_cases() + ambiguous_cases()


def expected(case, with_key=True):
    """``(status, row bytes, spans)`` of an accepted case from the references alone: the runtime's id and payload, the bare
    route over the payload, the spans moved by where the payload lies (it is the value's last field)."""
    rid, payload = runtime_fields(case.value)
    assert rid == case.key
    rc, st, spans = decode_state_host(case.template, payload, case.key if with_key else None)
    base = len(case.value) - len(payload)
    named = {int(p[1]) for p in case.template.parts if isinstance(p, tuple) and p[0] == 6}
    return rc, st.tobytes(), [(o + base, n) if c in named else (o, n) for c, (o, n) in enumerate(spans)]


def sdk_balance(value: bytes) -> int:
    """The SDK sample's balance by ``json.loads`` of the runtime's payload."""
    return int(json.loads(runtime_fields(value)[1])["balance"])


_ALPHABET = bytes([0x0A, 0x12, 0x1A, 0x08, 0x10, 0x00, 0x01, 0x7F, 0x80, 0x81, 0xFF, 0x85, 0x22, 0x5C, 0x7B, 0x7D]) + b"0123456789-.eE"


def mutations(cases, per_case, seed=2024):
    """Seeded byte mutations of the cases' values: tag / varint / quote bytes written or inserted anywhere, short erasures,
    random bytes, cuts; and, for a third of them, edits that tend to keep the value well-formed — a digit for a digit, a
    letter for a letter (an id byte, mostly), a one-byte length re-spelled over-long.  Long values are mutated near their
    head and tail, where the envelope and the payload's ends lie."""
    rng = np.random.default_rng(seed)
    out = []
    for c in cases:
        for _ in range(per_case):
            m = bytearray(c.value)
            for _ in range(1 + int(rng.integers(3))):
                if not m:
                    m = bytearray(b"\x0a")
                at = int(rng.integers(len(m))) if len(m) < 64 or rng.random() < 0.2 else int(rng.choice([rng.integers(0, 24), len(m) - 1 - rng.integers(0, 24)]))
                op = int(rng.integers(6))
                if op >= 4:
                    if 0x30 <= m[at] <= 0x39:
                        m[at] = 0x30 + int(rng.integers(10))
                    elif chr(m[at]).isalpha() and m[at] < 0x80:
                        m[at] = ord("a") + int(rng.integers(26))
                    elif len(m) > 1 and m[0] in (0x0A, 0x12) and m[1] < 0x80:
                        m[1:2] = bytes([m[1] | 0x80, 0x00])
                elif op == 0:
                    m[at] = _ALPHABET[int(rng.integers(len(_ALPHABET)))]
                elif op == 1:
                    m.insert(at, _ALPHABET[int(rng.integers(len(_ALPHABET)))])
                elif op == 2:
                    del m[at:at + 1 + int(rng.integers(3))]
                else:
                    m[at] = int(rng.integers(256))
            if rng.random() < 0.25:
                del m[int(rng.integers(len(m) + 1)):]
            out.append(Case(c.name + " mutated", c.template, bytes(m), c.key, -1))
    return out
