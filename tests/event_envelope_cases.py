"""The corpus of protobuf ``Event{aggregateId, payload}`` record values for the envelope route of the event decoders, and its
references (no test functions; shared by tests/test_event_envelope.py and tests/test_event_envelope_gpu.py).

The reference for a value's id and payload is the protobuf runtime (``Event.FromString``; the class is built the way
``state_out_cases.protobuf_state_class`` builds ``State``); for the payload's event it is the BARE template's
``EventJsonTemplate.decode`` — the route tests/test_event_decode.py pins.  Accepted values are built by the runtime's own
encoder; only the over-long varints and the refusals are spelled by hand, byte by byte.

A case is a RECORD: the key a producer would write (``<id>`` or ``<id>:<seq>``) and the value.  The id a decoder compares
the envelope with is the key up to its first ``:``."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import state_out_cases as soc
from fixture_models import CounterCommandModel, protobuf_varint
from surge_amd.ingest import ARG_F64, ARG_I32, EventJsonTemplate

PE = "protobuf_event"
ID_LENGTHS = (0, 1, 127, 128, 16383, 16384)
# the three Doubles of tests/test_state_decode.py:125-126 that Eisel-Lemire cannot decide
AMBIGUOUS_DOUBLES = ("0.1000000000000000055511151231257827021181583404541015625", "9007199254740993.00000000000000000001",
                     "123456789012345678901234567890")
# what a refusal says: a fragment of the host's message (surge_event_json_last_error) and of the device decoder's
HOST_REASON = {"envelope": "not the protobuf Event envelope", "mismatch": "is not the record's aggregate id", "json": "not a JSON object"}
DEVICE_REASON = {"envelope": "is not the protobuf Event envelope", "mismatch": "names another aggregateId", "json": "is not the JSON object"}


def _pair(discriminator, types):
    return EventJsonTemplate(discriminator, types, envelope=PE), EventJsonTemplate(discriminator, types)


SDK, SDK_BARE = _pair("", [("", 0, "", "amount", ARG_I32)])       # the SDK sample: json4s write(MoneyDeposited(amount)), Main.scala:21, 42-58
V, V_BARE = _pair("", [("", 3, "", "v", ARG_I32)])                # Event("a", b'{"v":12345}') is exactly 16 bytes
F64, F64_BARE = _pair("", [("", 1, "", "x", ARG_F64)])
_counter = CounterCommandModel().event_json_template()
COUNTER, COUNTER_BARE = _pair(_counter.discriminator, _counter.types)  # a sealed family inside the envelope: the discriminator still selects
BARE_OF = {id(SDK): SDK_BARE, id(V): V_BARE, id(F64): F64_BARE, id(COUNTER): COUNTER_BARE}

_EVENT_CLASS = None


def Event():
    """message Event { string aggregateId = 1; bytes payload = 2; } (multilanguage-protocol.proto:17-20), built with the
    real protobuf runtime so the accepted bytes come from Google's encoder, not from a restatement."""
    global _EVENT_CLASS
    if _EVENT_CLASS is None:
        from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

        fd = descriptor_pb2.FileDescriptorProto(name="surge_multilanguage_event.proto", syntax="proto3")
        m = fd.message_type.add(name="Event")
        F = descriptor_pb2.FieldDescriptorProto
        m.field.add(name="aggregateId", number=1, type=F.TYPE_STRING, label=F.LABEL_OPTIONAL)
        m.field.add(name="payload", number=2, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
        pool = descriptor_pool.DescriptorPool()
        pool.Add(fd)
        _EVENT_CLASS = message_factory.GetMessageClass(pool.FindMessageTypeByName("Event"))
    return _EVENT_CLASS


def wrap(aggregate_id, payload: bytes) -> bytes:
    """The protobuf runtime's bytes of ``Event(aggregateId=aggregate_id, payload=payload)``; the id: ``str`` or UTF-8 ``bytes``."""
    aggregate_id = aggregate_id.decode("utf-8") if isinstance(aggregate_id, bytes) else aggregate_id
    return Event()(aggregateId=aggregate_id, payload=payload).SerializeToString()


def runtime_fields(value: bytes):
    """``(id bytes, payload)`` as the protobuf runtime parses ``value``, or ``None`` when it rejects it."""
    try:
        m = Event().FromString(value)
    except Exception:
        return None
    return m.aggregateId.encode("utf-8"), bytes(m.payload)


def id_of_key(key: bytes) -> bytes:
    """PartitionStringUpToColon: the aggregate id a decoder interns for a record key."""
    return key.split(b":", 1)[0]


@dataclass
class Case:
    name: str
    template: EventJsonTemplate    # the enveloped template
    key: bytes                     # the record's key
    value: bytes
    reason: Optional[str] = None   # None: accepted; else a key of HOST_REASON / DEVICE_REASON

    @property
    def bare(self) -> EventJsonTemplate:
        return BARE_OF[id(self.template)]

    @property
    def aggregate_id(self) -> bytes:
        return id_of_key(self.key)


def id_of(length: int) -> bytes:
    return soc._id_of(length)


def amount_payload(amount: int, length: int = 0) -> bytes:
    """``{"amount":N}``, or the same event padded to exactly ``length`` bytes by a string field behind it."""
    text = b'{"amount":%d}' % amount
    if length:
        text = b'{"amount":%d,"pad":"' % amount
        text += b"p" * (length - len(text) - 2) + b'"}'
        assert len(text) == length
    return text


def accepted_cases():
    """All on the SDK template (one decoder takes the whole list), every key distinct up to its colon."""
    out = []
    for n in ID_LENGTHS:  # (length 0: the runtime leaves field 1 out; the record's key is empty too)
        aid = id_of(n)
        out.append(Case(f"id{n}", SDK, aid, wrap(aid, amount_payload(n - 7))))
        if n:
            out.append(Case(f"id{n} key with a sequence number", SDK, aid + b":%d" % n, wrap(aid, amount_payload(-n))))
    for key in ("ünï-✓-ключ", "\U0001d11e\U00010348", 'we"ird\\id', '"', "tab\there\nnl"):
        kb = key.encode("utf-8")
        out.append(Case(f"id {key!r}", SDK, kb, wrap(kb, amount_payload(2147483647))))
    for n in (126, 127, 128, 129, 16383, 16384):  # payload lengths on both sides of the varint steps
        aid = b"pay%d" % n
        out.append(Case(f"payload{n}", SDK, aid + b":1", wrap(aid, amount_payload(-2**31, n))))
        assert len(runtime_fields(out[-1].value)[1]) == n
    out.append(Case("colon key, id without", SDK, b"id:7", wrap(b"id", amount_payload(7))))
    out.append(Case("whitespace and other fields in the payload", SDK, b"ws", wrap(b"ws", b' { "x" : [1, {"amount": 3}], "amount" : 5 , "s":"}" } ')))
    return out + overlong_cases()


def overlong_cases():
    """Non-minimal length varints the runtime accepts: 2-byte and 5-byte spellings of the id's 5 and of the payload's length."""
    pay = amount_payload(-12)
    five = bytes([0x85, 0x80, 0x80, 0x80, 0x00])
    plen = len(pay)
    return [Case("2-byte varint for 5", SDK, b"hello:2", b"\x0a\x85\x00hello\x12" + protobuf_varint(plen) + pay),
            Case("5-byte varint for 5", SDK, b"hello:5", b"\x0a" + five + b"hello\x12" + protobuf_varint(plen) + pay),
            Case("2-byte payload length", SDK, b"hello:p2", b"\x0a\x05hello\x12" + bytes([0x80 | plen, 0x00]) + pay),
            Case("5-byte payload length", SDK, b"hello:p5", b"\x0a\x05hello\x12" + bytes([0x80 | plen, 0x80, 0x80, 0x80, 0x00]) + pay),
            Case("over-long, no id", SDK, b"", b"\x12" + bytes([0x80 | plen, 0x00]) + pay)]


def other_template_cases():
    """Accepted values of the other templates: the 16-byte value, a sealed family inside the envelope."""
    sixteen = wrap(b"a", b'{"v":12345}')
    assert len(sixteen) == 16
    return [Case("16-byte value", V, b"a", sixteen), Case("16-byte value, key with a colon", V, b"a:9", sixteen),
            Case("counter incremented", COUNTER, b"c1:4", wrap(b"c1", b'{"aggregateId":"c1","incrementBy":3,"sequenceNumber":4,"_type":"countIncremented"}')),
            Case("counter no-op", COUNTER, b"c2:1", wrap(b"c2", b'{"_type":"no-op","sequenceNumber":1}'))]


def ambiguous_cases():
    return [Case(f"ambiguous {text[:12]}", F64, b"d%d:1" % i, wrap(b"d%d" % i, b'{"x":' + text.encode() + b"}")) for i, text in enumerate(AMBIGUOUS_DOUBLES)]


def decided_double_cases(n=6):
    return [Case(f"double {i}", F64, b"e%d" % i, wrap(b"e%d" % i, b'{"x":%s}' % repr((i - 2) * 1.37e-3 * 10.0 ** (7 * i)).encode())) for i in range(n)]


def refused_cases():
    pay = amount_payload(1)
    good = wrap(b"k1", pay)
    f1, f2 = b"\x0a\x02k1", b"\x12" + protobuf_varint(len(pay)) + pay
    assert good == f1 + f2
    E, M = "envelope", "mismatch"
    k = b"k1:3"
    return [
        Case("unknown tag 0x1A in front of field 2", SDK, k, f1 + b"\x1a\x01x" + f2, E),
        Case("unknown tag 0x1A behind field 2", SDK, k, good + b"\x1a\x00", E),
        Case("wrong wire type 0x08", SDK, k, b"\x08\x02k1" + f2, E),
        Case("wrong wire type 0x10", SDK, k, f1 + b"\x10" + f2[1:], E),
        Case("field 1 twice", SDK, k, f1 + f1 + f2, E),
        Case("field 2 twice", SDK, k, f1 + f2 + f2, E),
        Case("field 2 in front of field 1", SDK, k, f2 + f1, E),
        Case("id length beyond the end", SDK, k, b"\x0a\x7fk1", E),
        Case("payload length beyond the end", SDK, k, f1 + b"\x12" + protobuf_varint(len(pay) + 1) + pay, E),
        Case("payload length one short of the end", SDK, k, f1 + b"\x12" + protobuf_varint(len(pay) - 1) + pay, E),
        Case("ends inside a tag's field: behind a tag", SDK, k, f1 + b"\x12", E),
        Case("ends inside a varint", SDK, k, f1 + b"\x12\x8d", E),
        Case("a varint whose 5th byte continues", SDK, k, b"\x0a\x82\x80\x80\x80\x80\x00k1" + f2, E),
        Case("a length of 2^31", SDK, k, b"\x0a\x80\x80\x80\x80\x08k1" + f2, E),
        Case("bare JSON where an envelope is named", SDK, k, pay, E),
        Case("id longer than the key's", SDK, k, wrap(b"k1x", pay), M),
        Case("id shorter than the key's", SDK, k, wrap(b"k", pay), M),
        Case("id differs in the last byte", SDK, k, wrap(b"k2", pay), M),
        Case("id holds the key's colon part", SDK, b"id:7", wrap(b"id:7", amount_payload(7)), M),
        Case("field 1 absent under a non-empty key", SDK, k, f2, M),
        Case("empty payload spelled out", SDK, k, f1 + b"\x12\x00", "json"),
        Case("absent payload", SDK, k, f1, "json"),
    ]


def expected_event(case) -> bytes:
    """The 16 bytes of an accepted case from the references alone: the runtime's id (it must be the key's) and payload, the
    bare template over the payload."""
    rid, payload = runtime_fields(case.value)
    assert rid == case.aggregate_id, case.name
    return case.bare.decode(payload).tobytes()


_ALPHABET = bytes([0x0A, 0x12, 0x1A, 0x08, 0x10, 0x00, 0x01, 0x7F, 0x80, 0x81, 0xFF, 0x85, 0x22, 0x5C, 0x7B, 0x7D]) + b"0123456789-.eE"


def mutations(cases, per_case, seed=2025):
    """Seeded byte mutations of the cases' values: tag / varint / quote bytes written or inserted anywhere, short erasures,
    random bytes, cuts; and, for a third of them, edits that tend to keep the value well-formed — a digit for a digit, a
    letter for a letter (an id byte, mostly), a one-byte length re-spelled over-long.  Long values are mutated near their
    head and tail, where the envelope and the payload's ends lie.  The mutated case keeps its key; its ``reason`` is ``"?"``."""
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
            out.append(Case(c.name + " mutated", c.template, c.key, bytes(m), "?"))
    return out
