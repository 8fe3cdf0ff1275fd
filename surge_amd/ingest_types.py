"""What the units of the events-topic ingest share (``include/surge_ingest.h`` as Python sees it): the flags, the record
layouts, the ctypes mirrors of the templates with the classes that fill them, ``IngestError`` and the one way a status
becomes it.  A leaf: ``host_framer``, ``framing`` and ``device_decoder`` stand on it, ``ingest`` is their import point."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native
from .schema import EVENT_DTYPE

READ_UNCOMMITTED, READ_COMMITTED = 0, 1
FRAMES = 0x100  # SURGE_INGEST_FRAMES: frame on the host, decode the records on the GPU (DeviceDecoder)
DEVICE_LZ4 = 0x200  # SURGE_INGEST_DEVICE_LZ4: ... and leave LZ4 frames and snappy chunks for the GPU as well
DEVICE_DECOMPRESS = DEVICE_LZ4  # SURGE_INGEST_DEVICE_DECOMPRESS: the same bit, by the name of what it has come to mean
DEVICE_CRC = 0x400  # SURGE_INGEST_DEVICE_CRC: ... and finish a data batch's CRC-32C on the GPU (the host checksums its 40 header bytes only)
SECTION_CRC_PENDING = 0x100  # in a section's codec: {crc, register after the 40 covered header bytes} lie in front of the section
SECTION_CRC_WIRE = 0x200  # ... (in-place framing) the batch's own crc field and the 40 header bytes it covers do: the device runs the whole CRC
SECTION_FLOORED = 0x400  # ... the section straddles the framer's start offset: the floors list names it

SECTION_DTYPE = np.dtype([("byte_off", "<i8"), ("byte_len", "<i8"), ("base_offset", "<i8"), ("n_records", "<i4"), ("codec", "<i4")])
assert SECTION_DTYPE.itemsize == 32

FLOOR_DTYPE = np.dtype([("part", "<i4"), ("reserved", "<i4"), ("section", "<i8"), ("first_offset", "<i8")])  # surge_section_floor
assert FLOOR_DTYPE.itemsize == 24
NO_FLOORS = np.zeros(0, dtype=FLOOR_DTYPE)

RECORD_DTYPE = np.dtype([("offset", "<i8"), ("agg_idx", "<i8"), ("key_off", "<i8"), ("key_len", "<i4"),
                         ("value_len", "<i4"), ("value_off", "<i8")])
assert RECORD_DTYPE.itemsize == 40


COUNTER_NAMES = ("batches", "records_decoded", "records_delivered", "records_aborted", "control_batches",
                 "flush_records_skipped", "bytes_decompressed", "open_transactions")  # surge_ingest_counters / surge_ingest_group_counters

EVJ_NAME, EVJ_MAX_TYPES = 64, 16
ARG_NONE, ARG_I32, ARG_F64 = 0, 1, 2
EVJ_ENVELOPES = {"none": 0, "protobuf_event": 1}  # SURGE_EVJ_ENVELOPE_*


class IngestError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"surge_ingest status {status}: {message}")
        self.status = status


def raise_for(rc: int, last_error, *handle) -> None:
    """``rc != 0`` -> ``IngestError`` with what ``last_error`` — the ``*_last_error`` of the kind of handle that answered, and
    that handle — has to say."""
    if rc != 0:
        raise IngestError(rc, (last_error(*handle) or b"").decode("utf-8", "replace"))  # (a message may quote a value's own bytes)


class _CEventJsonType(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * EVJ_NAME), ("event_type", ctypes.c_uint32), ("arg_kind", ctypes.c_uint32),
                ("seq_field", ctypes.c_char * EVJ_NAME), ("arg_field", ctypes.c_char * EVJ_NAME)]


class CEventJsonTemplate(ctypes.Structure):
    _fields_ = [("n_types", ctypes.c_uint32), ("envelope", ctypes.c_uint32), ("discriminator", ctypes.c_char * EVJ_NAME),
                ("types", _CEventJsonType * EVJ_MAX_TYPES)]


EVS_MAX = 16  # SURGE_EVS_MAX
EVENT_STRING_OK, EVENT_STRING_MISSING, EVENT_STRING_RECORD, EVENT_STRING_ABSENT = 0, 12, 13, 254  # SURGE_EVENT_STRING_*


class _CEventStringField(ctypes.Structure):
    _fields_ = [("type_name", ctypes.c_char * EVJ_NAME), ("field", ctypes.c_char * EVJ_NAME), ("column", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class CEventStrings(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("entry", _CEventStringField * EVS_MAX)]


class EventStrings:
    """``surge_event_strings``: which event class carries which string.  ``entries``: ``(type name, field name, column)`` —
    the discriminator value of the class as in ``EventJsonTemplate.types`` (``""`` for a template without a discriminator), the
    JSON field that holds the string, and the side string column (``0 .. encode.STRING_COLUMNS - 1``) it lands in.  Per aggregate
    and column the last event in topic order whose class names the column wins (``include/surge_ingest.h``, "the STRING fields of
    events")."""

    def __init__(self, entries):
        self.entries = [(str(t), str(f), int(c)) for t, f, c in entries]

    def to_c(self) -> CEventStrings:
        if len(self.entries) > EVS_MAX:
            raise ValueError(f"at most {EVS_MAX} event string fields")
        s = CEventStrings()
        s.n = len(self.entries)
        for i, (type_name, field, column) in enumerate(self.entries):
            if not 0 <= column < 1 << 32:
                raise ValueError(f"string column {column} out of range")
            tn, fn = type_name.encode(), field.encode()
            if len(tn) >= EVJ_NAME or len(fn) >= EVJ_NAME:
                raise ValueError(f"a name of more than {EVJ_NAME - 1} bytes")
            s.entry[i].type_name, s.entry[i].field, s.entry[i].column = tn, fn, column
        return s

    def validate(self, template: "EventJsonTemplate") -> None:
        """``surge_event_strings_validate`` against ``template``; ``ValueError`` with the library's reason."""
        lib = _native.load()
        t, c = template.to_c(), self.to_c()
        if lib.surge_event_strings_validate(ctypes.byref(t), ctypes.byref(c)) != 0:
            raise ValueError((lib.surge_event_json_last_error() or b"").decode())


class EventJsonTemplate:
    """``surge_event_json_template``: how a model's JSON event text maps onto the 16-byte fixed event.

    ``types``: ``(discriminator value, event type, seq field or "", arg field or "", ARG_*)`` per event class;
    ``discriminator``: the field naming the class (play-json's sealed-family ``"_type"``), ``""`` for single-class topics.
    ``envelope``: what lies around the JSON text in a record's value — ``"none"``, or ``"protobuf_event"`` for the events topic
    of a multilanguage (SDK) application, whose values are the protobuf message ``Event{aggregateId, payload}`` with the text
    as payload (``GenericSurgeCommandBusinessLogic.scala:30-34``).  It travels with the template to every decoder: the host
    drain, ``DeviceDecoder`` and the store's recoveries."""

    def __init__(self, discriminator: str, types, envelope: str = "none"):
        if envelope not in EVJ_ENVELOPES:
            raise ValueError(f"envelope must be one of {sorted(EVJ_ENVELOPES)}, not {envelope!r}")
        self.discriminator, self.types, self.envelope = discriminator, list(types), envelope

    def to_c(self) -> CEventJsonTemplate:
        t = CEventJsonTemplate()
        t.n_types = len(self.types)
        t.envelope = EVJ_ENVELOPES[self.envelope]
        t.discriminator = self.discriminator.encode()
        for i, (name, ev_type, seq_field, arg_field, arg_kind) in enumerate(self.types):
            e = t.types[i]
            e.name, e.event_type, e.arg_kind = name.encode(), ev_type, arg_kind
            e.seq_field, e.arg_field = seq_field.encode(), arg_field.encode()
        return t

    def decode(self, value: bytes) -> np.ndarray:
        """One record value -> one ``EVENT_DTYPE`` record (``surge_event_json_decode``; an enveloped template reads the
        envelope and compares its id with nothing)."""
        return self.decode_keyed(None, value)

    def decode_keyed(self, aggregate_id: Optional[bytes], value: bytes) -> np.ndarray:
        """``surge_event_json_decode_keyed``: like ``decode``, and with an enveloped template the envelope's ``aggregateId`` must
        equal ``aggregate_id`` byte for byte — the record's key already cut at its first ``:``.  ``None``: no comparison."""
        lib = _native.load()
        out = np.zeros(1, dtype=EVENT_DTYPE)
        c = self.to_c()
        if lib.surge_event_json_validate(ctypes.byref(c)) != 0:
            raise_for(-1, lib.surge_event_json_last_error)
        buf = (ctypes.c_uint8 * max(len(value), 1)).from_buffer_copy(value or b"\0")
        key = None if aggregate_id is None else bytes(aggregate_id)
        kbuf = None if key is None else (ctypes.c_uint8 * max(len(key), 1)).from_buffer_copy(key or b"\0")
        rc = lib.surge_event_json_decode_keyed(ctypes.byref(c), kbuf, -1 if key is None else len(key), buf, len(value), out.ctypes.data_as(ctypes.c_void_p))
        raise_for(rc, lib.surge_event_json_last_error)
        return out[0]

    def string_spans(self, strings: "EventStrings", value: bytes):
        """``surge_event_json_string_spans``: the rule the device applies to one record value, on the host.  Returns ``(rc,
        spans, status)``: ``rc`` 0 or ``-7`` (CORRUPT: a column is refused), ``spans`` one ``(offset into value, length)`` per
        string column — the still-escaped bytes between the quotes — and ``status`` one ``EVENT_STRING_*`` / ``DECODE_*`` per
        column.  ``ValueError`` for strings that do not validate against this template."""
        lib = _native.load()
        t, c = self.to_c(), strings.to_c()
        strings.validate(self)
        buf = (ctypes.c_uint8 * max(len(value), 1)).from_buffer_copy(value or b"\0")
        spans = np.zeros(8, dtype=np.int64)
        status = np.zeros(4, dtype=np.uint8)
        rc = lib.surge_event_json_string_spans(ctypes.byref(t), ctypes.byref(c), buf, len(value), spans.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p))
        if rc != -7:
            raise_for(rc, lib.surge_event_json_last_error)
        return int(rc), [(int(spans[2 * k]), int(spans[2 * k + 1])) for k in range(4)], [int(x) for x in status]
