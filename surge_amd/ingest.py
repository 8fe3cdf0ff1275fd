"""Events-topic ingest: Kafka record batches of one partition -> records in offset order
with their aggregate index, through the C ABI in ``include/surge_ingest.h`` (host side, no GPU).

``EventsTopicIngest.feed(bytes)`` takes what a fetch of the events topic returns (RecordBatch v2, lz4 or
uncompressed, ``read_committed`` by default like ``SurgeStateStoreConsumer.scala:38``);
``drain_fixed16()`` returns ``(agg_idx, events, offsets)`` for GPU-ready topics whose record value is the
16-byte fixed event, ``drain_records()`` returns ``(offset, key, value)`` tuples for plugin-decoded values.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np

from . import _native
from .encode import key_table_utf8
from .log import KeyTable
from .schema import EVENT_DTYPE

READ_UNCOMMITTED, READ_COMMITTED = 0, 1
FRAMES = 0x100  # SURGE_INGEST_FRAMES: frame on the host, decode the records on the GPU (DeviceDecoder)
DEVICE_LZ4 = 0x200  # SURGE_INGEST_DEVICE_LZ4: ... and leave LZ4 frames for the GPU as well
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
            raise IngestError(-1, (lib.surge_event_json_last_error() or b"").decode())
        buf = (ctypes.c_uint8 * max(len(value), 1)).from_buffer_copy(value or b"\0")
        key = None if aggregate_id is None else bytes(aggregate_id)
        kbuf = None if key is None else (ctypes.c_uint8 * max(len(key), 1)).from_buffer_copy(key or b"\0")
        rc = lib.surge_event_json_decode_keyed(ctypes.byref(c), kbuf, -1 if key is None else len(key), buf, len(value), out.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise IngestError(rc, (lib.surge_event_json_last_error() or b"").decode("utf-8", "replace"))  # (the message may quote the value's own bytes)
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
        if rc not in (0, -7):
            raise IngestError(rc, (lib.surge_event_json_last_error() or b"").decode())
        return int(rc), [(int(spans[2 * k]), int(spans[2 * k + 1])) for k in range(4)], [int(x) for x in status]


class IngestError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"surge_ingest status {status}: {message}")
        self.status = status


class Framed(tuple):
    """What a framer with start offsets yields per fetch: the ``(sections, arena_address)`` pair it always yielded — it
    destructures and indexes as that — with ``floors`` (``FLOOR_DTYPE`` records naming the sections that straddle a start offset:
    what ``DeviceDecoder.push`` / ``push_async`` take beside the sections) and ``positions`` (the offset each partition would
    resume from behind this fetch: ``surge_ingest_position``)."""

    def __new__(cls, sections, address, floors=NO_FLOORS, positions=()):
        self = super().__new__(cls, (sections, address))
        self.floors, self.positions = floors, tuple(positions)
        return self


class EventsTopicIngest:
    """``start_offset``: the offset a consumer that sought into the partition begins at (``surge_ingest_set_start_offset``): records
    below it are not delivered, transactions are read as ever; ``None`` / ``<= 0``: from the beginning."""

    def __init__(self, isolation_level: int = READ_COMMITTED, frames: bool = False, device_lz4: bool = False, threads: int = 1, device_crc: bool = False,
                 start_offset: Optional[int] = None):
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        self.frames = frames
        rc = self._lib.surge_ingest_create(isolation_level | (FRAMES if frames else 0) | (DEVICE_LZ4 if device_lz4 else 0) | (DEVICE_CRC if device_crc else 0),
                                           ctypes.byref(self._h))
        if rc != 0:
            raise IngestError(rc, (self._lib.surge_ingest_last_error(None) or b"").decode())
        if (frames or device_lz4 or device_crc) and os.environ.get("SURGE_INGEST_PAGEABLE_ARENA") != "1":
            # page-locked arena when a GPU is there: the device decoder copies out of it in place (a pageable arena works too)
            self._lib.surge_ingest_use_pinned_arena(self._h)
        if threads != 1:  # host threads verifying the batches' CRC-32C of one feed (surge_ingest_set_threads)
            self._check(self._lib.surge_ingest_set_threads(self._h, int(threads)))
        if start_offset is not None:
            self.set_start_offset(start_offset)
        self._tail = b""

    def close(self):
        if self._h:
            self._lib.surge_ingest_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise IngestError(rc, (self._lib.surge_ingest_last_error(self._h) or b"").decode())

    def feed(self, data: bytes) -> int:
        """Decode whole batches; a trailing partial batch is kept and completed by the next call."""
        buf = self._tail + bytes(data) if self._tail else (data if isinstance(data, bytes) else bytes(data))
        consumed = ctypes.c_int64(0)
        # a bytes object is handed over in place (the library copies what it keeps): no per-feed copy of the fetch
        arr = ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p) if buf else None
        rc = self._lib.surge_ingest_feed(self._h, arr, len(buf), ctypes.byref(consumed))
        # also on failure: batches decoded before the failing one ARE queued and must not be fed again
        self._tail = buf[consumed.value:]
        self._check(rc)
        return consumed.value

    @property
    def ready(self) -> int:
        return int(self._lib.surge_ingest_ready(self._h))

    def set_start_offset(self, first_offset: int) -> None:
        """Before the first feed (``IngestError`` STATE afterwards)."""
        self._check(self._lib.surge_ingest_set_start_offset(self._h, int(first_offset)))

    def position(self) -> int:
        """The offset a consumer would resume from: behind the last batch decided, in front of an open transaction and of
        anything not drained yet, never below the start — what a publisher commits with a snapshot."""
        return int(self._lib.surge_ingest_position(self._h))

    def positions(self) -> List[int]:
        return [self.position()]

    def take_floors(self) -> np.ndarray:
        """``FLOOR_DTYPE`` records for the sections the last ``drain_sections`` handed out (at most one, once per framer)."""
        out = np.zeros(1, dtype=FLOOR_DTYPE)
        got = ctypes.c_int64(0)
        self._check(self._lib.surge_ingest_take_floors(self._h, 1, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)))
        return out[: got.value]

    def below_start(self) -> dict:
        c = (ctypes.c_int64 * 2)()
        self._check(self._lib.surge_ingest_below_start(self._h, ctypes.byref(c)))
        return {"batches_discarded": int(c[0]), "records_dropped": int(c[1])}

    def counters(self) -> dict:
        c = (ctypes.c_int64 * 8)()
        self._check(self._lib.surge_ingest_counters(self._h, ctypes.byref(c)))
        return dict(zip(COUNTER_NAMES, [int(x) for x in c]))

    def drain_sections(self, max_sections: int = 1 << 30) -> Tuple[np.ndarray, int]:
        """FRAMES mode: the records sections of the deliverable batches (``SECTION_DTYPE`` records whose spans point into
        the arena) and the arena's address — what ``DeviceDecoder.push`` takes."""
        out = np.zeros(min(max_sections, max(self.ready, 1)), dtype=SECTION_DTYPE)  # ready counts records: an upper bound
        got = ctypes.c_int64(0)
        self._check(self._lib.surge_ingest_drain_sections(self._h, out.shape[0], out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)))
        return out[: got.value], int(self._lib.surge_ingest_arena(self._h) or 0)

    def _drain_events(self, max_records: Optional[int], drain) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(agg_idx, events, offsets)`` of up to ``max_records`` ready records: ``drain(n, agg, ev, off, got)`` is the library
        call that fills the three arrays and says how many records it wrote."""
        n = self.ready if max_records is None else min(self.ready, max_records)
        out = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=EVENT_DTYPE), np.zeros(n, dtype=np.int64)
        got = ctypes.c_int64(0)
        self._check(drain(n, *(a.ctypes.data_as(ctypes.c_void_p) for a in out), ctypes.byref(got)))
        return tuple(a[: got.value] for a in out)

    def drain_fixed16(self, max_records: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self._drain_events(max_records, lambda n, *arrays: self._lib.surge_ingest_drain_fixed16(self._h, n, *arrays))

    def drain_json(self, template: EventJsonTemplate, max_records: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(agg_idx, events, offsets)`` for topics whose record values are JSON events, decoded in the library through the
        model's template (``surge_ingest_drain_json``): no per-record Python."""
        c = template.to_c()
        return self._drain_events(max_records, lambda n, *arrays: self._lib.surge_ingest_drain_json(self._h, n, ctypes.byref(c), *arrays))

    def drain_records(self, max_records: Optional[int] = None) -> List[Tuple[int, int, Optional[bytes], Optional[bytes]]]:
        """``(offset, agg_idx, key, value)`` per record (``None`` for null key / value)."""
        n = self.ready if max_records is None else min(self.ready, max_records)
        recs = np.zeros(n, dtype=RECORD_DTYPE)
        got = ctypes.c_int64(0)
        self._check(self._lib.surge_ingest_drain(self._h, n, recs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)))
        base = self._lib.surge_ingest_arena(self._h) or 0  # NULL while the arena is empty (only empty keys / values so far)

        def span(off, ln):
            return None if ln < 0 else (b"" if ln == 0 else ctypes.string_at(base + int(off), int(ln)))

        out = []
        for r in recs[: got.value]:
            key, val = span(r["key_off"], r["key_len"]), span(r["value_off"], r["value_len"])
            out.append((int(r["offset"]), int(r["agg_idx"]), key, val))
        return out

    def key_table(self) -> KeyTable:
        kt = KeyTable()
        n = int(self._lib.surge_ingest_key_count(self._h))
        p, ln = ctypes.c_char_p(), ctypes.c_int64()
        for i in range(n):
            self._check(self._lib.surge_ingest_key(self._h, i, ctypes.byref(p), ctypes.byref(ln)))
            kt.intern(ctypes.string_at(p, ln.value).decode("utf-8"))
        return kt


class _FramingAhead:
    """The one-fetch-ahead protocol both framers keep, written once.  A worker thread takes the items of ``fetches`` and
    frames them (``_frame(item)``, the subclass's host stage — and the fetch itself, when ``fetches`` is a generator that
    polls) ONE FETCH AHEAD of whoever iterates.  The native framer rotates through six arenas / slabs, so what fetch i's
    sections point to stays as it is while fetches i + 1 .. i + ``hold`` are framed: ``hold`` (1 .. 5) is how many fetches
    the consumer keeps alive at a time, and the worker holds a slot for each of them plus the one it frames.  ASKING for the
    next fetch while ``hold`` are held is what releases the oldest one's slot — nothing else does: a consumer with pushes in
    flight finishes the oldest push first, then asks (``pushes_in_flight``, ``PushPipeline``).  The worker's exception is
    handed over and re-raised in the consumer's thread; ``None`` marks the end and is put back, so a repeated ``next()``
    raises ``StopIteration`` again.  ``overlap=False`` frames inline (same results, one thread).

    A subclass names its thread (``_thread_name``) and what there are six of (``_six_of``), creates its native handle
    after ``super().__init__`` and calls ``_start()`` when it is ready to frame; it supplies ``_frame``, ``_close_handle``,
    ``counters``, ``positions`` and ``below_start``."""

    _thread_name = _six_of = None

    def __init__(self, fetches, overlap: bool, hold: int):
        import queue
        import threading

        if not 1 <= hold <= 5:
            raise ValueError(f"hold must be 1 .. 5 ({self._six_of})")
        self._fetches = iter(fetches)
        self._overlap, self._hold = overlap, hold
        self.framing_seconds: List[float] = []
        self._q: "queue.Queue" = queue.Queue()
        self._slots = threading.Semaphore(hold + 1)  # framed fetches alive at once: the ones being read + the one being framed
        self._stop = False
        self._held = 0
        self._thread = threading.Thread(target=self._run, name=self._thread_name, daemon=True) if overlap else None

    def _start(self):
        if self._thread:
            self._thread.start()

    def _run(self):
        try:
            for data in self._fetches:
                self._slots.acquire()
                if self._stop:
                    break
                self._q.put(self._frame(data))
        except BaseException as e:  # handed to the consumer, which re-raises it in its own thread
            self._q.put(e)
        finally:
            self._q.put(None)

    def __iter__(self):
        return self

    def __next__(self):
        if not self._overlap:
            return self._frame(next(self._fetches))
        if self._held == self._hold:  # the consumer is done with the oldest fetch it holds: its arena may be framed into again
            self._held -= 1
            self._slots.release()
        item = self._q.get()
        if item is None:
            self._q.put(None)
            raise StopIteration
        if isinstance(item, BaseException):
            self._q.put(None)
            raise item
        self._held += 1
        return item

    def close(self):
        self._stop = True
        if self._thread:
            for _ in range(self._hold + 1):
                self._slots.release()
            self._thread.join()
            self._thread = None
        self._close_handle()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FramedFetches(_FramingAhead):
    """Frames a sequence of fetches one fetch ahead of whoever consumes them (:class:`_FramingAhead`): the worker thread runs
    the host stage (``feed`` = batch headers, CRC-32C, ``read_committed``) while the caller's thread keeps the device busy
    with the previous fetch (``DeviceDecoder.push`` + the fold).  One ``EventsTopicIngest`` in FRAMES mode does all the
    framing, so transactions and partial batches carry from fetch to fetch; its six rotating arenas
    (``surge_ingest_drain_sections`` in ``surge_ingest.h``) are what makes the overlap safe.  ``hold``: 1 for
    push-then-fold, 2 .. 5 when the consumer keeps that many ``DeviceDecoder.push_async`` in flight
    (``store.restore_from_fetches``).

    Iterating yields ``(sections, arena_address)`` per fetch, in order."""

    _thread_name, _six_of = "surge-framing", "the framer has six arenas"

    def __init__(self, fetches, isolation_level: int = READ_COMMITTED, device_lz4: bool = True, overlap: bool = True, threads: int = 1, hold: int = 1,
                 device_crc: bool = True, start_offset: Optional[int] = None):
        super().__init__(fetches, overlap, hold)
        # device_crc needs the sections as they are on the wire: with host-side LZ4 (device_lz4=False) the host has the bytes in hand anyway
        self._g = EventsTopicIngest(isolation_level, frames=True, device_lz4=device_lz4, threads=threads, device_crc=device_crc and device_lz4,
                                    start_offset=start_offset)
        self._started = start_offset is not None  # with a start every item is a Framed: the pair, its floors, the position behind it
        self._start()

    def _frame(self, data):
        import time

        t0 = time.perf_counter()
        self._g.feed(data)
        item = self._g.drain_sections()
        if self._started:
            item = Framed(item[0], item[1], self._g.take_floors(), self._g.positions())
        self.framing_seconds.append(time.perf_counter() - t0)
        return item

    def _close_handle(self):
        self._g.close()

    def counters(self) -> dict:
        """The ingest counters; call it when the iteration has ended (the handle belongs to the framing thread)."""
        return self._g.counters()

    def positions(self) -> List[int]:
        """Where the partition would be resumed from (``EventsTopicIngest.position``); when the iteration has ended, like ``counters``."""
        return self._g.positions()

    def below_start(self) -> dict:
        return self._g.below_start()


class PartitionedFramedFetches(_FramingAhead):
    """The same one-fetch-ahead framing for a consumer that is assigned several partitions: ``fetches`` yields, per fetch
    response, the next bytes of every partition (a sequence of ``bytes`` / ``None``, always in the same partition order).
    A ``surge_ingest_group`` frames them: one framer per partition — transactions, last stable offsets and cut batches are
    per partition (``SurgeStateStoreConsumer.scala:33-46``: ``isolation.level`` as configured) — side by side on
    ``threads`` host threads (C++ threads inside the library call), all of a fetch's records sections laid out in ONE
    page-locked slab.  Iterating yields ``(sections, slab_address)`` per fetch — partition after partition, offset order
    inside a partition: one ``DeviceDecoder.push_async``, one host-to-device copy.  ``hold`` as in :class:`FramedFetches`
    (the group rotates through six slabs)."""

    _thread_name, _six_of = "surge-framing-driver", "the group has six slabs"

    def __init__(self, fetches, n_partitions: int, threads: int = 8, hold: int = 3, isolation_level: int = READ_COMMITTED, device_lz4: bool = True,
                 overlap: bool = True, device_crc: bool = True, in_place: bool = False, start_offsets=None):
        super().__init__(fetches, overlap, hold)
        if start_offsets is not None and len(start_offsets) != n_partitions:
            raise ValueError(f"start_offsets holds {len(start_offsets)} entries for {n_partitions} partitions (<= 0: a partition without a start)")
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        self._check(self._lib.surge_ingest_group_create(n_partitions, isolation_level | (DEVICE_LZ4 if device_lz4 else 0) | (DEVICE_CRC if device_crc and device_lz4 else 0),
                                                        ctypes.byref(self._h)))
        if os.environ.get("SURGE_INGEST_PAGEABLE_ARENA") != "1":
            self._lib.surge_ingest_group_use_pinned_slabs(self._h)  # (fails without a GPU: the slabs stay pageable, which works too)
        self._started = start_offsets is not None
        if self._started:
            self._check(self._lib.surge_ingest_group_set_start_offsets(self._h, (ctypes.c_int64 * n_partitions)(*[int(o) for o in start_offsets])))
        self._threads = max(1, min(threads, n_partitions))
        # in_place: the fetch response is RECEIVED into the group's next page-locked slab (surge_ingest_group_receive_copy: one copy out of
        # the bytes objects on the framing threads, standing in for the socket reads a consumer would aim there) and framed
        # where it lies — with device_lz4 and device_crc the host reads the batches' 61-byte headers and nothing else
        self._in_place = in_place and device_lz4
        self.receive_seconds: List[float] = []      # wall time of that stand-in receive copy, per fetch
        self._n = n_partitions
        self._tails = [b""] * n_partitions
        self._ring = [None] * (hold + 2)  # section tables, reused (the consumer keeps `hold` fetches alive while the next is framed)
        self._start()

    def _check(self, rc: int):
        if rc != 0:  # (a group that was not created has a null handle: the library's message of the failed create)
            raise IngestError(rc, (self._lib.surge_ingest_group_last_error(self._h) or b"").decode())

    def _frame(self, fetch):
        """One library call per fetch (``surge_ingest_group_feed``): no per-partition Python."""
        import time

        t0 = time.perf_counter()
        n = self._n
        fetch = list(fetch)
        if len(fetch) != n:  # (before anything is fed: a short response must not leave some partitions fed and others not)
            raise ValueError(f"a fetch response holds {len(fetch)} entries for {n} partitions (pass None for a partition without bytes)")
        bufs = []
        for tail, data in zip(self._tails, fetch):  # a partition's cut batch from the last fetch goes in front (rare: whole batches are the rule)
            data = data or b""
            bufs.append(tail + bytes(data) if tail else (data if isinstance(data, bytes) else bytes(data)))
        len_arr = (ctypes.c_int64 * n)(*[len(b) for b in bufs])
        if self._in_place:
            tr = time.perf_counter()
            src_arr = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None for b in bufs])
            data_arr = (ctypes.c_void_p * n)()
            self._check(self._lib.surge_ingest_group_receive_copy(self._h, src_arr, len_arr, self._threads, data_arr))
            self.receive_seconds.append(time.perf_counter() - tr)
            t0 = time.perf_counter()  # (framing_seconds: the framing proper)
        else:
            data_arr = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None for b in bufs])
        # a batch is at least its 61-byte header; a feed also delivers what the partitions still hold from earlier feeds (a
        # transaction whose COMMIT marker only arrives now)
        max_sec = sum(len(b) for b in bufs) // 61 + int(self._lib.surge_ingest_group_queued_sections(self._h)) + 16
        slot = len(self.framing_seconds) % len(self._ring)
        n_sec = ctypes.c_int64()
        slab = ctypes.c_void_p()
        consumed = (ctypes.c_int64 * n)()
        while True:
            if self._ring[slot] is None or self._ring[slot].shape[0] < max_sec:
                self._ring[slot] = np.empty(max_sec + max_sec // 4, dtype=SECTION_DTYPE)
            secs = self._ring[slot]
            rc = self._lib.surge_ingest_group_feed(self._h, data_arr, len_arr, self._threads, consumed, secs.shape[0], secs.ctypes.data_as(ctypes.c_void_p),
                                                   ctypes.byref(n_sec), ctypes.byref(slab))
            if rc != 0 and n_sec.value > secs.shape[0]:  # table too small: the feed was undone and says what it needs
                max_sec = int(n_sec.value)
                continue
            break
        self._check(rc)  # all or nothing: the group is what it was before the call (the tails too)
        self._tails = [bufs[p][consumed[p]:] for p in range(n)]
        item = secs[: n_sec.value], int(slab.value or 0)
        if self._started:
            floors = np.zeros(n, dtype=FLOOR_DTYPE)  # (at most one per partition over the group's life)
            got = ctypes.c_int64(0)
            self._lib.surge_ingest_group_take_floors(self._h, n, floors.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got))
            item = Framed(item[0], item[1], floors[: got.value], self.positions())
        self.framing_seconds.append(time.perf_counter() - t0)
        return item

    def slab_bytes(self):
        """``(bytes, page_locked)``: what the group's six slabs take (``surge_ingest_group_slab_bytes``)."""
        b, c = ctypes.c_int64(), ctypes.c_int32()
        self._lib.surge_ingest_group_slab_bytes(self._h, ctypes.byref(b), ctypes.byref(c))
        return int(b.value), bool(c.value)

    def positions(self) -> List[int]:
        """Per partition the offset a consumer would resume from (``surge_ingest_group_positions``); when the iteration has
        ended, like ``counters`` — or read ``Framed.positions`` of the items of a framer with ``start_offsets``."""
        out = (ctypes.c_int64 * self._n)()
        self._lib.surge_ingest_group_positions(self._h, out)
        return [int(x) for x in out]

    def below_start(self) -> dict:
        c = (ctypes.c_int64 * 2)()
        self._lib.surge_ingest_group_below_start(self._h, ctypes.byref(c))
        return {"batches_discarded": int(c[0]), "records_dropped": int(c[1])}

    def cpu_seconds(self):
        """``(receive copy, framing)``: thread CPU seconds the group's host threads have spent so far (``surge_ingest_group_cpu_seconds``)."""
        out = (ctypes.c_double * 2)()
        self._lib.surge_ingest_group_cpu_seconds(self._h, ctypes.byref(out))
        return float(out[0]), float(out[1])

    def counters(self) -> dict:
        """The partitions' ingest counters, summed; call it when the iteration has ended."""
        c = (ctypes.c_int64 * 8)()
        self._lib.surge_ingest_group_counters(self._h, ctypes.byref(c))
        return dict(zip(COUNTER_NAMES, [int(x) for x in c]))

    def _close_handle(self):
        if self._h:
            self._lib.surge_ingest_group_destroy(self._h)
            self._h = ctypes.c_void_p()


def pushes_in_flight(framed, push, depth: int):
    """The one-thread way to keep up to ``depth`` pushes in flight over a framer made with ``hold=depth``: ``push(item)`` is
    called for every fetch of ``framed`` (a falsy return = nothing was pushed for that fetch: it takes no slot), and the
    generator yields each time the caller has to finish the OLDEST push — before it asks ``framed`` for the next fetch when
    ``depth`` are pending (asking is what lets the framer reuse the oldest fetch's slab, and a push reads its bytes until it is
    finished), and once per push still pending at the end: ``for _ in pushes_in_flight(framed, push, depth): finish_one()``.
    ``PushPipeline`` is the same protocol with the pushes on a worker thread."""
    pending = 0
    fetches = iter(framed)
    while True:
        if pending == depth:
            yield
            pending -= 1
        item = next(fetches, None)
        if item is None:
            break
        if push(item):
            pending += 1
    while pending:
        yield
        pending -= 1


class PushPipeline:
    """Keeps ``depth`` pushes in flight with the host work of ENQUEUEING them off the consumer's thread: a worker takes the
    framed fetches from ``source`` (a ``FramedFetches`` / ``PartitionedFramedFetches`` made with ``hold=depth``) and calls
    ``push(item)`` — section tables, staging, a dozen launches: about a millisecond of host time per 10^6-record fetch —
    while the caller's thread finishes the oldest push and folds it.  Iterating yields once per enqueued push (whatever
    ``push`` returned; a falsy return = nothing was pushed for that fetch, nothing is yielded); the caller finishes that
    push and calls ``done()``.  The worker asks ``source`` for fetch i + depth only after ``done()`` for fetch i — asking is
    what lets the framer reuse fetch i's slab.  ``threaded=False``: the same protocol inline on the caller's thread — every
    ``next()`` takes one of the ``depth`` permits (``RuntimeError`` when none is left) and every ``done()`` returns one."""

    def __init__(self, source, push, depth: int, threaded: bool = True):
        import queue
        import threading

        self._source, self._push, self._depth = iter(source), push, depth
        self._free = threading.Semaphore(depth)
        self._q: "queue.Queue" = queue.Queue()
        self._stop = False
        self.push_seconds: List[float] = []
        self._thread = threading.Thread(target=self._run, name="surge-push", daemon=True) if threaded else None
        if self._thread:
            self._thread.start()

    def _one(self):
        """-> a token to yield, None to skip this fetch, or StopIteration"""
        import time

        item = next(self._source)
        t0 = time.perf_counter()
        token = self._push(item)
        if token:
            self.push_seconds.append(time.perf_counter() - t0)
        return token

    def _run(self):
        try:
            while True:
                self._free.acquire()
                if self._stop:
                    break
                try:
                    token = self._one()
                except StopIteration:
                    break
                if token:
                    self._q.put(token)
                else:
                    self._free.release()
        except BaseException as e:  # handed to the consumer
            self._q.put(e)
        finally:
            self._q.put(None)

    def __iter__(self):
        return self

    def __next__(self):
        if self._thread is None:
            while True:
                if not self._free.acquire(blocking=False):
                    raise RuntimeError("PushPipeline(threaded=False): call done() for the previous push before asking for the next")
                token = self._one()  # (StopIteration ends the iteration)
                if token:
                    return token
                self._free.release()
        item = self._q.get()
        if item is None:
            self._q.put(None)
            raise StopIteration
        if isinstance(item, BaseException):
            self._q.put(None)
            raise item
        return item

    def done(self) -> None:
        self._free.release()

    def close(self) -> None:
        """Stops the worker (it finishes the push it is in).  ``source`` must still be open: the worker may be waiting for
        its next fetch."""
        self._stop = True
        if self._thread:
            for _ in range(self._depth):
                self._free.release()
            self._thread.join()
            self._thread = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _device_view(ptr, shape, typestr: str, dev):
    """A CUDA tensor over ``shape`` elements of ``typestr`` at the device address ``ptr`` holds (``__cuda_array_interface__``:
    no copy, the memory stays its owner's)."""
    import torch

    iface = {"shape": shape, "typestr": typestr, "data": (ptr.value, False), "version": 2}
    return torch.as_tensor(type("_Span", (), {"__cuda_array_interface__": iface})(), device=dev)


class DeviceDecoder:
    """``surge_device_decoder``: records sections (host bytes) -> device-resident ``(agg_idx, events, offsets)`` and a
    device key table.  ``template=None``: record values are 16-byte events; otherwise the model's ``EventJsonTemplate``.
    ``states=True`` (instead of a template): a decoder for the compacted *state* topic
    (``surge_device_decoder_create_states``) — the id is the whole key, a null value is a delivered tombstone, the values
    are kept as bytes (``state_result()``) and handed to the engine with ``load_states_into``; ``result`` / ``fold_into`` /
    ``stage_into`` are an events decoder's and fail on it (STATE)."""

    def __init__(self, template: Optional[EventJsonTemplate] = None, device: int = 0, stream=None, states: bool = False, keep_strings: bool = False,
                 event_strings: Optional[EventStrings] = None):
        if states and template is not None:
            raise ValueError("DeviceDecoder: states=True is the alternative to an event template")
        if keep_strings and not states:
            raise ValueError("DeviceDecoder: keep_strings belongs to a state decoder (states=True)")
        if event_strings is not None and template is None:
            raise ValueError("DeviceDecoder: event_strings name fields of the event template's classes (a state decoder takes them behind continue_as_events)")
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        self.device = device
        self.states = bool(states)
        self._stream = stream  # the hipStream_t stage 2 and the lookups run on (None: the default stream)
        self._inflight = []
        self.order_passes = 0  # passes of the key order's last build, as the last ``key_order()`` reported them
        c = template.to_c() if template is not None else None
        if states:
            rc = self._lib.surge_device_decoder_create_states(device, stream, ctypes.byref(self._h))
        else:
            rc = self._lib.surge_device_decoder_create(device, stream, ctypes.byref(c) if c is not None else None, ctypes.byref(self._h))
        if rc != 0:
            raise IngestError(rc, (self._lib.surge_device_decoder_last_error(None) or b"").decode())
        if keep_strings:  # (before the first load: every load_states_into then merges the STR columns its template names)
            rc = self._lib.surge_device_decoder_keep_strings(self._h, 1)
            if rc != 0:
                msg = (self._lib.surge_device_decoder_last_error(self._h) or b"").decode()
                self.close()
                raise IngestError(rc, msg)
        self.event_strings = None
        if event_strings is not None:
            try:
                self.keep_event_strings(event_strings)
            except Exception:  # (the library's refusal, or entries that do not fit the C struct: the handle goes either way)
                self.close()
                raise

    def keep_event_strings(self, strings: EventStrings) -> None:
        """``surge_device_decoder_keep_event_strings``: from here on every push keeps, on the device, the strings ``strings``
        names — before the decoder's first push (a continued state decoder: before its first push of events; STATE anywhere
        else).  A record whose class names a string it does not carry, or carries a string that is no valid JSON string, fails
        its push (CORRUPT, naming the record's offset).  The columns are read with ``state_strings()``; a continued decoder that
        kept the state topic's strings goes on merging into the same columns."""
        c = strings.to_c()
        self._check(self._lib.surge_device_decoder_keep_event_strings(self._h, ctypes.byref(c)))
        self.event_strings = strings

    def event_strings_pending(self) -> dict:
        """What an armed decoder holds until the next merge (``surge_device_decoder_event_strings_pending``): ``records``,
        ``bytes``, ``capacity`` (of the values buffer), ``merges`` so far, and ``values`` / ``value_off`` / ``rows`` — CUDA tensors
        viewing the pending values (the whole buffer, ``capacity`` bytes), their ``records + 1`` offsets and their rows, or
        ``None`` while nothing was ever kept."""
        import torch

        out = (ctypes.c_int64 * 4)()
        pv, po, pr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_event_strings_pending(self._h, ctypes.byref(out), ctypes.byref(pv), ctypes.byref(po), ctypes.byref(pr)))
        dev = torch.device("cuda", self.device)
        torch.cuda.synchronize(dev)
        n, cap = int(out[0]), int(out[2])
        return {"records": n, "bytes": int(out[1]), "capacity": cap, "merges": int(out[3]),
                "values": _device_view(pv, (cap,), "|u1", dev) if pv.value and cap else None,
                "value_off": _device_view(po, (n + 1,), "<i8", dev) if po.value and n else None,
                "rows": _device_view(pr, (n,), "<i8", dev) if pr.value and n else None}

    def event_strings_next_column(self, column: int):
        """Where the next merge writes ``column`` (``surge_device_decoder_event_strings_next_column``: the call reserves what
        that merge would): ``(utf8, off)`` — CUDA ``uint8`` tensors over the WHOLE capacity of the two buffers — or ``None``
        for a column the next merge would not write.  A ``state_strings()`` right behind it merges into exactly these."""
        import torch

        out = (ctypes.c_int64 * 3)()
        pu, po = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_event_strings_next_column(self._h, column, ctypes.byref(out), ctypes.byref(pu), ctypes.byref(po)))
        if not pu.value or not po.value:
            return None
        dev = torch.device("cuda", self.device)
        torch.cuda.synchronize(dev)
        return _device_view(pu, (int(out[0]),), "|u1", dev), _device_view(po, (int(out[1]),), "|u1", dev)

    def close(self):
        if self._h:
            self._lib.surge_device_decoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise IngestError(rc, (self._lib.surge_device_decoder_last_error(self._h) or b"").decode())

    def push(self, sections: np.ndarray, arena_address: int, floors=None) -> None:
        """``floors``: the ``FLOOR_DTYPE`` records of these sections (``take_floors`` / ``Framed.floors``): records below a
        section's floor are passed over on the device (``surge_device_decoder_push_floored``)."""
        sections = np.ascontiguousarray(sections, dtype=SECTION_DTYPE)
        floors = NO_FLOORS if floors is None else np.ascontiguousarray(floors, dtype=FLOOR_DTYPE)
        self._check(self._lib.surge_device_decoder_push_floored(self._h, ctypes.c_void_p(arena_address), sections.ctypes.data_as(ctypes.c_void_p),
                                                                sections.shape[0], floors.shape[0], floors.ctypes.data_as(ctypes.c_void_p)))

    def push_async(self, parts, floors=None) -> None:
        """Stage 1 of a push — copy, LZ4, record parsing, value decode — enqueued on a stream of its own; ``parts`` is one
        ``(sections, arena_address)`` pair or a list of them (e.g. one per partition of a fetch response: one push, records
        delivered part after part).  The arenas must stay as they are until the matching ``finish()``; up to five pushes
        may be in flight.  A part that is a ``Framed`` brings its floors along; ``floors`` gives them for plain pairs, their
        ``section`` counting through the parts' sections in order."""
        if isinstance(parts, tuple):
            parts = [parts]
        secs = [np.ascontiguousarray(s, dtype=SECTION_DTYPE) for s, _ in parts]
        n = len(parts)
        if floors is None:  # each Framed part's floors, its section indices moved behind the parts in front of it
            moved, first = [], 0
            for part, s in zip(parts, secs):
                f = getattr(part, "floors", NO_FLOORS)
                if f.shape[0]:
                    f = f.copy()
                    f["section"] += first
                    moved.append(f)
                first += s.shape[0]
            floors = np.concatenate(moved) if moved else NO_FLOORS
        floors = np.ascontiguousarray(floors, dtype=FLOOR_DTYPE)
        bytes_arr = (ctypes.c_void_p * n)(*[ctypes.c_void_p(a) for _, a in parts])
        secs_arr = (ctypes.c_void_p * n)(*[s.ctypes.data_as(ctypes.c_void_p) for s in secs])
        cnt = (ctypes.c_int64 * n)(*[s.shape[0] for s in secs])
        self._check(self._lib.surge_device_decoder_push_parts_floored_async(self._h, n, bytes_arr, secs_arr, cnt, floors.shape[0],
                                                                            floors.ctypes.data_as(ctypes.c_void_p)))
        self._inflight.append((secs, bytes_arr, secs_arr, cnt, floors))  # (kept until finish(); list.append / pop are atomic: a pushing and a finishing thread share it)

    def finish(self, wait: bool = True) -> None:
        """Stage 2 of the oldest unfinished push: key interning, append to the result (``result()``).  ``wait=False``
        (``surge_device_decoder_push_finish_async``) returns without the closing wait for the device: the results are
        complete in the order of the decoder's stream — hand them over with ``fold_into(engine, wait=False)``.  One thread
        may call ``push_async`` while another calls ``finish`` / ``fold_into`` (``PushPipeline``)."""
        rc = (self._lib.surge_device_decoder_push_finish if wait else self._lib.surge_device_decoder_push_finish_async)(self._h)
        if self._inflight:
            self._inflight.pop(0)
        self._check(rc)

    def fold_into(self, engine, wait: bool = True):
        """Everything decoded since the last clear, folded onto ``engine``'s resident state (grown first for ids seen for the
        first time), and cleared: ``surge_replay_append_decoded``; with ``wait=False`` its ``_async`` form — no host wait,
        the two streams are ordered by events, so the host goes on to enqueue the next push while this fold runs (and with
        the engine on a stream of its own the interning of the next fetch overlaps it on the device too: the decoder then
        rotates stage 1 over two streams instead of three — hardware queues, ``include/surge_ingest.h``).  What the fold
        has to report it reports at the engine's next ``synchronize``.  Returns ``(n_events, n_keys)``."""
        n_ev, n_keys = ctypes.c_int64(), ctypes.c_int64()
        fn = self._lib.surge_replay_append_decoded if wait else self._lib.surge_replay_append_decoded_async
        self._check(fn(engine._h, self._h, ctypes.byref(n_ev), ctypes.byref(n_keys)))
        return int(n_ev.value), int(n_keys.value)

    def stage_into(self, engine):
        """Everything decoded since the last clear, appended to ``engine``'s staging log instead of folded, and cleared
        (``surge_replay_stage_decoded``; no host wait).  A recovery that folds the topic once ends with
        ``engine.pack_staged(n_keys)`` + one ``engine.fold()``.  Returns ``(n_events, n_keys)``."""
        n_ev, n_keys = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.surge_replay_stage_decoded(engine._h, self._h, ctypes.byref(n_ev), ctypes.byref(n_keys)))
        return int(n_ev.value), int(n_keys.value)

    @property
    def n_keys(self) -> int:
        n = ctypes.c_int64()
        if self.states:
            self._check(self._lib.surge_device_decoder_state_result(self._h, None, None, None, None, None, ctypes.byref(n)))
        else:
            self._check(self._lib.surge_device_decoder_result(self._h, None, None, None, None, ctypes.byref(n)))
        return int(n.value)

    def reserve(self, n_keys: int, key_bytes: int) -> None:
        """Capacity hint (``surge_device_decoder_reserve``): room for ``n_keys`` aggregate ids of ``key_bytes`` bytes in all."""
        self._check(self._lib.surge_device_decoder_reserve(self._h, int(n_keys), int(key_bytes)))

    @property
    def pending(self) -> int:
        return int(self._lib.surge_device_decoder_pending(self._h))

    def push_records(self, keys: List[bytes], values: List[bytes], offsets=None) -> None:
        """Records that are already framed (a consumer's key / value byte arrays), in bulk."""
        def table(items):
            off = np.zeros(len(items) + 1, dtype=np.int64)
            if items:
                np.cumsum([len(x) for x in items], out=off[1:])
            data = np.frombuffer(b"".join(items), dtype=np.uint8) if off[-1] else np.zeros(1, np.uint8)
            return data, off

        kd, ko = table(keys)
        vd, vo = table(values)
        of = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        self._check(self._lib.surge_device_decoder_push_records(
            self._h, kd.ctypes.data_as(ctypes.c_void_p), ko.ctypes.data_as(ctypes.c_void_p), vd.ctypes.data_as(ctypes.c_void_p),
            vo.ctypes.data_as(ctypes.c_void_p), of.ctypes.data_as(ctypes.c_void_p) if of is not None else None, len(keys)))

    def push_from(self, ingest: EventsTopicIngest) -> int:
        """Everything ``ingest`` (created with ``frames=True``) can deliver now; returns the number of batches."""
        sections, arena = ingest.drain_sections()
        if sections.shape[0]:
            self.push(sections, arena, ingest.take_floors())
        return int(sections.shape[0])

    def result(self):
        """``(agg_idx, events, offsets)`` as CUDA tensors viewing the decoder's arrays (valid until the next push / clear)
        and the number of keys so far."""
        import torch

        n, nk = ctypes.c_int64(), ctypes.c_int64()
        pa, pe, po = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_result(self._h, ctypes.byref(n), ctypes.byref(pa), ctypes.byref(pe), ctypes.byref(po), ctypes.byref(nk)))
        dev = torch.device("cuda", self.device)
        if n.value == 0:
            z = torch.zeros(0, dtype=torch.int64, device=dev)
            return z, torch.zeros((0, 2), dtype=torch.int64, device=dev), z.clone(), nk.value
        return _device_view(pa, (n.value,), "<i8", dev), _device_view(pe, (n.value, 2), "<i8", dev), _device_view(po, (n.value,), "<i8", dev), nk.value

    def state_result(self):
        """A state decoder's records since the last clear: ``(agg_idx, values, value_off, offsets, n_keys)`` — CUDA tensors
        viewing the decoder's arrays (valid until the next ``finish`` / ``clear`` / ``load_states_into``): record ``r`` names
        aggregate ``agg_idx[r]``, its value is ``values[value_off[r]:value_off[r+1]]`` (empty: a tombstone) and its Kafka
        offset ``offsets[r]``."""
        import torch

        n, nk = ctypes.c_int64(), ctypes.c_int64()
        pa, pv, pvo, po = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_state_result(self._h, ctypes.byref(n), ctypes.byref(pa), ctypes.byref(pv), ctypes.byref(pvo), ctypes.byref(po),
                                                                ctypes.byref(nk)))
        dev = torch.device("cuda", self.device)
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        if n.value == 0:
            return z, torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), z.clone(), nk.value
        torch.cuda.synchronize(dev)  # (a finish(wait=False) leaves the arrays complete in stream order only)
        value_off = _device_view(pvo, (n.value + 1,), "<i8", dev)
        total = int(value_off[-1].item())
        values = _device_view(pv, (total,), "|u1", dev) if total else torch.zeros(0, dtype=torch.uint8, device=dev)
        return _device_view(pa, (n.value,), "<i8", dev), values, value_off, _device_view(po, (n.value,), "<i8", dev), nk.value

    def load_states_into(self, engine, template, envelope: str = "none"):
        """A state decoder's hand-over (``surge_device_decoder_load_states``; ``envelope="protobuf_state"``:
        ``surge_device_decoder_load_protobuf_states``, the values are the multilanguage module's ``State`` messages around the
        template's text): everything delivered since the last clear is
        decoded through ``template`` (the model's serialized state, ``encode.JsonTemplate``) into ``engine``'s resident state
        — grown first for ids seen for the first time; per aggregate the last record wins, a tombstone zeroes the row — and
        the decoder is cleared.  Returns the decode's counts ``(rows written, tombstones, winners refused, Doubles re-parsed
        on the host)``; a refused winner raises ``IngestError`` (CORRUPT, naming the record's topic offset) after everything
        else was loaded."""
        from .encode import check_envelope

        fn = self._lib.surge_device_decoder_load_protobuf_states if check_envelope(envelope) else self._lib.surge_device_decoder_load_states
        counts = (ctypes.c_int64 * 4)()
        t = template.to_c()
        rc = fn(self._h, engine._h, ctypes.byref(t), ctypes.byref(counts))
        engine.n_agg = max(engine.n_agg, self.n_keys)  # (grown inside the call)
        self._check(rc)
        return tuple(int(c) for c in counts)

    def state_strings(self):
        """The STR columns a ``keep_strings=True`` state decoder has kept, or an events decoder armed with ``event_strings``
        (``surge_device_decoder_state_strings``; on the latter the call merges what the pushes since the last one kept): one
        entry per string column, ``(d_utf8, d_off)`` CUDA tensors viewing the decoder's buffers (valid until the next
        ``load_states_into`` / ``finish`` / ``clear`` / ``close``: clone what has to live longer) — aggregate ``a``'s string is
        ``d_utf8[d_off[a]:d_off[a+1]]`` — or ``None`` for a column nothing has named."""
        import torch

        from .encode import STRING_COLUMNS

        dev = torch.device("cuda", self.device)
        cols = []
        for c in range(STRING_COLUMNS):
            pu, po, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
            self._check(self._lib.surge_device_decoder_state_strings(self._h, c, ctypes.byref(pu), ctypes.byref(po), ctypes.byref(n)))
            if not po.value:
                cols.append(None)
                continue
            d_off = _device_view(po, (n.value + 1,), "<i8", dev)
            total = int(d_off[-1].item())
            cols.append((_device_view(pu, (total,), "|u1", dev) if total else torch.zeros(0, dtype=torch.uint8, device=dev), d_off))
        return cols

    def clear(self) -> None:
        self._check(self._lib.surge_device_decoder_clear(self._h))

    def continue_as_events(self, template: Optional[EventJsonTemplate] = None) -> None:
        """A state decoder that has loaded its topic goes on as the events decoder of the same aggregates
        (``surge_device_decoder_continue_as_events``): the key table stays — the ids it interned are the resident state's rows —
        and from here on the decoder reads events (``template`` as in the constructor), numbering new ids behind the known
        ones.  Needs every push finished and every record loaded or cleared; one-way.  Kept string columns stay readable
        (``state_strings``)."""
        c = template.to_c() if template is not None else None
        self._check(self._lib.surge_device_decoder_continue_as_events(self._h, ctypes.byref(c) if c is not None else None))
        self.states = False

    def below_floor(self) -> int:
        """Records passed over below a section's floor so far (``surge_device_decoder_below_floor``)."""
        n = ctypes.c_int64()
        self._check(self._lib.surge_device_decoder_below_floor(self._h, ctypes.byref(n)))
        return int(n.value)

    def keys(self) -> List[str]:
        n, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.surge_device_decoder_keys(self._h, None, 0, None, ctypes.byref(n), ctypes.byref(nb)))
        data = np.zeros(max(nb.value, 1), np.uint8)
        off = np.zeros(n.value + 1, np.int64)
        self._check(self._lib.surge_device_decoder_keys(self._h, data.ctypes.data_as(ctypes.c_void_p), data.shape[0], off.ctypes.data_as(ctypes.c_void_p),
                                                        ctypes.byref(n), ctypes.byref(nb)))
        raw = data.tobytes()
        return [raw[off[i]:off[i + 1]].decode("utf-8") for i in range(n.value)]

    def device_key_table(self):
        """``(d_utf8, d_key_off)``: CUDA tensors viewing the key table where it lives (``surge_device_decoder_key_table``; what the
        state encoders and ``encode.encode_rows`` take), valid until the next push that finds a new id, or ``close``.  ``d_utf8`` covers
        the ids' bytes; the arena behind it is the decoder's."""
        import torch

        n, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.surge_device_decoder_keys(self._h, None, 0, None, ctypes.byref(n), ctypes.byref(nb)))
        pk, po = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_key_table(self._h, ctypes.byref(pk), ctypes.byref(po)))
        dev = torch.device("cuda", self.device)
        d_utf8 = _device_view(pk, (nb.value,), "|u1", dev) if nb.value else torch.zeros(0, dtype=torch.uint8, device=dev)
        return d_utf8, _device_view(po, (n.value + 1,), "<i8", dev)

    def lookup(self, ids) -> np.ndarray:
        """Which row is each id (``surge_device_decoder_lookup``): ``ids`` are ``str`` (UTF-8) or ``bytes``; returns ``np.int64[n]``,
        an id's dense index — its position in first-delivered order — or ``-1`` when the table does not hold it.  Compared byte
        for byte as it stands (no cut at ``:``).  Every push has to be finished (``IngestError``, STATE, otherwise)."""
        data, off = key_table_utf8(ids, slack=1)  # (one byte, so that no id at all still has an address)
        n = off.shape[0] - 1
        out = np.empty(n, dtype=np.int64)
        self._check(self._lib.surge_device_decoder_lookup(self._h, data.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), n,
                                                          out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def lookup_device(self, d_ids, d_off):
        """The same for queries that are on the device already (``surge_device_decoder_lookup_device``): ``d_ids`` a ``uint8`` CUDA
        tensor READABLE 16 BYTES BEHIND ITS LAST ID (pad it: ids are compared four bytes a load), ``d_off`` ``n + 1`` ``int64``
        offsets into it.  Returns an ``int64`` CUDA tensor.  Nothing waits on the host: the work is enqueued on the decoder's stream,
        behind what torch's current stream has enqueued so far (the queries), and torch's current stream is made to wait for it —
        the tensor is complete in the order of that stream, like any tensor torch computes."""
        import torch

        n = int(d_off.numel()) - 1
        dev = torch.device("cuda", self.device)
        out = torch.empty(max(n, 0), dtype=torch.int64, device=dev)
        if n > 0:
            with torch.cuda.device(dev):
                mine = torch.cuda.ExternalStream(int(self._stream)) if self._stream else torch.cuda.default_stream(dev)
                current = torch.cuda.current_stream(dev)
                mine.wait_stream(current)  # (the queries may have been written on another stream than the decoder's)
                self._check(self._lib.surge_device_decoder_lookup_device(self._h, ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), n,
                                                                         ctypes.c_void_p(out.data_ptr())))
                current.wait_stream(mine)
        return out

    # -- the key table in key order (unsigned bytes, a proper prefix first: Kafka's ``Bytes`` order, ``sorted`` on ``bytes``) --------
    def _behind_torch(self):
        """The decoder's stream waits for what torch's current stream has enqueued (a row list torch computed).  The calls below
        return when their results are there, so nothing has to wait the other way round."""
        import torch

        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            mine = torch.cuda.ExternalStream(int(self._stream)) if self._stream else torch.cuda.default_stream(dev)
            mine.wait_stream(torch.cuda.current_stream(dev))

    def key_order(self):
        """The dense indices in key order (``surge_device_decoder_key_order``): an ``int64`` CUDA tensor viewing the decoder's
        array — valid until the next push that interns an id, or ``close`` — built now if the table has grown since the last
        build.  ``order_passes`` says what that build took."""
        import torch

        po, n, passes = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.surge_device_decoder_key_order(self._h, ctypes.byref(po), ctypes.byref(n), ctypes.byref(passes)))
        self.order_passes = int(passes.value)
        dev = torch.device("cuda", self.device)
        return _device_view(po, (n.value,), "<i8", dev) if n.value else torch.zeros(0, dtype=torch.int64, device=dev)

    def range_rows(self, from_key=None, to_key=None):
        """The rows whose id lies in ``[from_key, to_key]`` — both ends inclusive, as a Kafka Streams ``range`` — ascending by id
        (``surge_device_decoder_range_device``): an ``int64`` CUDA tensor of the caller's.  A bound is ``str`` (its UTF-8), ``bytes``
        or ``None`` (unbounded: ``range_rows()`` is every row in key order); ``b""`` is the empty id, not ``None``.  ``from_key >
        to_key``: no row.  Two calls: the count, then the rows."""
        import torch

        def bound(k):
            if k is None:
                return None, 0
            raw = k.encode("utf-8") if isinstance(k, str) else bytes(k)
            return ctypes.create_string_buffer(raw, len(raw) + 1), len(raw)  # (never NULL, also for the empty id)

        (pf, nf), (pt, nt) = bound(from_key), bound(to_key)
        dev = torch.device("cuda", self.device)
        n = ctypes.c_int64()
        rc = self._lib.surge_device_decoder_range_device(self._h, pf, nf, pt, nt, None, 0, ctypes.byref(n))
        if rc != -6:  # (SURGE_E_RANGE: there are rows, and no room was given)
            self._check(rc)
            return torch.zeros(0, dtype=torch.int64, device=dev)
        out = torch.empty(n.value, dtype=torch.int64, device=dev)
        self._behind_torch()
        self._check(self._lib.surge_device_decoder_range_device(self._h, pf, nf, pt, nt, ctypes.c_void_p(out.data_ptr()), n.value, ctypes.byref(n)))
        return out[: n.value]

    def gather_keys(self, d_rows) -> List[bytes]:
        """The ids of ``d_rows`` (an ``int64`` CUDA tensor of rows inside the table), in that order
        (``surge_device_decoder_gather_keys_device``; one copy back).  A row outside ``[0, n_keys)`` raises ``IngestError`` (INVALID)."""
        import torch

        n = int(d_rows.numel())
        if n == 0:
            return []
        dev = torch.device("cuda", self.device)
        d_rows = d_rows.contiguous()
        d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        total = ctypes.c_int64(-1)
        cap = 0
        self._behind_torch()
        for _ in range(2):  # (the first call says how many bytes the ids are)
            d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            rc = self._lib.surge_device_decoder_gather_keys_device(self._h, ctypes.c_void_p(d_rows.data_ptr()), n, ctypes.c_void_p(d_out.data_ptr()), cap,
                                                                   ctypes.c_void_p(d_off.data_ptr()), ctypes.byref(total))
            if rc != -6 or total.value <= cap:
                break
            cap = total.value
        self._check(rc)
        raw, off = d_out[: total.value].cpu().numpy().tobytes(), d_off.cpu().numpy().tolist()
        return [raw[off[q]:off[q + 1]] for q in range(n)]

    def counters(self) -> dict:
        c = (ctypes.c_int64 * 4)()
        self._lib.surge_device_decoder_counters(self._h, ctypes.byref(c))
        return dict(zip(["records_seen", "records_delivered", "flush_records_skipped", "doubles_parsed_on_host"], [int(x) for x in c]))

    def stats(self) -> dict:
        """The counters plus the key table's: re-seeds after a detected 64-bit hash collision, slots, pushes, hash function."""
        c = (ctypes.c_int64 * 8)()
        self._lib.surge_device_decoder_stats(self._h, ctypes.byref(c))
        return dict(zip(["records_seen", "records_delivered", "flush_records_skipped", "doubles_parsed_on_host", "hash_reseeds", "table_slots", "pushes",
                         "hash_function"], [int(x) for x in c]))
