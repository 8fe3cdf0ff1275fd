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
from .ingest_types import COUNTER_NAMES, DEVICE_CRC, DEVICE_LZ4, FLOOR_DTYPE, FRAMES, READ_COMMITTED, RECORD_DTYPE, SECTION_DTYPE, EventJsonTemplate, raise_for
from .log import KeyTable
from .schema import EVENT_DTYPE


class EventsTopicIngest:
    """``start_offset``: the offset a consumer that sought into the partition begins at (``surge_ingest_set_start_offset``): records
    below it are not delivered, transactions are read as ever; ``None`` / ``<= 0``: from the beginning."""

    def __init__(self, isolation_level: int = READ_COMMITTED, frames: bool = False, device_lz4: bool = False, threads: int = 1, device_crc: bool = False,
                 start_offset: Optional[int] = None):
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        self.frames = frames
        # (a framer that was not created has a null handle: the library's message of the failed create)
        self._check(self._lib.surge_ingest_create(isolation_level | (FRAMES if frames else 0) | (DEVICE_LZ4 if device_lz4 else 0) | (DEVICE_CRC if device_crc else 0),
                                                  ctypes.byref(self._h)))
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
        raise_for(rc, self._lib.surge_ingest_last_error, self._h)

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
