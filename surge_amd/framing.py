"""Framing one fetch ahead and keeping pushes in flight: the worker-thread protocols a recovery runs between the host framers
(``host_framer.EventsTopicIngest``, a ``surge_ingest_group``) and ``device_decoder.DeviceDecoder``."""
from __future__ import annotations

import ctypes
import os
import queue
import threading
import time
from typing import List, Optional

import numpy as np

from . import _native
from .host_framer import EventsTopicIngest
from .ingest_types import COUNTER_NAMES, DEVICE_CRC, DEVICE_LZ4, FLOOR_DTYPE, NO_FLOORS, READ_COMMITTED, SECTION_DTYPE, raise_for


class Framed(tuple):
    """What a framer with start offsets yields per fetch: the ``(sections, arena_address)`` pair it always yielded — it
    destructures and indexes as that — with ``floors`` (``FLOOR_DTYPE`` records naming the sections that straddle a start offset:
    what ``DeviceDecoder.push`` / ``push_async`` take beside the sections) and ``positions`` (the offset each partition would
    resume from behind this fetch: ``surge_ingest_position``)."""

    def __new__(cls, sections, address, floors=NO_FLOORS, positions=()):
        self = super().__new__(cls, (sections, address))
        self.floors, self.positions = floors, tuple(positions)
        return self


def _next_of(q):
    """The consumer's end of a worker's queue: the next item — ``None`` marks the end and is put back, so a repeated ``next()``
    raises ``StopIteration`` again; the worker's exception is re-raised in the consumer's thread, the end put back behind it."""
    item = q.get()
    if item is None or isinstance(item, BaseException):
        q.put(None)
        if item is None:
            raise StopIteration
        raise item
    return item


class _FramingAhead:
    """The one-fetch-ahead protocol both framers keep, written once.  A worker thread takes the items of ``fetches`` and
    frames them (``_frame(item)``, the subclass's host stage — and the fetch itself, when ``fetches`` is a generator that
    polls) ONE FETCH AHEAD of whoever iterates.  The native framer rotates through six arenas / slabs, so what fetch i's
    sections point to stays as it is while fetches i + 1 .. i + ``hold`` are framed: ``hold`` (1 .. 5) is how many fetches
    the consumer keeps alive at a time, and the worker holds a slot for each of them plus the one it frames.  ASKING for the
    next fetch while ``hold`` are held is what releases the oldest one's slot — nothing else does: a consumer with pushes in
    flight finishes the oldest push first, then asks (``pushes_in_flight``, ``PushPipeline``).  The worker's exception is
    handed over and re-raised in the consumer's thread (``_next_of``).  ``overlap=False`` frames inline (same results, one thread).

    A subclass names its thread (``_thread_name``) and what there are six of (``_six_of``), creates its native handle
    after ``super().__init__`` and calls ``_start()`` when it is ready to frame; it supplies ``_frame``, ``_close_handle``,
    ``counters``, ``positions`` and ``below_start``."""

    _thread_name = _six_of = None

    def __init__(self, fetches, overlap: bool, hold: int):
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
        item = _next_of(self._q)
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

    def _check(self, rc: int):  # (a group that was not created has a null handle: the library's message of the failed create)
        raise_for(rc, self._lib.surge_ingest_group_last_error, self._h)

    def _frame(self, fetch):
        """One library call per fetch (``surge_ingest_group_feed``): no per-partition Python."""
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
        return _next_of(self._q)

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
