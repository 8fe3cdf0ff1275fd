"""``DeviceDecoder``: the records sections a host framer hands out -> device-resident events (or state values) and a device
key table, through ``surge_device_decoder_*`` in ``include/surge_ingest.h``."""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np

from . import _native
from .encode import STRING_COLUMNS, check_envelope, key_table_utf8
from .ingest_types import FLOOR_DTYPE, NO_FLOORS, SECTION_DTYPE, EventJsonTemplate, EventStrings, raise_for
from .replay import device_view


def _record_table(items, what: str):
    """``(data_uint8, off_int64)`` of one side of a poll: a list of ``bytes`` (``None``: empty) joined, or the pair of arrays as
    it is — contiguous, ``off`` inside ``data``."""
    if isinstance(items, tuple) and len(items) == 2 and isinstance(items[1], np.ndarray):
        data, off = np.ascontiguousarray(items[0], dtype=np.uint8).reshape(-1), np.ascontiguousarray(items[1], dtype=np.int64).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError(f"push_records: {what} offsets need n + 1 entries (got none)")
        if off[0] < 0 or off[-1] < off[0] or off[-1] > data.shape[0]:
            raise ValueError(f"push_records: {what} offsets [{int(off[0])}, {int(off[-1])}] do not lie inside the {data.shape[0]} bytes given")
        return (data if data.shape[0] else np.zeros(1, np.uint8)), off
    items = [b"" if x is None else x for x in items]
    off = np.zeros(len(items) + 1, dtype=np.int64)
    if items:
        np.cumsum([len(x) for x in items], out=off[1:])
    return (np.frombuffer(b"".join(items), dtype=np.uint8) if off[-1] else np.zeros(1, np.uint8)), off


def records_arguments(keys, values, offsets=None):
    """What ``surge_device_decoder_push_records[_async]`` takes behind the handle, for a poll in either form (lists of
    ``bytes``, or ``(data_uint8, off_int64)`` arrays): ``((keys, key_off, values, value_off, offsets, n), arrays)`` — the
    pointers as ``c_void_p`` and the arrays they point into, to be held until the call has returned.  A poll whose sides
    differ in length, or whose offsets are not one per record, raises ``ValueError`` before the library is touched."""
    kd, ko = _record_table(keys, "key")
    vd, vo = _record_table(values, "value")
    n = ko.shape[0] - 1
    if vo.shape[0] - 1 != n:
        raise ValueError(f"push_records: {n} keys for {vo.shape[0] - 1} values")
    of = None
    if offsets is not None:
        of = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if of.shape[0] != n:
            raise ValueError(f"push_records: {of.shape[0]} offsets for {n} records")
    arrays = (kd, ko, vd, vo, of)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    return (ptr(kd), ptr(ko), ptr(vd), ptr(vo), ptr(of) if of is not None and n else None, n), arrays


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
        # (a decoder that was not created has a null handle: the library's message of the failed create)
        if states:
            self._check(self._lib.surge_device_decoder_create_states(device, stream, ctypes.byref(self._h)))
        else:
            self._check(self._lib.surge_device_decoder_create(device, stream, ctypes.byref(c) if c is not None else None, ctypes.byref(self._h)))
        self.event_strings = None
        try:
            if keep_strings:  # (before the first load: every load_states_into then merges the STR columns its template names)
                self._check(self._lib.surge_device_decoder_keep_strings(self._h, 1))
            if event_strings is not None:
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
        torch.cuda.synchronize(torch.device("cuda", self.device))
        n, cap = int(out[0]), int(out[2])
        return {"records": n, "bytes": int(out[1]), "capacity": cap, "merges": int(out[3]),
                "values": self._view(pv, (cap,), "|u1") if pv.value and cap else None,
                "value_off": self._view(po, (n + 1,), "<i8") if po.value and n else None,
                "rows": self._view(pr, (n,), "<i8") if pr.value and n else None}

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
        torch.cuda.synchronize(torch.device("cuda", self.device))
        return self._view(pu, (int(out[0]),), "|u1"), self._view(po, (int(out[1]),), "|u1")

    def close(self):
        if self._h:
            self._lib.surge_device_decoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        raise_for(rc, self._lib.surge_device_decoder_last_error, self._h)

    def _view(self, ptr, shape, typestr: str):
        return device_view(ptr, shape, typestr, self.device)

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

    def push_records(self, keys, values, offsets=None) -> None:
        """Records that are already framed (a consumer's key / value byte arrays), in bulk: ``keys`` and ``values`` are lists
        of ``bytes``, or each a pair of arrays ``(data_uint8, off_int64)`` — record ``i`` is ``data[off[i]:off[i + 1]]`` —
        which go to the library as they are (no Python loop over the records); ``offsets``: the records' Kafka offsets
        (``None``: 0, 1, 2 ..)."""
        args = records_arguments(keys, values, offsets)
        self._check(self._lib.surge_device_decoder_push_records(self._h, *args[0]))

    def push_records_async(self, keys, values, offsets=None) -> None:
        """Stage 1 of ``push_records`` — the copy and the record stage — enqueued on a stream of its own
        (``surge_device_decoder_push_records_async``); ``finish()`` completes the oldest push, wire or records, up to five may
        be in flight.  The arrays are copied inside the call: the caller may reuse them as soon as it returns (a wire push's
        arena must stay until its ``finish()``).  No record at all takes no slot, and there is nothing to finish."""
        args = records_arguments(keys, values, offsets)
        self._check(self._lib.surge_device_decoder_push_records_async(self._h, *args[0]))
        if args[0][-1]:
            self._inflight.append(())  # (finish() pops one entry per push; this one keeps nothing alive)

    def push_from(self, ingest) -> int:
        """Everything ``ingest`` (an ``EventsTopicIngest`` created with ``frames=True``) can deliver now; returns the number of batches."""
        sections, arena = ingest.drain_sections()
        if sections.shape[0]:
            self.push(sections, arena, ingest.take_floors())
        return int(sections.shape[0])

    def result(self):
        """``(agg_idx, events, offsets)`` as CUDA tensors viewing the decoder's arrays (valid until the next push / clear)
        and the number of keys so far."""
        n, nk = ctypes.c_int64(), ctypes.c_int64()
        pa, pe, po = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_result(self._h, ctypes.byref(n), ctypes.byref(pa), ctypes.byref(pe), ctypes.byref(po), ctypes.byref(nk)))
        return self._view(pa, (n.value,), "<i8"), self._view(pe, (n.value, 2), "<i8"), self._view(po, (n.value,), "<i8"), nk.value

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
        if n.value == 0:  # (no offsets array yet, perhaps: the one offset of no record)
            value_off, total = torch.zeros(1, dtype=torch.int64, device=dev), 0
        else:
            torch.cuda.synchronize(dev)  # (a finish(wait=False) leaves the arrays complete in stream order only)
            value_off = self._view(pvo, (n.value + 1,), "<i8")
            total = int(value_off[-1].item())
        return self._view(pa, (n.value,), "<i8"), self._view(pv, (total,), "|u1"), value_off, self._view(po, (n.value,), "<i8"), nk.value

    def load_states_into(self, engine, template, envelope: str = "none", lenient: bool = False):
        """A state decoder's hand-over (``surge_device_decoder_load_states``; ``envelope="protobuf_state"``:
        ``surge_device_decoder_load_protobuf_states``, the values are the multilanguage module's ``State`` messages around the
        template's text): everything delivered since the last clear is
        decoded through ``template`` (the model's serialized state, ``encode.JsonTemplate``) into ``engine``'s resident state
        — grown first for ids seen for the first time; per aggregate the last record wins, a tombstone zeroes the row — and
        the decoder is cleared.  Returns the decode's counts ``(rows written, tombstones, winners refused, Doubles re-parsed
        on the host)``; a refused winner raises ``IngestError`` (CORRUPT, naming the record's topic offset) after everything
        else was loaded.  ``lenient``: the values are read in the engine's lenient mode (``ReplayEngine.reading_leniently``)."""
        fn = self._lib.surge_device_decoder_load_protobuf_states if check_envelope(envelope) else self._lib.surge_device_decoder_load_states
        counts = (ctypes.c_int64 * 4)()
        t = template.to_c()
        with engine.reading_leniently(lenient):
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
        cols = []
        for c in range(STRING_COLUMNS):
            pu, po, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
            self._check(self._lib.surge_device_decoder_state_strings(self._h, c, ctypes.byref(pu), ctypes.byref(po), ctypes.byref(n)))
            if not po.value:
                cols.append(None)
                continue
            d_off = self._view(po, (n.value + 1,), "<i8")
            cols.append((self._view(pu, (int(d_off[-1].item()),), "|u1"), d_off))
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
        n, nb = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.surge_device_decoder_keys(self._h, None, 0, None, ctypes.byref(n), ctypes.byref(nb)))
        pk, po = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.surge_device_decoder_key_table(self._h, ctypes.byref(pk), ctypes.byref(po)))
        return self._view(pk, (nb.value,), "|u1"), self._view(po, (n.value + 1,), "<i8")

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
                mine, current = self._behind_torch()  # (the queries may have been written on another stream than the decoder's)
                self._check(self._lib.surge_device_decoder_lookup_device(self._h, ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), n,
                                                                         ctypes.c_void_p(out.data_ptr())))
                current.wait_stream(mine)
        return out

    # -- the key table in key order (unsigned bytes, a proper prefix first: Kafka's ``Bytes`` order, ``sorted`` on ``bytes``) --------
    def _behind_torch(self):
        """The decoder's stream waits for what torch's current stream has enqueued (a row list torch computed, the queries of a
        lookup); returns the two streams.  The reads in key order return when their results are there, so nothing has to wait
        the other way round; ``lookup_device`` waits for nothing and makes torch's stream wait back."""
        import torch

        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            mine = torch.cuda.ExternalStream(int(self._stream)) if self._stream else torch.cuda.default_stream(dev)
            current = torch.cuda.current_stream(dev)
            mine.wait_stream(current)
        return mine, current

    def key_order(self):
        """The dense indices in key order (``surge_device_decoder_key_order``): an ``int64`` CUDA tensor viewing the decoder's
        array — valid until the next push that interns an id, or ``close`` — built now if the table has grown since the last
        build.  ``order_passes`` says what that build took."""
        po, n, passes = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.surge_device_decoder_key_order(self._h, ctypes.byref(po), ctypes.byref(n), ctypes.byref(passes)))
        self.order_passes = int(passes.value)
        return self._view(po, (n.value,), "<i8")

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

    def route_stats(self) -> dict:
        """What stands behind ``stats()`` (whose eight entries stay what they are): the routes compressed sections took in the pushes
        that delivered — snappy chunks decoded on the device, snappy sections decompressed on the host while the push was planned
        (``surge_device_decoder_route_stats``)."""
        r = (ctypes.c_int64 * 2)()
        self._lib.surge_device_decoder_route_stats(self._h, ctypes.byref(r))
        return dict(zip(["snappy_device_chunks", "snappy_host_sections"], [int(x) for x in r]))
