"""The reads of ``GpuReplayStateStore`` (seam S2 and the reads in key order): one path for both routes — the device decoder's
key table after a ``host_keys=False`` restore, the host table otherwise — and both shapes, a batch of ids and pages of a range.
(``torch`` is imported where it is used: importing the store must not load it.)"""
from __future__ import annotations

import bisect
import contextlib
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .core import write_state_of
from .encode import JP_STR, READ_POISONED, READ_VALUE, JsonTemplate, check_envelope, encode_rows, key_table_utf8, merge_state_strings
from .schema import STATE_DTYPE, STATE_POISONED, STATE_PRESENT


class AggregateInitializationException(RuntimeError):
    """Mirror of the error an actor gets when its state cannot be initialised
    (``PersistentActor.scala:328-333``); raised for aggregates whose replay hit a throwing event."""


def _poisoned(aggregate_id: str) -> AggregateInitializationException:
    return AggregateInitializationException(f"replay of aggregate {aggregate_id!r} hit an event whose handler throws; state is frozen before it")


def _str_columns(template) -> set:
    """The string columns a ``JsonTemplate``'s ``(JP_STR, column)`` parts name."""
    return {int(p[1]) for p in template.parts if isinstance(p, tuple) and int(p[0]) == JP_STR}


class StoreReads:
    """What ``GpuReplayStateStore`` answers reads with (its docstring lists the members used here)."""

    @contextlib.contextmanager
    def _on_device_route(self):
        """The route decision: on the device route ``_device_lock`` is taken, and the decoder is yielded if the store is still on
        that route once it is held; else ``None`` (the host route: its table and mirror serve any number of readers, no lock)."""
        with self._device_lock if self._decoder is not None else contextlib.nullcontext():
            yield self._decoder

    # -- the pieces every read composed on the GPU goes through --------------------------------------------------------------
    def _device_key_table(self, d):
        """``(d_utf8, d_key_off)``, the key table on the device: the decoder's where it lives, else the host table, uploaded once per size."""
        if d is not None:
            return d.device_key_table()
        import torch

        keys = self._keys
        if self._uploaded_keys is None or self._uploaded_keys[0] != len(keys):
            dev = torch.device("cuda", self.engine.device)
            kd, ko = key_table_utf8(keys.keys)
            self._uploaded_keys = (len(keys), torch.from_numpy(kd).to(dev), torch.from_numpy(ko).to(dev))
        return self._uploaded_keys[1:]

    def _strings_for(self, template):
        """``state_string_columns()``, checked to hold every string column ``template`` names."""
        strings = self.state_string_columns()
        for c in _str_columns(template):
            if c >= len(strings) or strings[c] is None:
                raise ValueError(f"the template names string column {c}, and nothing restored it")
        return strings

    def _encode(self, d, template, envelope: str, d_rows, strings):
        """``encode_rows`` and the copy back: ``(raw, offsets, kind)`` — row ``q``'s bytes are ``raw[offsets[q]:offsets[q + 1]]``, ``kind[q]`` its ``READ_*``."""
        out, out_off, kind = encode_rows(self.engine, template, *self._device_key_table(d), d_rows, envelope=envelope, strings=strings)
        return out.cpu().numpy().tobytes(), out_off.cpu().numpy().tolist(), kind.cpu().numpy()

    # -- S2 ---------------------------------------------------------------------------------
    def get_aggregate_bytes(self, aggregate_id: str) -> Optional[bytes]:
        """``None`` = no such aggregate (KTable miss) or tombstone; else ``writeState(state).value``.  On the device route
        (``host_keys=False``) the bytes are ``get_aggregate_bytes_many([aggregate_id])``' — ``read_template`` / ``read_envelope``
        composed on the GPU; one launch chain and two copies per call, so batches are what that route is for."""
        if self._decoder is not None:  # (see ``get_aggregate``)
            with self._on_device_route() as d:
                if d is not None:
                    return self.get_aggregate_bytes_many([aggregate_id], self.read_template, self.read_envelope)[0]
        agg = self.get_aggregate(aggregate_id)
        if agg is None:
            return None
        return write_state_of(self.business_logic.aggregate_write_formatting(), aggregate_id, agg).value

    def get_aggregate_bytes_many(self, aggregate_ids: Sequence[str], template=None, envelope: str = "none") -> List[Optional[bytes]]:
        """``get_aggregate_bytes`` for a batch of ids, composed on the GPU: the ids' rows — a lookup in the decoder's device key
        table on the device route, the host table otherwise (its ids uploaded once) — then ``encode.encode_rows`` through
        ``template`` (the model's serialized state; default ``JsonTemplate.counter()``, as in ``restore_from_state_topic``) and
        one copy back.  ``None`` for an id the store does not hold and for a tombstone; ``AggregateInitializationException`` when
        one of the ids is poisoned, as the single read raises it.  ``(JP_STR, column)`` parts take ``state_string_columns()``;
        a column nothing restored raises ``ValueError``.  ``envelope="protobuf_state"``: what a multilanguage application
        stores.  The columns come from a resume from the state topic or from ``restore_from_fetches(keep_strings=True)``; an events
        tail read as bytes with ``restore_from_state_topic(events_fetches=..., keep_event_strings=True)`` goes into the same
        columns, so its aggregates read the same on both paths.  What is left: aggregates that first appear through
        ``apply_events`` (decoded events, a host-side ``events_tail``), or through an events tail read without
        ``keep_event_strings``, have EMPTY strings in the columns — theirs are the host model's alone, so for such an aggregate a STR part is
        written ``""`` here while ``get_aggregate_bytes`` — the plugin's formatter over ``restore_static_strings`` — writes the real
        string.  Every other part, and every aggregate the topics carried, reads the same on both."""
        import torch

        check_envelope(envelope)
        template = template or JsonTemplate.counter()
        ids = list(aggregate_ids)
        if not ids:
            return []
        eng = self.engine
        dev = torch.device("cuda", eng.device)
        with self._device_lock, self._on_device_route() as d:  # (the host route composes on the device too: one reader at a time)
            strings = self._strings_for(template)
            if d is not None:
                data, off = key_table_utf8(ids, slack=16)  # (the slack behind the last id the lookup's loads may touch)
                d_rows = d.lookup_device(torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev))
                if eng.stream_ptr:  # (the rows are complete in the order of torch's current stream; an engine on a stream of its own is not in it)
                    torch.cuda.current_stream(dev).synchronize()
            else:
                n_agg = eng.n_agg
                rows = np.fromiter((-1 if i is None or i >= n_agg else i for i in map(self._keys.get, ids)), dtype=np.int64, count=len(ids))
                d_rows = torch.from_numpy(rows).to(dev)
            raw, off, kind = self._encode(d, template, envelope, d_rows, strings)
        bad = np.flatnonzero(kind == READ_POISONED)
        if bad.shape[0]:
            raise _poisoned(ids[int(bad[0])])
        value = (kind == READ_VALUE).tolist()
        return [raw[off[q]:off[q + 1]] if value[q] else None for q in range(len(ids))]

    def get_aggregate(self, aggregate_id: str):
        # A read on the host route pays one attribute read for the route decision and no context manager: entering one costs
        # what a tenth of such a read does, and 10^6 of them in a loop are a series ``scripts/point_read_bench.py`` measures.
        if self._decoder is None:
            return self._aggregate_at(aggregate_id, None)
        with self._on_device_route() as d:
            return self._aggregate_at(aggregate_id, d)

    def _aggregate_at(self, aggregate_id: str, d):  # d: the decoder on the device route, None on the host route
        if d is None:
            idx = self._keys.get(aggregate_id)
        else:
            idx = int(d.lookup([aggregate_id])[0])
            idx = None if idx < 0 else idx
        if idx is None or idx >= self.engine.n_agg:
            return None
        raw = self.engine.get_raw(idx) if d is None else self.engine.gather([idx])[0]  # (no mirror on the device route: surge_replay_gather)
        if int(raw["flags"]) & STATE_POISONED:
            raise _poisoned(aggregate_id)
        if not int(raw["flags"]) & STATE_PRESENT:
            return None
        hook = getattr(self.model, "restore_static_strings", None)
        if self.state_strings and hook is not None:  # string fields the state topic carried (the model keeps what it already knows)
            strings = self._restored_strings(idx)
            if any(x is not None for x in strings):
                hook(aggregate_id, strings)
        return self.model.state_from_fixed(aggregate_id, raw)

    # -- reads in key order: KafkaStreamsKeyValueStore.range / all, SurgeAggregateStore.getSubstatesForAggregate ----------------
    def _sorted_host_keys(self) -> List[str]:
        """The host table's ids in key order (code points: the order of their UTF-8 bytes), sorted once per table size."""
        keys = self._keys
        if self._sorted_keys is None or self._sorted_keys[0] != len(keys):
            self._sorted_keys = (len(keys), sorted(keys.keys))
        return self._sorted_keys[1]

    def range_bytes(self, from_key: Optional[str] = None, to_key: Optional[str] = None, template=None, envelope: Optional[str] = None,
                    page_rows: int = 1 << 20) -> Iterator[Tuple[str, bytes]]:
        """``(id, writeState(state).value)`` of every aggregate whose id lies in ``[from_key, to_key]`` — both ends inclusive,
        ``None``: unbounded — ascending by the ids' UTF-8 bytes: ``KafkaStreamsKeyValueStore.range``
        (``.../streams/KafkaStreamsKeyValueStore.scala:41-51``) over the recovered state.  On the device route the rows come from
        the decoder's key order (``DeviceDecoder.range_rows``: two binary searches and a slice), their bytes from
        ``encode.encode_rows`` and their ids from ``DeviceDecoder.gather_keys``, ``page_rows`` rows at a time: the store stays on
        the device route, no host table is built, no mirror published, and never more than a page of text is held.  With a host
        table the rows are a ``bisect`` over its sorted ids and the bytes the same encoders'.  Aggregates that are ``None`` or
        ended are passed over; a poisoned aggregate in the range raises ``AggregateInitializationException`` naming it when its
        page is reached, as the point read does.  ``template`` / ``envelope`` default to ``read_template`` / ``read_envelope``."""
        import torch

        envelope = self.read_envelope if envelope is None else envelope
        check_envelope(envelope)
        template = template or self.read_template or JsonTemplate.counter()
        page_rows = max(1, int(page_rows))
        dev = torch.device("cuda", self.engine.device)
        with self._device_lock:
            strings = self._strings_for(template)
            d = self._decoder
            if d is not None:
                d_rows = d.range_rows(from_key, to_key)
                host_ids = None
            else:
                order = self._sorted_host_keys()
                lo = 0 if from_key is None else bisect.bisect_left(order, from_key)
                hi = len(order) if to_key is None else bisect.bisect_right(order, to_key)
                index, n_agg = self._keys.index, self.engine.n_agg
                host_ids = [k for k in order[lo:hi] if index[k] < n_agg]
                d_rows = torch.from_numpy(np.fromiter((index[k] for k in host_ids), dtype=np.int64, count=len(host_ids))).to(dev)
        for first in range(0, int(d_rows.numel()), page_rows):
            with self._device_lock:
                if self._decoder is not d:
                    raise RuntimeError("the store's key table moved while a range was being read: start the range again")
                page = d_rows[first:first + page_rows]
                raw, off, kind = self._encode(d, template, envelope, page, strings)
                bad = np.flatnonzero(kind == READ_POISONED)
                if bad.shape[0]:
                    q = int(bad[0])
                    raise _poisoned(host_ids[first + q] if d is None else d.gather_keys(page[q:q + 1])[0].decode("utf-8"))
                kept = np.flatnonzero(kind == READ_VALUE)
                if d is None:
                    ids = [host_ids[first + int(q)] for q in kept]
                else:
                    ids = [k.decode("utf-8") for k in d.gather_keys(page[torch.from_numpy(kept).to(dev)])] if kept.shape[0] else []
            for k, q in zip(ids, kept.tolist()):
                yield k, raw[off[q]:off[q + 1]]

    def all_bytes(self, template=None, envelope: Optional[str] = None, page_rows: int = 1 << 20) -> Iterator[Tuple[str, bytes]]:
        """``KafkaStreamsKeyValueStore.all`` (``KafkaStreamsKeyValueStore.scala:28-39``): ``range_bytes`` without bounds."""
        return self.range_bytes(None, None, template, envelope, page_rows)

    def substates_for_aggregate(self, aggregate_id: str) -> List[Tuple[str, bytes]]:
        """``SurgeAggregateStore.getSubstatesForAggregate`` (``.../streams/SurgeAggregateStore.scala:13-21``): the range
        ``[aggregate_id, aggregate_id + ":~"]``, of which the keys are kept whose text in front of the first ``:`` is the id —
        the reference's filter, applied here over the few results."""
        return [(k, v) for k, v in self.range_bytes(aggregate_id, aggregate_id + ":~") if k.split(":", 1)[0] == aggregate_id]

    def num_entries(self) -> int:
        """How many aggregates ``all_bytes`` would list if none of them were poisoned: rows that are present and not poisoned,
        counted on the device from the resident states' flag words — no text is composed, no state copied."""
        with self._device_lock:
            eng = self.engine
            n = eng.n_agg
            if not n:
                return 0
            eng.synchronize()
            flags = eng.device_state()[:n, STATE_DTYPE.fields["flags"][1]]  # (both flags are in the word's low byte)
            return int(((flags & (STATE_PRESENT | STATE_POISONED)) == STATE_PRESENT).sum().item())

    # -- the string columns a resume from the state topic restored ----------------------------------------------------------------
    def state_string_columns(self):
        """The restored STR columns, extended (``merge_state_strings`` without records: aggregates that appeared after the
        resume get empty strings — theirs stay the host's) to the engine's current aggregate count: what
        ``encode.encode_states(strings=...)`` takes.  ``()`` when nothing was restored."""
        if not self.state_strings:
            return ()
        n_agg = self.engine.n_agg
        for c, col in enumerate(self.state_strings):
            if col is not None and int(col[1].numel()) - 1 < n_agg:
                self.state_strings[c] = merge_state_strings(self.engine, c, prev=col, n_agg=n_agg)
        return tuple(self.state_strings)

    def _restored_strings(self, idx: int):
        """Aggregate ``idx``'s restored strings (one ``bytes`` or ``None`` per column): two slices, no pass over the columns."""
        out = []
        for col in self.state_strings:
            if col is None or idx >= int(col[1].numel()) - 1:
                out.append(None)
                continue
            lo, hi = col[1][idx:idx + 2].tolist()
            out.append(col[0][lo:hi].cpu().numpy().tobytes())
        return out
