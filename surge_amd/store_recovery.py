"""The recoveries of ``GpuReplayStateStore`` that start from a topic — the events topic from its beginning, or the compacted
state topic and the events behind it — around one loop that keeps pushes in flight over a framer, one ending that settles the
key table and one tail for the two resumes.  (``torch`` is imported where it is used: importing the store must not load it.)"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Sequence

import numpy as np

from . import _native
from .core import SerializedMessage
from .encode import STRING_COLUMNS, JsonTemplate, check_envelope, decode_states, key_table_utf8, merge_state_strings
from .ingest import COUNTER_NAMES, DeviceDecoder, EventsTopicIngest, FramedFetches, IngestError, PartitionedFramedFetches, PushPipeline, pushes_in_flight
from .schema import ALGO_AUTO, EVENT_DTYPE
from .store_reads import _str_columns


class TopicRecoveries:
    """How ``GpuReplayStateStore`` recovers from a topic (its docstring lists the members used here)."""

    def _bind_all_none(self, n_agg: int) -> None:
        """The resident state becomes ``n_agg`` aggregates, every one None (an empty log, folded)."""
        self.engine.load_csr(np.zeros(n_agg + 1, dtype=np.int64), np.zeros(0, dtype=EVENT_DTYPE))
        self.engine.fold()

    def _recovery_ends(self, d, closing, host_keys: bool, publish: bool = True) -> None:
        """The end of a recovery through the device decoder ``d`` (``None``: no record was met, none was made), which ``closing``, the
        caller's ``ExitStack``, would close.  ``host_keys``, or no decoder: the host table adopts the decoder's ids, the decoder is
        closed and — ``publish`` — the host mirror that serves point reads is published.  Else the store keeps the decoder to answer
        the reads, and the host table stays empty until something asks for it (``keys``)."""
        if d is not None and not host_keys:
            self._adopt_keys_of(None)
            closing.pop_all()  # the decoder outlives the caller's block
            self._decoder = d
            return
        self._adopt_keys_of(d)
        closing.close()
        if publish:
            self.engine.snapshot()

    def restore_from_topic(self, record_batches: bytes, capacity: int = 0, algo: int = ALGO_AUTO) -> dict:
        """Recover from the raw bytes of one events-topic partition (Kafka record batches v2, lz4 or none,
        ``read_committed``): ingest (``include/surge_ingest.h``) -> CSR pack -> GPU fold.

        Record values that are exactly 16 bytes are taken as fixed-width events; the plugin's JSON event text is decoded
        through the model's ``event_json_template``.  Both go the device way: the host only frames the batches (headers,
        CRC, transactions, LZ4), the GPU parses the records, interns the aggregate ids, decodes the values and groups
        them (``surge_device_decoder`` + the K3 group-by) — no per-record work in any host language.  A model without a
        template falls back to the host decoder and the plugin's ``SurgeEventReadFormatting.read_event`` per record.
        A template that names an envelope (``EventJsonTemplate(envelope="protobuf_event")``: a multilanguage application's
        topic) decides by itself: its values are never looked at to tell the kind — an enveloped value can be exactly 16
        bytes long.  Returns the ingest counters."""
        template = self.model.event_json_template()
        try:
            return self.restore_from_fetches([record_batches], capacity=capacity, overlap=False)
        except _NotDeviceDecodable:
            pass  # JSON values and a model without a template: the host decoder + the plugin's reader below
        with EventsTopicIngest() as g:
            g.feed(record_batches)
            recs = fixed = None
            if not _enveloped(template):  # (an enveloped value may be 16 bytes long: never taken for a fixed event)
                try:
                    # GPU-ready topic (every value IS the 16-byte fixed event): one vectorised drain, no per-record Python
                    fixed = g.drain_fixed16()
                except IngestError:
                    pass
            if fixed is not None:
                agg_idx, events, _ = fixed
            elif template is not None:
                # the plugin's JSON event text, decoded in the library through the model's template
                agg_idx, events, _ = g.drain_json(template)
            else:
                recs = g.drain_records()  # no template: every value through the plugin's own event reader
            keys = g.key_table()
            counters = g.counters()
        if recs is not None:
            reader = self.business_logic.event_write_formatting()
            events = np.zeros(len(recs), dtype=EVENT_DTYPE)
            agg_idx = np.zeros(len(recs), dtype=np.int64)
            for i, (_, idx, key, value) in enumerate(recs):
                agg_idx[i] = idx
                if value is not None and len(value) == 16:
                    events[i] = np.frombuffer(value, dtype=EVENT_DTYPE)[0]
                else:
                    evt = reader.read_event(SerializedMessage(key.decode("utf-8"), value or b""))
                    events[i] = self.model.encode_events([evt])[0]
        # The records are in topic (offset) order, tagged with their aggregate's dense index: exactly a micro-batch.  The
        # group-by runs on the device (stable radix sort + head scan, the K3 path) onto an all-None resident state; no
        # host-side sort of the whole topic.
        n_agg = max(len(keys), capacity)
        self.keys = keys
        self._bind_all_none(n_agg)  # `algo` only names kernels for bound logs (restore / restore_log)
        if events.shape[0]:
            self.engine.append_events(agg_idx, events)
        self.engine.snapshot()  # publishes the host mirror that serves point reads
        self._restored = True
        return counters

    def restore_from_fetches(self, fetches, capacity: int = 0, overlap: bool = True, n_partitions: int = 0, framing_threads: int = 8,
                             consumer_threads: int = 1, bound_log: bool = False, algo: int = ALGO_AUTO, device_crc: bool = True, in_place: bool = True,
                             host_keys: bool = True, keep_strings: bool = False) -> dict:
        """Recover from the events topic as a consumer receives it: ``fetches`` yields the record-batch bytes of one
        partition, fetch by fetch, in offset order (a list, or a generator that polls) — or, with ``n_partitions``, per
        fetch response the next bytes of each of the consumer's partitions (``PartitionedFramedFetches``: one framer per
        partition on ``framing_threads`` host threads, one device push per fetch).  The host frames the next fetches
        (headers, CRC-32C, transactions) while the GPU works on up to four earlier ones: their copy, LZ4 blocks, record
        parsing and value decode (``DeviceDecoder.push_async``) run ahead of the one whose keys are being interned and
        whose events are grouped and folded onto the resident state (the K3 path), so neither side waits for the other;
        the resident state and the device key table grow as new aggregates appear.  What
        ``SurgeStateStoreConsumer.scala:33-46,57-76`` does record by record through Kafka Streams' restore.
        One consumer thread enqueues a push, waits for the interning of the oldest one and hands its events to the fold by an
        event (``surge_replay_append_decoded_async``): no host wait behind the fold.  ``consumer_threads=2`` moves the host
        work of enqueueing a push (section tables, staging, launches: 0.3 ms per 10^6-record fetch) to a worker thread
        (``PushPipeline``) and drops the wait behind the interning too; measured on the 10^7-aggregate topic it is not
        faster, so one thread is the default.
        ``bound_log=True``: a recovery that folds ONCE — every fetch's decoded events are staged on the device instead of
        folded (``surge_replay_stage_decoded``), the topic's end packs them into one CSR log (``surge_replay_pack_staged``:
        stable device sort by aggregate, topic order kept inside an aggregate) and ONE fold with ``algo`` (AUTO: the
        lane-per-row kernels for a log large enough) produces the states; the packed log stays bound, so ``engine.fold`` /
        ``engine.prepare`` can replay it.  What the reference's restore gets from RocksDB's key order
        (``SurgeStateStoreConsumer.scala:57-76``).
        Needs values the device decoder reads (16-byte fixed events, or JSON with the model's
        ``event_json_template``); returns the ingest + decoder counters.
        ``host_keys=False``: the recovery ends where the GPU does — the decoder stays alive and its key table answers the reads
        (``get_aggregate_bytes`` / ``get_aggregate_bytes_many`` / ``get_aggregate``: a lookup and an encode on the device); no id
        is downloaded, no Python dictionary is built and no host mirror of the states is copied until something asks for the
        host table (``keys``: ``apply_events``, the key/value store's ``all`` / ``range``), which then builds both as the default
        does here.  On that route the bytes of a read are NOT the plugin's ``aggregate_write_formatting``'s: they are composed on
        the GPU through ``read_template`` / ``read_envelope`` — reset here to ``None`` / ``"none"``, that is ``JsonTemplate.counter()``;
        a model with another serialized form sets ``read_template`` after the restore (or passes ``template`` to
        ``get_aggregate_bytes_many``).
        ``keep_strings=True``: the string fields the events carry stay on the device.  The model's optional hook
        ``event_string_fields()`` (an ``ingest.EventStrings``: which event class carries which string, into which column) arms the
        decoder (``DeviceDecoder(event_strings=...)``); a model without the hook raises ``ValueError`` before anything of the
        store changes.  Per aggregate and column the last event in topic order whose class names the column wins; an event
        that lacks a string its class names fails the recovery like any value that does not decode.  At the end
        ``state_strings`` holds the columns (cloned: the decoder may be closed), as after ``restore_from_state_topic`` — so
        ``restore_static_strings``, ``get_aggregate_bytes_many`` / ``range_bytes`` / ``all_bytes`` with a template that has STR
        parts, ``state_string_columns()`` and ``encode_states(strings=...)`` work on top.  The default does what it always did."""
        strings = _event_strings_of(self.model) if keep_strings else None
        with contextlib.ExitStack() as closing:
            def new_decoder(template):
                if strings is not None and template is None:
                    raise ValueError("keep_strings: the topic's values are 16-byte fixed events, which carry no strings")
                # (an earlier device-route restore's decoder goes here, not sooner: up to this point — the fetches' first record, whose
                # values may turn out not to be device-decodable — nothing of the store has changed, and its reads still answer)
                self._drop_decoder()
                return closing.enter_context(DeviceDecoder(template, device=self.engine.device, event_strings=strings))

            counters, n_agg, d = self._fold_fetches(fetches, new_decoder, -1, capacity=capacity, overlap=overlap, n_partitions=n_partitions, framing_threads=framing_threads,
                                                    consumer_threads=consumer_threads, bound_log=bound_log, device_crc=device_crc, in_place=in_place)
            if d is None:  # (made for the first fetch with a record in it)
                self._drop_decoder()  # (no record in the whole topic: the earlier restore's decoder has not been replaced yet)
            self.read_template, self.read_envelope = None, "none"  # (an earlier restore_from_state_topic's)
            if bound_log and d is not None:
                n_agg = max(n_agg, capacity, d.n_keys)
                self.engine.pack_staged(n_agg)  # decoded fetches -> ONE bound CSR log
                self.engine.fold(algo)
                self.engine.synchronize()
            elif n_agg < 0:  # nothing deliverable in the whole topic
                self._bind_all_none(capacity)
            if d is not None:
                counters.update(d.counters())
            if strings is not None:  # (the decoder's buffers go with it: the columns are cloned out, as the state-topic resume does)
                self.state_strings = None if d is None else [None if col is None else (col[0].clone(), col[1].clone()) for col in d.state_strings()]
            self._recovery_ends(d, closing, host_keys)
        self._restored = True
        return counters

    def _fold_fetches(self, fetches, decoder_for, n_agg: int, *, capacity: int = 0, overlap: bool = True, n_partitions: int = 0, framing_threads: int = 8,
                      consumer_threads: int = 1, bound_log: bool = False, device_crc: bool = True, in_place: bool = True, start_offsets=None):
        """The loop of ``restore_from_fetches``, shared with the tail of ``restore_from_state_topic``: the fetches framed ahead,
        up to four pushes in flight, the oldest finished and folded (or staged) without a host wait behind the fold.
        ``decoder_for(template_or_None)`` answers the decoder when the first fetch with a record in it says what the values
        are (a new events decoder; a state decoder that continues as one) — the caller owns and closes it.  ``n_agg``: the
        resident state's aggregate count, ``-1`` while nothing is bound (the first fold then binds ``capacity`` aggregates,
        all None).  ``start_offsets``: per partition (a single int without ``n_partitions``) where the consumer begins
        (``surge_ingest_set_start_offset``): the framers drop what lies below, the floors of the straddling batches travel
        with the pushes.  Returns ``(the framer's counters, n_agg, the decoder or None)``."""
        template = self.model.event_json_template()
        d = None
        # pushes in flight (measured on the 10 M-aggregate topic: 2 / 3 / 4 / 5 in flight = 4.1 / 4.3 / 4.65 / 4.7e8 events/s on
        # one box): stage 1 of the next fetches runs while this one is interned and folded
        depth = 4 if overlap else 1

        def push(item):
            """(the pipeline's worker thread) stage 1 of one fetch; the decoder is made for the first fetch with a record in it"""
            nonlocal d
            parts = _parts_with_records(item)
            if not parts and d is None:
                return False  # (nothing pushed yet: nothing in flight that the framer could overtake)
            if d is None:
                kind = "json" if _enveloped(template) else None  # an envelope is the template's word: the values are not sniffed
                for sec, arena in parts:
                    kind = kind or _sniff_value_kind(sec, arena)  # "fixed16", "json" or None (no deliverable record)
                if kind == "json" and template is None:
                    raise _NotDeviceDecodable("JSON event values need the model's event_json_template")
                d = decoder_for(template if kind == "json" else None)
            d.push_async(parts)
            return True

        two_threads = overlap and consumer_threads >= 2

        def finish_one():
            nonlocal n_agg
            if bound_log:
                d.finish(wait=not two_threads)
                _, n_keys = d.stage_into(self.engine)  # no fold: the topic's end packs what was staged
                n_agg = max(n_agg, n_keys)
                return
            if n_agg < 0:
                n_agg = capacity
                self._bind_all_none(n_agg)
            # No host wait behind the fold: the decoder's stream and the engine's are ordered by events, so the next push is
            # enqueued — and, with two threads (no wait behind the interning either), the next fetch interned — beside this
            # one's group-by and fold (one thread: 7.7 -> 8.7e8 events/s, profiles/r06_e2e_consumer_waits_queues2.txt).  What a
            # fold has to report (a bad index, a poisoned state) it reports at the synchronisation that ends the restore.
            d.finish(wait=not two_threads)
            _, n_keys = d.fold_into(self.engine, wait=False)  # grows the resident state for new ids, group-by + fold (K3), clears
            if n_keys > n_agg:
                self.engine.n_agg = n_agg = n_keys  # (grown inside the call)

        framer = _framer(fetches, n_partitions, framing_threads, depth, overlap, device_crc, in_place, start_offsets)
        with _pushes_driven(framer, push, finish_one, depth, lambda: d, pipelined=two_threads,
                            beside=self.engine.on_own_stream() if two_threads else None) as framed:
            if d is not None:
                self.engine.synchronize()
            counters = framed.counters()
            if start_offsets is not None:
                counters.update(framed.below_start())
        return counters, n_agg, d

    def _resumed(self, n_agg: int, counts, events_tail: Sequence, publish: bool = True, settle=None) -> dict:
        """The end the two resumes from the state topic share: the loaded states become the snapshot baseline (a publish right
        after the load has nothing to say), ``settle()`` does what the caller has left before the store counts as restored, then
        ``events_tail`` is folded on top or — ``publish`` — the host mirror published.  Returns the decode ``counts`` under their names."""
        if n_agg:
            self.engine.snapshot_delta(self.engine.device_state().new_zeros(n_agg), commit=True)  # (a uint8 tensor on the engine's device)
        if settle is not None:
            settle()
        self._restored = True
        if len(events_tail):
            self.apply_events(events_tail)  # grows for new ids, group-by + fold on the device, refreshes the mirror
        elif publish:
            self.engine.snapshot()
        return dict(zip(("rows_written", "tombstones", "refused", "reparsed_on_host"), counts))

    def restore_from_state_records(self, records, events_tail: Sequence = (), template=None, envelope: str = "none", lenient: bool = False) -> dict:
        """Resume from the compacted *state* topic instead of replaying every event — what the reference's restore does
        (``SurgeStateStoreConsumer.scala:57-76``, records written by ``SurgeModel.scala:57-65``).  ``records``: ``(key,
        value_or_None)`` pairs or ``snapshot.StateRecord`` objects in offset order; per key the last record wins and
        ``None`` deletes.  The values are decoded on the device (``encode.decode_states``; ``template``: the model's
        serialized state, default ``JsonTemplate.counter()``) straight into the engine's resident state, the loaded states
        become the snapshot baseline (a publish right after the load has nothing to say), then ``events_tail`` — the
        events behind the snapshot — is folded on top.  Fields the template does not name take the algebra's defaults,
        as ``state_to_fixed`` gives them on the ``restore(prior=...)`` path; the POISONED flag and the sign of ``-0.0``
        are not in the text and are not restored.  A winning value that does not decode raises ``ReplayError`` (CORRUPT).
        ``envelope="protobuf_state"``: the values are what a multilanguage (SDK) application stores, the protobuf
        ``State{aggregateId, payload}`` message around the template's text (``GenericSurgeCommandBusinessLogic.scala:25-27,
        36-39``); any other field, order or repetition is refused, not skipped.  ``lenient=True``: the texts are read as the
        reference's ``Json.parse(bytes).asOpt[State]`` reads them — members in any order, whitespace between the tokens, members
        the template does not name skipped (``surge_replay_set_decode_mode``); the default reads compact text in template order
        only.  Returns the decoder's counts."""
        import torch

        check_envelope(envelope)
        template = template or JsonTemplate.counter()
        str_columns = _str_columns(template)
        self.state_strings = None
        agg_idx, values, lens = [], [], []
        for rec in records:
            key, value = (rec.key, rec.value) if hasattr(rec, "key") else rec
            agg_idx.append(self.keys.intern(key))
            value = b"" if value is None else bytes(value)
            values.append(value)
            lens.append(len(value))
        n_agg, n_rec = len(self.keys), len(agg_idx)
        eng = self.engine
        self._bind_all_none(0)  # no aggregate yet ...
        eng.grow(n_agg)  # ... then every interned id, None
        counts = (0, 0, 0, 0)
        dev = torch.device("cuda", eng.device)
        if n_rec:
            off = np.zeros(n_rec + 1, dtype=np.int64)
            np.cumsum(lens, out=off[1:])
            data, key_off = key_table_utf8(self.keys.keys)
            to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            d_values = to_dev(np.frombuffer(b"".join(values), dtype=np.uint8).copy()) if off[-1] else torch.zeros(0, dtype=torch.uint8, device=dev)
            d_off, d_agg = to_dev(off), to_dev(np.asarray(agg_idx, dtype=np.int64))
            with eng.decoding_onto(self.model.event_algebra().to_c().default_state, lenient=lenient):
                res = decode_states(eng, template, d_values, d_off, to_dev(data), to_dev(key_off), d_agg,
                                    out=eng.device_state(), want_spans=bool(str_columns), raise_on_refused=True, envelope=envelope, lenient=lenient)
            counts = res[2]
            if str_columns:  # the STR fields the values carry, kept beside the rows
                self.state_strings = [merge_state_strings(eng, c, d_values, d_off, d_agg, res[1], res.spans, n_agg=n_agg) if c in str_columns else None
                                      for c in range(STRING_COLUMNS)]
        if str_columns and self.state_strings is None:
            self.state_strings = [merge_state_strings(eng, c, n_agg=n_agg) if c in str_columns else None for c in range(STRING_COLUMNS)]
        return self._resumed(n_agg, counts, events_tail)

    def restore_from_state_topic(self, fetches, n_partitions: int = 0, template=None, events_tail: Sequence = (), framing_threads: int = 4,
                                 device_crc: bool = True, in_place: bool = True, envelope: str = "none", events_fetches=None, events_from=None,
                                 events_partitions: int = 0, host_keys: bool = True, keep_event_strings: bool = False, lenient: bool = False) -> dict:
        """``restore_from_state_records`` from what a consumer of the state topic actually receives: ``fetches`` yields the
        topic's bytes — message-format-v2 record batches, LZ4 or uncompressed, transactional, with the producer's flush
        records, tombstones as null values and the offset gaps log compaction leaves — one ``bytes`` per fetch, or with
        ``n_partitions`` a sequence of that many per fetch (``None`` for a partition without bytes).  Framing is
        ``restore_from_fetches``' (``FramedFetches`` / ``PartitionedFramedFetches``, ``read_committed``); a state-mode
        ``DeviceDecoder`` finds the records and interns the ids on the device (up to four pushes in flight; the oldest is
        finished, then loaded: ``load_states_into``) — no per-record work in Python.  The loaded states become the snapshot
        baseline, then ``events_tail`` is folded on top, exactly as ``restore_from_state_records`` does (``envelope`` and
        ``lenient`` as there).
        ``events_fetches`` (instead of a non-empty ``events_tail``: both raise ``ValueError``) is the tail as BYTES — what a
        consumer of the events topic that seeks to ``events_from`` is sent, fetch by fetch, from the batch that contains each
        first offset on (``events_partitions`` as ``n_partitions``; ``events_from``: one first offset per events partition, or
        one int, the positions committed with the snapshot — ``PartitionedFramedFetches.positions``).  The state decoder then
        CONTINUES as the events decoder (``DeviceDecoder.continue_as_events`` with the model's ``event_json_template``, or
        16-byte fixed events when the values are those): the ids it interned are the resident state's rows, so the tail's
        events find their aggregates, and new ids are numbered behind them.  The tail runs through ``restore_from_fetches``'
        loop with the framers started at ``events_from``: records below a first offset are dropped where records are parsed,
        on the device.  Aggregates that first appear in the tail have the strings ``restore_from_fetches`` gives them (none) —
        unless ``keep_event_strings=True`` (with ``events_fetches`` and a ``template`` that has STR parts; ``ValueError``
        otherwise, and for a model without the hook ``event_string_fields()``, before anything of the store changes): the
        continued decoder is armed with the model's ``event_string_fields()`` as ``restore_from_fetches(keep_strings=True)``
        arms its own, and the tail's events replace and extend the restored columns — aggregates that first appear in the tail,
        and tombstoned ids it creates again, have the tail's strings on both read paths.
        Returns the framer's and the decoder's counters plus the summed decode counts; with ``events_fetches`` the tail's own
        under ``tail_*`` names.  ``host_keys=False``: as in ``restore_from_fetches`` — the decoder (state, or continued as the
        tail's events decoder) stays and serves the reads; a non-empty ``events_tail`` needs the host table and builds it."""
        check_envelope(envelope)
        if events_fetches is not None and len(events_tail):
            raise ValueError("events_tail (decoded events) and events_fetches (the tail's bytes) are two ways to hand over the same tail: give one")
        if events_fetches is None and (events_from is not None or events_partitions):
            raise ValueError("events_from / events_partitions describe events_fetches: there is none")
        if events_fetches is not None and events_partitions:
            events_from = [0] * events_partitions if events_from is None else ([int(events_from)] * events_partitions if np.isscalar(events_from) else list(events_from))
        elif events_fetches is not None and events_from is not None and not np.isscalar(events_from):
            if len(events_from) != 1:
                raise ValueError("one events partition (events_partitions=0) takes one first offset")
            events_from = int(events_from[0])
        template = template or JsonTemplate.counter()
        tail_strings = None
        if keep_event_strings:
            if events_fetches is None or not _str_columns(template):
                raise ValueError("keep_event_strings: the tail's strings go into the columns a template with STR parts restores, from events_fetches")
            tail_strings = _event_strings_of(self.model)
        self._drop_decoder()  # an earlier device-route restore's — behind every refusal of an argument: a call that is refused changes nothing
        self.read_template, self.read_envelope = template, envelope
        eng = self.engine
        self._bind_all_none(0)  # no aggregate yet: the loads grow the state for the ids they meet
        depth = 4
        totals = [0, 0, 0, 0]
        self.state_strings = None
        keep = bool(_str_columns(template))  # the STR fields the values carry are kept beside the rows (a template without them pays nothing)
        with contextlib.ExitStack() as closing:
            d = closing.enter_context(DeviceDecoder(states=True, device=eng.device, keep_strings=keep))

            def push(item):
                parts = _parts_with_records(item)
                if parts:
                    d.push_async(parts)
                return bool(parts)

            def finish_one():  # the oldest push is finished, then loaded, BEFORE the next fetch is asked for
                d.finish()
                for i, c in enumerate(d.load_states_into(eng, template, envelope=envelope, lenient=lenient)):
                    totals[i] += c

            with eng.decoding_onto(self.model.event_algebra().to_c().default_state, lenient=lenient):
                with _pushes_driven(_framer(fetches, n_partitions, framing_threads, depth, True, device_crc, in_place), push, finish_one, depth, lambda: d) as framed:
                    counters = framed.counters()
            counters.update(d.counters())

            def settle():
                if events_fetches is not None:  # fold(prev snapshot, new events): the same decoder reads the events behind the snapshot
                    def as_events_decoder(event_template):
                        d.continue_as_events(event_template)
                        if tail_strings is not None:  # the tail's strings go into the same columns
                            if event_template is None:
                                raise ValueError("keep_event_strings: the tail's values are 16-byte fixed events, which carry no strings")
                            d.keep_event_strings(tail_strings)
                        return d

                    state_counts, below_before = d.counters(), d.below_floor()
                    tail, _, _ = self._fold_fetches(events_fetches, as_events_decoder, d.n_keys, n_partitions=events_partitions, framing_threads=framing_threads,
                                                    device_crc=device_crc, in_place=in_place, start_offsets=events_from)
                    after = d.counters()
                    tail.update({k: after[k] - state_counts[k] for k in after})
                    tail["below_floor"] = d.below_floor() - below_before
                    tail["records_decoded"] -= tail["below_floor"]  # (the framer counts a floored section's whole recordCount: what the device passed over is neither decoded nor delivered)
                    counters.update({"tail_" + k: v for k, v in tail.items()})
                if keep:  # (the decoder's buffers go with it — a decoder that went on as an events decoder still has them: the columns are cloned out)
                    self.state_strings = [None if col is None else (col[0].clone(), col[1].clone()) for col in d.state_strings()]
                self._recovery_ends(d, closing, host_keys, publish=False)

            counters.update(self._resumed(d.n_keys, totals, events_tail, publish=host_keys, settle=settle))
        return counters

    # -- recoveries from records that are already framed: a KafkaConsumer's polls (keys, values, offsets) -------------------------
    def restore_from_consumer_records(self, polls, capacity: int = 0, depth: int = 4, bound_log: bool = False, host_keys: bool = True,
                                      keep_strings: bool = False, algo: int = ALGO_AUTO) -> dict:
        """``restore_from_fetches`` for a consumer that is handed RECORDS, not fetch bytes — what Kafka Streams' restore callback and
        every JVM ``KafkaConsumer`` receive (``SurgeStateStoreConsumer.scala:57-76``, in polls of ``restore-consumer-max-poll-records``).
        ``polls`` yields ``(keys, values, offsets)`` per poll, in offset order per partition: ``keys`` and ``values`` are lists of
        ``bytes`` or ``(data_uint8, off_int64)`` array pairs (``DeviceDecoder.push_records``), ``offsets`` the records' offsets or
        ``None``; transactions are resolved already (a consumer hands over committed records only).  Per poll: stage 1 enqueued
        (``push_records_async``: the arrays are copied inside the call, a generator may reuse them), up to ``depth`` (1 .. 5) polls in
        flight; the oldest is finished without the closing wait and folded onto the resident state without a host wait (or, with
        ``bound_log``, staged for the one fold at the end) — the loop ``restore_from_fetches`` runs behind its framer.  The values
        are 16-byte fixed events, or JSON read through the model's ``event_json_template`` (a model without one is refused by
        name).  ``capacity``, ``bound_log`` / ``algo``, ``host_keys`` and ``keep_strings`` as in ``restore_from_fetches``.  Returns the
        same counters: there is no framer, so ``batches`` counts the polls that carried a record, ``records_decoded`` their
        records, and what a framer alone knows is 0.  Polls of flush records only that come before the first deliverable record —
        before the values have said which decoder the topic gets — are not pushed; they are counted (``records_decoded``,
        ``records_seen``, ``flush_records_skipped``) as if they had been."""
        if not 1 <= depth <= 5:
            raise ValueError("depth must be 1 .. 5 (the decoder has five push slots)")
        strings = _event_strings_of(self.model) if keep_strings else None
        with contextlib.ExitStack() as closing:
            def new_decoder(template):
                if strings is not None and template is None:
                    raise ValueError("keep_strings: the topic's values are 16-byte fixed events, which carry no strings")
                self._drop_decoder()  # (not sooner: until the first record says what the values are nothing of the store has changed)
                return closing.enter_context(DeviceDecoder(template, device=self.engine.device, event_strings=strings))

            counters, n_agg, d, lead = self._fold_polls(polls, new_decoder, -1, capacity=capacity, depth=depth, bound_log=bound_log)
            if d is None:
                self._drop_decoder()
            self.read_template, self.read_envelope = None, "none"
            if bound_log and d is not None:
                n_agg = max(n_agg, capacity, d.n_keys)
                self.engine.pack_staged(n_agg)
                self.engine.fold(algo)
                self.engine.synchronize()
            elif n_agg < 0:  # nothing deliverable in any poll
                self._bind_all_none(capacity)
            if d is not None:
                counters.update(_plus_leading_flush(d.counters(), lead))
            if strings is not None:
                self.state_strings = None if d is None else [None if col is None else (col[0].clone(), col[1].clone()) for col in d.state_strings()]
            self._recovery_ends(d, closing, host_keys)
        self._restored = True
        return counters

    def _fold_polls(self, polls, decoder_for, n_agg: int, *, capacity: int = 0, depth: int = 4, bound_log: bool = False):
        """``_fold_fetches`` without a framer: every poll pushed as records, up to ``depth`` in flight, the oldest finished and
        folded (or staged).  ``decoder_for`` and ``n_agg`` as there.  Returns ``(counters, n_agg, the decoder or None, the flush
        records of the polls that came before a decoder existed and were counted instead of pushed)``."""
        template = self.model.event_json_template()
        d = None
        lead = 0
        counters = dict.fromkeys(COUNTER_NAMES, 0)

        def push(poll):
            nonlocal d, lead
            keys, values, offsets = poll
            n = _poll_records(keys)
            if n == 0:
                return False
            if d is None:
                kind = "json" if _enveloped(template) else _poll_value_kind(keys, values)
                if kind is None:  # flush records only, and no decoder yet to skip them: counted here
                    lead += n
                    counters["records_decoded"] += n
                    return False
                if kind == "json" and template is None:
                    raise _NotDeviceDecodable(f"JSON event values need an event_json_template(): {type(self.model).__name__} has none")
                d = decoder_for(template if kind == "json" else None)
            d.push_records_async(keys, values, offsets)
            counters["batches"] += 1
            counters["records_decoded"] += n
            return True

        def finish_one():
            nonlocal n_agg
            d.finish(wait=False)
            if bound_log:
                _, n_keys = d.stage_into(self.engine)
                n_agg = max(n_agg, n_keys)
                return
            if n_agg < 0:
                n_agg = capacity
                self._bind_all_none(n_agg)
            _, n_keys = d.fold_into(self.engine, wait=False)
            if n_keys > n_agg:
                self.engine.n_agg = n_agg = n_keys  # (grown inside the call)

        with _pushes_finished_on_the_way_out(lambda: d):
            for _ in pushes_in_flight(polls, push, depth):
                finish_one()
        if d is not None:
            self.engine.synchronize()
        return counters, n_agg, d, lead

    def restore_from_state_consumer_records(self, polls, template=None, envelope: str = "none", lenient: bool = False, host_keys: bool = True,
                                            keep_strings: bool = False, events_polls=None, keep_event_strings: bool = False) -> dict:
        """``restore_from_state_topic`` for a consumer that is handed the state topic's RECORDS: ``polls`` yields ``(keys, values,
        offsets)`` as in ``restore_from_consumer_records``, the key being the aggregate id and a ``None`` or empty value its
        tombstone.  A state-mode ``DeviceDecoder`` interns the ids (stage 1 of up to four polls in flight; a finish here includes the
        closing wait, which the load behind it needs); every finished poll is loaded
        (``load_states_into``: ``template``, ``envelope`` and ``lenient`` as in ``restore_from_state_records``), the loaded states
        become the snapshot baseline.  ``events_polls``: the events behind the snapshot, as polls — the decoder then continues as
        the events decoder of the same aggregates and the tail is folded as ``restore_from_consumer_records`` folds a topic (a
        consumer that has sought hands over no record below its position: there are no start offsets here).
        ``keep_strings=True`` (a ``template`` with STR parts; ``ValueError`` otherwise): the string fields the values carry stay
        on the device beside the rows, as ``restore_from_state_topic`` keeps them; ``keep_event_strings=True`` (with
        ``keep_strings`` and ``events_polls``; a model without the hook ``event_string_fields()`` is refused by name): the
        tail's events replace and extend those columns.  Every refusal of an argument comes before anything of the store
        changes — also that of a model without an ``event_json_template`` when ``events_polls`` is a list whose values are JSON.
        Returns the counters of ``restore_from_consumer_records`` for the state polls, the summed decode counts, and the tail's
        under ``tail_*`` names."""
        check_envelope(envelope)
        template = template or JsonTemplate.counter()
        if keep_strings and not _str_columns(template):
            raise ValueError("keep_strings: the template names no STR part whose strings could be kept")
        tail_strings = None
        if keep_event_strings:
            if events_polls is None or not keep_strings:
                raise ValueError("keep_event_strings: the tail's strings go into the columns keep_strings restores, from events_polls")
            tail_strings = _event_strings_of(self.model)
        event_template = self.model.event_json_template()
        if isinstance(events_polls, (list, tuple)) and event_template is None:
            for keys, values, _ in events_polls:
                if _poll_value_kind(keys, values) == "json":
                    raise _NotDeviceDecodable(f"JSON event values need an event_json_template(): {type(self.model).__name__} has none")
        self._drop_decoder()
        self.read_template, self.read_envelope = template, envelope
        eng = self.engine
        self._bind_all_none(0)  # no aggregate yet: the loads grow the state for the ids they meet
        totals = [0, 0, 0, 0]
        self.state_strings = None
        counters = dict.fromkeys(COUNTER_NAMES, 0)
        with contextlib.ExitStack() as closing:
            d = closing.enter_context(DeviceDecoder(states=True, device=eng.device, keep_strings=keep_strings))

            def push(poll):
                keys, values, offsets = poll
                n = _poll_records(keys)
                if n:
                    d.push_records_async(keys, values, offsets)
                    counters["batches"] += 1
                    counters["records_decoded"] += n
                return bool(n)

            def finish_one():  # the oldest poll is finished, then loaded
                d.finish()
                for i, c in enumerate(d.load_states_into(eng, template, envelope=envelope, lenient=lenient)):
                    totals[i] += c

            with eng.decoding_onto(self.model.event_algebra().to_c().default_state, lenient=lenient):
                with _pushes_finished_on_the_way_out(lambda: d):
                    for _ in pushes_in_flight(polls, push, 4):
                        finish_one()
            counters.update(d.counters())

            def settle():
                if events_polls is not None:
                    def as_events_decoder(tmpl):
                        d.continue_as_events(tmpl)
                        if tail_strings is not None:
                            if tmpl is None:
                                raise ValueError("keep_event_strings: the tail's values are 16-byte fixed events, which carry no strings")
                            d.keep_event_strings(tail_strings)
                        return d

                    state_counts = d.counters()
                    tail, _, _, lead = self._fold_polls(events_polls, as_events_decoder, d.n_keys)
                    after = _plus_leading_flush(d.counters(), lead)
                    tail.update({k: after[k] - state_counts[k] for k in after})
                    counters.update({"tail_" + k: v for k, v in tail.items()})
                if keep_strings:  # (the decoder's buffers go with it: the columns are cloned out)
                    self.state_strings = [None if col is None else (col[0].clone(), col[1].clone()) for col in d.state_strings()]
                self._recovery_ends(d, closing, host_keys, publish=False)

            counters.update(self._resumed(d.n_keys, totals, (), publish=host_keys, settle=settle))
        return counters


def _plus_leading_flush(decoder_counters: dict, lead: int) -> dict:
    """A decoder's counters with the ``lead`` flush records ``_fold_polls`` counted instead of pushing them."""
    return {**decoder_counters, "records_seen": decoder_counters["records_seen"] + lead, "flush_records_skipped": decoder_counters["flush_records_skipped"] + lead}


def _poll_records(side) -> int:
    """How many records one side of a poll holds (a list, or ``(data, off)`` arrays)."""
    return int(side[1].shape[0]) - 1 if isinstance(side, tuple) and len(side) == 2 and isinstance(side[1], np.ndarray) else len(side)


def _poll_value_kind(keys, values):
    """``_sniff_value_kind`` for a poll: what its first deliverable record's value looks like — ``"fixed16"``, ``"json"``, or ``None``
    when it holds flush records only (or nothing)."""
    def spans(side):
        if isinstance(side, tuple) and len(side) == 2 and isinstance(side[1], np.ndarray):
            return np.asarray(side[0], dtype=np.uint8).reshape(-1), np.asarray(side[1], dtype=np.int64)
        return None, None

    (kd, ko), (vd, vo) = spans(keys), spans(values)
    n = min(_poll_records(keys), _poll_records(values))
    if ko is not None and vo is not None and n:  # the first record that is not a flush record, without a Python loop
        live = np.flatnonzero((np.diff(ko[: n + 1]) > 0) | (np.diff(vo[: n + 1]) > 0))
        if not live.shape[0]:
            return None
        first = int(live[0])
        value = vd[vo[first]:vo[first + 1]].tobytes()
        return "fixed16" if len(value) == 16 and value[:1] != b"{" else "json"
    for i in range(n):
        key = bytes(kd[ko[i]:ko[i + 1]]) if ko is not None else (keys[i] or b"")
        value = bytes(vd[vo[i]:vo[i + 1]]) if vo is not None else (values[i] or b"")
        if key or value:
            return "fixed16" if len(value) == 16 and value[:1] != b"{" else "json"
    return None


def _framer(fetches, n_partitions: int, framing_threads: int, depth: int, overlap: bool, device_crc: bool, in_place: bool, start_offsets=None):
    """The framer of a recovery that keeps ``depth`` pushes in flight: a group of ``n_partitions`` framers, or one (0).
    device_crc: the batches' CRC-32C is finished on the GPU where their bytes go anyway (SURGE_INGEST_DEVICE_CRC): the framing
    threads touch a batch's header, not its bytes.  in_place: a fetch response is received into the framer's page-locked slab
    and framed where it lies (no copy of the sections)."""
    if n_partitions:
        return PartitionedFramedFetches(fetches, n_partitions, threads=framing_threads, hold=depth, overlap=overlap, device_crc=device_crc, in_place=in_place,
                                        start_offsets=start_offsets)
    return FramedFetches(fetches, overlap=overlap, hold=depth, device_crc=device_crc, start_offset=start_offsets)


def _parts_with_records(item) -> list:
    """A framed fetch's ``(sections, arena)`` parts, one or a list, without those whose sections are empty (a ``Framed`` keeps its floors)."""
    return [part for part in (item if isinstance(item, list) else [item]) if part[0].shape[0]]


@contextlib.contextmanager
def _pushes_driven(framer, push, finish_one, depth: int, decoder_if_any, pipelined: bool = False, beside=None):
    """The loop of every recovery from a topic's bytes, inside ``framer`` (made with ``hold=depth``) and ``beside``, a context that
    lasts as long: ``push(item)`` for every framed fetch, up to ``depth`` in flight — on a worker thread if ``pipelined`` —, and
    ``finish_one()`` for the oldest before the next fetch is asked for; then the block runs, the framer still open (its counters)."""
    with framer as framed, (beside or contextlib.nullcontext()):
        with _pushes_finished_on_the_way_out(decoder_if_any):
            if pipelined:
                # the framer's thread (headers, CRC-32C, transactions of the next fetch), the pipeline's worker (stage 1 of
                # up to `depth` fetches ahead) and this one (interning + fold of the oldest push).  The worker asks for
                # fetch i + depth only after push i is finished: asking tells the framer that fetch i's arena / slab may
                # be framed into again, and a push reads its bytes until then.
                with PushPipeline(framed, push, depth) as pipe:
                    for _ in pipe:
                        finish_one()
                        pipe.done()
            else:  # the same on one thread: the oldest push is finished BEFORE the next fetch is asked for
                for _ in pushes_in_flight(framed, push, depth):
                    finish_one()
        yield framed


@contextlib.contextmanager
def _pushes_finished_on_the_way_out(decoder_if_any):
    """However the block ends, no push is left in flight behind it: pushes that are enqueued read the framer's slabs until
    they are finished (an error path; nothing is pending after a loop that ran to its end).  ``decoder_if_any()``: the
    decoder, or ``None`` while none has been made."""
    try:
        yield
    finally:
        d = decoder_if_any()
        if d is not None:
            while d.pending:
                try:
                    d.finish()
                except Exception:
                    pass


def _event_strings_of(model):
    """The model's ``event_string_fields()`` (an optional hook: read with ``getattr``), or ``ValueError`` for a model without it."""
    hook = getattr(model, "event_string_fields", None)
    if hook is None:
        raise ValueError(f"keep_strings: {type(model).__name__} has no event_string_fields() hook (which event class carries which string)")
    return hook()


class _NotDeviceDecodable(ValueError):
    """The topic's values are not something the device decoder reads (JSON text, and the model has no template)."""


def _enveloped(template) -> bool:
    """The model's event template names an envelope around its JSON text: such a topic always gets the template decoder."""
    return template is not None and getattr(template, "envelope", "none") != "none"


def _varlong(buf, pos: int):  # the zigzag varint at buf[pos] -> (value, the position behind it)
    v, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            break
        shift += 7
    return (v >> 1) ^ -(v & 1), pos


def _sniff_value_kind(sections, arena_address: int):
    """What the first deliverable record's value looks like — a 16-byte fixed event or JSON text: decides which device
    decoder a topic gets (a topic is written by one plugin: its values are all of one kind; a value that is not fails the
    push loudly)."""
    for s in sections:
        if int(s["codec"]) & 0xFF == 3:  # still an LZ4 frame (decoded on the GPU): look into it with the library's host decoder
            frame = ctypes.string_at(arena_address + int(s["byte_off"]), int(s["byte_len"]))
            cap = max(1 << 16, 64 * len(frame))
            out = ctypes.create_string_buffer(cap)
            got = _native.load().surge_lz4_frame_decompress(frame, len(frame), out, cap)
            if got < 0:
                return "json"  # too large to peek into, or damaged: the decoder will say which
            buf = out.raw[: min(got, 4096)]
        else:
            buf = ctypes.string_at(arena_address + int(s["byte_off"]), min(int(s["byte_len"]), 4096))
        pos = 0
        try:
            for _ in range(int(s["n_records"])):
                rlen, pos = _varlong(buf, pos)  # record length
                end = pos + rlen
                pos += 1                        # attributes
                _, pos = _varlong(buf, pos)     # timestampDelta
                _, pos = _varlong(buf, pos)     # offsetDelta
                klen, pos = _varlong(buf, pos)
                pos += max(klen, 0)
                vlen, pos = _varlong(buf, pos)
                if klen == 0 and vlen == 0:     # the producer's flush record: look at the next one
                    pos = end
                    continue
                return "fixed16" if vlen == 16 and buf[pos:pos + 1] != b"{" else "json"
        except IndexError:
            return "json"
    return None
