"""GPU-backed aggregate state store behind the reference's read seams.

* S2 ``getAggregateBytes(aggregateId): Future[Option[Array[Byte]]]`` —
  ``modules/common/src/main/scala/surge/kafka/streams/AggregateStateStoreKafkaStreams.scala:83-85``,
  called once per actor start by ``KTableInitializationSupport.fetchState``
  (``modules/command-engine/core/src/main/scala/surge/internal/persistence/KTableInitializationSupport.scala:63-74``).
* S1 ``SurgeKafkaStreamsPersistencePlugin.createSupplier(storeName)`` —
  ``.../streams/SurgeKafkaStreamsPersistencePlugin.scala:12-15``: the key/value store the KTable
  topology writes state-topic records into (last value per key wins, ``null`` deletes —
  ``SurgeStateStoreConsumer.scala:69``).

The reference rebuilds this store by replaying the compacted *state* topic into RocksDB; here the
same bytes are produced by folding the *events* topic on the GPU (equal by the reference's own
invariant: events and snapshot are published in one transaction).  The serialized
format stays the plugin's: the engine hands a fixed-width state to ``writeState``.

A restore with ``host_keys=False`` keeps the device decoder instead: its key table on the GPU says which row an id is
(``DeviceDecoder.lookup``) and the state encoders write the bytes of the rows asked for (``encode.encode_rows``), so no id
is downloaded and no state mirrored until something needs the host table (``GpuReplayStateStore.keys``).  Reads in key order —
``range_bytes`` / ``all_bytes`` / ``substates_for_aggregate`` / ``num_entries``, and ``GpuReplayKeyValueStore(device_scans=True)``
over them — stay on that route too: the decoder keeps its ids sorted (``DeviceDecoder.range_rows``).
"""
from __future__ import annotations

import bisect
import contextlib
import threading
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .command import ReplayableCommandModel, SurgeCommandBusinessLogic
from .core import write_state_of
from .log import EventLog, KeyTable, pack_events
from .replay import ReplayEngine
from .schema import ALGO_AUTO, STATE_DTYPE, STATE_POISONED, STATE_PRESENT


class AggregateInitializationException(RuntimeError):
    """Mirror of the error an actor gets when its state cannot be initialised
    (``PersistentActor.scala:328-333``); raised for aggregates whose replay hit a throwing event."""


class GpuReplayStateStore:
    """Recover aggregate state by GPU replay and serve it through ``get_aggregate_bytes``."""

    def __init__(self, business_logic: SurgeCommandBusinessLogic, device: int = 0):
        model = business_logic.command_model()
        if not isinstance(model, ReplayableCommandModel):
            raise TypeError("GPU replay needs a ReplayableCommandModel (event algebra + fixed-width codecs)")
        self.business_logic = business_logic
        self.model = model
        self.engine = ReplayEngine(model.event_algebra(), device)
        self._keys = KeyTable()
        #: the device decoder a ``host_keys=False`` restore left alive: its key table on the GPU answers the reads until something
        #: needs the host table (``keys``)
        self._decoder = None
        self._device_lock = threading.RLock()  # the device route serves one reader at a time (decoder and engine scratch)
        self._uploaded_keys = None  # a host-keys store's key table on the device, for ``get_aggregate_bytes_many``: (n_keys, d_utf8, d_off)
        self._sorted_keys = None  # ... and its ids in key order, for ``range_bytes``: (n_keys, ids)
        #: what ``get_aggregate_bytes`` writes on the device route: the ``encode.JsonTemplate`` of the model's serialized state
        #: (``None``: ``JsonTemplate.counter()``) and its envelope; ``restore_from_state_topic`` sets both from its arguments
        self.read_template = None
        self.read_envelope = "none"
        self.store_name = f"{business_logic.aggregate_name}AggregateStateStore"  # SurgeStateStoreConsumer.scala:110
        self._restored = False
        #: the STR columns of the states a resume from the state topic loaded: per string column ``(d_utf8, d_off)`` CUDA
        #: tensors or ``None`` (``None`` altogether: nothing restored) — see ``state_string_columns``
        self.state_strings = None

    def close(self):
        self._drop_decoder()
        self.engine.close()

    # -- the key table: on the device after a ``host_keys=False`` restore, on the host once something needs it there --------
    @property
    def device_route(self) -> bool:
        """``True`` while reads are answered from the device key table (no host dictionary, no host mirror)."""
        return self._decoder is not None

    @property
    def keys(self) -> KeyTable:
        """The host key table.  On a device-route store the first use builds it: the decoder's ids are adopted, the host mirror
        is published exactly as a ``host_keys=True`` restore does, the decoder is dropped — from then on the store is that store."""
        if self._decoder is not None:
            with self._device_lock:
                d = self._decoder
                if d is not None:
                    self._adopt_keys_of(d)
                    self.engine.snapshot()  # publishes the host mirror that serves point reads
                    self._decoder = None
                    d.close()
        return self._keys

    @keys.setter
    def keys(self, table: KeyTable) -> None:
        self._drop_decoder()
        self._keys = table
        self._uploaded_keys = None
        self._sorted_keys = None

    def _drop_decoder(self) -> None:
        with self._device_lock:
            d, self._decoder = self._decoder, None
            if d is not None:
                d.close()

    def _bind_all_none(self, n_agg: int) -> None:
        """The resident state becomes ``n_agg`` aggregates, every one None (an empty log, folded)."""
        from .schema import EVENT_DTYPE

        self.engine.load_csr(np.zeros(n_agg + 1, dtype=np.int64), np.zeros(0, dtype=EVENT_DTYPE))
        self.engine.fold()

    def _loaded_is_baseline(self, n_agg: int) -> None:
        """What was loaded is the snapshot baseline: a publish right after the load has nothing to say."""
        import ctypes

        import torch

        if n_agg:
            eng = self.engine
            d_kind = torch.zeros(n_agg, dtype=torch.uint8, device=torch.device("cuda", eng.device))
            nv, nt = ctypes.c_int64(), ctypes.c_int64()
            eng._check(eng._lib.surge_replay_snapshot_delta(eng._h, ctypes.c_void_p(d_kind.data_ptr()), ctypes.byref(nv), ctypes.byref(nt), 1))

    def _adopt_keys_of(self, decoder) -> None:
        """The host key table is the device decoder's (``None``: no decoder was made, no id was met)."""
        keys = KeyTable()
        for k in (decoder.keys() if decoder is not None else ()):
            keys.intern(k)
        self._keys = keys
        self._uploaded_keys = None
        self._sorted_keys = None

    @contextlib.contextmanager
    def _decoding_onto_the_defaults(self):
        """Inside the block the bytes a decoded state's template does not name are the algebra's defaults
        (``surge_replay_set_decode_base``); zeros again on the way out."""
        import ctypes

        eng = self.engine
        defaults = self.model.event_algebra().to_c().default_state
        eng._check(eng._lib.surge_replay_set_decode_base(eng._h, ctypes.byref(defaults)))
        try:
            yield
        finally:
            eng._check(eng._lib.surge_replay_set_decode_base(eng._h, None))

    # -- recovery ---------------------------------------------------------------------------
    def restore(self, events_in_offset_order: Sequence, prior: Optional[Dict[str, object]] = None,
                capacity: int = 0, algo: int = ALGO_AUTO) -> None:
        """Fold the whole events topic.  ``prior`` (id -> aggregate) is an earlier snapshot to fold onto."""
        if prior:
            for k in prior:
                self.keys.intern(k)
        log = pack_events(self.model, events_in_offset_order, self.keys, capacity)
        init = None
        if prior:
            init = np.zeros(log.n_aggregates, dtype=STATE_DTYPE)
            for k, agg in prior.items():
                init[self.keys.index[k]] = self.model.state_to_fixed(agg)[0]
        self.restore_log(log, init, algo)

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
        from .core import SerializedMessage
        from .ingest import EventsTopicIngest, IngestError
        from .schema import EVENT_DTYPE

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
                             host_keys: bool = True) -> dict:
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
        ``get_aggregate_bytes_many``)."""
        from .ingest import DeviceDecoder

        made = []  # the decoder, made for the first fetch with a record in it
        kept = False

        def new_decoder(template):
            # (an earlier device-route restore's decoder goes here, not sooner: up to this point — the fetches' first record, whose
            # values may turn out not to be device-decodable — nothing of the store has changed, and its reads still answer)
            self._drop_decoder()
            made.append(DeviceDecoder(template, device=self.engine.device))
            return made[0]

        try:
            counters, n_agg = self._fold_fetches(fetches, new_decoder, -1, capacity=capacity, overlap=overlap, n_partitions=n_partitions, framing_threads=framing_threads,
                                                 consumer_threads=consumer_threads, bound_log=bound_log, device_crc=device_crc, in_place=in_place)
            d = made[0] if made else None
            if d is None:
                self._drop_decoder()  # (no record in the whole topic: the earlier restore's decoder has not been replaced yet)
            self.read_template, self.read_envelope = None, "none"  # (an earlier restore_from_state_topic's)
            if bound_log and d is not None:
                n_agg = max(n_agg, capacity, d.n_keys)
                self.engine.pack_staged(n_agg)  # decoded fetches -> ONE bound CSR log
                self.engine.fold(algo)
                self.engine.synchronize()
            elif n_agg < 0:  # nothing deliverable in the whole topic
                self._bind_all_none(capacity)
            if host_keys or d is None:
                self._adopt_keys_of(d)
            else:
                self._adopt_keys_of(None)  # (the host table is built when something asks for it: ``keys``)
            if d is not None:
                counters.update(d.counters())
            kept = not host_keys and d is not None
        finally:
            if made and not kept:
                made[0].close()
        if kept:
            self._decoder = made[0]
        else:
            self.engine.snapshot()  # publishes the host mirror that serves point reads
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
        with the pushes.  Returns ``(the framer's counters, n_agg)``."""
        from .ingest import PushPipeline, pushes_in_flight

        template = self.model.event_json_template()
        d = None
        # pushes in flight (measured on the 10 M-aggregate topic: 2 / 3 / 4 / 5 in flight = 4.1 / 4.3 / 4.65 / 4.7e8 events/s on
        # one box): stage 1 of the next fetches runs while this one is interned and folded
        depth = 4 if overlap else 1

        def push(item):
            """(the pipeline's worker thread) stage 1 of one fetch; the decoder is made for the first fetch with a record in it"""
            nonlocal d
            parts = item if isinstance(item, list) else [item]
            parts = [part for part in parts if part[0].shape[0]]  # (a Framed part keeps its floors)
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
        with framer as framed, (self.engine.on_own_stream() if two_threads else contextlib.nullcontext()):
            with _pushes_finished_on_the_way_out(lambda: d):
                if two_threads:
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
            if d is not None:
                self.engine.synchronize()
            counters = framed.counters()
            if start_offsets is not None:
                counters.update(framed.below_start())
        return counters, n_agg

    def restore_from_state_records(self, records, events_tail: Sequence = (), template=None, envelope: str = "none") -> dict:
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
        36-39``); any other field, order or repetition is refused, not skipped.  Returns the decoder's counts."""
        import torch

        from .encode import STRING_COLUMNS, JsonTemplate, check_envelope, decode_states, key_table_utf8, merge_state_strings

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
            with self._decoding_onto_the_defaults():
                res = decode_states(eng, template, d_values, d_off, to_dev(data), to_dev(key_off), d_agg,
                                    out=eng.device_state(), want_spans=bool(str_columns), raise_on_refused=True, envelope=envelope)
            counts = res[2]
            if str_columns:  # the STR fields the values carry, kept beside the rows
                self.state_strings = [merge_state_strings(eng, c, d_values, d_off, d_agg, res[1], res.spans, n_agg=n_agg) if c in str_columns else None
                                      for c in range(STRING_COLUMNS)]
        if str_columns and self.state_strings is None:
            self.state_strings = [merge_state_strings(eng, c, n_agg=n_agg) if c in str_columns else None for c in range(STRING_COLUMNS)]
        self._loaded_is_baseline(n_agg)
        self._restored = True
        if len(events_tail):
            self.apply_events(events_tail)  # grows for new ids, group-by + fold on the device, refreshes the mirror
        else:
            eng.snapshot()
        return {"rows_written": counts[0], "tombstones": counts[1], "refused": counts[2], "reparsed_on_host": counts[3]}

    def restore_from_state_topic(self, fetches, n_partitions: int = 0, template=None, events_tail: Sequence = (), framing_threads: int = 4,
                                 device_crc: bool = True, in_place: bool = True, envelope: str = "none", events_fetches=None, events_from=None,
                                 events_partitions: int = 0, host_keys: bool = True) -> dict:
        """``restore_from_state_records`` from what a consumer of the state topic actually receives: ``fetches`` yields the
        topic's bytes — message-format-v2 record batches, LZ4 or uncompressed, transactional, with the producer's flush
        records, tombstones as null values and the offset gaps log compaction leaves — one ``bytes`` per fetch, or with
        ``n_partitions`` a sequence of that many per fetch (``None`` for a partition without bytes).  Framing is
        ``restore_from_fetches``' (``FramedFetches`` / ``PartitionedFramedFetches``, ``read_committed``); a state-mode
        ``DeviceDecoder`` finds the records and interns the ids on the device (up to four pushes in flight; the oldest is
        finished, then loaded: ``load_states_into``) — no per-record work in Python.  The loaded states become the snapshot
        baseline, then ``events_tail`` is folded on top, exactly as ``restore_from_state_records`` does (``envelope`` as there).
        ``events_fetches`` (instead of a non-empty ``events_tail``: both raise ``ValueError``) is the tail as BYTES — what a
        consumer of the events topic that seeks to ``events_from`` is sent, fetch by fetch, from the batch that contains each
        first offset on (``events_partitions`` as ``n_partitions``; ``events_from``: one first offset per events partition, or
        one int, the positions committed with the snapshot — ``PartitionedFramedFetches.positions``).  The state decoder then
        CONTINUES as the events decoder (``DeviceDecoder.continue_as_events`` with the model's ``event_json_template``, or
        16-byte fixed events when the values are those): the ids it interned are the resident state's rows, so the tail's
        events find their aggregates, and new ids are numbered behind them.  The tail runs through ``restore_from_fetches``'
        loop with the framers started at ``events_from``: records below a first offset are dropped where records are parsed,
        on the device.  Aggregates that first appear in the tail have the strings ``restore_from_fetches`` gives them (none).
        Returns the framer's and the decoder's counters plus the summed decode counts; with ``events_fetches`` the tail's own
        under ``tail_*`` names.  ``host_keys=False``: as in ``restore_from_fetches`` — the decoder (state, or continued as the
        tail's events decoder) stays and serves the reads; a non-empty ``events_tail`` needs the host table and builds it."""
        from .encode import JsonTemplate, check_envelope
        from .ingest import DeviceDecoder, pushes_in_flight

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
        self._drop_decoder()  # an earlier device-route restore's — behind every refusal of an argument: a call that is refused changes nothing
        self.read_template, self.read_envelope = template, envelope
        eng = self.engine
        self._bind_all_none(0)  # no aggregate yet: the loads grow the state for the ids they meet
        depth = 4
        totals = [0, 0, 0, 0]
        self.state_strings = None
        keep = bool(_str_columns(template))  # the STR fields the values carry are kept beside the rows (a template without them pays nothing)
        with contextlib.ExitStack() as closing, self._decoding_onto_the_defaults():
            d = closing.enter_context(DeviceDecoder(states=True, device=eng.device, keep_strings=keep))

            def push(item):
                parts = [(sec, arena) for sec, arena in (item if isinstance(item, list) else [item]) if sec.shape[0]]
                if parts:
                    d.push_async(parts)
                return bool(parts)

            def finish_one():
                d.finish()
                for i, c in enumerate(d.load_states_into(eng, template, envelope=envelope)):
                    totals[i] += c

            with _framer(fetches, n_partitions, framing_threads, depth, True, device_crc, in_place) as framed:
                with _pushes_finished_on_the_way_out(lambda: d):
                    for _ in pushes_in_flight(framed, push, depth):  # the oldest push is finished, then loaded, BEFORE the next fetch is asked for
                        finish_one()
                counters = framed.counters()
            counters.update(d.counters())
            n_agg = d.n_keys
            self._loaded_is_baseline(n_agg)
            if events_fetches is not None:  # fold(prev snapshot, new events): the same decoder reads the events behind the snapshot
                def as_events_decoder(event_template):
                    d.continue_as_events(event_template)
                    return d

                state_counts, below_before = d.counters(), d.below_floor()
                tail, _ = self._fold_fetches(events_fetches, as_events_decoder, n_agg, n_partitions=events_partitions, framing_threads=framing_threads,
                                             device_crc=device_crc, in_place=in_place, start_offsets=events_from)
                after = d.counters()
                tail.update({k: after[k] - state_counts[k] for k in after})
                tail["below_floor"] = d.below_floor() - below_before
                tail["records_decoded"] -= tail["below_floor"]  # (the framer counts a floored section's whole recordCount: what the device passed over is neither decoded nor delivered)
                counters.update({"tail_" + k: v for k, v in tail.items()})
            if keep:  # (the decoder's buffers go with it — a decoder that went on as an events decoder still has them: the columns are cloned out)
                self.state_strings = [None if col is None else (col[0].clone(), col[1].clone()) for col in d.state_strings()]
            if host_keys:
                self._adopt_keys_of(d)
            else:  # the decoder outlives the block: its key table answers the reads
                self._adopt_keys_of(None)
                closing.pop_all()
                self._decoder = d
        self._restored = True
        if len(events_tail):
            self.apply_events(events_tail)
        elif host_keys:
            eng.snapshot()
        counters.update({"rows_written": totals[0], "tombstones": totals[1], "refused": totals[2], "reparsed_on_host": totals[3]})
        return counters

    def state_string_columns(self):
        """The restored STR columns, extended (``merge_state_strings`` without records: aggregates that appeared after the
        resume get empty strings — theirs stay the host's) to the engine's current aggregate count: what
        ``encode.encode_states(strings=...)`` takes.  ``()`` when nothing was restored."""
        from .encode import merge_state_strings

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

    def restore_log(self, log: EventLog, init_state: Optional[np.ndarray] = None, algo: int = ALGO_AUTO) -> None:
        self.keys = log.keys
        self.engine.load_csr(log.seg_off, log.events, init_state)
        self.engine.fold(algo)
        self.engine.snapshot()  # publishes the host mirror that serves point reads
        self._restored = True

    def apply_events(self, events_in_offset_order: Sequence) -> None:
        """Streaming micro-batch (config C5): fold new events onto the resident state."""
        if not self._restored:
            raise RuntimeError("restore() first")
        enc = self.model.encode_events(events_in_offset_order)  # may raise: nothing has been interned yet
        ids = [self.model.aggregate_id_of(e) for e in events_in_offset_order]
        # aggregates that first appear after recovery are the normal Surge case: the resident state grows
        # (surge_replay_grow) BEFORE any id is interned, so a failure leaves the key table consistent
        fresh = len({k for k in ids if self.keys.get(k) is None})
        if len(self.keys) + fresh > self.engine.n_agg:
            self.engine.grow(len(self.keys) + fresh)
        agg_idx = np.fromiter((self.keys.intern(k) for k in ids), dtype=np.int64, count=len(ids))
        self.engine.append_events(agg_idx, enc)  # stable group-by + K3 inside the library
        self.engine.snapshot()

    # -- S2 ---------------------------------------------------------------------------------
    def get_aggregate_bytes(self, aggregate_id: str) -> Optional[bytes]:
        """``None`` = no such aggregate (KTable miss) or tombstone; else ``writeState(state).value``.  On the device route
        (``host_keys=False``) the bytes are ``get_aggregate_bytes_many([aggregate_id])``' — ``read_template`` / ``read_envelope``
        composed on the GPU; one launch chain and two copies per call, so batches are what that route is for."""
        if self._decoder is not None:
            with self._device_lock:
                if self._decoder is not None:
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
        stores.  The restored columns hold EMPTY strings for aggregates that first appeared after the resume (``apply_events``, an
        events tail): their strings are the host model's alone, so for such an aggregate a STR part is written ``""`` here while
        ``get_aggregate_bytes`` — the plugin's formatter over ``restore_static_strings`` — writes the real string.  Every other
        part, and every aggregate the state topic carried, reads the same on both."""
        import torch

        from .encode import READ_POISONED, READ_VALUE, JsonTemplate, check_envelope, encode_rows, key_table_utf8

        check_envelope(envelope)
        template = template or JsonTemplate.counter()
        ids = list(aggregate_ids)
        if not ids:
            return []
        eng = self.engine
        dev = torch.device("cuda", eng.device)
        with self._device_lock:
            strings = self.state_string_columns()
            for c in _str_columns(template):
                if c >= len(strings) or strings[c] is None:
                    raise ValueError(f"the template names string column {c}, and nothing restored it")
            d = self._decoder
            if d is not None:
                enc = [k.encode("utf-8") for k in ids]
                off = np.zeros(len(enc) + 1, dtype=np.int64)
                np.cumsum([len(e) for e in enc], out=off[1:])
                data = np.zeros(int(off[-1]) + 16, dtype=np.uint8)  # (the slack behind the last id the lookup's loads may touch)
                data[: int(off[-1])] = np.frombuffer(b"".join(enc), dtype=np.uint8)
                d_rows = d.lookup_device(torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev))
                if eng.stream_ptr:  # (the rows are complete in the order of torch's current stream; an engine on a stream of its own is not in it)
                    torch.cuda.current_stream(dev).synchronize()
                d_utf8, d_key_off = d.device_key_table()
            else:
                keys = self._keys
                n_agg = eng.n_agg
                rows = np.fromiter((-1 if i is None or i >= n_agg else i for i in map(keys.get, ids)), dtype=np.int64, count=len(ids))
                if self._uploaded_keys is None or self._uploaded_keys[0] != len(keys):
                    kd, ko = key_table_utf8(keys.keys)
                    self._uploaded_keys = (len(keys), torch.from_numpy(kd).to(dev), torch.from_numpy(ko).to(dev))
                _, d_utf8, d_key_off = self._uploaded_keys
                d_rows = torch.from_numpy(rows).to(dev)
            out, out_off, kind = encode_rows(eng, template, d_utf8, d_key_off, d_rows, envelope=envelope, strings=strings)
            raw, off, kind = out.cpu().numpy().tobytes(), out_off.cpu().numpy().tolist(), kind.cpu().numpy()
        bad = np.flatnonzero(kind == READ_POISONED)
        if bad.shape[0]:
            raise AggregateInitializationException(
                f"replay of aggregate {ids[int(bad[0])]!r} hit an event whose handler throws; state is frozen before it"
            )
        value = (kind == READ_VALUE).tolist()
        return [raw[off[q]:off[q + 1]] if value[q] else None for q in range(len(ids))]

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

        from .encode import READ_POISONED, READ_VALUE, JsonTemplate, check_envelope, encode_rows, key_table_utf8

        envelope = self.read_envelope if envelope is None else envelope
        check_envelope(envelope)
        template = template or self.read_template or JsonTemplate.counter()
        page_rows = max(1, int(page_rows))
        eng = self.engine
        dev = torch.device("cuda", eng.device)
        with self._device_lock:
            strings = self.state_string_columns()
            for c in _str_columns(template):
                if c >= len(strings) or strings[c] is None:
                    raise ValueError(f"the template names string column {c}, and nothing restored it")
            d = self._decoder
            if d is not None:
                d_rows = d.range_rows(from_key, to_key)
                host_ids = None
            else:
                order = self._sorted_host_keys()
                lo = 0 if from_key is None else bisect.bisect_left(order, from_key)
                hi = len(order) if to_key is None else bisect.bisect_right(order, to_key)
                index, n_agg = self._keys.index, eng.n_agg
                host_ids = [k for k in order[lo:hi] if index[k] < n_agg]
                d_rows = torch.from_numpy(np.fromiter((index[k] for k in host_ids), dtype=np.int64, count=len(host_ids))).to(dev)
        for first in range(0, int(d_rows.numel()), page_rows):
            with self._device_lock:
                if self._decoder is not d:
                    raise RuntimeError("the store's key table moved while a range was being read: start the range again")
                page = d_rows[first:first + page_rows]
                if d is not None:
                    d_utf8, d_key_off = d.device_key_table()
                else:
                    if self._uploaded_keys is None or self._uploaded_keys[0] != len(self._keys):
                        kd, ko = key_table_utf8(self._keys.keys)
                        self._uploaded_keys = (len(self._keys), torch.from_numpy(kd).to(dev), torch.from_numpy(ko).to(dev))
                    _, d_utf8, d_key_off = self._uploaded_keys
                out, out_off, d_kind = encode_rows(eng, template, d_utf8, d_key_off, page, envelope=envelope, strings=strings)
                kind = d_kind.cpu().numpy()
                bad = np.flatnonzero(kind == READ_POISONED)
                if bad.shape[0]:
                    q = int(bad[0])
                    name = host_ids[first + q] if d is None else d.gather_keys(page[q:q + 1])[0].decode("utf-8")
                    raise AggregateInitializationException(f"replay of aggregate {name!r} hit an event whose handler throws; state is frozen before it")
                kept = np.flatnonzero(kind == READ_VALUE)
                if d is None:
                    ids = [host_ids[first + int(q)] for q in kept]
                else:
                    ids = [k.decode("utf-8") for k in d.gather_keys(page[torch.from_numpy(kept).to(dev)])] if kept.shape[0] else []
                raw, off = out.cpu().numpy().tobytes(), out_off.cpu().numpy().tolist()
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

    def _row_of(self, aggregate_id: str):
        """The id's row, or ``None``: from the device key table while the store is on the device route."""
        d = self._decoder
        if d is not None:
            idx = int(d.lookup([aggregate_id])[0])
            return None if idx < 0 else idx
        return self._keys.get(aggregate_id)

    def get_aggregate(self, aggregate_id: str):
        if self._decoder is not None:
            with self._device_lock:
                if self._decoder is not None:
                    return self._get_aggregate(aggregate_id, device=True)
        return self._get_aggregate(aggregate_id, device=False)

    def _get_aggregate(self, aggregate_id: str, device: bool):
        idx = self._row_of(aggregate_id) if device else self._keys.get(aggregate_id)
        if idx is None or idx >= self.engine.n_agg:
            return None
        raw = self.engine.gather([idx])[0] if device else self.engine.get_raw(idx)  # (no mirror on the device route: surge_replay_gather)
        if int(raw["flags"]) & STATE_POISONED:
            raise AggregateInitializationException(
                f"replay of aggregate {aggregate_id!r} hit an event whose handler throws; state is frozen before it"
            )
        if not int(raw["flags"]) & STATE_PRESENT:
            return None
        hook = getattr(self.model, "restore_static_strings", None)
        if self.state_strings and hook is not None:  # string fields the state topic carried (the model keeps what it already knows)
            strings = self._restored_strings(idx)
            if any(x is not None for x in strings):
                hook(aggregate_id, strings)
        return self.model.state_from_fixed(aggregate_id, raw)


def _str_columns(template) -> set:
    """The string columns a ``JsonTemplate``'s ``(JP_STR, column)`` parts name."""
    from .encode import JP_STR

    return {int(p[1]) for p in template.parts if isinstance(p, tuple) and int(p[0]) == JP_STR}


class GpuReplayKeyValueStore:
    """The store a ``GpuReplayPersistencePlugin.create_supplier`` hands to the KTable topology.

    Reads fall through to the GPU-recovered snapshot; ``put`` overlays later state-topic records
    (last write wins, ``None`` is a tombstone).  Read API and semantics follow
    ``KafkaStreamsKeyValueStore`` (``.../streams/KafkaStreamsKeyValueStore.scala:24-54``,
    pinned by ``KafkaStreamsKeyValueStoreSpec.scala:37-91``).
    """

    _TOMBSTONE = object()

    def __init__(self, name: str, recovered: Optional[GpuReplayStateStore] = None, device_scans: bool = False):
        self.name = name
        self.recovered = recovered
        #: ``True``: while ``recovered`` is on the device route, ``all`` / ``range`` / ``all_values`` / ``approximate_num_entries``
        #: read it through ``range_bytes`` / ``num_entries`` and leave it there; ``False``: they build its host table, as ever
        self.device_scans = bool(device_scans)
        self._overlay: Dict[str, object] = {}

    def put(self, key: str, value: Optional[bytes]) -> None:
        self._overlay[key] = self._TOMBSTONE if value is None else bytes(value)

    def delete(self, key: str) -> None:
        self.put(key, None)

    def get(self, key: str) -> Optional[bytes]:
        if key in self._overlay:
            v = self._overlay[key]
            return None if v is self._TOMBSTONE else v
        if self.recovered is not None:
            return self.recovered.get_aggregate_bytes(key)
        return None

    def _all_keys(self) -> List[str]:
        ks = set(self._overlay)
        if self.recovered is not None:
            ks.update(self.recovered.keys.keys)
        return sorted(ks)

    def _scans_on_the_device(self) -> bool:
        return self.device_scans and self.recovered is not None and self.recovered.device_route

    def _merged(self, from_key: Optional[str], to_key: Optional[str]) -> Iterator[Tuple[str, bytes]]:
        """The overlay's keys inside the bounds, sorted, merged with ``recovered.range_bytes`` on the keys' UTF-8 bytes: the
        overlay wins, a tombstone drops the key."""
        lo = None if from_key is None else from_key.encode("utf-8")
        hi = None if to_key is None else to_key.encode("utf-8")
        over = sorted((kb, k, v) for kb, k, v in ((k.encode("utf-8"), k, v) for k, v in self._overlay.items())
                      if (lo is None or lo <= kb) and (hi is None or kb <= hi))
        at = 0
        for k, v in self.recovered.range_bytes(from_key, to_key):
            kb = k.encode("utf-8")
            while at < len(over) and over[at][0] < kb:
                if over[at][2] is not self._TOMBSTONE:
                    yield over[at][1], over[at][2]
                at += 1
            if at < len(over) and over[at][0] == kb:
                continue  # (the overlay's entry for this key comes in the next round, or behind the loop)
            yield k, v
        for _, k, v in over[at:]:
            if v is not self._TOMBSTONE:
                yield k, v

    def all(self) -> Iterator[Tuple[str, bytes]]:
        if self._scans_on_the_device():
            yield from self._merged(None, None)
            return
        for k in self._all_keys():
            v = self.get(k)
            if v is not None:
                yield k, v

    def all_values(self) -> List[bytes]:
        return [v for _, v in self.all()]

    def range(self, from_key: str, to_key: str) -> Iterator[Tuple[str, bytes]]:
        if self._scans_on_the_device():
            yield from self._merged(from_key, to_key)
            return
        ks = self._all_keys()
        for k in ks[bisect.bisect_left(ks, from_key): bisect.bisect_right(ks, to_key)]:
            v = self.get(k)
            if v is not None:
                yield k, v

    def approximate_num_entries(self) -> int:
        if self._scans_on_the_device():
            # what the device counts (``num_entries``: no text composed), corrected by the overlay's keys: one more for a value
            # over nothing, one fewer for a tombstone over a value
            rec = self.recovered
            keys = list(self._overlay)
            try:
                there = [v is not None for v in rec.get_aggregate_bytes_many(keys, rec.read_template, rec.read_envelope)]
            except AggregateInitializationException:  # (a poisoned aggregate under the overlay: it is not counted, ask one by one)
                there = []
                for k in keys:
                    try:
                        there.append(rec.get_aggregate_bytes(k) is not None)
                    except AggregateInitializationException:
                        there.append(False)
            return rec.num_entries() + sum((self._overlay[k] is not self._TOMBSTONE) - t for k, t in zip(keys, there))
        return sum(1 for _ in self.all())


class GpuReplayPersistencePlugin:
    """``SurgeKafkaStreamsPersistencePlugin`` (…PersistencePlugin.scala:12-15) for the GPU store.

    ``enable_logging`` is False: the store is rebuilt from the events topic, so it needs no
    changelog (the reference then builds the topology un-optimised, SurgeStateStoreConsumer.scala:63-75).
    """

    enable_logging = False

    def __init__(self, recovered: Optional[GpuReplayStateStore] = None):
        self.recovered = recovered

    def create_supplier(self, store_name: str) -> GpuReplayKeyValueStore:
        return GpuReplayKeyValueStore(store_name, self.recovered)


def _framer(fetches, n_partitions: int, framing_threads: int, depth: int, overlap: bool, device_crc: bool, in_place: bool, start_offsets=None):
    """The framer of a recovery that keeps ``depth`` pushes in flight: a group of ``n_partitions`` framers, or one (0).
    device_crc: the batches' CRC-32C is finished on the GPU where their bytes go anyway (SURGE_INGEST_DEVICE_CRC): the framing
    threads touch a batch's header, not its bytes.  in_place: a fetch response is received into the framer's page-locked slab
    and framed where it lies (no copy of the sections)."""
    from .ingest import FramedFetches, PartitionedFramedFetches

    if n_partitions:
        return PartitionedFramedFetches(fetches, n_partitions, threads=framing_threads, hold=depth, overlap=overlap, device_crc=device_crc, in_place=in_place,
                                        start_offsets=start_offsets)
    return FramedFetches(fetches, overlap=overlap, hold=depth, device_crc=device_crc, start_offset=start_offsets)


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


class _NotDeviceDecodable(ValueError):
    """The topic's values are not something the device decoder reads (JSON text, and the model has no template)."""


def _enveloped(template) -> bool:
    """The model's event template names an envelope around its JSON text: such a topic always gets the template decoder."""
    return template is not None and getattr(template, "envelope", "none") != "none"


def _sniff_value_kind(sections, arena_address: int):
    """What the first deliverable record's value looks like — a 16-byte fixed event or JSON text: decides which device
    decoder a topic gets (a topic is written by one plugin: its values are all of one kind; a value that is not fails the
    push loudly)."""
    import ctypes

    def varlong(buf, pos):
        v, shift = 0, 0
        while True:
            b = buf[pos]
            pos += 1
            v |= (b & 0x7F) << shift
            if not b & 0x80:
                break
            shift += 7
        return (v >> 1) ^ -(v & 1), pos

    from . import _native

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
                rlen, pos = varlong(buf, pos)  # record length
                end = pos + rlen
                pos += 1                       # attributes
                _, pos = varlong(buf, pos)     # timestampDelta
                _, pos = varlong(buf, pos)     # offsetDelta
                klen, pos = varlong(buf, pos)
                pos += max(klen, 0)
                vlen, pos = varlong(buf, pos)
                if klen == 0 and vlen == 0:    # the producer's flush record: look at the next one
                    pos = end
                    continue
                return "fixed16" if vlen == 16 and buf[pos:pos + 1] != b"{" else "json"
        except IndexError:
            return "json"
    return None
