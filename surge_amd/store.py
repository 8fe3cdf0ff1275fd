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

import threading
from typing import Dict, Optional, Sequence

import numpy as np

from .command import ReplayableCommandModel, SurgeCommandBusinessLogic
from .log import EventLog, KeyTable, pack_events
from .replay import ReplayEngine
from .schema import ALGO_AUTO, STATE_DTYPE
from .store_kv import GpuReplayKeyValueStore, GpuReplayPersistencePlugin  # noqa: F401  (this module stays the import point)
from .store_reads import AggregateInitializationException, StoreReads, _str_columns  # noqa: F401
from .store_recovery import TopicRecoveries, _enveloped, _framer, _NotDeviceDecodable, _pushes_finished_on_the_way_out, _sniff_value_kind  # noqa: F401


class GpuReplayStateStore(TopicRecoveries, StoreReads):
    """Recover aggregate state by GPU replay and serve it through ``get_aggregate_bytes``.

    The class is composed of this module (what the store holds, its key table and the host-table recoveries),
    ``store_recovery.TopicRecoveries`` (the recoveries that start from a topic) and ``store_reads.StoreReads`` (the reads).
    The two bases touch these members and no others: ``engine``, ``model``, ``business_logic``, ``_keys``, ``_decoder``,
    ``_device_lock``, ``_restored``, ``state_strings``, ``read_template``, ``read_envelope`` — beside the methods here
    (``keys``, ``_drop_decoder``, ``_adopt_keys_of``, ``apply_events``) and the reads' two caches, which the key table's
    setters reset (``_uploaded_keys``, ``_sorted_keys``)."""

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

    def _adopt_keys_of(self, decoder) -> None:
        """The host key table is the device decoder's (``None``: no decoder was made, no id was met)."""
        keys = KeyTable()
        for k in (decoder.keys() if decoder is not None else ()):
            keys.intern(k)
        self._keys = keys
        self._uploaded_keys = None
        self._sorted_keys = None

    def snapshot_publisher(self, n_partitions: int, **kw):
        """The ``snapshot.BulkSnapshotPublisher`` of this store's state topic (``kw``: its keyword arguments).  On the host route
        that is what callers write themselves — ``BulkSnapshotPublisher(store.engine, store.keys.keys, n_partitions, **kw)``.  On
        the device route the publisher follows the decoder's key table instead (``snapshot.StoreSnapshotPublisher``): the ids are
        partitioned from their UTF-8 bytes on the GPU, none is downloaded, and the store STAYS on the device route however
        often it publishes; ``template`` / ``envelope`` / ``strings`` default to ``read_template`` / ``read_envelope`` /
        ``state_string_columns()``.  Such a publisher belongs to the recovery it was made after: once the store has left the
        route or been restored again, its ``publish`` raises ``RuntimeError`` — ask for a new one."""
        from .snapshot import BulkSnapshotPublisher, StoreSnapshotPublisher

        with self._device_lock:
            if self._decoder is not None:
                return StoreSnapshotPublisher(self, n_partitions, **kw)
        return BulkSnapshotPublisher(self.engine, self.keys.keys, n_partitions, **kw)

    # -- recovery through the host key table ---------------------------------------------------------------
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
