"""Seam S1 (see ``store.py``): the key/value store the KTable topology writes into and the plugin that supplies it, both over
``GpuReplayStateStore``'s public methods only."""
from __future__ import annotations

import bisect
from typing import TYPE_CHECKING, Dict, Iterator, List, Optional, Tuple

from .store_reads import AggregateInitializationException

if TYPE_CHECKING:  # (the annotations only: store.py imports this module)
    from .store import GpuReplayStateStore


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
