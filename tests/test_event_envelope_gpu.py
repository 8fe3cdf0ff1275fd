"""Enveloped event values on the device: protobuf ``Event{aggregateId, payload}`` record values through ``DeviceDecoder`` with
``EventJsonTemplate(envelope="protobuf_event")`` — ``records_kernel<true>`` (``push_records``) and the
``section_kernel<.., false, true>`` instantiations (the wire path) — and through ``GpuReplayStateStore``.

Everything the device delivers is held, bit for bit, to the host decoder of the same bytes (``drain_json`` /
``EventJsonTemplate.decode_keyed``, pinned on the protobuf runtime by tests/test_event_envelope.py); there is no tolerance.
Shapes are the smallest at which the record stage takes each of its paths: a section in each LDS class and one read from
global memory, each workgroup width, a batch chained in two rounds, every alignment of a section and of a value in it."""
import numpy as np
import pytest

import event_envelope_cases as cases
import kafka_wire as kw
from surge_amd import schema as S
from surge_amd.ingest import ARG_I32, SECTION_DTYPE, DeviceDecoder, EventJsonTemplate, EventsTopicIngest, IngestError

pytestmark = pytest.mark.gpu

PE = cases.PE
SDK = cases.SDK


def host_drain(wire, template):
    with EventsTopicIngest() as g:
        g.feed(wire)
        agg, ev, off = g.drain_json(template)
        return agg, ev, off, g.key_table().keys


def device_result(d):
    agg, ev, off, n_keys = d.result()
    keys = d.keys()
    assert n_keys == len(keys)
    return agg.cpu().numpy(), ev.cpu().numpy().view(S.EVENT_DTYPE).reshape(-1), off.cpu().numpy(), keys


def same(host, dev):
    assert dev[3] == host[3]
    for h, g in zip(host[:3], dev[:3]):
        assert h.shape == g.shape and h.tobytes() == g.tobytes()


def wire_and_compare(wire, template, device_lz4=True, sizes=None):
    """The wire bytes through the host drain and through host framing + one device push; ``sizes``: the sections' byte lengths
    are appended to it."""
    host = host_drain(wire, template)
    with EventsTopicIngest(frames=True, device_lz4=device_lz4) as g, DeviceDecoder(template) as d:
        g.feed(wire)
        sections, arena = g.drain_sections()
        if sizes is not None:
            sizes += [int(s["byte_len"]) for s in sections]
        d.push(sections, arena)
        dev = device_result(d)
        counters = d.counters()
    same(host, dev)
    assert counters["records_delivered"] == host[0].shape[0]
    return host, counters


def expected_of(group):
    """(agg_idx, events bytes, keys) of accepted cases delivered in this order, from the references alone."""
    keys, agg = [], []
    for c in group:
        aid = c.aggregate_id.decode("utf-8")
        if aid not in keys:
            keys.append(aid)
        agg.append(keys.index(aid))
    return np.asarray(agg, dtype=np.int64), b"".join(cases.expected_event(c) for c in group), keys


def template_groups():
    out = [(SDK, cases.accepted_cases())]
    other = cases.other_template_cases()
    out.append((cases.V, other[:2]))
    out.append((cases.COUNTER, other[2:]))
    out.append((cases.F64, cases.decided_double_cases()))
    return out


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
def test_the_accepted_corpus_in_one_push_records():
    for template, group in template_groups():
        agg, events, keys = expected_of(group)
        with DeviceDecoder(template) as d:
            d.push_records([c.key for c in group], [c.value for c in group], [100 + 3 * i for i in range(len(group))])
            dev = device_result(d)
            assert d.counters()["doubles_parsed_on_host"] == 0
        assert dev[3] == keys and dev[0].tobytes() == agg.tobytes() and dev[1].tobytes() == events
        assert list(dev[2]) == [100 + 3 * i for i in range(len(group))]
        # ... and each value is what the host makes of it with the record's id
        assert events == b"".join(template.decode_keyed(c.aggregate_id, c.value).tobytes() for c in group)


def test_the_accepted_corpus_through_the_wire_path_uncompressed_and_lz4():
    for template, group in template_groups():
        agg, events, keys = expected_of(group)
        for compression in ("none", "lz4"):
            recs = [(c.key, c.value) for c in group]
            wire = b"".join(kw.record_batch(7 + s // 9 * 10, recs[s:s + 9] + [(b"", b"")], compression=compression) for s in range(0, len(recs), 9))
            host, counters = wire_and_compare(wire, template)
            assert host[1].tobytes() == events and host[3] == keys and host[0].tobytes() == agg.tobytes()
            assert counters["doubles_parsed_on_host"] == 0 and counters["flush_records_skipped"] == (len(recs) + 8) // 9


def test_the_bare_template_and_the_fixed16_decoder_refuse_the_same_bytes():
    """A zeroed envelope field behaves as before: the envelope is the template's to name."""
    c = cases.other_template_cases()[0]
    assert len(c.value) == 16
    for template in (cases.V_BARE, None):
        with DeviceDecoder(template) as d:
            if template is None:  # sixteen bytes are a fixed event to the decoder that is told so: whatever they hold
                d.push_records([c.key], [c.value], [0])
                assert device_result(d)[1].tobytes() == c.value
            else:
                with pytest.raises(IngestError) as ei:
                    d.push_records([c.key], [c.value], [0])
                assert ei.value.status == -7 and cases.DEVICE_REASON["json"] in str(ei.value)


# ---- section_kernel, branch by branch -----------------------------------------------------------------------------------------
def padded_topic(n_records, value_bytes, n_ids=37, base=1000):
    """One uncompressed batch of ``n_records`` enveloped deposits, each value padded to about ``value_bytes``."""
    recs = []
    for i in range(n_records):
        aid = b"agg-%d" % (i % n_ids)
        recs.append((aid + b":%d" % i, cases.wrap(aid, cases.amount_payload(i * 7919 - 2**30, max(value_bytes, 40) + i % 5))))
    return kw.record_batch(base, recs)


@pytest.mark.parametrize("n_records,value_bytes,lo,hi", [(50, 100, 1, 8320), (100, 100, 8321, 16640), (150, 250, 16641, 65536), (200, 400, 65537, 1 << 20)],
                         ids=["lds 8 KiB, 64 lanes", "lds 16 KiB, 128 lanes", "lds 64 KiB, 192 lanes", "global memory, 256 lanes"])
def test_a_section_in_each_lds_class_and_beyond_at_each_workgroup_width(n_records, value_bytes, lo, hi):
    sizes = []
    wire_and_compare(padded_topic(n_records, value_bytes), SDK, sizes=sizes)
    assert len(sizes) == 1 and lo <= sizes[0] <= hi, sizes


@pytest.mark.parametrize("n_records", [64, 65, 128, 129, 192, 193, 256, 257])
def test_record_counts_on_both_sides_of_each_workgroup_width_and_of_a_second_chaining_round(n_records):
    sizes = []
    wire_and_compare(padded_topic(n_records, 40), SDK, sizes=sizes)
    assert sizes[0] <= 65536  # staged: 257 records are chained in two rounds out of LDS


def test_257_records_read_from_global_memory_and_several_sections_of_different_classes_in_one_push():
    sizes = []
    wire = padded_topic(257, 300) + padded_topic(10, 40, base=5000) + padded_topic(120, 100, base=6000) + padded_topic(70, 600, base=7000)
    wire_and_compare(wire, SDK, sizes=sizes)
    assert sizes[0] > 65536 and sizes[1] <= 8320 < sizes[2] <= 16640 < sizes[3] <= 65536


# ---- every alignment: hand-built sections ---------------------------------------------------------------------------------------
def zigzag(v: int) -> bytes:
    u = (v << 1) ^ (v >> 63)
    out = bytearray()
    while u >= 0x80:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


def raw_record(offset_delta, key, value, headers_count=True):
    """A v2 record; ``headers_count=False`` leaves the closing header count out, so that the VALUE is the record's — and a
    section's — last byte (the record stage reads no headers: the chain knows where a record ends)."""
    body = b"\x00" + zigzag(0) + zigzag(offset_delta) + zigzag(len(key)) + key + zigzag(len(value)) + value + (b"\x00" if headers_count else b"")
    return zigzag(len(body)) + body


def aligned_sections(bad: bool):
    """An anchor section at offset 0 (one good record: a push's staged copy starts at its lowest section, so with the anchor in
    every push a section keeps its own offset mod 16 on the device) and 64 sections, one for every section offset mod 16 and
    every value start mod 4 (the key grows by a byte), each of two records.  ``bad=False``: the last record's value ends
    exactly at the section's end.  ``bad=True``: the FIRST record's value is one byte short — its payload length reaches one
    byte beyond the value, where the next record begins."""
    anchor = raw_record(0, b"anchor", cases.wrap(b"anchor", cases.amount_payload(0)))
    arena = bytearray(anchor) + bytes(64 - len(anchor))
    secs, recs = [(0, len(anchor), 0, 1, 0)], []
    for skew in range(16):
        for shift in range(4):
            aid = b"k%02d" % skew + b"x" * shift
            good = cases.wrap(aid, cases.amount_payload(1000 * skew + shift))
            first = good[:-1] if bad else good
            body = raw_record(0, aid + b":1", first) + raw_record(1, aid + b":2", good, headers_count=False)
            at = (len(arena) + 15) // 16 * 16 + 16 + skew
            arena += bytes(at - len(arena)) + body
            base = 100 * len(secs)
            secs.append((at, len(body), base, 2, 0))
            recs.append((aid, good, base))
    arena += bytes(64)
    return np.frombuffer(bytes(arena), dtype=np.uint8).copy(), np.array(secs, dtype=SECTION_DTYPE), recs


def test_a_value_that_ends_exactly_at_its_sections_end_at_every_section_and_value_alignment():
    arena, secs, recs = aligned_sections(bad=False)
    assert {int(s["byte_off"]) % 16 for s in secs[1:]} == set(range(16)) and len({(len(aid) + int(s["byte_off"])) % 4 for (aid, _, _), s in zip(recs, secs[1:])}) == 4
    with DeviceDecoder(SDK) as d:
        d.push(secs, arena.ctypes.data)
        agg, ev, off, keys = device_result(d)
    assert keys == ["anchor"] + [aid.decode() for aid, _, _ in recs] and list(agg) == [0] + [1 + i // 2 for i in range(2 * len(recs))]
    assert ev[1:].tobytes() == b"".join(2 * SDK.decode_keyed(aid, good).tobytes() for aid, good, _ in recs)
    assert list(off) == [0] + [b + k for _, _, b in recs for k in (0, 1)]


def test_a_value_one_byte_short_never_borrows_the_next_records_first_byte_at_any_alignment():
    arena, secs, recs = aligned_sections(bad=True)
    with DeviceDecoder(SDK) as d:
        for i, (aid, good, base) in enumerate(recs):
            with pytest.raises(IngestError) as ei:
                d.push(secs[[0, i + 1]], arena.ctypes.data)
            assert ei.value.status == -7 and f"(offset {base})" in str(ei.value) and cases.DEVICE_REASON["envelope"] in str(ei.value), str(ei.value)
            with pytest.raises(IngestError):
                SDK.decode_keyed(aid, good[:-1])  # the host agrees
        assert d.result()[0].numel() == 0 and d.keys() == []  # not even the anchor's record: nothing of a failed push is delivered
        d.push(secs[:1], arena.ctypes.data)  # the decoder goes on
        assert device_result(d)[3] == ["anchor"]


# ---- several parts ----------------------------------------------------------------------------------------------------------------
def test_one_push_of_several_parts():
    acc = cases.accepted_cases()
    parts = [acc[0::3], acc[1::3], acc[2::3]]
    agg, events, keys = expected_of(parts[0] + parts[1] + parts[2])
    framers = [EventsTopicIngest(frames=True, device_lz4=True) for _ in parts]
    try:
        items = []
        for g, part, compression in zip(framers, parts, ("lz4", "none", "lz4")):
            g.feed(kw.record_batch(50, [(c.key, c.value) for c in part], compression=compression))
            items.append(g.drain_sections())
        with DeviceDecoder(SDK) as d:
            d.push_async(items)
            d.finish()
            dev = device_result(d)
    finally:
        for g in framers:
            g.close()
    assert dev[3] == keys and dev[0].tobytes() == agg.tobytes() and dev[1].tobytes() == events


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["push_records", "wire", "wire lz4"])
def test_each_named_refusal_fails_its_push_names_offset_and_reason_and_leaves_the_decoder_usable(route):
    good = cases.accepted_cases()[1:4]
    before = expected_of(good)
    with DeviceDecoder(SDK) as d:
        d.push_records([c.key for c in good], [c.value for c in good], [1, 2, 3])
        delivered = list(good)
        for n, c in enumerate(cases.refused_cases()):
            filler = cases.Case("filler", SDK, b"fill-%d:1" % n, cases.wrap(b"fill-%d" % n, cases.amount_payload(n)))
            recs = [filler, c, filler]
            with pytest.raises(IngestError) as ei:
                if route == "push_records":
                    d.push_records([r.key for r in recs], [r.value for r in recs], [40, 41, 42])
                else:
                    with EventsTopicIngest(frames=True, device_lz4=True) as g:
                        g.feed(kw.record_batch(40, [(r.key, r.value) for r in recs], compression="lz4" if "lz4" in route else "none"))
                        d.push_from(g)
            msg = str(ei.value)
            assert ei.value.status == -7 and "(offset 41)" in msg and cases.DEVICE_REASON[c.reason] in msg, (c.name, msg)
            # nothing of the push was delivered: not its records, not the filler's key
            dev = device_result(d)
            agg, events, keys = expected_of(delivered)
            assert dev[3] == keys and dev[1].tobytes() == events and dev[0].tobytes() == agg.tobytes(), c.name
            if n % 5 == 0:  # a following good push is delivered
                d.push_records([filler.key], [filler.value], [43])
                delivered.append(filler)
        dev = device_result(d)
        agg, events, keys = expected_of(delivered)
        assert dev[3] == keys and dev[1].tobytes() == events and len(keys) == len(before[2]) + 5


# ---- Doubles the fast parser cannot decide ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["push", "push_async", "push_records"])
def test_undecidable_doubles_inside_an_envelope_are_handed_back_to_the_host_and_come_back_exact(mode):
    decided, amb = cases.decided_double_cases(), cases.ambiguous_cases()
    group = decided[:2] + amb[:1] + decided[2:4] + amb[1:] + decided[4:]  # losers in front, between and behind
    wire = b"".join(kw.record_batch(10 + s, [(c.key, c.value) for c in group[s:s + 4]], compression="lz4" if s else "none") for s in range(0, len(group), 4))
    host = host_drain(wire, cases.F64)
    assert host[1].tobytes() == b"".join(cases.expected_event(c) for c in group)
    for c, text in zip(amb, cases.AMBIGUOUS_DOUBLES):
        assert cases.F64.decode_keyed(c.aggregate_id, c.value)["raw"] == np.float64(float(text)).view(np.uint64)
    with DeviceDecoder(cases.F64) as d:
        if mode == "push_records":
            d.push_records([c.key for c in group], [c.value for c in group], list(host[2]))
        else:
            with EventsTopicIngest(frames=True, device_lz4=True) as g:
                g.feed(wire)
                if mode == "push":
                    d.push_from(g)
                else:
                    d.push_async(g.drain_sections())
                    d.finish()
        same(host, device_result(d))
        assert d.counters()["doubles_parsed_on_host"] == len(amb)


# ---- the store ----------------------------------------------------------------------------------------------------------------------
def test_a_topic_of_16_byte_enveloped_values_is_not_taken_for_fixed_events():
    from fixture_models import SDK_DEPOSITED, SdkBankAccount, SdkSampleBusinessLogic, SdkSampleCommandModel
    from surge_amd.store import GpuReplayStateStore

    class VModel(SdkSampleCommandModel):
        def event_json_template(self):
            return EventJsonTemplate("", [("", SDK_DEPOSITED, "", "v", ARG_I32)], envelope=PE)

    class VLogic(SdkSampleBusinessLogic):
        def __init__(self):
            super().__init__()
            self._model = VModel()

    recs = [(b"a", 12345), (b"b", 54321), (b"a", 10000), (b"c", 99999), (b"a", 11111)]
    values = [cases.wrap(k, b'{"v":%d}' % v) for k, v in recs]
    assert all(len(v) == 16 and not v.startswith(b"{") for v in values)
    wire = kw.record_batch(0, [(k, v) for (k, _), v in zip(recs, values)])
    for restore in ("fetches", "topic"):
        store = GpuReplayStateStore(VLogic())
        try:
            counters = store.restore_from_fetches([wire]) if restore == "fetches" else store.restore_from_topic(wire)
            assert counters["records_delivered"] == 5
            assert store.get_aggregate("a") == SdkBankAccount(12345 + 10000 + 11111) and store.get_aggregate("b") == SdkBankAccount(54321)
            assert store.get_aggregate("c") == SdkBankAccount(99999)
        finally:
            store.close()


def sdk_topic(history, n_partitions, abort_every=0, pid=21, batch=70, start=None):
    """The history as the gateway writes it: per partition (PartitionStringUpToColon of the key) transactional lz4 batches and
    their markers; every ``abort_every``-th transaction of partition 0 carries decoys and is aborted.  Returns per partition the
    bytes; ``start``: the partitions' next offsets, continued."""
    from fixture_models import MoneyDeposited, SdkEvent, SdkSampleBusinessLogic
    from surge_amd.kafka import partition_for_keys

    fmt = SdkSampleBusinessLogic().event_write_formatting()
    msgs = [fmt.write_event(e) for e in history]
    parts = partition_for_keys([m.key for m in msgs], n_partitions, up_to_colon=True)
    start = start if start is not None else [0] * n_partitions
    out, aborted = [], 0
    for p in range(n_partitions):
        log, wire, off = [m for m, q in zip(msgs, parts) if q == p], [], start[p]
        for t, s in enumerate(range(0, len(log), batch)):
            if p == 0 and abort_every and t % abort_every == 1:  # a transaction that never happened
                decoys = [fmt.write_event(SdkEvent(m.key, MoneyDeposited(1))) for m in log[s:s + 9]]
                wire += [kw.record_batch(off, [(m.key.encode(), m.value) for m in decoys], compression="lz4", transactional=True, producer_id=pid),
                         kw.control_batch(off + len(decoys), pid, kw.ABORT)]
                off += len(decoys) + 1
                aborted += 1
            chunk = log[s:s + batch]
            wire += [kw.record_batch(off, [(m.key.encode(), m.value) for m in chunk], compression="lz4", transactional=True, producer_id=pid),
                     kw.control_batch(off + len(chunk), pid, kw.COMMIT)]
            off += len(chunk) + 1
        out.append(b"".join(wire))
        start[p] = off
    assert not abort_every or aborted >= 1
    return out


def fetches_of(per_partition, n_fetches=3):
    rows = []
    for f in range(n_fetches):
        rows.append([b[f * len(b) // n_fetches:(f + 1) * len(b) // n_fetches] or None for b in per_partition])  # cut wherever it falls
    return rows


def sdk_history(n_ids, n_events, seed, first_id=0):
    from fixture_models import MoneyDeposited, SdkEvent

    rng = np.random.default_rng(seed)
    ids = [f"0c3f1d9e-7a55-4a5c-9d5e-{i:012x}" for i in range(first_id, first_id + n_ids)]
    return ids, [SdkEvent(ids[int(a)], MoneyDeposited(int(m))) for a, m in zip(rng.integers(0, n_ids, size=n_events), rng.integers(0, 2**31, size=n_events))]


def want_of(ids, history):
    from fixture_models import SDK_SAMPLE_MODEL

    per = {k: [] for k in ids}
    for e in history:
        per[e.aggregateId].append(e.payload)
    return {k: SDK_SAMPLE_MODEL.apply_events(None, v) for k, v in per.items()}


def check_store(store, want):
    from fixture_models import sdk_sample_state_bytes

    for k, w in want.items():
        assert store.get_aggregate(k) == w, k
        assert store.get_aggregate_bytes(k) == (None if w is None else sdk_sample_state_bytes(k, w)), k


@pytest.mark.parametrize("bound_log", [False, True])
def test_the_sdk_sample_store_recovers_from_its_enveloped_events_topic(bound_log):
    from fixture_models import SdkSampleBusinessLogic
    from surge_amd.store import GpuReplayStateStore

    ids, history = sdk_history(300, 3000, 11)
    want = want_of(ids + ["never-written"], history)
    assert want["never-written"] is None and sum(w is not None for w in want.values()) >= 290
    topic = sdk_topic(history, 2, abort_every=4)
    store = GpuReplayStateStore(SdkSampleBusinessLogic())
    try:
        counters = store.restore_from_fetches(fetches_of(topic), n_partitions=2, framing_threads=2, bound_log=bound_log)
        assert counters["records_delivered"] == len(history) and counters["records_aborted"] >= 9 and counters["doubles_parsed_on_host"] == 0
        check_store(store, want)
    finally:
        store.close()


def test_the_full_cycle_and_one_more_events_topic_to_state_topic_and_back():
    """A store recovered from the enveloped events topic publishes its states in the State envelope; a store resumed from that
    state topic equals it — and, with the next stretch of events folded on top, equals the store recovered from the events
    topic of the whole history; then once more from the state topic that store publishes."""
    from fixture_models import SdkSampleBusinessLogic
    from surge_amd.encode import JP_I32, JsonTemplate
    from surge_amd.snapshot import BulkSnapshotPublisher
    from surge_amd.store import GpuReplayStateStore

    state_tmpl = JsonTemplate((b'{"balance":', (JP_I32, 0), b"}"))
    ids1, h1 = sdk_history(120, 1200, 21)
    ids2, h2 = sdk_history(150, 900, 22, first_id=60)  # half of them new
    ids = sorted(set(ids1) | set(ids2))
    bl = SdkSampleBusinessLogic()
    stores, pubs = [], []

    def new_store():
        stores.append(GpuReplayStateStore(bl))
        return stores[-1]

    def publish(store):
        pubs.append(BulkSnapshotPublisher(store.engine, store.keys.keys, 2, template=state_tmpl, compression="lz4", device_compression=True, envelope="protobuf_state"))
        topic = {p: bytes(b) for p, b in pubs[-1].publish().items()}
        return [[topic.get(p) for p in range(2)]]

    def equal(a, b, keys):
        for k in keys:
            assert a.get_aggregate_bytes(k) == b.get_aggregate_bytes(k), k

    try:
        offsets = [0, 0]
        t1 = sdk_topic(h1, 2, start=offsets)
        e1 = new_store()
        e1.restore_from_fetches(fetches_of(t1), n_partitions=2, framing_threads=2)
        check_store(e1, want_of(ids1, h1))
        states1 = publish(e1)
        r1 = new_store()
        counts = r1.restore_from_state_topic(states1, n_partitions=2, template=state_tmpl, envelope="protobuf_state")
        assert counts["refused"] == 0 and counts["rows_written"] == len(e1.keys.keys)
        equal(r1, e1, ids)
        # one more cycle: the events topic grows; the resumed store folds the new stretch on top of the first state topic
        t2 = sdk_topic(h2, 2, start=offsets, pid=22)
        e2 = new_store()
        e2.restore_from_fetches(fetches_of([a + b for a, b in zip(t1, t2)], 4), n_partitions=2, framing_threads=2)
        check_store(e2, want_of(ids, h1 + h2))
        r2 = new_store()
        r2.restore_from_state_topic(states1, n_partitions=2, template=state_tmpl, envelope="protobuf_state", events_tail=h2)
        equal(r2, e2, ids)
        # ... and the second cycle's own state topic (published by the store that read the events topic: a resumed store's
        # loaded states are its snapshot baseline, it would publish the tail's changes only)
        r3 = new_store()
        counts = r3.restore_from_state_topic(publish(e2), n_partitions=2, template=state_tmpl, envelope="protobuf_state")
        assert counts["refused"] == 0 and counts["rows_written"] == len(e2.keys.keys)
        equal(r3, e2, ids)
        equal(r3, r2, ids)
    finally:
        for p in pubs:
            p.close()
        for s in stores:
            s.close()
