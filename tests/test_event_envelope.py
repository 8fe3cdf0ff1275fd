"""The host half of the enveloped events route: a protobuf ``Event{aggregateId, payload}`` record value -> the 16-byte fixed
event (``surge_event_json_decode_keyed``, ``surge_ingest_drain_json`` with ``EventJsonTemplate(envelope="protobuf_event")``).
The envelope reader is the text the device kernels compile (``sp_envelope``, state_parse.h), so what is pinned here is what
tests/test_event_envelope_gpu.py holds the device to.  The references are the protobuf runtime for ``(id, payload)`` and the
BARE template's decode of the payload (tests/event_envelope_cases.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import event_envelope_cases as cases
import kafka_wire as kw
from surge_amd import _native
from surge_amd.ingest import CEventJsonTemplate, EventJsonTemplate, EventsTopicIngest, IngestError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PE = cases.PE


def refusal(case, keyed=True):
    with pytest.raises(IngestError) as ei:
        case.template.decode_keyed(case.aggregate_id, case.value) if keyed else case.template.decode(case.value)
    assert ei.value.status == -7
    return str(ei.value)


def test_the_field_keeps_its_place_and_only_the_two_values_are_valid():
    assert CEventJsonTemplate.envelope.offset == 4 and CEventJsonTemplate.envelope.size == 4 and CEventJsonTemplate.discriminator.offset == 8
    header = open(os.path.join(ROOT, "include", "surge_ingest.h")).read()
    assert "#define SURGE_EVJ_ENVELOPE_NONE           0" in header and "#define SURGE_EVJ_ENVELOPE_PROTOBUF_EVENT 1" in header
    assert "surge_event_json_decode_keyed" in header and "surge_event_json_decode_keyed" in _native.INGEST_EXPORTS
    lib = _native.load()
    c = cases.SDK.to_c()
    assert c.envelope == 1 and cases.SDK_BARE.to_c().envelope == 0 and lib.surge_event_json_validate(ctypes.byref(c)) == 0
    for bad in (2, 3, 0xFFFFFFFF):
        c.envelope = bad
        assert lib.surge_event_json_validate(ctypes.byref(c)) != 0 and b"envelope" in lib.surge_event_json_last_error()
    with pytest.raises(ValueError):
        EventJsonTemplate("", [("", 0, "", "amount", 1)], envelope="protobuf_state")
    with pytest.raises(ValueError):
        EventJsonTemplate("", [("", 0, "", "amount", 1)], envelope=None)


ACCEPTED = cases.accepted_cases() + cases.other_template_cases() + cases.decided_double_cases()


@pytest.mark.parametrize("case", ACCEPTED, ids=[c.name for c in ACCEPTED])
def test_values_the_protobuf_runtime_wrote_decode_to_the_event_of_their_payload(case):
    want = cases.expected_event(case)
    assert case.template.decode(case.value).tobytes() == want  # no comparison
    assert case.template.decode_keyed(case.aggregate_id, case.value).tobytes() == want
    assert case.template.decode_keyed(None, case.value).tobytes() == want
    # the id is compared raw, byte for byte, and with the id, not with the whole key
    aid = case.aggregate_id
    for other in (aid + b"x", aid + b":1", aid[:-1], aid[:-1] + bytes([aid[-1] ^ 1]) if aid else b"\x00"):
        if other != aid:
            with pytest.raises(IngestError) as ei:
                case.template.decode_keyed(other, case.value)
            assert ei.value.status == -7 and cases.HOST_REASON["mismatch"] in str(ei.value)
    # a zeroed field behaves as before: the bare template does not read an envelope
    with pytest.raises(IngestError):
        case.bare.decode(case.value)


def test_the_corpus_covers_the_lengths_the_varints_step_at():
    acc = cases.accepted_cases()
    ids = {len(c.aggregate_id) for c in acc}
    pays = {len(cases.runtime_fields(c.value)[1]) for c in acc}
    assert set(cases.ID_LENGTHS) <= ids and {127, 128, 16383, 16384} <= pays
    assert any(b'"' in c.key for c in acc) and any(max(c.key, default=0) >= 0xF0 for c in acc)
    assert not any(c.value.startswith(b"\x0a") for c in acc if not c.aggregate_id)  # proto3 leaves an empty field 1 out
    for c in cases.overlong_cases():
        rid, payload = cases.runtime_fields(c.value)
        assert (rid, payload) == (c.aggregate_id, cases.amount_payload(-12)) and c.value != cases.wrap(rid, payload), c.name  # (not the minimal spelling)
        assert int(c.template.decode_keyed(c.aggregate_id, c.value)["raw"]) == np.uint32(np.int32(-12))


REFUSED = cases.refused_cases()


@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_each_refusal_is_reached_by_a_named_input_and_says_why(case):
    assert cases.HOST_REASON[case.reason] in refusal(case)
    if case.reason == "envelope":
        assert cases.HOST_REASON["envelope"] in refusal(case, keyed=False)  # the grammar comes before the comparison
        other = cases.Case(case.name, case.template, b"another-id", case.value, case.reason)
        assert cases.HOST_REASON["envelope"] in refusal(other)
    if case.reason == "mismatch":
        assert cases.runtime_fields(case.value) is not None
        case.template.decode(case.value)  # without a key the value is a good one
    assert {c.reason for c in REFUSED} == {"envelope", "mismatch", "json"}


def test_every_proper_prefix_is_refused_and_one_more_byte_is_an_envelope_error():
    for c in (cases.Case("sdk", cases.SDK, b"0c3f1d9e-7a55", cases.wrap(b"0c3f1d9e-7a55", cases.amount_payload(-123456))),
              cases.other_template_cases()[2]):
        for cut in range(len(c.value)):
            for key in (c.aggregate_id, None):
                with pytest.raises(IngestError):
                    c.template.decode_keyed(key, c.value[:cut])
        for extra in (b"\x00", b"\x0a", b"\x12", b"}", b" "):
            with pytest.raises(IngestError) as ei:
                c.template.decode_keyed(c.aggregate_id, c.value + extra)
            assert cases.HOST_REASON["envelope"] in str(ei.value)


def test_a_double_the_fast_algorithm_cannot_decide_comes_back_as_strtod_reads_it_inside_an_envelope():
    for case, text in zip(cases.ambiguous_cases(), cases.AMBIGUOUS_DOUBLES):
        got = case.template.decode_keyed(case.aggregate_id, case.value)
        assert got["raw"] == np.float64(float(text)).view(np.uint64) and got.tobytes() == cases.expected_event(case)


def test_whenever_the_host_says_ok_the_protobuf_runtime_reads_the_same_id_and_payload():
    """Over the whole corpus and a few thousand seeded mutations of it.  A mutation the runtime itself rejects may be left
    out (the grammar here never validates the id's UTF-8) — but never a value of the unmutated corpus, and there must be
    plenty of both outcomes among the mutations."""
    corpus = ACCEPTED + REFUSED + cases.ambiguous_cases()
    muts = cases.mutations([c for c in corpus if len(c.value) < 4000], 60) + cases.mutations([c for c in corpus if len(c.value) >= 4000], 6)
    assert len(muts) >= 3000
    ok = {False: 0, True: 0}
    refused = left_out = 0
    for mutated, group in ((False, corpus), (True, muts)):
        for c in group:
            try:
                got = c.template.decode(c.value)
            except IngestError:
                assert mutated or c.reason in ("envelope", "json"), c.name
                refused += mutated
                continue
            assert mutated or c.reason in (None, "mismatch"), c.name
            fields = cases.runtime_fields(c.value)
            if fields is None:
                assert mutated, c.name  # the unmutated corpus passes with nothing left out
                left_out += 1
                continue
            ok[mutated] += 1
            rid, payload = fields
            assert c.template.decode_keyed(rid, c.value).tobytes() == got.tobytes() == c.bare.decode(payload).tobytes(), (c.name, c.value[:40])
            with pytest.raises(IngestError):
                c.template.decode_keyed(rid + b"\x00", c.value)
    assert ok[False] >= 40 and ok[True] >= 100 and refused >= 1000 and left_out < ok[True], (ok, refused, left_out)


# ---- the drain -----------------------------------------------------------------------------------------------------------------
def topic_of(groups, rng):
    """Record batches over the accepted corpus: lz4 and none, transactions with commits and aborts, the producer's flush
    record.  Returns ``(wire, delivered cases in offset order)``."""
    wire, off, delivered = [kw.record_batch(0, [(b"", b"")])], 1, []
    for i, group in enumerate(groups):
        recs = [(c.key, c.value) for c in group]
        if i % 3 == 1:
            recs.insert(len(recs) // 2, (b"", b""))  # KafkaProducerActorImpl.scala:322-329
        txn = i % 2 == 0
        outcome = kw.ABORT if txn and i % 6 == 4 else kw.COMMIT
        wire.append(kw.record_batch(off, recs, compression="lz4" if rng.random() < 0.5 else "none", transactional=txn, producer_id=9))
        off += len(recs)
        if txn:
            wire.append(kw.control_batch(off, 9, outcome))
            off += 1
        if outcome == kw.COMMIT:
            delivered += group
    return b"".join(wire), delivered


def test_drain_json_reads_an_enveloped_topic_with_the_keyed_comparison_the_flush_record_and_transactions():
    rng = np.random.default_rng(5)
    acc = cases.accepted_cases()
    groups = [acc[i:i + 5] for i in range(0, len(acc), 5)]
    wire, delivered = topic_of(groups, rng)
    assert 0 < len(delivered) < len(acc)  # an aborted transaction's records never arrive
    with EventsTopicIngest() as g:
        g.feed(wire)
        agg_idx, events, offsets = g.drain_json(cases.SDK)
        keys = g.key_table()
        counters = g.counters()
    assert events.tobytes() == b"".join(cases.expected_event(c) for c in delivered)
    assert [keys.keys[i].encode("utf-8") for i in agg_idx] == [c.aggregate_id for c in delivered]
    assert list(offsets) == sorted(set(offsets)) and counters["flush_records_skipped"] >= 2 and counters["records_aborted"] > 0
    # each refusal in a topic of its own: nothing is popped, the error names the record's offset and the reason
    good = acc[1]
    for c in cases.refused_cases():
        with EventsTopicIngest() as g:
            g.feed(kw.record_batch(40, [(good.key, good.value), (c.key, c.value), (good.key, good.value)]))
            with pytest.raises(IngestError) as ei:
                g.drain_json(cases.SDK)
            assert ei.value.status == -7 and "offset 41" in str(ei.value) and cases.HOST_REASON[c.reason] in str(ei.value), (c.name, str(ei.value))
            assert g.ready == 3
    # the bare template over the same topic refuses its first value; the 16-byte enveloped value is no fixed event to the template
    with EventsTopicIngest() as g:
        g.feed(wire)
        with pytest.raises(IngestError):
            g.drain_json(cases.SDK_BARE)
    sixteen = cases.other_template_cases()[:2]
    with EventsTopicIngest() as g:
        g.feed(kw.record_batch(0, [(c.key, c.value) for c in sixteen]))
        _, events, _ = g.drain_json(cases.V)
    assert events.tobytes() == b"".join(cases.expected_event(c) for c in sixteen) and all(int(e["raw"]) == 12345 and int(e["type"]) == 3 for e in events)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------
def sdk_history(n_ids, n_events, seed):
    from fixture_models import MoneyDeposited, SdkEvent

    rng = np.random.default_rng(seed)
    ids = [f"0c3f1d9e-7a55-4a5c-9d5e-{i:012x}" for i in range(n_ids)]
    return ids, [SdkEvent(ids[int(a)], MoneyDeposited(int(m))) for a, m in zip(rng.integers(0, n_ids, size=n_events), rng.integers(0, 2**31, size=n_events))]


def test_the_sdk_sample_writes_the_runtimes_event_bytes_and_reads_them_back():
    from fixture_models import MoneyDeposited, SdkEvent, SdkSampleBusinessLogic, sdk_sample_event_bytes

    bl = SdkSampleBusinessLogic()
    fmt, tmpl = bl.event_write_formatting(), bl.command_model().event_json_template()
    assert tmpl.envelope == PE and tmpl.discriminator == ""
    for key in ("", "k", "0c3f1d9e-7a55-4a5c-9d5e-00000000002a", "ünï-✓", 'we"ird\\id', "k" * 128, "k" * 16384):
        for amount in (0, 1, 2**31 - 1):
            evt = SdkEvent(key, MoneyDeposited(amount))
            msg = fmt.write_event(evt)
            assert msg.key == key and msg.value == sdk_sample_event_bytes(key, evt.payload) == cases.wrap(key, b'{"amount":%d}' % amount)
            assert fmt.read_event(msg) == evt
            assert tmpl.decode_keyed(key.encode("utf-8"), msg.value).tobytes() == bl.command_model().encode_events([evt])[0].tobytes()
    for c in cases.refused_cases():
        if c.reason == "envelope":  # what the decoders refuse as no envelope, the fixture's reader refuses
            from surge_amd.core import SerializedMessage

            with pytest.raises(Exception):
                fmt.read_event(SerializedMessage(c.key.decode(), c.value))


def test_the_host_drain_of_an_sdk_sample_events_topic_folds_to_the_samples_own_apply_events():
    """The host route of a recovery without a device: drain_json over the enveloped topic, then the model's own fold of the
    decoded events per aggregate, against ``SDK_SAMPLE_MODEL.apply_events`` over the events written."""
    from fixture_models import SDK_SAMPLE_MODEL, SdkBankAccount, SdkSampleBusinessLogic

    bl = SdkSampleBusinessLogic()
    model, fmt = bl.command_model(), bl.event_write_formatting()
    ids, history = sdk_history(60, 900, 3)
    msgs = [fmt.write_event(e) for e in history]
    wire = b"".join(kw.record_batch(s, [(m.key.encode(), m.value) for m in msgs[s:s + 64]], compression="lz4") for s in range(0, len(msgs), 64))
    with EventsTopicIngest() as g:
        g.feed(wire)
        agg_idx, events, _ = g.drain_json(model.event_json_template())
        keys = g.key_table().keys
    assert events.tobytes() == model.encode_events(history).tobytes()
    balance = {}
    for a, e in zip(agg_idx, events):
        balance[keys[a]] = (balance.get(keys[a], 0) + int(e["raw"]) + 2**31) % 2**32 - 2**31
    for k in ids:
        want = SDK_SAMPLE_MODEL.apply_events(None, [e.payload for e in history if e.aggregateId == k])
        assert (SdkBankAccount(balance[k]) if k in balance else None) == want


@pytest.mark.gpu
def test_restore_from_topic_of_the_sdk_sample_store_on_the_host_route_equals_apply_events(monkeypatch):
    """``restore_from_topic`` with the device decode switched off: the host fallback must go to the template's drain at once
    (an enveloped value is never tried as a fixed event) and the store must equal the sample's own fold."""
    import surge_amd.store as store_mod
    from fixture_models import SDK_SAMPLE_MODEL, MoneyDeposited, SdkEvent, SdkSampleBusinessLogic, sdk_sample_state_bytes

    bl = SdkSampleBusinessLogic()
    fmt = bl.event_write_formatting()
    ids, history = sdk_history(40, 500, 4)
    history = [SdkEvent("a", MoneyDeposited(12345))] * 3 + history  # (with payload field "amount" these are 20 bytes; see the 16-byte test on the device)
    msgs = [fmt.write_event(e) for e in history]
    wire = b"".join(kw.record_batch(s, [(m.key.encode(), m.value) for m in msgs[s:s + 50]]) for s in range(0, len(msgs), 50))

    def no_device(self, *a, **k):
        raise store_mod._NotDeviceDecodable("host route under test")

    def no_fixed(self, *a, **k):
        raise AssertionError("an enveloped topic was tried as 16-byte fixed events")

    monkeypatch.setattr(store_mod.GpuReplayStateStore, "restore_from_fetches", no_device)
    monkeypatch.setattr(EventsTopicIngest, "drain_fixed16", no_fixed)
    store = store_mod.GpuReplayStateStore(bl)
    try:
        counters = store.restore_from_topic(wire)
        assert counters["records_delivered"] == len(history)
        for k in ids + ["a"]:
            want = SDK_SAMPLE_MODEL.apply_events(None, [e.payload for e in history if e.aggregateId == k])
            assert store.get_aggregate(k) == want
            assert store.get_aggregate_bytes(k) == (None if want is None else sdk_sample_state_bytes(k, want))
    finally:
        store.close()


def test_no_prefix_or_mutation_makes_the_decoder_read_outside_the_value_under_asan_and_ubsan(tmp_path):
    """tests/cpp/event_envelope_prefixes.cpp: every prefix and a few thousand mutations of enveloped values, each in a malloc
    of exactly its length, through ``surge_event_json_decode_keyed`` built with -fsanitize=address,undefined — a stand-alone
    program, nothing of it is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "event_envelope_prefixes")
    srcs = [os.path.join(ROOT, "tests", "cpp", "event_envelope_prefixes.cpp")] + [os.path.join(ROOT, "surge_amd", "csrc", f) for f in ("event_decode.cpp", "f64_text.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]
