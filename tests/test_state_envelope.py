"""The host half of the envelope route (``surge_decode_protobuf_state``): a protobuf ``State{aggregateId, payload}`` value ->
the fixed 64-byte state.  It is the routine the device kernel runs (``state_parse_protobuf_state``, state_parse.h), so what is
pinned here is what tests/test_state_envelope_gpu.py holds the kernel to.  The references are the protobuf runtime and the
bare route (tests/state_envelope_cases.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import state_envelope_cases as cases
from surge_amd.encode import (DECODE_AMBIGUOUS, DECODE_ENVELOPE, DECODE_KEY_MISMATCH, DECODE_LITERAL, DECODE_OK, DECODE_TRAILING, decode_state_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = "protobuf_state"


def dec(case, key="case"):
    return decode_state_host(case.template, case.value, case.key if key == "case" else key, envelope=PB)


def test_the_new_status_keeps_the_existing_numbers():
    from surge_amd import encode

    assert DECODE_ENVELOPE == 11 and encode.DECODE_STATUS[11] == "ENVELOPE"
    assert [encode.DECODE_STATUS[i] for i in range(11)] == ["OK", "LITERAL", "STRING", "ESCAPE", "KEY_MISMATCH", "INT", "RANGE", "NUMBER", "TRAILING",
                                                            "AMBIGUOUS", "SURROGATE"] and encode.DECODE_STATUS[255] == "SKIPPED"
    header = open(os.path.join(ROOT, "include", "surge_replay.h")).read()
    assert "#define SURGE_STATE_DECODE_ENVELOPE    11" in header


ACCEPTED = cases.accepted_cases()


@pytest.mark.parametrize("case", ACCEPTED, ids=[c.name for c in ACCEPTED])
def test_values_the_protobuf_runtime_wrote_decode_to_the_fields_the_references_name(case):
    rid, payload = cases.runtime_fields(case.value)
    assert rid == case.key
    for with_key in (True, False):
        rc, st, spans = dec(case) if with_key else dec(case, None)
        want = cases.expected(case, with_key)
        assert want[0] == DECODE_OK  # (the bare route reads the payload: the case is an accepted one by the reference, too)
        assert (rc, st.tobytes(), spans) == want
    if case.template is cases.SDK:
        assert int(dec(case)[1]["count"][0]) == cases.sdk_balance(case.value)
    # the id is compared raw, byte for byte: the payload's escaped spelling of it is not the id
    assert dec(case, case.key + b"x")[0] == DECODE_KEY_MISMATCH
    if case.key:
        assert dec(case, case.key[:-1])[0] == DECODE_KEY_MISMATCH
        assert dec(case, case.key[:-1] + bytes([case.key[-1] ^ 1]))[0] == DECODE_KEY_MISMATCH


def test_the_corpus_covers_the_lengths_the_varints_step_at():
    ids = {len(c.key) for c in ACCEPTED}
    pays = {len(cases.runtime_fields(c.value)[1]) for c in ACCEPTED}
    assert set(cases.ID_LENGTHS) <= ids and {127, 128, 16383, 16384} <= pays
    assert any(b'"' in c.key for c in ACCEPTED) and any(max(c.key, default=0) >= 0xF0 for c in ACCEPTED)
    assert not any(c.value.startswith(b"\x0a") for c in ACCEPTED if not c.key)  # proto3 leaves an empty field 1 out


def test_over_long_varints_are_accepted_as_the_runtime_accepts_them():
    for case in cases.overlong_cases():
        rid, payload = cases.runtime_fields(case.value)
        assert (rid, payload) == (case.key, b'{"balance":-12}'), case.name
        assert case.value != cases.wrap(rid, payload)  # (not the minimal spelling)
        rc, st, _ = dec(case)
        assert rc == DECODE_OK and int(st["count"][0]) == -12, case.name


REFUSED = cases.refused_cases() + cases.other_status_cases()


@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_each_refusal_is_reached_by_a_named_input(case):
    rc, st, _ = dec(case)
    assert rc == case.status, (case.name, rc)
    assert st.tobytes() == bytes(64)  # state64_out is written only for a value that decodes
    if case.status == DECODE_ENVELOPE:
        assert dec(case, None)[0] == DECODE_ENVELOPE  # the grammar comes before the comparison
    assert {c.status for c in REFUSED} == {DECODE_ENVELOPE, DECODE_KEY_MISMATCH, DECODE_LITERAL, DECODE_TRAILING}


def test_every_proper_prefix_is_refused_and_one_more_byte_is_an_envelope_error():
    from fixture_models import SdkBankAccount, sdk_sample_state_bytes

    sdk = cases.Case("sdk", cases.SDK, sdk_sample_state_bytes("0c3f1d9e-7a55", SdkBankAccount(-123456)), b"0c3f1d9e-7a55")
    bank = cases.Case("bank", cases.BANK, cases.wrap(cases.BANK_KEY, cases.BANK_PAYLOAD), cases.BANK_KEY.encode("utf-8"))
    for c in (sdk, bank):
        assert dec(c)[0] == DECODE_OK and dec(c, None)[0] == DECODE_OK
        for cut in range(len(c.value)):
            for key in (c.key, None):
                rc = decode_state_host(c.template, c.value[:cut], key, envelope=PB)[0]
                assert rc not in (DECODE_OK, DECODE_AMBIGUOUS), (c.name, cut, rc)
        for extra in (b"\x00", b"\x0a", b"\x12", b"}", b" "):
            assert decode_state_host(c.template, c.value + extra, c.key, envelope=PB)[0] == DECODE_ENVELOPE


def test_str_spans_are_relative_to_the_value_not_to_the_payload():
    import json

    value = cases.wrap(cases.BANK_KEY, cases.BANK_PAYLOAD)
    rc, st, spans = decode_state_host(cases.BANK, value, cases.BANK_KEY, envelope=PB)
    assert rc == DECODE_OK and st["balance"][0] == -1250.0
    (o0, l0), (o1, l1) = spans[0], spans[1]
    assert json.loads(b'"' + value[o0:o0 + l0] + b'"') == 'J "q" / €' and l1 == 0 and value[o1 - 1:o1 + 1] == b'""'
    bare = decode_state_host(cases.BANK, cases.BANK_PAYLOAD, cases.BANK_KEY)[2]
    shift = len(value) - len(cases.BANK_PAYLOAD)
    assert shift > 0 and spans[:2] == [(o + shift, n) for o, n in bare[:2]]


def test_a_double_the_fast_algorithm_cannot_decide_comes_back_as_strtod_reads_it_inside_an_envelope():
    for case, text in zip(cases.ambiguous_cases(), cases.AMBIGUOUS_DOUBLES):
        rc, st, _ = dec(case)
        assert rc == DECODE_OK  # never AMBIGUOUS from the host export
        assert st["balance"].view(np.uint64)[0] == np.float64(float(text)).view(np.uint64)


def test_whenever_the_host_says_ok_the_protobuf_runtime_reads_the_same_id_and_payload():
    """Over the whole corpus and a few thousand seeded mutations of it.  A mutation the runtime itself rejects may be left
    out (the grammar here is narrower in what it spells out, e.g. it never validates the id's UTF-8) — but never a value of
    the unmutated corpus, and there must be plenty of both outcomes among the mutations."""
    corpus = cases.corpus()
    muts = cases.mutations([c for c in corpus if len(c.value) < 4000], 60) + cases.mutations([c for c in corpus if len(c.value) >= 4000], 6)
    assert len(muts) >= 3000
    ok = {False: 0, True: 0}
    left_out = 0
    for mutated, group in ((False, corpus), (True, muts)):
        for c in group:
            rc, st, _ = decode_state_host(c.template, c.value, None, envelope=PB)
            if not mutated and c.status in (DECODE_OK, DECODE_KEY_MISMATCH):
                assert rc == DECODE_OK, c.name
            if rc != DECODE_OK:
                continue
            fields = cases.runtime_fields(c.value)
            if fields is None:
                assert mutated, c.name  # the unmutated corpus passes with nothing left out
                left_out += 1
                continue
            ok[mutated] += 1
            rid, payload = fields
            # the same id: the host compares field 1 with a key byte for byte ...
            assert decode_state_host(c.template, c.value, rid, envelope=PB)[0] in (DECODE_OK, DECODE_KEY_MISMATCH)
            if c.template is cases.SDK or c.template is cases.F64_ONLY:  # (no KEY part in the payload: only field 1 is compared)
                assert decode_state_host(c.template, c.value, rid, envelope=PB)[0] == DECODE_OK, (c.name, c.value[:40])
                assert decode_state_host(c.template, c.value, rid + b"\x00", envelope=PB)[0] == DECODE_KEY_MISMATCH
            # ... and the same payload: the bare route over the runtime's payload gives the same row
            rc2, st2, _ = decode_state_host(c.template, payload, None)
            assert rc2 == DECODE_OK and st2.tobytes() == st.tobytes(), (c.name, c.value[:40])
    assert ok[False] >= 40 and ok[True] >= 100 and left_out < ok[True], (ok, left_out)


def test_no_prefix_or_mutation_makes_the_envelope_parser_read_outside_the_value_under_asan_and_ubsan(tmp_path):
    """tests/cpp/state_envelope_prefixes.cpp: every prefix and a few thousand mutations of enveloped values, each in a malloc
    of exactly its length, through the export built with -fsanitize=address,undefined — a stand-alone program, nothing of
    it is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "state_envelope_prefixes")
    srcs = [os.path.join(ROOT, "tests", "cpp", "state_envelope_prefixes.cpp")] + [os.path.join(ROOT, "surge_amd", "csrc", f) for f in ("state_decode_host.cpp", "f64_text.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]


def test_the_sdk_sample_format_writes_the_runtimes_bytes_and_reads_them_back():
    from fixture_models import SdkBankAccount, SdkSampleBusinessLogic, SdkSampleCommandModel, SdkSampleStateFormat, parse_state_envelope
    from surge_amd.core import write_state_of

    fmt = SdkSampleStateFormat()
    for key in ("", "k", "0c3f1d9e-7a55-4a5c-9d5e-00000000002a", "ünï-✓", 'we"ird\\id', "k" * 128, "k" * 16384):
        for balance in (0, 1, -1, 2**31 - 1, -(2**31)):
            x = SdkBankAccount(balance)
            data = fmt.write_state_with_id(key, x).value
            assert data == cases.wrap(key, b'{"balance":%d}' % balance) == write_state_of(fmt, key, x).value
            assert fmt.read_state(data) == x and fmt.read_state_with_id(data) == (key, x)
            assert parse_state_envelope(data) == (key, b'{"balance":%d}' % balance)
            assert decode_state_host(cases.SDK, data, key, envelope=PB)[0] == DECODE_OK
        assert fmt.read_state(fmt.write_state(SdkBankAccount(5)).value) == SdkBankAccount(5)
    for c in cases.refused_cases():  # what the device refuses, the fixture's reader refuses
        assert fmt.read_state(c.value) is None, c.name
    bl = SdkSampleBusinessLogic()
    assert isinstance(bl.command_model(), SdkSampleCommandModel) and bl.aggregate_write_formatting() is bl.aggregate_read_formatting()


def test_an_unknown_envelope_spelling_is_a_value_error():
    with pytest.raises(ValueError):
        decode_state_host(cases.SDK, b"\x12\x00", None, envelope="nonsense")
    with pytest.raises(ValueError):
        decode_state_host(cases.SDK, b"\x12\x00", None, envelope=None)
