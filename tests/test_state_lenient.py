"""The lenient reading mode of the state decoder on the host (``surge_decode_json_state_lenient`` /
``surge_decode_protobuf_state_lenient``, ``decode_state_host(lenient=True)``): the parser the device kernel runs, held to
``json.loads`` over the corpus of tests/state_lenient_cases.py — the expected row, strings and status come from the parsed
document and the template's own parts — and to the strict export over every corpus the strict mode already has."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import number_text_cases as numbers
import state_envelope_cases as envelope_cases
import state_lenient_cases as L
import state_strings_gen
import state_topic_gen
from surge_amd import _native
from surge_amd.encode import DECODE_STATUS, JP_F64, JP_I32, JP_I64, JP_U32, CJsonTemplate, JsonTemplate, decode_state_host, unescape_json_string

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("surge_replay_set_decode_mode", "surge_decode_json_state_lenient", "surge_decode_protobuf_state_lenient")


def lenient(case, key="case"):
    return decode_state_host(case.template, case.value, case.key if key == "case" else key, envelope="protobuf_state" if case.envelope else "none", lenient=True)


def held_to_the_document(case, members, rc, state, spans):
    """``rc == 0`` exactly when the document has every field with a value of its type, and then this row and these strings."""
    want = L.expected_row(case.template, members, case.key)
    assert (rc == 0) == (want is not None), (case.name, DECODE_STATUS[rc])
    if want is None:
        return
    row, strings = want
    assert state.tobytes() == row, case.name
    for column, text in strings.items():
        off, n = spans[column]
        assert case.value[off - 1:off] == b'"' and case.value[off + n:off + n + 1] == b'"', case.name
        assert unescape_json_string(case.value[off:off + n]) == text, case.name  # (the LAST occurrence's: an earlier one holds another string)


# ---- the corpus against json.loads ------------------------------------------------------------------------------------------
def test_accepted_values_give_the_row_and_the_strings_of_the_parsed_document():
    n = 0
    for case in L.corpus():
        if case.status != L.OK:
            continue
        rc, state, spans = lenient(case)
        assert rc == 0, (case.name, DECODE_STATUS[rc])
        held_to_the_document(case, L.document(case.value), rc, state, spans)
        rc2, state2, spans2 = lenient(case, key=None)  # and without a key to compare
        assert rc2 == 0 and state2.tobytes() == state.tobytes() and spans2 == spans
        n += 1
    assert n > 250
    print(f"{n} accepted values")


def test_the_corpus_has_what_it_claims():
    cases = L.corpus()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("counter order") for n in names) == 6 and sum(n.startswith("bank order") for n in names) == 24
    assert len({c.value for c in cases if c.name.startswith("bank order")}) == 24  # four fields have 24 orders: all of them
    assert sum(n.startswith("ws ") for n in names) == 4 * 15 + 3
    for depth in (1, 31, 32, 33):
        assert any(f"depth {depth}" in n for n in names)
    blob = next(c for c in cases if c.name.startswith("40 KB"))
    assert len(blob.value) > 40 * 1024
    by_status = {}
    for c in cases:
        by_status.setdefault(c.status, []).append(c)
    for status in (L.STRING, L.ESCAPE, L.KEY_MISMATCH, L.INT, L.RANGE, L.NUMBER, L.TRAILING, L.SURROGATE, L.SYNTAX, L.MISSING):
        assert by_status.get(status), DECODE_STATUS[status]


@pytest.mark.parametrize("case", [c for c in L.corpus() if c.status > 0], ids=lambda c: c.name[:60])
def test_each_refusal_is_reached_by_a_named_input(case):
    rc, state, _ = lenient(case)
    assert rc == case.status, (DECODE_STATUS[rc], DECODE_STATUS[case.status])
    assert not state.tobytes().strip(b"\0")
    if case.status in (L.SYNTAX, L.TRAILING) and "depth 33" not in case.name:  # (nesting beyond 32 is JSON: the limit is the decoder's own)
        with pytest.raises(ValueError):  # json.loads refuses them too (JSONDecodeError is a ValueError)
            L.document(case.value)
    if case.status == L.MISSING:
        assert L.expected_row(case.template, L.document(case.value), case.key) is None


def test_a_value_cut_after_any_byte_is_refused():
    cuts = [c for c in L.corpus() if c.status == L.REFUSED]
    assert len(cuts) == len(L.LONG)
    seen = set()
    for case in cuts:
        rc = lenient(case)[0]
        assert rc != 0, case.name
        seen.add(rc)
    assert {L.SYNTAX, L.STRING} <= seen
    whole = next(c for c in L.corpus() if c.name == "the long case")
    rc, state, _ = lenient(whole)
    assert rc == 0 and int(state["count"][0]) == -17 and int(state["version"][0]) == 42


def test_null_is_refused_with_the_status_of_the_kind():
    tmpl = JsonTemplate((b'{"k":', "KEY", b',"a":', (JP_I32, 0), b',"b":', (JP_U32, 4), b',"c":', (JP_I64, 8), b',"d":', (JP_F64, 16), b',"s":', (6, 0), b"}"))
    good = {"k": b'"id"', "a": b"-1", "b": b"4294967295", "c": b"-9223372036854775808", "d": b"0.5", "s": b'"x"'}
    text = lambda m: L.text_of([(k.encode(), v) for k, v in m.items()])  # noqa: E731
    rc, st, _ = decode_state_host(tmpl, text(good), "id", lenient=True)
    assert rc == 0 and int(st["count"][0]) == -1 and st.tobytes()[8:16] == (-2 ** 63).to_bytes(8, "little", signed=True)
    for name, status in (("k", L.STRING), ("a", L.INT), ("b", L.INT), ("c", L.INT), ("d", L.NUMBER), ("s", L.STRING)):
        assert decode_state_host(tmpl, text(dict(good, **{name: b"null"})), "id", lenient=True)[0] == status, name
    for name, value in (("a", b"2147483648"), ("b", b"-1"), ("b", b"4294967296"), ("c", b"9223372036854775808")):
        assert decode_state_host(tmpl, text(dict(good, **{name: value})), "id", lenient=True)[0] == L.RANGE, (name, value)


# ---- the envelope -----------------------------------------------------------------------------------------------------------
def test_enveloped_values_read_as_their_payload_does_with_spans_relative_to_the_value():
    cases = L.envelope_cases()
    lengths = {len(c.value) - c.payload_at for c in cases}
    assert {127, 128, 16383, 16384} <= lengths
    n_ok = 0
    for case in cases:
        rc, state, spans = lenient(case)
        if case.status >= 0:
            assert rc == case.status, (case.name, DECODE_STATUS[rc])
        if rc == 0:
            n_ok += 1
            held_to_the_document(case, L.document(case.value[case.payload_at:]), rc, state, spans)
    assert n_ok > 60


# ---- mutations --------------------------------------------------------------------------------------------------------------
_NUMBER = re.compile(rb"[+-]?[0-9][0-9+\-.eE]*")


def known_number_rule(text: bytes) -> bytes:
    """``text`` with every number outside a string re-spelled without a leading ``+`` and without leading zeros.  A member the
    template names is read by the strict mode's routine for its kind: the integer rule ``-?[0-9]+`` and the Double parser
    take leading zeros (``007``), and the Double parser a leading ``+``, as they always have (tests/number_text_cases.py
    holds such spellings, and the strict mode's values must read the same in the lenient mode).  ``json.loads`` does not.
    This is the whole difference in what is accepted: a mutated text that ``json.loads`` refuses is looked at once more
    spelled this way before the decoder is held to refusing it."""
    out, i = bytearray(), 0
    while i < len(text):
        if text[i:i + 1] == b'"':
            j = i + 1
            while j < len(text) and text[j:j + 1] != b'"':
                j += 2 if text[j:j + 1] == b"\\" else 1
            out += text[i:j + 1]
            i = j + 1
            continue
        m = _NUMBER.match(text, i)
        if m and (i == 0 or text[i - 1:i] not in b"0123456789.eE+-"):
            tok = m.group()
            sign = b"-" if tok[:1] == b"-" else b""
            body = tok[1:] if tok[:1] in b"+-" else tok
            digits = re.match(rb"[0-9]+", body).group()
            out += sign + (digits.lstrip(b"0") or b"0") + body[len(digits):]
            i = m.end()
            continue
        out += text[i:i + 1]
        i += 1
    return bytes(out)


def test_the_known_number_rule_is_what_it_says():
    assert known_number_rule(b'{"a":007,"b":+1.5,"c":-00,"s":"+01","d":[0,10,1e+05]}') == b'{"a":7,"b":1.5,"c":-0,"s":"+01","d":[0,10,1e+05]}'


def test_seeded_mutations_never_decode_what_json_loads_refuses_and_decode_the_rest_to_its_document():
    base = [c for c in L.corpus() if c.status == L.OK and len(c.value) < 4000] + [c for c in L.envelope_cases() if c.status == L.OK and len(c.value) < 4000]
    muts = L.mutations(base, 12)
    assert len(muts) > 3000
    refused_by_both = accepted_by_both = refused_by_us_alone = respelled = 0
    for case in muts:
        rc, state, spans = lenient(case)
        text = case.value[case.payload_at:] if case.envelope else case.value
        if case.envelope and rc == L.ENVELOPE:
            continue  # (the mutation hit the envelope: its grammar is pinned by tests/test_state_envelope.py)
        try:
            members = L.document(text)
        except (ValueError, RecursionError):
            try:
                members = L.document(known_number_rule(text))
                respelled += 1
            except (ValueError, RecursionError):
                assert rc != 0, (case.name, case.value)
                refused_by_both += 1
                continue
        if rc == 0:
            held_to_the_document(case, members, rc, state, spans)
            accepted_by_both += 1
        else:
            refused_by_us_alone += 1  # a surrogate in a known string, a fraction for an Int, a field gone, another id, ...
    print(f"{len(muts)} mutations: {refused_by_both} refused by both, {accepted_by_both} decoded to json.loads' document, "
          f"{refused_by_us_alone} refused by the decoder alone, {respelled} read with the known-number rule")
    assert refused_by_both > 500 and accepted_by_both > 200


# ---- the superset property --------------------------------------------------------------------------------------------------
def both_modes_agree_where_strict_accepts(template, value, key, envelope="none"):
    rc, state, spans = decode_state_host(template, value, key, envelope=envelope)
    if rc != 0:
        return False
    rc2, state2, spans2 = decode_state_host(template, value, key, envelope=envelope, lenient=True)
    assert rc2 == 0 and state2.tobytes() == state.tobytes() and spans2 == spans, (value[:200], DECODE_STATUS[rc2])
    return True


def test_every_value_the_strict_mode_accepts_reads_the_same_in_the_lenient_mode():
    n = 0
    units = state_topic_gen.make_topic(seed=3, n_ids=120, n_records=600)
    for part in units:
        for _, key, value in state_topic_gen.concat(part)[1]:
            if value:
                n += both_modes_agree_where_strict_accepts(L.COUNTER, value, key)
    units, _ = state_strings_gen.make_topic(seed=4, n_ids=80, n_records=400)
    for part in units:
        for _, key, value in state_strings_gen.concat(part)[1]:
            if value:
                n += both_modes_agree_where_strict_accepts(L.BANK, value, key)
    assert n > 800
    n_env = n_padded = 0
    for case in envelope_cases.corpus():
        if isinstance(case.template.parts[-1], bytes) and case.template.parts[-1] != b"}":
            # the encoder's length cases pad the payload with a constant member inside the last literal: not a shape the field
            # table describes, and refused as such
            with pytest.raises(ValueError, match="lenient"):
                decode_state_host(case.template, case.value, case.key, envelope="protobuf_state", lenient=True)
            n_padded += 1
            continue
        n_env += both_modes_agree_where_strict_accepts(case.template, case.value, case.key, "protobuf_state")
    assert n_env > 30 and n_padded <= 12
    state = JsonTemplate((b'{"k":', "KEY", b',"v":', (JP_F64, 16), b"}"))
    n_num = 0
    for text in numbers.decimal_texts()[::7] + numbers.long_texts():
        n_num += both_modes_agree_where_strict_accepts(state, b'{"k":"id","v":' + text.encode() + b"}", "id")
    ints = JsonTemplate((b'{"a":', (JP_I32, 0), b',"b":', (JP_U32, 4), b',"c":', (JP_I64, 8), b"}"))
    for a in numbers.integer_texts("I32"):
        for b, c in zip(numbers.integer_texts("U32"), numbers.integer_texts("I64")):
            n_num += both_modes_agree_where_strict_accepts(ints, f'{{"a":{a},"b":{b},"c":{c}}}'.encode(), None)
    assert n_num > 3500
    print(f"{n} topic values, {n_env} enveloped values and {n_num} number spellings read the same in both modes")


# ---- the field table --------------------------------------------------------------------------------------------------------
def test_the_shipped_templates_are_all_usable():
    from fixture_models import SdkBankAccount, sdk_sample_state_bytes

    for tmpl, value, key in ((JsonTemplate.counter(), b'{"version":2,"count":1,"aggregateId":"a"}', "a"),
                             (JsonTemplate.bank_account(), b'{"balance":1,"securityCode":"","accountOwner":"","accountNumber":"a"}', "a"),
                             (L.SDK, b' {"balance":1}', None), (envelope_cases.SDK, b'{"balance" :1}', None)):
        assert decode_state_host(tmpl, value, key, lenient=True)[0] == 0
    assert decode_state_host(L.SDK, sdk_sample_state_bytes("k1", SdkBankAccount(5)), "k1", envelope="protobuf_state", lenient=True)[0] == 0


@pytest.mark.parametrize("parts", [
    (b'{"a":1}',),                                                  # one literal and no value
    (b'{"a":', (JP_I32, 0)),                                        # an even number of parts
    (b'{"a":', (JP_I32, 0), (JP_I32, 4), b"}", b"}"),               # two values in a row
    (b'{"a" :', (JP_I32, 0), b"}"),                                 # a space in the first literal
    (b'"a":', (JP_I32, 0), b"}"),                                   # no opening brace
    (b'{"":', (JP_I32, 0), b"}"),                                   # an empty name
    (b'{"a\\"b":', (JP_I32, 0), b"}"),                              # a name with a backslash and a quote
    (b'{"a":', (JP_I32, 0), b', "b":', (JP_I32, 4), b"}"),          # a space in an inner literal
    (b'{"a":', (JP_I32, 0), b'{"b":', (JP_I32, 4), b"}"),           # an inner literal that opens another object
    (b'{"a":', (JP_I32, 0), b',"a":', (JP_I32, 4), b"}"),           # the same name twice
    (b'{"a":', (JP_I32, 0), b"} "),                                 # a last literal that is more than the brace
    (b'{"a":', (JP_I32, 0), b"]"),
    (b"balance=", (JP_I32, 0), b"\n"),                              # no JSON at all
], ids=lambda p: repr(p[0])[:16] + f"~{len(p)}")
def test_a_template_of_another_shape_is_unsupported_in_lenient_mode_only(parts):
    lib = _native.load()
    t = JsonTemplate(parts).to_c()
    state, span = (ctypes.c_uint8 * 64)(), (ctypes.c_int64 * 8)()
    for fn in (lib.surge_decode_json_state_lenient, lib.surge_decode_protobuf_state_lenient):
        assert fn(ctypes.byref(t), b"{}", 2, None, -1, state, span) == -5  # SURGE_E_UNSUPPORTED
    assert lib.surge_decode_json_state(ctypes.byref(t), b"{}", 2, None, -1, state, span) >= 0  # consistent: the strict mode reads it
    with pytest.raises(ValueError, match="lenient"):
        decode_state_host(JsonTemplate(parts), b"{}", lenient=True)


def test_seven_fields_fit_and_an_inconsistent_template_stays_invalid():
    parts = []
    for i in range(7):
        parts += [(b"{" if i == 0 else b",") + b'"f%d":' % i, (JP_I32, 4 * i)]
    seven = JsonTemplate(tuple(parts) + (b"}",))
    rc, st, _ = decode_state_host(seven, b'{"f6":6,"f5":5,"f4":4,"f3":3,"f2":2,"f1":1,"f0":-1}', lenient=True)
    assert rc == 0 and np.frombuffer(st.tobytes()[:28], dtype="<i4").tolist() == [-1, 1, 2, 3, 4, 5, 6]
    lib = _native.load()
    bad = CJsonTemplate()
    bad.n_parts = 17
    state = (ctypes.c_uint8 * 64)()
    assert lib.surge_decode_json_state_lenient(ctypes.byref(bad), b"{}", 2, None, -1, state, None) == -1  # SURGE_E_INVALID, as the strict export
    assert lib.surge_decode_json_state_lenient(None, b"{}", 2, None, -1, state, None) == -1
    t = seven.to_c()
    assert lib.surge_decode_json_state_lenient(ctypes.byref(t), None, 2, None, -1, state, None) == -1
    assert lib.surge_decode_json_state_lenient(ctypes.byref(t), b"{}", 2, None, -1, None, None) == -1


# ---- the C surface ----------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_listed_and_exported():
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "surge_replay.h")).read()
    defines = dict(re.findall(r"#define (SURGE_STATE_\w+)\s+(\d+)", header))
    assert defines["SURGE_STATE_DECODE_SYNTAX"] == "12" and defines["SURGE_STATE_DECODE_MISSING"] == "13"
    assert defines["SURGE_STATE_READ_STRICT"] == "0" and defines["SURGE_STATE_READ_LENIENT"] == "1"
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in _native.REPLAY_H
        assert (name in _native.STATE_EXPORTS) == name.startswith("surge_decode_")
        assert (name in _native.EXPORTS) == name.startswith("surge_replay_")
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in surge_replay.h"
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int32 and fn.argtypes
    assert lib.surge_decode_json_state_lenient.argtypes == lib.surge_decode_json_state.argtypes
    assert lib.surge_decode_protobuf_state_lenient.argtypes == lib.surge_decode_protobuf_state.argtypes
    assert DECODE_STATUS[12] == "SYNTAX" and DECODE_STATUS[13] == "MISSING"


def test_the_mode_setter_checks_its_arguments_without_a_device():
    lib = _native.load()
    assert lib.surge_replay_set_decode_mode(None, 0) == -1  # SURGE_E_INVALID: no handle
    assert lib.surge_replay_set_decode_mode(None, 1) == -1
    assert lib.surge_replay_set_decode_mode(None, 2) == -1


def test_the_python_layers_take_the_option_and_default_to_strict():
    import inspect

    from surge_amd.encode import decode_states
    from surge_amd.ingest import DeviceDecoder
    from surge_amd.replay import ReplayEngine
    from surge_amd.store import GpuReplayStateStore

    for fn in (decode_state_host, decode_states, ReplayEngine.decoding_onto, DeviceDecoder.load_states_into, GpuReplayStateStore.restore_from_state_records,
               GpuReplayStateStore.restore_from_state_topic):
        assert inspect.signature(fn).parameters["lenient"].default is False, fn.__qualname__
    assert decode_state_host(L.COUNTER, b'{"count":1,"version":2,"aggregateId":"a"}', "a")[0] == 1  # LITERAL: the default is the strict mode


# ---- the sanitizer program --------------------------------------------------------------------------------------------------
def test_no_prefix_or_mutation_makes_the_lenient_parser_read_outside_the_value_under_asan_and_ubsan(tmp_path):
    """tests/cpp/state_lenient_prefixes.cpp: every prefix and seeded mutations of lenient texts, bare and enveloped, each copied
    into a malloc of exactly its length, through both lenient exports built with -fsanitize=address,undefined — a stand-alone
    program, nothing of it is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "state_lenient_prefixes")
    srcs = [os.path.join(ROOT, "tests", "cpp", "state_lenient_prefixes.cpp")] + [os.path.join(ROOT, "surge_amd", "csrc", f) for f in ("state_decode_host.cpp", "f64_text.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]
