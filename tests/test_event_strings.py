"""The host half of the string fields of events (``include/surge_ingest.h``, "the STRING fields of events"):
``surge_event_json_string_spans`` — the rule the device pass of ``ingest_strings.hip`` runs, ``event_strings_parse.h`` — against
``json.loads`` on the corpus of ``tests/event_strings_cases.py``, ``surge_event_strings_validate`` on every refusal it names, and a
stand-alone sanitizer run over every prefix of every corpus value."""
import json
import os
import shutil
import struct
import subprocess

import pytest

import event_strings_cases as esc
from surge_amd.encode import unescape_json_string
from surge_amd.ingest import ARG_NONE, EVENT_STRING_ABSENT, EVENT_STRING_OK, EventJsonTemplate, EventStrings, IngestError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spans_of(case):
    template, strings = esc.RULES[case.rule]
    return template.string_spans(strings, case.value)


def check(case):
    rc, spans, status = spans_of(case)
    assert rc == (-7 if case.refused else 0), case.name
    for c, want in enumerate(case.want):
        if want is None:
            assert status[c] == EVENT_STRING_ABSENT, (case.name, c)
        elif isinstance(want, int):
            assert status[c] == want, (case.name, c, status)
        else:
            off, n = spans[c]
            assert status[c] == EVENT_STRING_OK and 0 <= off and off + n <= len(case.value), (case.name, c, status)
            assert case.value[off - 1:off] == b'"' and case.value[off + n:off + n + 1] == b'"', case.name  # the bytes between the quotes
            assert unescape_json_string(case.value[off:off + n]) == want.encode("utf-8"), (case.name, c)


@pytest.mark.parametrize("group", ["escape_cases", "dumped_cases", "position_cases", "envelope_cases", "refused_cases"])
def test_the_host_export_gives_what_json_loads_reads_and_refuses_what_is_named(group):
    cases = getattr(esc, group)()
    assert len(cases) >= 10
    for case in cases:
        check(case)


def test_the_corpus_covers_what_it_says():
    cases = esc.all_cases()
    values = [c.value for c in cases]
    assert any(len(v) == 16 for v in values)
    assert any(b"\\u" in v for v in values) and any(max(v, default=0) >= 0xF0 for v in values)
    refusals = {w for c in cases for w in c.want if isinstance(w, int)}
    assert refusals == {esc.DECODE_STRING, esc.DECODE_ESCAPE, esc.DECODE_SURROGATE, esc.EVENT_STRING_MISSING, esc.EVENT_STRING_RECORD}
    assert {c.rule for c in cases} == set(esc.RULES)
    # the enveloped ones are the protobuf runtime's bytes: it reads back the payload the spans point into
    for c in esc.envelope_cases():
        rid, payload = esc.eec.runtime_fields(c.value)
        assert rid == c.key and c.value.endswith(payload)


def test_an_accepted_value_is_one_the_event_decoder_decodes_and_its_class_is_the_decoders():
    for case in esc.accepted_cases():
        template, _ = esc.RULES[case.rule]
        ev = template.decode(case.value)  # (raises where the event decoder refuses: the rule's class is that decoder's)
        names_owner = case.want[0] is not None or case.want[2] is not None or case.want[3] is not None
        if case.rule.startswith("bank"):
            assert int(ev["type"]) == (0 if names_owner else 1), case.name


def test_mutated_values_are_refused_or_give_spans_that_unescape_as_json_reads_them():
    ok = refused = compared = decoded = 0
    for case in esc.mutations(esc.accepted_cases() + esc.refused_cases(), per_case=4):
        template, strings = esc.RULES[case.rule]
        rc, spans, status = spans_of(case)
        assert rc in (0, -7)
        refused += rc != 0
        try:  # the walk restates the event decoder's grammar: what that decoder accepts, the walk reads as an event too
            template.decode(case.value)
            decoded += 1
            assert esc.EVENT_STRING_RECORD not in status, case.value
        except IngestError:
            pass  # (the decoder also refuses for its own fields, a missing balance: the walk does not judge those)
        for c in range(4):
            if status[c] != EVENT_STRING_OK:
                continue
            off, n = spans[c]
            assert 0 < off and off + n < len(case.value) and case.value[off - 1:off] == b'"' and case.value[off + n:off + n + 1] == b'"'
            got = unescape_json_string(case.value[off:off + n])  # (raises where the span is not a string the rule accepts)
            ok += 1
            if case.rule != "bank":
                continue
            try:  # where Python reads the value as an object without duplicates, short enough for the rule, it reads the same string
                pairs = json.loads(case.value, object_pairs_hook=list)
            except Exception:
                continue
            names = [k for k, _ in pairs] if isinstance(pairs, list) and all(isinstance(p, tuple) for p in pairs) else None
            field = ("accountOwner", "securityCode")[c] if c < 2 else None
            if names and field and len(names) <= 24 and len(set(names)) == len(names) and b"\\u00" not in case.value and field in names:
                v = dict(pairs)[field]
                if isinstance(v, str):
                    assert got == v.encode("utf-8"), case.name
                    compared += 1
    assert ok > 200 and refused > 200 and compared > 100 and decoded > 150


# ---- surge_event_strings_validate ------------------------------------------------------------------------------------------
def test_validate_accepts_the_fixtures_and_refuses_every_input_it_names():
    for template, strings in esc.RULES.values():
        strings.validate(template)
    created = esc.CREATED
    refusals = {
        "a type name the event template does not have": EventStrings([("docs.command.BankAccountClosed", "accountOwner", 0)]),
        "a string column out of range": EventStrings([(created, "accountOwner", 4)]),
        "the same (type, column) named twice": EventStrings([(created, "accountOwner", 1), (created, "securityCode", 1)]),
        "an empty field name": EventStrings([(created, "", 0)]),
        "strings.n out of range": EventStrings([]),
    }
    for reason, strings in refusals.items():
        with pytest.raises(ValueError, match="event strings: " + reason.replace("(", r"\(").replace(")", r"\)")):
            strings.validate(esc.BANK)
        with pytest.raises(ValueError):
            esc.BANK.string_spans(strings, esc.created(b"x"))
    EventStrings([(created, "accountOwner", 1), (esc.UPDATED, "securityCode", 1)]).validate(esc.BANK)  # the same column from two classes is allowed
    EventStrings([(created, "f%d" % i, i % 4) for i in range(4)] + [(esc.UPDATED, "g%d" % i, i % 4) for i in range(4)]).validate(esc.BANK)
    with pytest.raises(ValueError):
        EventStrings([(created, "f", 0)] * 17).to_c()
    with pytest.raises(ValueError, match="discriminator"):  # a template that does not validate itself
        EventStrings([("a", "f", 0)]).validate(EventJsonTemplate("", [("a", 0, "", "", ARG_NONE), ("b", 1, "", "", ARG_NONE)]))
    with pytest.raises((ValueError, IngestError)):
        EventStrings([("", "o", 0)]).validate(esc.BANK)  # "" is no type name of a template with a discriminator


# ---- the sanitizer run ---------------------------------------------------------------------------------------------------------
def test_no_prefix_or_mutation_makes_the_walk_read_outside_its_value_under_asan_and_ubsan(tmp_path):
    """tests/cpp/event_strings_prefixes.cpp: every prefix of every corpus value and the seeded mutations, each in a malloc of
    exactly its length, through the export built with -fsanitize=address,undefined — a stand-alone program that reads the
    corpus from a file; nothing of it is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    rules = sorted(esc.RULES)
    corpus = str(tmp_path / "corpus.bin")
    cases = esc.all_cases()
    with open(corpus, "wb") as f:
        for c in cases + esc.mutations(cases, per_case=3):
            mutated = c.want == ["?"]
            want = [0xFF] * 4 if mutated else [EVENT_STRING_ABSENT if w is None else w if isinstance(w, int) else EVENT_STRING_OK for w in c.want]
            f.write(struct.pack("<BBI4B", rules.index(c.rule), 0 if mutated else 1, len(c.value), *want) + c.value)
    exe = str(tmp_path / "event_strings_prefixes")
    srcs = [os.path.join(ROOT, "tests", "cpp", "event_strings_prefixes.cpp")] + [os.path.join(ROOT, "surge_amd", "csrc", f) for f in ("event_decode.cpp", "f64_text.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]
