"""The host half of the state decoder (``surge_decode_json_state``): serialized state text -> the fixed 64-byte state.

It is the parser the device kernel runs (``surge_amd/csrc/state_parse.h``), so what is pinned here — round trips against
the encoders' text, the integer and Double rules, every refusal — is what the GPU tests hold the kernel to."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle
from surge_amd import schema as S
from surge_amd.encode import (DECODE_AMBIGUOUS, DECODE_ESCAPE, DECODE_INT, DECODE_KEY_MISMATCH, DECODE_LITERAL, DECODE_NUMBER, DECODE_OK,
                              DECODE_RANGE, DECODE_STRING, DECODE_SURROGATE, DECODE_TRAILING, JP_F64, JP_I32, JP_I64, JP_U32, JsonTemplate,
                              decode_state_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIRD_IDS = ['we"ird\\id', "tab\there\nnl", "ünï-✓-ключ", "\x01\x1f"]  # the ids of the encoder test (test_gpu_parity.py)
COUNTER, BANK = JsonTemplate.counter(), JsonTemplate.bank_account()
COUNTER_TEXT = b'{"aggregateId":"agg-\\u00e9\\n","count":-12,"version":34}'
BANK_TEXT = b'{"accountNumber":"a-1","accountOwner":"J \\"q\\" \\/ \\u20ac","securityCode":"","balance":-1.25E+3}'


def bank_text(balance: str, key="k", owner='"Jane"', code='"1234"') -> bytes:
    return f'{{"accountNumber":"{key}","accountOwner":{owner},"securityCode":{code},"balance":{balance}}}'.encode()


def test_counter_text_of_both_writers_decodes_to_the_exact_fields_with_and_without_key_comparison():
    from fixture_models import CounterAggregateFormat, State

    fmt = CounterAggregateFormat()
    for key in WEIRD_IDS + ["agg-00001", ""]:
        for count, version in ((0, 0), (-7, 3), (2**31 - 1, -(2**31)), (-(2**31), 2**31 - 1)):
            texts = {oracle.counter_state_json(key, count, version), fmt.write_state(State(key, count, version)).value}
            for text in texts:
                for k in (key, None):
                    rc, st, _ = decode_state_host(COUNTER, text, k)
                    assert rc == DECODE_OK, (text, k, rc)
                    want = np.zeros(1, dtype=S.STATE_DTYPE)
                    want["count"], want["version"], want["flags"] = count, version, S.STATE_PRESENT
                    assert st.tobytes() == want.tobytes()  # every byte the template does not name is zero
    # \uXXXX for any BMP code point, '/' escaped or not: the same id
    rc, _, _ = decode_state_host(COUNTER, COUNTER_TEXT, "agg-é\n")
    assert rc == DECODE_OK
    assert decode_state_host(COUNTER, b'{"aggregateId":"\\u20ac\\/\\u0041","count":1,"version":1}', "€/A")[0] == DECODE_OK


def test_one_flipped_key_byte_is_a_key_mismatch():
    for key in WEIRD_IDS + ["agg-00001"]:
        text = oracle.counter_state_json(key, 1, 2)
        kb = bytearray(key.encode("utf-8"))
        for i in range(len(kb)):
            flipped = bytes(kb[:i]) + bytes([kb[i] ^ 1]) + bytes(kb[i + 1:])
            assert decode_state_host(COUNTER, text, flipped)[0] == DECODE_KEY_MISMATCH
        assert decode_state_host(COUNTER, text, bytes(kb) + b"x")[0] == DECODE_KEY_MISMATCH
        assert decode_state_host(COUNTER, text, bytes(kb[:-1]))[0] == DECODE_KEY_MISMATCH
        assert decode_state_host(COUNTER, text, bytes(kb))[0] == DECODE_OK


def test_integers_at_and_one_past_every_range_and_the_forms_the_event_decoders_integer_rule_refuses():
    tmpl = JsonTemplate((b'{"a":', (JP_I32, 0), b',"b":', (JP_U32, 4), b',"c":', (JP_I64, 8), b"}"))

    def dec(a, b, c):
        rc, st, _ = decode_state_host(tmpl, f'{{"a":{a},"b":{b},"c":{c}}}'.encode())
        return rc, int(st["count"][0]), int(st["version"].view(np.uint32)[0]), int(st["sum64"][0])

    assert dec(-(2**31), 0, -(2**63)) == (DECODE_OK, -(2**31), 0, -(2**63))
    assert dec(2**31 - 1, 2**32 - 1, 2**63 - 1) == (DECODE_OK, 2**31 - 1, 2**32 - 1, 2**63 - 1)
    assert dec("-0", "-0", "007") == (DECODE_OK, 0, 0, 7)  # accepted by parse_i32 (event_decode.cpp) as well
    for a, b, c in ((2**31, 0, 0), (-(2**31) - 1, 0, 0), (0, 2**32, 0), (0, -1, 0), (0, 0, 2**63), (0, 0, -(2**63) - 1),
                    (0, 0, 2**64), (0, 0, 10**30), (10**12, 0, 0)):
        assert dec(a, b, c)[0] == DECODE_RANGE, (a, b, c)  # reported, never wrapped
    for bad in ("+5", "1.0", "1.5", "1e3", "1E3", "", "-", "- 1", "1-", "1+1", ".5", "null", '"1"', " 1"):
        assert dec(bad, 0, 0)[0] == DECODE_INT, bad
        assert dec(0, 0, bad)[0] == DECODE_INT, bad
    for text in ("1 ", "0x10"):  # a complete integer, then not the template's next literal (the event decoder's token ends there too)
        assert dec(text, 0, 0)[0] == DECODE_LITERAL


def _bank_account_bit_patterns(n, seed=21):
    # drawn as test_gpu_json_encoder_writes_bank_account_states_with_play_json_double_text draws its balances
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 6, size=n)
    vals = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4],
                     [np.round(rng.random(n) * 1e7) / 100, rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.float64),
                      rng.random(n) * 10.0 ** rng.integers(-12, 25, size=n), rng.standard_normal(n) * 1e3,
                      rng.choice([0.0, -0.0, 1e20, 1e-7, 5e-324, 1.7976931348623157e308, 0.1 + 0.2, 1e21, 100.0], size=n)],
                     default=rng.integers(0, 0x7FF0000000000000, size=n, dtype=np.uint64).view(np.float64))
    return vals


def test_doubles_written_as_play_json_writes_them_decode_to_the_same_bits():
    tmpl = JsonTemplate((b'{"balance":', (JP_F64, 16), b"}"))
    specials = [5e-324, 1.7976931348623157e308, 0.1 + 0.2, 1e21, 1e-7, 0.0, 1e20, 100.0, 2.2250738585072014e-308, -1.5]
    values = list(_bank_account_bit_patterns(20000)) + specials
    assert len(values) >= 20000
    for x in values:
        x = float(x)
        text = oracle.play_json_double_text(x)
        rc, st, _ = decode_state_host(tmpl, b'{"balance":' + text.encode() + b"}")
        assert rc == DECODE_OK, (x, text, rc)
        want = np.float64(0.0 if x == 0 else x).view(np.uint64)  # the one exception: -0.0 is written as 0 and reads back as +0.0
        assert st["balance"].view(np.uint64)[0] == want, (x, text)
    assert oracle.play_json_double_text(1e-7) == "1E-7"  # (the spelling the issue names)
    assert oracle.play_json_double_text(-0.0) == "0"
    rc, st, _ = decode_state_host(tmpl, b'{"balance":0}')
    assert rc == DECODE_OK and st["balance"].view(np.uint64)[0] == 0
    # a spelled-out minus zero keeps its sign; other spellings of a number give the same bits
    assert decode_state_host(tmpl, b'{"balance":-0.0}')[1]["balance"].view(np.uint64)[0] == 1 << 63
    for text, v in (("1.1E+3", 1100.0), ("1100", 1100.0), ("1100.000", 1100.0), ("-2.5e-3", -0.0025), ("1E400", float("inf"))):
        assert decode_state_host(tmpl, b'{"balance":' + text.encode() + b"}")[1]["balance"][0] == v


def test_a_double_the_fast_algorithm_cannot_decide_comes_back_as_strtod_reads_it():
    import ctypes

    from surge_amd import _native

    tmpl = JsonTemplate((b'{"balance":', (JP_F64, 16), b"}"))
    lib = _native.load()
    # more than 19 significant digits (the 55-digit case of the parser's own test) and the exact decimal of a double's
    # upper neighbour's midpoint: Eisel-Lemire reports both as undecided (surge_parse_f64_json returns 1: strtod decided)
    for text in ("0.1000000000000000055511151231257827021181583404541015625", "9007199254740993.00000000000000000001",
                 "123456789012345678901234567890"):
        bits = ctypes.c_uint64()
        assert lib.surge_parse_f64_json(text.encode(), len(text), ctypes.byref(bits)) == 1
        rc, st, _ = decode_state_host(tmpl, b'{"balance":' + text.encode() + b"}")
        assert rc == DECODE_OK  # never AMBIGUOUS from the host export
        assert st["balance"].view(np.uint64)[0] == bits.value == np.float64(float(text)).view(np.uint64)


def test_every_proper_prefix_is_refused_and_one_more_byte_is_trailing():
    for tmpl, text, key in ((COUNTER, COUNTER_TEXT, "agg-é\n"), (BANK, BANK_TEXT, "a-1")):
        assert decode_state_host(tmpl, text, key)[0] == DECODE_OK
        for cut in range(len(text)):
            for k in (key, None):
                rc = decode_state_host(tmpl, text[:cut], k)[0]
                assert rc not in (DECODE_OK, DECODE_AMBIGUOUS), (text[:cut], rc)
        for extra in (b" ", b"}", b"\x00", b"\n"):
            assert decode_state_host(tmpl, text + extra, key)[0] == DECODE_TRAILING


def test_str_parts_report_the_raw_span_between_the_quotes():
    rc, st, spans = decode_state_host(BANK, BANK_TEXT, "a-1")
    assert rc == DECODE_OK and st["balance"][0] == -1250.0
    (o0, l0), (o1, l1) = spans[0], spans[1]
    assert json.loads(b'"' + BANK_TEXT[o0:o0 + l0] + b'"') == 'J "q" / €' and l1 == 0 and BANK_TEXT[o1 - 1:o1 + 1] == b'""'


NAMED_INPUTS = {
    "OK": (COUNTER, COUNTER_TEXT, "agg-é\n", DECODE_OK),
    "LITERAL (a wrong byte in a field name)": (COUNTER, COUNTER_TEXT.replace(b'"count"', b'"cound"'), None, DECODE_LITERAL),
    "LITERAL (whitespace the compact form never has)": (COUNTER, COUNTER_TEXT.replace(b"-12,", b"-12 ,"), None, DECODE_LITERAL),
    "STRING (no opening quote)": (COUNTER, b'{"aggregateId":agg,"count":1,"version":1}', None, DECODE_STRING),
    "STRING (a raw control character)": (COUNTER, b'{"aggregateId":"a\tb","count":1,"version":1}', None, DECODE_STRING),
    "STRING (unterminated)": (COUNTER, b'{"aggregateId":"abc', None, DECODE_STRING),
    "ESCAPE (\\x)": (COUNTER, b'{"aggregateId":"a\\x41","count":1,"version":1}', None, DECODE_ESCAPE),
    "ESCAPE (\\u with a non-hex digit)": (COUNTER, b'{"aggregateId":"a\\u00g1","count":1,"version":1}', None, DECODE_ESCAPE),
    "SURROGATE": (COUNTER, b'{"aggregateId":"\\ud83d\\ude00","count":1,"version":1}', None, DECODE_SURROGATE),
    "KEY_MISMATCH": (COUNTER, COUNTER_TEXT, "agg-e\n", DECODE_KEY_MISMATCH),
    "INT": (COUNTER, COUNTER_TEXT.replace(b"-12", b"-12.0"), None, DECODE_INT),
    "RANGE": (COUNTER, COUNTER_TEXT.replace(b"34", b"2147483648"), None, DECODE_RANGE),
    "NUMBER (no digits)": (BANK, bank_text("-"), None, DECODE_NUMBER),
    "NUMBER (null)": (BANK, bank_text("null"), None, DECODE_NUMBER),
    "NUMBER (bare fraction point)": (BANK, bank_text("1."), None, DECODE_NUMBER),
    "TRAILING": (BANK, bank_text("1") + b"}", None, DECODE_TRAILING),
}


@pytest.mark.parametrize("name", sorted(NAMED_INPUTS))
def test_each_status_is_reached_by_a_named_input(name):
    tmpl, text, key, want = NAMED_INPUTS[name]
    rc, st, _ = decode_state_host(tmpl, text, key)
    assert rc == want, (name, text, rc)
    if want != DECODE_OK:
        assert st.tobytes() == bytes(64)  # state64_out is written only for a value that decodes
    assert {v[3] for v in NAMED_INPUTS.values()} == {DECODE_OK, DECODE_LITERAL, DECODE_STRING, DECODE_ESCAPE, DECODE_KEY_MISMATCH, DECODE_INT,
                                                     DECODE_RANGE, DECODE_NUMBER, DECODE_TRAILING, DECODE_SURROGATE}


def test_an_inconsistent_template_is_refused_before_any_byte_is_read():
    with pytest.raises(ValueError):
        decode_state_host(JsonTemplate((b"{", (JP_I64, 60), b"}")), b"{1}")  # outside the 64-byte state
    with pytest.raises(ValueError):
        decode_state_host(JsonTemplate((b"{", (JP_I32, 36), b"}")), b"{1}")  # the flags word is the decoder's
    with pytest.raises(ValueError):
        decode_state_host(JsonTemplate((b"{", (JP_F64, 20), b"}")), b"{1}")  # misaligned


def test_no_prefix_or_mutation_makes_the_parser_read_outside_the_value_under_asan_and_ubsan(tmp_path):
    """tests/cpp/state_parse_prefixes.cpp: every prefix and a few thousand mutations of valid Counter / BankAccount texts, each
    copied into a malloc of exactly its length, through the export built with -fsanitize=address,undefined — a stand-alone
    program, nothing of it is loaded into this process."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "state_parse_prefixes")
    srcs = [os.path.join(ROOT, "tests", "cpp", "state_parse_prefixes.cpp")] + [os.path.join(ROOT, "surge_amd", "csrc", f) for f in ("state_decode_host.cpp", "f64_text.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]
