"""tests/state_out_cases.py on the CPU: every builder has the property it is named for, read from the reference's own
offsets -- without this the GPU tests could pass without reaching the branch they are about --, and the references
themselves are tied to the oracle, the fixtures' writeState, ``json.loads`` and the protobuf runtime, so that they cannot
be bent to the kernel."""
import json
import re

import numpy as np
import pytest

import state_out_cases as c
from oracle import oracle


def test_constants_are_the_packages():
    from surge_amd import encode, schema

    assert (c.JP_LITERAL, c.JP_KEY, c.JP_I32, c.JP_U32, c.JP_I64, c.JP_F64, c.JP_STR) == (
        encode.JP_LITERAL, encode.JP_KEY, encode.JP_I32, encode.JP_U32, encode.JP_I64, encode.JP_F64, encode.JP_STR)
    assert (c.PRESENT, c.POISONED) == (schema.STATE_PRESENT, schema.STATE_POISONED)
    assert c.FLAGS_AT == schema.STATE_DTYPE.fields["flags"][1]
    assert c.COUNTER == tuple(encode.JsonTemplate.counter().parts) and c.BANK_ACCOUNT == tuple(encode.JsonTemplate.bank_account().parts)
    for case in c.integer_cases() + c.envelope_cases() + c.escape_cases():
        encode.JsonTemplate(case.template).to_c()  # within 16 parts and the 256-byte literal pool


# ---- the delta --------------------------------------------------------------------------------------------------------------
def plain_kind(now, base, full64):
    span = 64 if full64 else 40
    fl = int.from_bytes(bytes(now[36:40]), "little")
    if bytes(now[:span]) == bytes(base[:span]) or fl & 2:
        return 0
    return 1 if fl & 1 else 2


@pytest.mark.parametrize("full64", [False, True])
def test_delta_kinds_equals_a_plain_loop_over_the_transition_table(full64):
    base, now, labels = c.delta_cases(full64, np.random.default_rng(3))
    words = 16 if full64 else 10
    assert len(labels) == 4 * words + 32 and base.shape == now.shape == (len(labels), 64)
    if not full64:
        assert not base[:, 40:].any() and not now[:, 40:].any()  # v1 keeps the tail zero: no row differs there only
    for baseline in (base, c.committed(np.zeros_like(base), base, c.delta_kinds(base, np.zeros_like(base), full64)[0])):
        kind, nv, nt = c.delta_kinds(now, baseline, full64)
        want = [plain_kind(now[a], baseline[a], full64) for a in range(len(labels))]
        assert kind.tolist() == want and (nv, nt) == (want.count(1), want.count(2))
        assert {0, 1, 2} == set(want)
    # the single-bit rows: exactly one bit differs, in the word and byte the label names, both PRESENT; every word is met
    seen = set()
    for a in range(4 * words):
        diff = np.unpackbits(base[a] ^ now[a])
        assert diff.sum() == 1
        byte = int(np.nonzero(base[a] ^ now[a])[0][0])
        assert labels[a] == f"bit word {byte // 4} byte {byte % 4}"
        assert c.flags_of(base[a:a + 1])[0] & 3 == 1 and c.flags_of(now[a:a + 1])[0] & 3 == 1
        assert c.delta_kinds(now[a:a + 1], base[a:a + 1], full64)[0][0] == c.VALUE
        seen.add((byte // 4, "edge" if byte % 4 in (0, 3) else "middle"))
    assert {w for w, _ in seen} == set(range(words)) and all((w, "middle") in seen for w in range(words))
    # a poisoned first state is never committed: its baseline stays what it was
    k0 = c.delta_kinds(base, np.zeros_like(base), full64)[0]
    poisoned = (c.flags_of(base) & 2) != 0
    assert poisoned.any() and (k0[poisoned] == 0).all() and not c.committed(np.zeros_like(base), base, k0)[poisoned].any()
    assert (c.invalidated(base, k0)[k0 != 0] == 0xFF).all() and (c.invalidated(base, k0)[k0 == 0] == base[k0 == 0]).all()


def test_mutate_flips_one_compared_bit_and_keeps_the_two_flags():
    rng = np.random.default_rng(4)
    for full64 in (False, True):
        st = c.random_rows(5000, rng, full64)
        idx = np.unique(rng.integers(0, 5000, size=900))
        out = c.mutate(st, idx, rng, full64)
        changed = np.nonzero((st != out).any(axis=1))[0]
        assert changed.tolist() == idx.tolist()
        assert (np.unpackbits(st[idx] ^ out[idx], axis=1).sum(axis=1) == 1).all()
        assert ((c.flags_of(st) & 3) == (c.flags_of(out) & 3)).all()
        assert full64 or not out[:, 40:].any()
        assert (st[:, 36] != out[:, 36]).any()  # the flags word is among the mutated ones


# ---- the encoder's reference, tied to its four witnesses -------------------------------------------------------------------
def test_reference_equals_the_oracle_and_the_fixtures_on_the_escape_cases():
    from fixture_models import BankAccount, BankAccountFormat, CounterAggregateFormat, State

    (case,) = c.escape_cases()
    owners, codes = case.strings
    n = len(case.keys)
    assert {b for k in case.keys for b in k} >= case.prop["bytes"]
    for col_byte in range(0x80):  # every byte once in a string column (beside the marker letters)
        assert sum(s.count(bytes([col_byte])) for col in case.strings for s in col[:0x80]) >= 1
    assert b"" in case.keys and b"" in owners and b"" in codes
    assert any(k and all(b < 0x20 and len(c.JACKSON[b]) == 6 for b in k) for k in case.keys)
    assert any(len(ch.encode()) == w for w in (2, 3, 4) for k in case.keys + owners + codes for ch in k.decode())
    # BankAccount: the fixture's writeState.  Python's json.dumps writes \u00xx in lower case where Jackson (and the
    # fixture's own jackson_quote, and the oracle) write upper case: the fixture's text is compared with those six-byte
    # escapes upper-cased, nothing else touched
    text, off, nan = case.reference()
    assert nan == 0 and off[0] == 0 and off[-1] == len(text)
    fmt = BankAccountFormat()
    upper = lambda b: re.sub(rb"\\u00[0-9a-f]{2}", lambda m: m.group(0)[:2] + m.group(0)[2:].upper(), b)  # noqa: E731
    for a in range(n):
        got = text[off[a]:off[a + 1]]
        bal = float(np.frombuffer(case.states[a, 16:24].tobytes(), "<f8")[0])
        want = fmt.write_state(BankAccount(case.keys[a].decode(), owners[a].decode(), codes[a].decode(), bal)).value
        assert got == upper(want), (a, got, want)
        back = json.loads(got)
        assert back["accountNumber"] == case.keys[a].decode() and back["accountOwner"] == owners[a].decode()
        assert back["securityCode"] == codes[a].decode() and float(back["balance"]) == bal
    # Counter over the same keys: the oracle's C writer (it takes a C string: the keys without a NUL) and the fixture
    st = c.rows(n)
    rng = np.random.default_rng(8)
    c.put(st, 0, rng.integers(-2 ** 31, 2 ** 31, size=n), "<i4")
    c.put(st, 4, rng.integers(-2 ** 31, 2 ** 31, size=n), "<i4")
    c.put(st, c.FLAGS_AT, [c.PRESENT] * n, "<u4")
    text, off, _ = c.encode_reference(c.COUNTER, st, case.keys)
    fmt = CounterAggregateFormat()
    through_oracle = 0
    for a in range(n):
        got = text[off[a]:off[a + 1]]
        count, version = (int(x) for x in np.frombuffer(st[a, 0:8].tobytes(), "<i4"))
        key = case.keys[a].decode()
        assert got == fmt.write_state(State(key, count, version)).value
        if "\x00" not in key:
            through_oracle += 1
            assert got == oracle.counter_state_json(key, count, version)
        assert json.loads(got) == {"aggregateId": key, "count": count, "version": version}
    assert through_oracle >= n - 3


def test_reference_filter_presence_and_not_a_number_rules():
    st = c.rows(6)
    c.put(st, 16, [1.5, float("nan"), float("inf"), 2.5, float("-inf"), 3.5], "<f8")
    c.put(st, c.FLAGS_AT, [1, 1, 1, 0, 3, 3], "<u4")
    keys = [b"a", b"b", b"c", b"d", b"e", b"f"]
    cols = ([b""] * 6, [b""] * 6)
    text, off, nan = c.encode_reference(c.BANK_ACCOUNT, st, keys, cols)
    assert nan == 2 and np.diff(off).astype(bool).tolist() == [True, False, False, False, False, False]  # poisoned ones do not count
    text, off, nan = c.encode_reference(c.BANK_ACCOUNT, st, keys, cols, filter=np.array([2, 1, 0, 1, 1, 1], np.uint8))
    assert nan == 1 and text == b"" and off.tolist() == [0] * 7
    assert json.loads(c.encode_reference(c.BANK_ACCOUNT, st, keys, cols, filter=np.array([1, 0, 0, 0, 0, 0], np.uint8))[0])["balance"] == 1.5


def test_i32_only_reference_equals_the_per_aggregate_reference():
    for n in (1, 1023, 1025, 2600):
        case = c.scan_case(n)
        text, off, nan = c.encode_reference(c.I32_ONLY, case.states, [b""] * n)
        vt, voff = c.i32_only_reference(case.states)
        assert nan == 0 and vt == text and voff.tolist() == off.tolist()
    st = c.rows(len(c.I32_VALUES))
    c.put(st, 0, c.I32_VALUES, "<i4")
    c.put(st, c.FLAGS_AT, [c.PRESENT] * len(c.I32_VALUES), "<u4")
    vt, voff = c.i32_only_reference(st)
    assert vt == "".join(map(str, c.I32_VALUES)).encode() and np.diff(voff).tolist() == [len(str(v)) for v in c.I32_VALUES]


# ---- every builder has its property ----------------------------------------------------------------------------------------
def spans_of(case, lead=0):
    return c.block_spans(case.reference()[1], lead)


def test_shift_cases_start_block_one_at_every_residue():
    cases = c.shift_cases()
    assert len(cases) == 16
    for r, case in enumerate(cases):
        assert case.states.shape == (512, 64) and case.template == c.COUNTER
        (b0, e0, s0), (b1, e1, s1) = spans_of(case)
        assert (b0, s0) == (0, 0) and e0 % 16 == r == case.prop["residue"] and s1 == r and e1 > b1 + 16
        assert all(c.copy_shape(*sp)[0] for sp in spans_of(case))  # staged
        assert [s for _, _, s in spans_of(case, lead=7)] == [7, (7 + r) % 16]
        fl = c.flags_of(case.states)
        assert (fl == 0).any() and (fl == 3).any()  # None and poisoned aggregates lie between the emitting ones


def test_tiny_block_cases_reach_both_branches_of_the_copy():
    cases = {case.name: case for case in c.tiny_block_cases()}
    shapes = set()
    for name, case in cases.items():
        assert case.template == c.I32_ONLY and case.states.shape == (768, 64)
        (b0, e0, _), (b1, e1, s1), (b2, e2, _) = spans_of(case)
        assert e0 - b0 == 256 + case.prop["start"] and s1 == case.prop["start"] and e1 - b1 == case.prop["total"] and e2 > b2
        staged, body_lo, body_hi = c.copy_shape(b1, e1, s1)
        assert staged
        present = (c.flags_of(case.states[256:512]) & 1).sum()
        if name.startswith(("tiny", "straddle")):
            assert present == 1 and 1 <= e1 - b1 <= 11
        if case.prop["inside_one_word"]:
            assert s1 + (e1 - b1) <= 16
        else:
            assert s1 + (e1 - b1) > 16 and (name == "aligned_17" or e1 - b1 < 16)
        shapes.add("gt" if body_lo > body_hi else "eq" if body_lo == body_hi else "body")
    assert shapes == {"gt", "eq", "body"}
    assert {case.prop["start"] for name, case in cases.items() if name.startswith("tiny")} == set(range(16))
    assert {case.prop["total"] for name, case in cases.items() if name.startswith("tiny")} >= {1, 2, 5, 10, 11}
    # the straddling blocks: head and tail bytes but no 16-byte body; the one-word blocks behind residue 0: no head
    for name in ("straddle_s12_l8", "straddle_s15_l11", "straddle_s9_l11", "straddle_s15_l2"):
        _, lo, hi = c.copy_shape(*spans_of(cases[name])[1])
        assert lo == hi == 16
    assert c.copy_shape(*spans_of(cases["tiny_s5_l1"])[1])[1:] == (16, 0)
    b, e, s = spans_of(cases["exact_word"])[1]
    assert (b % 16, e - b, s) == (0, 16, 0) and c.copy_shape(b, e, s)[1:] == (0, 16)
    for name in ("silent_block_s0", "silent_block_s5"):
        (b0, e0, _), (b1, e1, _), (b2, e2, _) = spans_of(cases[name])
        assert e0 > b0 and e1 == b1 and e2 > b2 and not (c.flags_of(cases[name].states[256:512]) & 1).any()


def test_stage_threshold_cases_sit_on_the_threshold():
    cases = c.stage_threshold_cases()
    assert sorted((x.prop["sum"], x.prop["shift"]) for x in cases) == sorted((s, sh) for s in (32767, 32768, 32769, 32768 + 4096) for sh in (0, 15))
    for case in cases:
        (b0, e0, s0), (b1, e1, s1), (b2, e2, s2) = spans_of(case)
        assert s1 == case.prop["shift"] and (e1 - b1) + s1 == case.prop["sum"]
        assert c.copy_shape(b1, e1, s1)[0] == (case.prop["sum"] <= c.STAGE_BYTES)
        assert c.copy_shape(b0, e0, s0)[0] and c.copy_shape(b2, e2, s2)[0] and e0 - b0 > 1000 and e2 - b2 > 1000
        key = case.keys[case.prop["long_at"]]
        assert {len(c.JACKSON[b]) for b in key} == {1, 2, 6} and len(key) > 8000
        assert sum(len(k) > 100 for k in case.keys) == 1 and 256 <= case.prop["long_at"] < 512


def test_integer_cases_hold_the_stated_values_at_the_stated_offsets():
    for vals, lo, hi in ((c.I32_VALUES, -2 ** 31, 2 ** 31 - 1), (c.U32_VALUES, 0, 2 ** 32 - 1), (c.I64_VALUES, -2 ** 63, 2 ** 63 - 1)):
        assert {0, lo, hi} <= set(vals) and all(lo <= v <= hi for v in vals)
        p = 1
        while p <= hi:
            assert {p, p - 1} <= set(vals) and (lo == 0 or {-p, -(p - 1)} <= set(vals))
            p *= 10
    a, b, d = c.integer_cases()
    text, off, nan = d.reference()
    lines = [[int(x) for x in text[off[i]:off[i + 1]].split(b",")] for i in range(len(off) - 1)]
    assert nan == 0 and [line[0] for line in lines] == c.I32_VALUES  # the whole I32 list at offset 32 ...
    assert sorted(line[1] for line in lines) == sorted(v & ~3 | 1 for v in c.I32_VALUES)  # ... and, but for its two flag bits, at 36
    assert all(line[2] == line[0] % 2 ** 32 for line in lines)
    text, off, nan = a.reference()
    lines = [text[off[i]:off[i + 1]].split(b",") for i in range(len(off) - 1)]
    assert nan == 0 and a.prop["offsets"] == [0, 4, 8, 12, 16, 20, 24, 28]
    for j in range(8):  # every value at every offset
        assert sorted(int(line[j]) for line in lines) == c.I32_VALUES
    text, off, nan = b.reference()
    lines = [[int(x) for x in text[off[i]:off[i + 1]].split(b",")] for i in range(len(off) - 1)]
    assert nan == 0 and all(len(line) == 4 for line in lines)
    assert [line[3] for line in lines] == c.I64_VALUES
    assert set(c.U32_VALUES) == {line[2] for line in lines} and {2 ** 32 - 1, 2 ** 31, 10 ** 9} <= set(c.U32_VALUES)
    assert all(line[0] == (line[2] if line[2] < 2 ** 31 else line[2] - 2 ** 32) for line in lines) and any(line[0] == -1 for line in lines)
    flag_words = {line[1] for line in lines}  # the word at 36: PRESENT set, POISONED clear, every magnitude and both signs
    assert all(w & 3 == 1 for w in flag_words) and min(flag_words) == -2 ** 31 + 1 and max(flag_words) >= 2 ** 31 - 3
    assert {len(str(abs(w))) for w in flag_words} == set(range(1, 11))


def test_envelope_cases_have_the_stated_id_and_payload_lengths():
    State = c.protobuf_state_class()
    seen = set()
    for case in c.envelope_cases():
        assert case.envelope and "KEY" not in case.template and case.states.shape[0] < 3000
        text, off, nan = case.reference()
        assert nan == 0
        assert len({a // 256 for a in case.prop["at"]}) == len(case.prop["at"])  # one measured aggregate per block
        for a, idlen, plen in zip(case.prop["at"], case.prop["ids"], case.prop["payloads"]):
            msg = State.FromString(text[off[a]:off[a + 1]])
            assert len(msg.aggregateId.encode()) == idlen == len(case.keys[a]) and len(msg.payload) == plen
            assert msg.payload.startswith(b'{"v":') and json.loads(msg.payload)["v"] == int.from_bytes(case.states[a, 8:16].tobytes(), "little")
            varint = lambda v: 1 if v < 128 else 2 if v < 16384 else 3  # noqa: E731
            assert off[a + 1] - off[a] == (1 + varint(idlen) + idlen if idlen else 0) + 1 + varint(plen) + plen
            seen.add((idlen, plen))
    assert seen == {(i, p) for i in (0, 127, 128, 16383, 16384) for p in (127, 128, 16383, 16384)}


def test_scan_cases_reach_two_totals_per_thread():
    assert c.SCAN_SIZES == (1023, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, 1024 * 1024 + 1025)
    want = {1023: (1, 1), 1024: (1, 1), 1025: (2, 1), 1024 * 1024: (1024, 1), 1024 * 1024 + 1: (1025, 2), 1024 * 1024 + 1025: (1026, 2)}
    for n in c.SCAN_SIZES[:3] + (c.SCAN_SIZES[-1],):
        case = c.scan_case(n)
        assert (case.prop["nb"], case.prop["per"]) == want[n] and case.states.shape == (n, 64) and case.template == c.I32_ONLY
        absent = (c.flags_of(case.states) == 0).mean()
        assert 0.2 < absent < 0.3
    # nb = 1026, per = 2: thread 512 holds the last two totals, thread 513's range starts at nb and every later one beyond it
    nb, per = want[c.SCAN_SIZES[-1]]
    assert 512 * per < nb == 513 * per and 1023 * per > nb
