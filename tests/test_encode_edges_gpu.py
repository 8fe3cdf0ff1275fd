"""-m gpu: json_encode_kernel, its length scan and the protobuf envelope (state_kernels.hip) at the edges their code
branches on, through ``surge_replay_encode_json`` / ``surge_replay_encode_protobuf_state`` with an output buffer of the
test's own: ``lead + total + 64`` bytes of 0xA5, the output ``lead`` bytes in, ``capacity = total`` exactly (the
``encode_states`` wrapper over-allocates and slices, which hides both the capacity rule and an overrun).  The bytes, the
n + 1 offsets and the not-a-number count equal ``state_out_cases``' reference, and the bytes around the output are untouched.

The states get on the device as in test_snapshot_delta_gpu.py: a log of empty segments over a ``prior``, so every state
byte is the test's."""
import ctypes

import numpy as np
import pytest

import state_out_cases as c
from surge_amd import schema as S
from surge_amd.encode import JsonTemplate
from surge_amd.replay import ReplayEngine

pytestmark = pytest.mark.gpu

E_UNSUPPORTED, E_RANGE = -5, -6
FILL = 0xA5
EMPTY = np.zeros(0, dtype=S.EVENT_DTYPE)


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


def table(items, n):
    """``(data, off)`` numpy arrays of a list of byte strings (``None``: n empty ones)."""
    off = np.zeros(n + 1, dtype=np.int64)
    if items is None:
        return np.zeros(0, np.uint8), off
    assert len(items) == n
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), off


def encode(eng, case, reference, lead=0, filter=None):
    """Run one case and compare everything; returns the status of the call with the exact capacity."""
    import torch

    dev = f"cuda:{eng.device}"
    lib = eng._lib
    text, off, nan = reference
    n = case.states.shape[0]
    total = len(text)
    assert off.shape == (n + 1,) and off[-1] == total
    eng.load_csr(np.zeros(n + 1, dtype=np.int64), EMPTY, case.states.view(S.STATE_DTYPE).reshape(n))
    eng.fold()
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
    d_keys, d_key_off = (up(a) for a in table(case.keys, n))
    cols = [tuple(up(a) for a in table(col, n)) for col in case.strings]
    for k in range(4):
        eng._check(lib.surge_replay_set_encode_strings(eng._h, k, ptr(cols[k][0]) if k < len(cols) else None,
                                                       ptr(cols[k][1]) if k < len(cols) else None))
    d_filter = None if filter is None else up(np.ascontiguousarray(filter, dtype=np.uint8))
    eng._check(lib.surge_replay_set_encode_filter(eng._h, None if d_filter is None else ptr(d_filter)))
    fn = lib.surge_replay_encode_protobuf_state if case.envelope else lib.surge_replay_encode_json
    t = JsonTemplate(case.template).to_c()
    try:
        # capacity 0: the exact total, SURGE_E_RANGE (unless nothing is emitted), and not a byte written
        probe = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
        d_off = torch.full((n + 2,), -1, dtype=torch.int64, device=dev)
        got_total = ctypes.c_int64(-1)
        rc = fn(eng._h, ctypes.byref(t), ptr(d_keys), ptr(d_key_off), ptr(probe), 0, ptr(d_off), ctypes.byref(got_total))
        assert got_total.value == total
        assert rc == (E_RANGE if total else (E_UNSUPPORTED if nan else 0))
        assert (probe.cpu().numpy() == FILL).all()
        # capacity = total, the output `lead` bytes behind a 16-byte boundary
        buf = torch.full((lead + total + 64,), FILL, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        got_total = ctypes.c_int64(-1)
        rc = fn(eng._h, ctypes.byref(t), ptr(d_keys), ptr(d_key_off), ctypes.c_void_p(buf.data_ptr() + lead), total, ptr(d_off),
                ctypes.byref(got_total))
        message = (lib.surge_replay_last_error(eng._h) or b"").decode()
    finally:
        lib.surge_replay_set_encode_filter(eng._h, None)
    assert got_total.value == total
    if nan:
        assert rc == E_UNSUPPORTED and message.startswith(f"{nan} aggregate(s) hold a NaN / infinite Double"), message
    else:
        assert rc == 0, message
    got_off = d_off.cpu().numpy()
    bad = np.nonzero(got_off[:n + 1] != off)[0]
    assert bad.size == 0, f"{bad.size} offsets differ, first at {bad[0]}: got {got_off[bad[0]]}, expected {off[bad[0]]}"
    assert got_off[n + 1] == -1
    out = buf.cpu().numpy()
    assert (out[:lead] == FILL).all(), "bytes before the output were written"
    assert (out[lead + total:] == FILL).all(), "bytes behind the output were written"
    got = out[lead:lead + total].tobytes()
    if got != text:
        at = next(i for i in range(total) if got[i] != text[i])
        a = int(np.searchsorted(off, at, side="right")) - 1
        raise AssertionError(f"byte {at} (aggregate {a}, block {a // 256}) differs: got {got[max(at - 20, 0):at + 20]!r}, expected {text[max(at - 20, 0):at + 20]!r}")
    return rc


SHIFT = c.shift_cases()
TINY = c.tiny_block_cases()
STAGE = c.stage_threshold_cases()
INTEGER = c.integer_cases()
ESCAPE = c.escape_cases()
ENVELOPE = c.envelope_cases()
name = lambda case: case.name  # noqa: E731


@pytest.mark.parametrize("lead", [0, 1, 7, 15])
@pytest.mark.parametrize("case", SHIFT, ids=name)
def test_a_block_starts_at_every_byte_of_a_16_byte_word(eng, case, lead):
    # shift = (output pointer + block base) mod 16: the block's text residue and the pointer's own alignment both move it
    encode(eng, case, case.reference(), lead)


@pytest.mark.parametrize("case", TINY, ids=name)
def test_blocks_shorter_than_a_word_and_blocks_that_emit_nothing(eng, case):
    encode(eng, case, case.reference())


@pytest.mark.parametrize("lead", [0, 1, 7, 15])
@pytest.mark.parametrize("case", STAGE, ids=name)
def test_both_sides_of_the_staging_threshold_give_the_same_bytes(eng, case, lead):
    encode(eng, case, case.reference(), lead)


@pytest.mark.parametrize("case", INTEGER, ids=name)
def test_integer_parts_at_the_ends_of_their_types_and_every_power_of_ten(eng, case):
    encode(eng, case, case.reference())


@pytest.mark.parametrize("case", ESCAPE, ids=name)
def test_every_ascii_byte_in_keys_and_string_columns(eng, case):
    encode(eng, case, case.reference())


@pytest.mark.parametrize("case", ENVELOPE, ids=name)
def test_envelope_varints_at_one_two_and_three_bytes(eng, case):
    encode(eng, case, case.reference())


@pytest.mark.parametrize("n", c.SCAN_SIZES)
def test_length_scan_up_to_two_block_totals_per_thread(eng, n):
    # more than 1024 x 1024 aggregates: scan_totals_kernel gives every thread two block totals, the last range cut by nb
    case = c.scan_case(n)
    text, off = c.i32_only_reference(case.states)
    encode(eng, case, (text, off, 0))


def test_filter_lets_only_value_aggregates_emit(eng):
    case = SHIFT[5]
    n = case.states.shape[0]
    kinds = np.array([c.SKIP, c.VALUE, c.TOMBSTONE], dtype=np.uint8)[np.arange(n) % 3]
    reference = case.reference(filter=kinds)
    assert 0 < reference[1][-1] < case.reference()[1][-1] and (np.diff(reference[1])[kinds != c.VALUE] == 0).all()
    encode(eng, case, reference, filter=kinds)


def test_not_a_number_counts_only_what_the_filter_lets_through(eng):
    (case,) = c.escape_cases()
    n = case.states.shape[0]
    c.put(case.states[3:4], 16, [float("nan")], "<f8")
    c.put(case.states[10:11], 16, [float("-inf")], "<f8")
    kinds = np.full(n, c.VALUE, dtype=np.uint8)
    kinds[10], kinds[20], kinds[21] = c.SKIP, c.TOMBSTONE, c.SKIP
    reference = case.reference(filter=kinds)
    assert reference[2] == 1 and case.reference()[2] == 2
    assert encode(eng, case, reference, filter=kinds) == E_UNSUPPORTED
