"""-m gpu: the state encoders over a row list (``surge_replay_encode_json_rows`` / ``_protobuf_state_rows``: json_encode_kernel's
ROWS instantiations, state_kernels.hip) — output ``q`` is the text of aggregate ``rows[q]``, in query order.

The states are the test's own, written into the resident state as tests/test_encode_edges_gpu.py writes them (a log of empty
segments over a prior snapshot).  What a slot must hold is the text Python writes for that aggregate (``state_out_cases``'
reference, per aggregate) — and, once, the pre-existing full encoder's output sliced at the row; its kind follows from the
flags word the test wrote.  The output lies between guard bytes with ``capacity`` exact, so both the capacity rule and an
overrun show."""
import ctypes
import struct

import numpy as np
import pytest

import state_out_cases as c
from surge_amd import encode
from surge_amd import schema as S
from surge_amd.encode import JsonTemplate
from surge_amd.replay import ReplayEngine, ReplayError

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_RANGE = -1, -5, -6
MISS, VALUE, NONE, POISONED, NOT_A_NUMBER = 0, 1, 2, 3, 4
FILL = 0xA5
EMPTY = np.zeros(0, dtype=S.EVENT_DTYPE)


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


def table(items, n):
    off = np.zeros(n + 1, dtype=np.int64)
    if items is None:
        return np.zeros(0, np.uint8), off
    np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), off


class Loaded:
    """One case resident on the device: its states, key table and string columns, with what each aggregate must read as."""

    def __init__(self, eng, case):
        import torch

        self.eng, self.case = eng, case
        self.dev = f"cuda:{eng.device}"
        n = self.n = case.states.shape[0]
        eng.load_csr(np.zeros(n + 1, dtype=np.int64), EMPTY, case.states.view(eng.state_dtype).reshape(n))
        eng.fold()
        up = self.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.d_keys, self.d_key_off = (up(a) for a in table(case.keys, n))
        self.cols = [tuple(up(a) for a in table(col, n)) for col in case.strings]
        text, off, _ = case.reference()
        self.texts = [text[off[a]:off[a + 1]] for a in range(n)]  # what Python writes for each aggregate
        fl = c.flags_of(case.states)
        finite = np.ones(n, dtype=bool)
        for p in case.template:
            if isinstance(p, tuple) and p[0] == c.JP_F64:
                finite &= np.isfinite(np.ascontiguousarray(case.states[:, p[1]:p[1] + 8]).view("<f8").reshape(-1))
        self.kinds = np.where(fl & c.POISONED, POISONED, np.where((fl & c.PRESENT) == 0, NONE, np.where(finite, VALUE, NOT_A_NUMBER))).astype(np.uint8)
        assert all((len(t) > 0) == (k == VALUE) for t, k in zip(self.texts, self.kinds))

    def want(self, rows):
        texts = [self.texts[a] if 0 <= a < self.n else b"" for a in rows]  # (a row outside the state never gets that far)
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            np.cumsum([len(t) for t in texts], out=off[1:])
        kinds = np.array([self.kinds[a] if 0 <= a < self.n else MISS for a in rows], dtype=np.uint8)
        return b"".join(texts), off, kinds

    def call(self, rows, capacity=None, lead=0):
        """One call with ``capacity`` (default: exactly what the rows need) and the output ``lead`` bytes behind a 16-byte
        boundary.  -> (status, total, the whole guarded buffer, out_off with one guard entry, kinds with one guard entry)"""
        import torch

        lib, eng = self.eng._lib, self.eng
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
        for k in range(4):
            eng._check(lib.surge_replay_set_encode_strings(eng._h, k, ptr(self.cols[k][0]) if k < len(self.cols) else None,
                                                           ptr(self.cols[k][1]) if k < len(self.cols) else None))
        n = len(rows)
        need = len(self.want(rows)[0])
        capacity = need if capacity is None else capacity
        buf = torch.full((lead + max(capacity, need) + 64,), FILL, dtype=torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        d_off = torch.full((n + 2,), -7, dtype=torch.int64, device=self.dev)
        d_kind = torch.full((n + 1,), 0xEE, dtype=torch.uint8, device=self.dev)
        d_rows = self.up(np.asarray(rows, dtype=np.int64)) if n else None
        total = ctypes.c_int64(-1)
        fn = lib.surge_replay_encode_protobuf_state_rows if self.case.envelope else lib.surge_replay_encode_json_rows
        t = JsonTemplate(self.case.template).to_c()
        rc = fn(eng._h, ctypes.byref(t), ptr(self.d_keys), ptr(self.d_key_off), ptr(d_rows), n, ctypes.c_void_p(buf.data_ptr() + lead), capacity, ptr(d_off),
                ptr(d_kind), ctypes.byref(total))
        self.message = (lib.surge_replay_last_error(eng._h) or b"").decode()
        return rc, total.value, buf.cpu().numpy(), d_off.cpu().numpy(), d_kind.cpu().numpy()

    def check(self, rows, lead=0, status=0):
        rows = [int(a) for a in rows]
        text, off, kinds = self.want(rows)
        n, need = len(rows), len(text)
        rc, total, out, got_off, got_kind = self.call(rows, lead=lead)
        assert rc == status, self.message
        assert total == need
        assert got_off[0] == 0 and (np.diff(got_off[:n + 1]) >= 0).all() and got_off[n + 1] == -7
        bad = np.nonzero(got_off[:n + 1] != off)[0]
        assert bad.size == 0, f"{bad.size} offsets differ, first at slot {bad[0]}: got {got_off[bad[0]]}, expected {off[bad[0]]}"
        assert got_kind[:n].tolist() == kinds.tolist() and got_kind[n] == 0xEE
        assert (out[:lead] == FILL).all(), "bytes before the output were written"
        assert (out[lead + need:] == FILL).all(), "bytes behind the output were written"
        got = out[lead:lead + need].tobytes()
        if got != text:
            at = next(i for i in range(need) if got[i] != text[i])
            q = int(np.searchsorted(off, at, side="right")) - 1
            raise AssertionError(f"byte {at} (slot {q}, row {rows[q]}, block {q // 256}) differs: got {got[max(at - 20, 0):at + 20]!r}, expected {text[max(at - 20, 0):at + 20]!r}")


@pytest.fixture(scope="module")
def counters():
    """512 Counter aggregates, an eighth None, a few poisoned, resident on an engine of their own (the other tests load theirs
    into ``eng``)."""
    with ReplayEngine() as own:
        ld = Loaded(own, c.shift_cases()[3])
        assert {VALUE, NONE, POISONED} <= set(ld.kinds.tolist())
        yield ld


def test_identity_reversed_duplicates_misses_and_a_mix(counters):
    ld = counters
    n = ld.n
    ld.check(range(n))
    ld.check(range(n - 1, -1, -1))
    ld.check([7] * 300 + [8, 7, 8] * 20)
    ld.check([-1] * 300)
    rng = np.random.default_rng(1)
    value, none, poisoned = (np.flatnonzero(ld.kinds == k) for k in (VALUE, NONE, POISONED))
    mix = np.concatenate([rng.choice(value, 150), rng.choice(none, 60), rng.choice(poisoned, 30), np.full(60, -1)])
    rng.shuffle(mix)
    ld.check(mix)


def test_the_full_encoder_sliced_at_the_row_is_what_a_slot_holds(counters):
    """The pre-existing ``encode_states`` over every aggregate, sliced, against ``encode.encode_rows`` (the wrapper, with its
    capacity retry: the first guess of 128 bytes a row is too small for nothing here, so a hint of 1 byte forces it)."""
    ld = counters
    out, off = encode.encode_states(ld.eng, JsonTemplate(ld.case.template), ld.d_keys, ld.d_key_off)
    full, off = out.cpu().numpy().tobytes(), off.cpu().numpy()
    rng = np.random.default_rng(2)
    rows = rng.integers(-1, ld.n, size=700)
    got, got_off, kind = encode.encode_rows(ld.eng, JsonTemplate(ld.case.template), ld.d_keys, ld.d_key_off, ld.up(rows), capacity_hint=1)
    got, got_off, kind = got.cpu().numpy().tobytes(), got_off.cpu().numpy(), kind.cpu().numpy()
    for q, a in enumerate(rows.tolist()):
        assert got[got_off[q]:got_off[q + 1]] == (full[off[a]:off[a + 1]] if a >= 0 else b"")
        assert kind[q] == (ld.kinds[a] if a >= 0 else MISS)
    assert got_off[0] == 0 and got_off[-1] == len(got)


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257, 513])
def test_row_counts_around_a_block(counters, n_rows):
    rng = np.random.default_rng(n_rows)
    rows = rng.integers(-1, counters.n, size=n_rows)
    if n_rows > 1:
        rows[-1] = rows[0] = int(np.flatnonzero(counters.kinds == VALUE)[3])  # the first and the last slot emit
    counters.check(rows)


@pytest.mark.parametrize("lead", range(16))
def test_the_output_at_each_of_the_16_alignments(counters, lead):
    rng = np.random.default_rng(100 + lead)
    counters.check(rng.integers(-1, counters.n, size=300 + lead), lead=lead)


@pytest.mark.parametrize("want,lead", [(c.STAGE_BYTES, 0), (c.STAGE_BYTES + 1, 0), (c.STAGE_BYTES, 15), (c.STAGE_BYTES + 4096, 7)])
def test_a_block_of_rows_on_either_side_of_the_lds_stage(eng, want, lead):
    """One id long enough that its block of 256 rows is exactly at, or beyond, what the 32 KiB stage takes: the row list decides
    which rows share a block, so the long id is asked for among other rows' slots too."""
    case = next(k for k in c.stage_threshold_cases() if k.prop["sum"] == want and k.prop["shift"] == 0)
    ld = Loaded(eng, case)
    long_at = case.prop["long_at"]
    ld.check(range(ld.n), lead=lead)  # the blocks of the full encoder: block 1 holds the long id and sums to `want`
    rng = np.random.default_rng(want)
    rows = rng.integers(0, ld.n, size=600)
    rows[300] = rows[301] = long_at  # block 1 of the row list holds the long id twice: beyond the stage, straight to global
    ld.check(rows, lead=lead)
    sums = [len(ld.want([int(a) for a in rows[q0:q0 + 256]])[0]) for q0 in range(0, 600, 256)]
    assert sums[1] > c.STAGE_BYTES and sums[0] + 16 <= c.STAGE_BYTES and sums[2] + 16 <= c.STAGE_BYTES  # both paths in one call
    rows[300], rows[40], rows[41] = 0, long_at, long_at  # twice in block 0
    ld.check(rows, lead=lead)


def test_one_byte_short_is_range_with_the_total_and_nothing_written(counters):
    ld = counters
    rows = [int(a) for a in np.flatnonzero(ld.kinds == VALUE)[:40]] + [-1, 3]
    need = len(ld.want(rows)[0])
    rc, total, out, off, kind = ld.call(rows, capacity=need - 1, lead=5)
    assert rc == E_RANGE and total == need
    assert (out == FILL).all() and (off == -7).all() and (kind == 0xEE).all()
    rc, total, out, off, kind = ld.call(rows, capacity=0)
    assert rc == E_RANGE and total == need and (out == FILL).all()
    ld.check(rows, lead=5)  # and with the room it asked for, the call works


@pytest.mark.parametrize("bad", ["n_agg", -2, 1 << 40, -(1 << 40)])
def test_a_row_outside_the_state_is_invalid_and_nothing_is_written(counters, bad):
    ld = counters
    bad = ld.n if bad == "n_agg" else bad
    rows = [int(a) for a in np.flatnonzero(ld.kinds == VALUE)[:300]]
    rows[271] = bad
    rc, total, out, off, kind = ld.call(rows, capacity=1 << 16)
    assert rc == E_INVALID and "outside" in ld.message
    assert (out == FILL).all() and (off == -7).all() and (kind == 0xEE).all()
    rows[271] = ld.n - 1  # the last row is a row
    ld.check(rows)


def test_a_nan_row_is_not_a_number_and_the_call_says_unsupported(eng):
    (case,) = c.escape_cases()
    c.put(case.states[3:4], 16, [float("nan")], "<f8")
    c.put(case.states[10:11], 16, [float("-inf")], "<f8")
    ld = Loaded(eng, case)
    assert ld.kinds[3] == ld.kinds[10] == NOT_A_NUMBER
    ld.check([5, 3, 6, -1, 10, 3, 7], status=E_UNSUPPORTED)
    assert ld.message.startswith("3 row(s) name an aggregate that holds a NaN / infinite Double")
    ld.check([5, 6, 7, 11])  # no such row asked for: nothing to report
    with pytest.raises(ReplayError) as ei:
        encode.encode_rows(eng, JsonTemplate(case.template), ld.d_keys, ld.d_key_off, ld.up(np.array([3, 4], dtype=np.int64)), strings=ld.cols)
    assert ei.value.status == E_UNSUPPORTED


def test_the_encode_filter_is_not_consulted(counters):
    ld = counters
    lib = ld.eng._lib
    kinds = ld.up(np.array([c.SKIP, c.VALUE, c.TOMBSTONE], dtype=np.uint8)[np.arange(ld.n) % 3])
    ld.eng._check(lib.surge_replay_set_encode_filter(ld.eng._h, ctypes.c_void_p(kinds.data_ptr())))
    try:
        ld.check(range(ld.n))  # rows the filter excludes are served all the same
        out, off = encode.encode_states(ld.eng, JsonTemplate(ld.case.template), ld.d_keys, ld.d_key_off)
        filtered = ld.case.reference(filter=kinds.cpu().numpy())
        assert out.cpu().numpy().tobytes() == filtered[0] and len(filtered[0]) < len(ld.case.reference()[0])  # ... while the full encoder still obeys it
    finally:
        lib.surge_replay_set_encode_filter(ld.eng._h, None)


def test_the_protobuf_envelope_at_the_steps_of_the_id_varint(eng):
    case = c.envelope_cases()[0]  # ids of 0, 127, 128, 16383 and 16384 bytes, one per block, payloads of 127 bytes
    ld = Loaded(eng, case)
    at, ids = case.prop["at"], case.prop["ids"]
    assert {127, 128} <= set(ids)
    rows = at[::-1] + [-1] + at + [int(a) for a in np.flatnonzero(ld.kinds == VALUE)[:40]]
    ld.check(rows)
    rc, _, out, off, kind = ld.call(rows)
    assert rc == 0
    State = c.protobuf_state_class()
    for q, a in enumerate(rows):
        raw = out[off[q]:off[q + 1]].tobytes()
        if kind[q] != VALUE:
            assert raw == b""
            continue
        msg = State.FromString(raw)  # the protobuf runtime reads what the device wrote
        assert msg.aggregateId.encode("utf-8") == case.keys[a]
        assert msg.payload == c.encode_reference(case.template, case.states[a:a + 1], [case.keys[a]])[0]


def test_string_columns_are_read_by_row(eng):
    (case,) = c.escape_cases()  # BankAccount: two string columns, every ASCII byte in keys and strings
    ld = Loaded(eng, case)
    rng = np.random.default_rng(9)
    rows = rng.permutation(ld.n).tolist() + [-1, 0, ld.n - 1, 0]
    ld.check(rows)
    got, off, kind = encode.encode_rows(eng, JsonTemplate(case.template), ld.d_keys, ld.d_key_off, ld.up(np.asarray(rows, dtype=np.int64)), strings=ld.cols)
    got, off = got.cpu().numpy().tobytes(), off.cpu().numpy()
    a = rows[17]
    assert got[off[17]:off[18]] == ld.texts[a] and c.quote(case.strings[0][a]) in ld.texts[a] and c.quote(case.strings[1][a]) in ld.texts[a]


def test_an_abi_v2_handle_with_an_i64_and_an_f64_slot():
    from surge_amd.schema import CLS_MATERIALIZE, OP_ADD, OP_SET, SLOT_F64, SLOT_I64, SRC_PAYLOAD, SRC_SEQ, Slot, SlotAlgebra

    algebra = SlotAlgebra(slots=(Slot("n", SLOT_I64, SRC_SEQ), Slot("x", SLOT_F64, SRC_PAYLOAD)), types=((CLS_MATERIALIZE, {"n": OP_SET, "x": OP_ADD}),))
    dt = algebra.state_dtype()
    at_n, at_x = dt.fields["n"][1], dt.fields["x"][1]
    assert dt.itemsize == 64 and dt.fields["flags"][1] == c.FLAGS_AT
    n = 300
    rng = np.random.default_rng(4)
    st = c.rows(n)
    c.put(st, at_n, rng.integers(-2 ** 62, 2 ** 62, size=n), "<i8")
    x = np.round(rng.random(n) * 1e6) / 8
    x[:4] = [0.0, 1e21, 5e-324, -2.5]
    c.put(st, at_x, x, "<f8")
    st[:, 40:] = rng.integers(0, 256, size=(n, 24), dtype=np.uint8)  # a slot schema may use all 64 bytes
    c.put(st, c.FLAGS_AT, np.where(np.arange(n) % 7 == 3, 0, np.where(np.arange(n) % 31 == 5, c.PRESENT | c.POISONED, c.PRESENT)), "<u4")
    case = c.EncodeCase("v2", (b'{"id":', "KEY", b',"n":', (c.JP_I64, at_n), b',"x":', (c.JP_F64, at_x), b"}"), st, [b"slot-%d" % i for i in range(n)])
    with ReplayEngine(algebra) as eng2:
        assert eng2.v2
        ld = Loaded(eng2, case)
        ld.check(rng.integers(-1, n, size=400))
        ld.check(range(n - 1, -1, -1))
        assert struct.unpack("<q", st[0, at_n:at_n + 8].tobytes())[0] == int(ld.texts[0].split(b'"n":')[1].split(b",")[0])
