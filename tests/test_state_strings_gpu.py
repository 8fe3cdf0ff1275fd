"""The restored string columns on the device: ``surge_replay_merge_state_strings`` (``state_strings.hip``) behind
``decode_states``, the state decoder that keeps the columns (``DeviceDecoder(states=True, keep_strings=True)``) and the store
that serves them (``GpuReplayStateStore.restore_from_state_topic``, BankAccount model).

The expectation is never the code under test: a column is ``json.loads`` of the text a record was written with, merged by
a Python dict.  Shapes are the smallest at which each path is taken: 256 records per workgroup (-1, +0, +1, several), a
workgroup whose values exceed the 32 KiB stage and one whose values do not, all 16 alignments of the value buffer, every
residue of a string's offset mod 16, and 16-byte pieces of kept strings that are whole, cut by a new string or at an end."""
import ctypes
import json
import uuid

import numpy as np
import pytest

import state_strings_gen as gen
from surge_amd import _native
from surge_amd import schema as S
from surge_amd.encode import JsonTemplate, decode_states, encode_states, key_table_utf8, merge_state_strings
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine, ReplayError

pytestmark = pytest.mark.gpu

BANK = JsonTemplate.bank_account()
STAGE = 32 * 1024  # kSsStageBytes (state_strings.hip): a workgroup of 256 records stages at most this many value bytes in LDS
BLOCK = 256
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = ReplayEngine()
    e.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    e.fold()
    yield e
    e.close()


def text(i, owner_raw: bytes, code_raw: bytes = b"0042", balance: bytes = b"1.5") -> bytes:
    """a BankAccount value with the given still-escaped strings"""
    return b'{"accountNumber":"k%d","accountOwner":"' % i + owner_raw + b'","securityCode":"' + code_raw + b'","balance":' + balance + b"}"


def unesc(raw: bytes) -> bytes:
    return json.loads(b'"' + raw + b'"').encode("utf-8")


def to_dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer arrays are read-only)


def decoded(eng, values, agg_idx=None, n_agg=None, shift=0):
    """values (bytes | None per record) -> decode_states' result and the device arrays it was given; the value bytes start
    `shift` bytes into a 16-byte aligned allocation"""
    import torch

    lens = [len(v or b"") for v in values]
    off = np.zeros(len(values) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    blob = b"".join(v or b"" for v in values)
    backing = torch.zeros(shift + len(blob) + 16, dtype=torch.uint8, device="cuda")
    assert backing.data_ptr() % 16 == 0
    d_values = backing[shift:shift + len(blob)]
    if blob:
        d_values.copy_(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    d_off = to_dev(off)
    d_agg = None if agg_idx is None else to_dev(np.asarray(agg_idx, dtype=np.int64))
    n_agg = len(values) if n_agg is None else n_agg
    out = torch.zeros((n_agg, 64), dtype=torch.uint8, device="cuda")
    res = decode_states(eng, BANK, d_values, d_off, d_agg_idx=d_agg, out=out, want_spans=True)
    return res, d_values, d_off, d_agg


def column_of(col):
    """(d_utf8, d_off) -> list of bytes"""
    data, off = col[0].cpu().numpy().tobytes(), col[1].cpu().tolist()
    assert off[0] == 0 and off == sorted(off) and off[-1] == len(data)
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def dev_column(strings):
    data, off = key_table_utf8([s.decode("utf-8") for s in strings])
    return to_dev(data) if data.size else to_dev(np.zeros(0, np.uint8)), to_dev(off)


def raw_merge(eng, column, d_values, d_off, d_agg, res, prev, n_agg, capacity, out_shift=0):
    """the export itself, with 64 guard bytes in front of and behind the output and a sentinel in the offsets"""
    import torch

    buf = torch.full((64 + out_shift + capacity + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_out_off = torch.full((n_agg + 1,), -7, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    n_rec = int(d_off.numel()) - 1 if d_off is not None else 0
    rc = _native.load().surge_replay_merge_state_strings(
        eng._h, column, ptr(d_values), ptr(d_off), n_rec, ptr(d_agg), ptr(res[1]) if res is not None else None, ptr(res.spans) if res is not None else None,
        ptr(prev[0]) if prev else None, ptr(prev[1]) if prev else None, int(prev[1].numel()) - 1 if prev else 0, n_agg,
        ctypes.c_void_p(buf.data_ptr() + 64 + out_shift), capacity, ctypes.c_void_p(d_out_off.data_ptr()), ctypes.byref(total))
    torch.cuda.synchronize()
    return rc, total.value, buf.cpu().numpy(), d_out_off.cpu().tolist()


# ---- 1: escapes ---------------------------------------------------------------------------------------------------------
def test_every_escape_kind_and_boundary_unescapes_as_json_loads_reads_it(eng):
    singles = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]
    bounds = [b"\\u007f", b"\\u0080", b"\\u07ff", b"\\u0800", b"\\uffff", b"\\uFFFF", b"\\ud7ff", b"\\ue000", b"\\u0000"]
    raw_utf8 = ["é".encode(), "€".encode(), "😀".encode()]
    raws = singles + bounds + raw_utf8
    raws += [b"\\nfirst", b"last\\t", b"\\u00e9first", b"last\\u20ac", b"".join(singles) + b"\\u0041\\u00e9\\u20ac", b"", b"plain"]
    long = (b"abc\\u00e9\\n" + "漢😀".encode() + b'\\"') * 15
    raws.append(long[:300])
    assert len(raws[-1]) == 300 and raws[-1][-1:] != b"\\"
    values = [text(i, r, code_raw=r[::-1] if b"\\" not in r and max(r, default=0) < 0x80 else b"c") for i, r in enumerate(raws)]
    res, d_values, d_off, _ = decoded(eng, values)
    assert res[2] == (len(raws), 0, 0, 0) and not res[1].any()
    got = column_of(merge_state_strings(eng, 0, d_values, d_off, None, res[1], res.spans, n_agg=len(raws)))
    assert got == [unesc(r) for r in raws]
    assert got[len(singles) + 4] == "\uffff".encode() and len(got[-1]) < 300
    codes = column_of(merge_state_strings(eng, 1, d_values, d_off, None, res[1], res.spans, n_agg=len(raws)))
    assert codes[-2] == b"nialp" and codes[0] == b"c"


# ---- 2: the merge rules, by hand --------------------------------------------------------------------------------------------
def test_merge_rules_losers_tombstones_refused_winners_and_new_aggregates(eng):
    records = [  # (aggregate, value)
        (1, text(1, b"loser", b"L")),                      # loses to record 3
        (2, None),                                          # a tombstone: the string is cleared
        (3, text(3, b"damaged winner", b"D")[:-4]),        # refused: aggregate 3 keeps what it had
        (1, text(1, b"winner-1 \\u00e9", b"W\\t1")),
        (6, text(6, b"new six", b"")),                     # beyond n_prev
        (0, text(0, b"damaged loser")[:-9]),               # never parsed
        (0, text(0, b"zero", b"Z")),
    ]
    prev_owner = [b"p0", b"p1", b"p2", "p3 é".encode(), b"p4"]
    prev_code = [b"c0", b"", b"c2", b"c3", b"c4"]
    res, d_values, d_off, d_agg = decoded(eng, [v for _, v in records], [a for a, _ in records], n_agg=8)
    assert res.refused and res[2] == (3, 1, 1, 0)
    assert res[1].cpu().tolist() == [255, 0, res[1][2].item(), 0, 0, 255, 0] and res[1][2].item() not in (0, 255)
    args = (d_values, d_off, d_agg, res[1], res.spans)
    owners = column_of(merge_state_strings(eng, 0, *args, prev=dev_column(prev_owner), n_agg=8))
    assert owners == [b"zero", "winner-1 é".encode(), b"", "p3 é".encode(), b"p4", b"", b"new six", b""]
    codes = column_of(merge_state_strings(eng, 1, *args, prev=dev_column(prev_code), n_agg=8))
    assert codes == [b"Z", b"W\t1", b"", b"c3", b"c4", b"", b"", b""]
    # no previous column (NULL pointers): whoever is not named comes out empty
    assert column_of(merge_state_strings(eng, 0, *args, prev=None, n_agg=8)) == [b"zero", "winner-1 é".encode(), b"", b"", b"", b"", b"new six", b""]
    # no records: the column is extended
    assert column_of(merge_state_strings(eng, 0, prev=dev_column(prev_owner), n_agg=8)) == prev_owner + [b"", b"", b""]
    assert column_of(merge_state_strings(eng, 0, prev=dev_column(prev_owner), n_agg=5)) == prev_owner
    assert column_of(merge_state_strings(eng, 2, prev=None, n_agg=3)) == [b"", b"", b""]
    # a long previous column around a single new string: whole 16-byte pieces, pieces cut by the new string, the ends
    many = [bytes([97 + (i + j) % 26 for j in range(i % 23)]) for i in range(600)]
    one, d_v1, d_o1, d_a1 = decoded(eng, [text(300, b"NEW \\u20ac")], [300], n_agg=600)
    got = column_of(merge_state_strings(eng, 0, d_v1, d_o1, d_a1, one[1], one.spans, prev=dev_column(many), n_agg=601))
    assert got == many[:300] + ["NEW €".encode()] + many[301:] + [b""]


def test_merge_argument_checks(eng):
    res, d_values, d_off, d_agg = decoded(eng, [text(0, b"a"), text(1, b"b")], [0, 8], n_agg=9)
    prev = dev_column([b"x", b"y", b"z"])
    for kw in (dict(column=4), dict(column=-1)):
        rc, *_ = raw_merge(eng, kw["column"], d_values, d_off, d_agg, res, prev, 9, 64)
        assert rc == -1
    assert raw_merge(eng, 0, d_values, d_off, d_agg, res, prev, 2, 64)[0] == -1  # n_agg < n_prev
    assert raw_merge(eng, 0, d_values, d_off, None, res, None, 1, 64)[0] == -1   # more records than aggregates, no index
    rc, _, buf, off = raw_merge(eng, 0, d_values, d_off, d_agg, res, prev, 8, 64)  # aggregate 8 is outside [0, 8)
    assert rc == -1 and (buf == GUARD).all() and off == [-7] * 9  # ... and nothing was written
    with pytest.raises(ReplayError) as ei:
        merge_state_strings(eng, 0, d_values, d_off, d_agg, res[1], res.spans, prev=prev, n_agg=8)
    assert ei.value.status == -1 and "outside" in str(ei.value)


# ---- 3: block and alignment edges ---------------------------------------------------------------------------------------------
def edge_records(n, long_until=0):
    """owner i unescapes to i % 17 bytes (every residue of the offsets mod 16 occurs); every third owner below `long_until`
    is about 500 bytes of escapes instead"""
    raws = []
    for i in range(n):
        if i < long_until and i % 3 == 0:
            raws.append(b"\\u00e9\\n\\u20ac\\\\" * 31 + b"%d" % (i % 10))  # 31 x 16 + 1 = 497 bytes -> 31 x 7 + 1
        else:
            k = i % 17
            raws.append((b"\\t" if k else b"") + bytes([65 + (i + j) % 26 for j in range(max(k - 1, 0))]))
    return raws


@pytest.mark.parametrize("n,shift", [(1, 0), (255, 3), (256, 11)] + [(257, s) for s in range(16)] + [(1500, 0), (1500, 5)])
def test_record_counts_around_a_workgroup_at_every_alignment_with_guard_bands(eng, n, shift):
    raws = edge_records(n, long_until=1024 if n == 1500 else 0)
    values = [text(i, r) for i, r in enumerate(raws)]
    spans = [sum(len(v) for v in values[b:b + BLOCK]) for b in range(0, n, BLOCK)]
    if n == 1500:  # workgroups that read from global because their values exceed the stage, and workgroups that stage
        assert all(s + 16 > STAGE for s in spans[:4]) and all(s + 16 <= STAGE for s in spans[4:]) and len(spans) == 6
    else:
        assert all(s + 16 <= STAGE for s in spans)
    res, d_values, d_off, _ = decoded(eng, values, shift=shift)
    assert d_values.data_ptr() % 16 == shift and res[2][0] == n
    want = [unesc(r) for r in raws]
    assert [len(w) for w in want[:17]] == list(range(17))[:n] or n == 1500
    total = sum(len(w) for w in want)
    rc, got_total, buf, off = raw_merge(eng, 0, d_values, d_off, None, res, None, n, total, out_shift=shift % 5)
    assert rc == 0 and got_total == total
    assert off == [0] + list(np.cumsum([len(w) for w in want]))
    lo = 64 + shift % 5
    assert buf[lo:lo + total].tobytes() == b"".join(want)
    assert (buf[:lo] == GUARD).all() and (buf[lo + total:] == GUARD).all()
    # the same strings as the PREVIOUS column of a load that renames every seventh aggregate: kept runs between new strings
    if n >= 255:
        prev = dev_column(want)
        idx = list(range(0, n, 7))
        res2, d_v2, d_o2, d_a2 = decoded(eng, [text(i, b"N\\u00e9w%d" % i) for i in idx], idx, n_agg=n, shift=(shift + 7) % 16)
        want2 = list(want)
        for i in idx:
            want2[i] = ("Néw%d" % i).encode()
        total2 = sum(len(w) for w in want2)
        rc, got_total, buf, off = raw_merge(eng, 0, d_v2, d_o2, d_a2, res2, prev, n + 2, total2, out_shift=shift)
        assert rc == 0 and got_total == total2 and off == [0] + list(np.cumsum([len(w) for w in want2 + [b"", b""]]))
        lo = 64 + shift
        assert buf[lo:lo + total2].tobytes() == b"".join(want2)
        assert (buf[:lo] == GUARD).all() and (buf[lo + total2:] == GUARD).all()


# ---- 4: capacity ---------------------------------------------------------------------------------------------------------------
def test_a_capacity_one_short_returns_range_the_total_and_writes_no_byte(eng):
    raws = edge_records(300)
    res, d_values, d_off, _ = decoded(eng, [text(i, r) for i, r in enumerate(raws)])
    prev = dev_column([b"kept-%d" % i for i in range(310)])
    want = [unesc(r) for r in raws] + [b"kept-%d" % i for i in range(300, 310)]
    total = sum(len(w) for w in want)
    rc, got_total, buf, off = raw_merge(eng, 0, d_values, d_off, None, res, prev, 310, total - 1)
    assert rc == -6 and got_total == total and (buf == GUARD).all()  # SURGE_E_RANGE: the total is reported, no byte written
    rc, got_total, buf, off = raw_merge(eng, 0, d_values, d_off, None, res, prev, 310, total)
    assert rc == 0 and got_total == total and buf[64:64 + total].tobytes() == b"".join(want)
    assert (buf[:64] == GUARD).all() and (buf[64 + total:] == GUARD).all() and off[-1] == total
    # the Python wrapper retries with the exact size
    assert column_of(merge_state_strings(eng, 0, d_values, d_off, None, res[1], res.spans, prev=prev, n_agg=310, capacity_hint=5)) == want


# ---- 5: wire bytes through the state decoder ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def topics():
    return {c: gen.make_topic(compression=c) for c in ("lz4", "none")}


def fresh_engine():
    e = ReplayEngine()
    e.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    e.fold()
    return e


def load_topic(units, n_push, keep):
    """-> (keys, rows, string columns as lists of bytes or None)"""
    ingests = [EventsTopicIngest(frames=True, device_lz4=True) for _ in units]
    try:
        with fresh_engine() as e, DeviceDecoder(states=True, keep_strings=keep) as d:
            for j in range(n_push):
                parts = []
                for g, part in zip(ingests, units):
                    g.feed(gen.concat(gen.split(part, n_push)[j])[0])
                    sec, arena = g.drain_sections()
                    if sec.shape[0]:
                        parts.append((sec, arena))
                d.push_async(parts)
                d.finish()
                counts = d.load_states_into(e, BANK)
                assert counts[2] == 0
            cols = [None if c is None else column_of(c) for c in d.state_strings()]
            return d.keys(), e.device_state().cpu().numpy().copy(), cols
    finally:
        for g in ingests:
            g.close()


@pytest.mark.parametrize("compression", ["lz4", "none"])
@pytest.mark.parametrize("n_push", [1, 3])
def test_the_generated_topic_through_a_decoder_that_keeps_its_strings(topics, compression, n_push):
    units, table = topics[compression]
    keys, rows, cols = load_topic(units, n_push, keep=True)
    assert sorted(keys) == sorted(table) and cols[2] is None and cols[3] is None
    assert cols[0] == [(table[k][0] if table[k] else "").encode("utf-8") for k in keys]
    assert cols[1] == [(table[k][1] if table[k] else "").encode("utf-8") for k in keys]
    keys0, rows0, cols0 = load_topic(units, n_push, keep=False)
    assert keys0 == keys and (rows0 == rows).all() and cols0 == [None] * 4
    view = rows.view(S.STATE_DTYPE).reshape(-1)
    for i, k in enumerate(keys):
        assert (float(view["balance"][i]) == table[k][2] and view["flags"][i] & S.STATE_PRESENT) if table[k] else not rows[i].any()


# ---- 6: the store ---------------------------------------------------------------------------------------------------------------
def test_a_store_resumed_from_the_state_topic_serves_and_re_encodes_the_string_fields(topics):
    from fixture_models import BankAccount, BankAccountBusinessLogic, BankAccountCreated, BankAccountFormat, BankAccountUpdated
    from surge_amd.store import GpuReplayStateStore

    units, table = topics["lz4"]
    fetches = [[gen.concat(gen.split(part, 3)[j])[0] or None for part in units] for j in range(3)]
    fmt = BankAccountFormat()
    text_of = lambda k, t: fmt.write_state(BankAccount(uuid.UUID(k), t[0], t[1], t[2])).value  # noqa: E731
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        counts = store.restore_from_state_topic(fetches, n_partitions=len(units), template=BANK)
        assert counts["refused"] == 0 and sorted(store.keys.keys) == sorted(table)
        for k, t in table.items():  # (on the parent commit owner and code came back empty here)
            assert store.get_aggregate_bytes(k) == (text_of(k, t) if t else None), k
        assert any(t and t[0] and t[1] for t in table.values())
        # the states it just read, encoded again from the restored columns: the same texts
        keys = store.keys.keys
        data, off = key_table_utf8(keys)
        out, out_off = encode_states(store.engine, BANK, to_dev(data), to_dev(off), strings=store.state_string_columns())
        blob, o = out.cpu().numpy().tobytes(), out_off.cpu().tolist()
        for i, k in enumerate(keys):
            assert blob[o[i]:o[i + 1]] == (text_of(k, table[k]) if table[k] else b""), k
    finally:
        store.close()
    # ... and with an events tail: one event for a new id, one for an id of the topic.  The columns extend; old ids keep theirs.
    live = next(k for k in table if table[k] and table[k][0] and table[k][1])
    fresh_id = uuid.UUID(int=12345)
    assert str(fresh_id) not in table
    tail = [BankAccountCreated(fresh_id, "Neu \"x\"", "999", 5.0), BankAccountUpdated(uuid.UUID(live), 77.25)]
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        store.restore_from_state_topic(fetches, n_partitions=len(units), template=BANK, events_tail=tail)
        n = len(table)
        assert store.engine.n_agg == n + 1 and len(store.state_strings[0][1]) == n + 1  # as restored: n aggregates
        cols = store.state_string_columns()
        owners, codes = column_of(cols[0]), column_of(cols[1])
        assert len(owners) == len(codes) == n + 1 and owners[-1] == b"" and codes[-1] == b""  # the new id's strings stay the host's
        for i, k in enumerate(store.keys.keys[:n]):
            assert (owners[i], codes[i]) == ((table[k][0].encode(), table[k][1].encode()) if table[k] else (b"", b""))
        assert store.get_aggregate_bytes(live) == text_of(live, (table[live][0], table[live][1], 77.25))
        assert store.get_aggregate_bytes(str(fresh_id)) == text_of(str(fresh_id), ("Neu \"x\"", "999", 5.0))
        gone = next(k for k in table if table[k] is None)
        assert store.get_aggregate_bytes(gone) is None
    finally:
        store.close()


def test_restore_from_state_records_keeps_the_columns_too():
    from fixture_models import BankAccount, BankAccountBusinessLogic, BankAccountFormat
    from surge_amd.store import GpuReplayStateStore

    fmt = BankAccountFormat()
    a, b, c = (str(uuid.UUID(int=i)) for i in (1, 2, 3))
    acct = lambda k, o, s, bal: fmt.write_state(BankAccount(uuid.UUID(k), o, s, bal)).value  # noqa: E731
    records = [(a, acct(a, "first", "1", 1.0)), (b, acct(b, "Bé \"b\"", "", 2.5)), (a, acct(a, "second\n", "11", 3.0)), (c, acct(c, "gone", "3", 4.0)), (c, None)]
    store = GpuReplayStateStore(BankAccountBusinessLogic())
    try:
        store.restore_from_state_records(records, template=BANK)
        assert store.get_aggregate_bytes(a) == acct(a, "second\n", "11", 3.0)
        assert store.get_aggregate_bytes(b) == acct(b, "Bé \"b\"", "", 2.5) and store.get_aggregate_bytes(c) is None
        cols = store.state_string_columns()
        assert column_of(cols[0]) == [b"second\n", "Bé \"b\"".encode(), b""] and column_of(cols[1]) == [b"11", b"", b""]
    finally:
        store.close()


# ---- 7: default off -----------------------------------------------------------------------------------------------------------------
def test_strings_are_kept_only_when_asked_and_only_by_a_state_decoder():
    lib = _native.load()
    with fresh_engine() as e, DeviceDecoder(states=True) as d:
        d.push_records([b"k0"], [text(0, b"owner")], [0])
        assert d.load_states_into(e, BANK) == (1, 0, 0, 0)
        assert d.state_strings() == [None] * 4
        assert lib.surge_device_decoder_keep_strings(d._h, 1) == -2  # SURGE_E_STATE: a load has run
    with DeviceDecoder() as events:
        assert lib.surge_device_decoder_keep_strings(events._h, 1) == -2
        with pytest.raises(IngestError) as ei:
            events.state_strings()
        assert ei.value.status == -2
    with pytest.raises(ValueError):
        DeviceDecoder(keep_strings=True)
    with fresh_engine() as e, DeviceDecoder(states=True, keep_strings=True) as d:
        assert d.state_strings() == [None] * 4  # nothing loaded yet
        d.push_records([b"k0", b"k1"], [text(0, b"o\\u00e9"), text(1, b"damaged")[:-4]], [0, 1])
        with pytest.raises(IngestError) as ei:  # a refused winner: CORRUPT, everything else loaded AND merged
            d.load_states_into(e, BANK)
        assert ei.value.status == -7
        cols = d.state_strings()
        assert column_of(cols[0]) == ["oé".encode(), b""] and column_of(cols[1]) == [b"0042", b""] and cols[2] is None
