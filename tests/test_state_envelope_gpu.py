"""The envelope route of the device state decoder (``surge_replay_decode_protobuf_states``, ``state_decode_kernel<true>``):
protobuf ``State{aggregateId, payload}`` values -> resident states, behind ``decode_states`` / ``load_states_into`` /
``GpuReplayStateStore.restore_from_state_topic`` with ``envelope="protobuf_state"``.

Every device input is first decoded by the host export (``surge_decode_protobuf_state``, pinned on the protobuf runtime by
tests/test_state_envelope.py); the device must give the same rows, statuses and spans.  Shapes are the smallest at which
the kernel takes each of its paths: one block, a partial last block, several blocks, a block span beyond the 32 KiB stage
(by one long value and by the sum of 256 medium ones), every 16-byte alignment of the value buffer."""
import ctypes
import json

import numpy as np
import pytest

import state_envelope_cases as cases
import state_topic_gen as gen
from surge_amd import schema as S
from surge_amd.encode import (DECODE_AMBIGUOUS, DECODE_ENVELOPE, DECODE_OK, DECODE_SKIPPED, JsonTemplate, decode_state_host, decode_states, encode_states,
                              key_table_utf8, merge_state_strings)
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine, ReplayError

pytestmark = pytest.mark.gpu

PB = "protobuf_state"
SDK, COUNTER, BANK = cases.SDK, cases.COUNTER, cases.BANK
SENTINEL = 0xAB  # what the rows hold before a call: "untouched" is checkable
STAGE = 32 * 1024


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(items):
    """(uint8 data, int64 offsets) of byte strings; ``None`` = empty (a null value)"""
    items = [t or b"" for t in items]
    off = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in items], out=off[1:])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), off


def host_expectation(template, values, keys, agg_idx=None, n_agg=None):
    """What the call must leave behind, from the host export alone: (rows over sentinel rows, status per record, counts,
    spans per record — defined where the status is OK)."""
    n = len(values)
    agg_idx = list(range(n)) if agg_idx is None else list(agg_idx)
    n_agg = n if n_agg is None else n_agg
    rows = np.full((n_agg, 64), SENTINEL, dtype=np.uint8)
    status = np.full(n, DECODE_SKIPPED, dtype=np.uint8)
    spans = np.zeros((n, 4, 2), dtype=np.int64)
    last = {}
    for r, a in enumerate(agg_idx):
        last[a] = r
    written = tombs = refused = 0
    for a, r in last.items():
        value = values[r] or b""
        if not value:  # a tombstone, decided before the envelope is looked at
            rows[a], status[r] = 0, DECODE_OK
            tombs += 1
            continue
        rc, st, sp = decode_state_host(template, value, None if keys is None else keys[a], envelope=PB)
        status[r] = rc
        if rc == DECODE_OK:
            rows[a] = np.frombuffer(st.tobytes(), dtype=np.uint8)
            spans[r] = sp
            written += 1
        else:
            refused += 1
    return rows, status, (written, tombs, refused), spans


def run_and_compare(eng, template, values, keys, agg_idx=None, n_agg=None, shift=0, expect=None, band=b""):
    """Decode on the device — the value buffer starts ``shift`` bytes behind a 16-byte boundary and is followed by ``band``
    — and hold rows, statuses, spans, counts and the return code to the host export.  Two sentinel rows lie behind the states."""
    import torch

    data, off = table(values)
    buf = torch.zeros(shift + data.shape[0] + len(band) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if len(band):
        buf[shift + data.shape[0]:shift + data.shape[0] + len(band)].copy_(torch.from_numpy(np.frombuffer(band, dtype=np.uint8).copy()))
    d_values = buf[shift:shift + data.shape[0]]
    d_values.copy_(torch.from_numpy(data))
    kd, ko = (None, None) if keys is None else (dev(x) for x in table(keys))
    n_agg = len(values) if n_agg is None else n_agg
    backing = torch.full((n_agg + 2, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    res = decode_states(eng, template, d_values, dev(off), kd, ko, None if agg_idx is None else dev(np.asarray(agg_idx, dtype=np.int64)),
                        out=backing[:n_agg], want_spans=True, envelope=PB)
    rows, status, counts, spans = expect or host_expectation(template, values, keys, agg_idx, n_agg)
    got_rows, got_status, got_spans = res[0].cpu().numpy(), res[1].cpu().numpy(), res.spans.cpu().numpy()
    assert (got_status == status).all(), [(int(r), int(got_status[r]), int(status[r])) for r in np.flatnonzero(got_status != status)[:10]]
    assert (got_rows == rows).all(), np.flatnonzero((got_rows != rows).any(axis=1))[:10]
    ok = status == DECODE_OK
    assert (got_spans[ok] == spans[ok]).all(), np.flatnonzero((got_spans != spans).any(axis=(1, 2)) & ok)[:10]
    assert res[2][:3] == counts
    assert (backing[n_agg:].cpu().numpy() == SENTINEL).all()  # nothing behind the states buffer is touched
    assert (res.refused is not None) == (counts[2] > 0)  # SURGE_E_CORRUPT exactly when a winner was refused
    if counts[2]:
        first = int(np.flatnonzero((status != DECODE_OK) & (status != DECODE_SKIPPED))[0])
        assert f"{counts[2]} state value(s)" in res.refused and f"record {first} " in res.refused, res.refused
    return res


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


def sdk_value(key: bytes, balance: int) -> bytes:
    return cases.wrap(key, b'{"balance":%d}' % balance)


# ---- sizes ------------------------------------------------------------------------------------------------------------------
def test_the_accepted_and_the_refused_corpus_in_one_launch(eng):
    groups = {}
    for c in cases.corpus():
        groups.setdefault(tuple(c.template.parts), []).append(c)
    sdk = groups[tuple(SDK.parts)]
    sdk = sdk + cases.mutations([c for c in sdk if len(c.value) < 4000], 12)
    assert sum(c.status == DECODE_ENVELOPE for c in sdk) >= 14 and len(sdk) > 256  # more than one block
    groups[tuple(SDK.parts)] = sdk
    assert len(groups) >= 6
    for parts, group in groups.items():
        res = run_and_compare(eng, JsonTemplate(parts), [c.value for c in group], [c.key for c in group])
        status = res[1].cpu().numpy()
        for c, st in zip(group, status):
            if c.status >= 0:
                assert st == c.status, (c.name, st)
        assert DECODE_AMBIGUOUS not in status
        run_and_compare(eng, JsonTemplate(parts), [c.value for c in group], None)  # without key comparison


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1500])
def test_record_counts_around_a_block_with_an_aggregate_index(eng, n):
    rng = np.random.default_rng(n)
    n_agg = max(1, n // 3) + 2  # the last two aggregates are never named: their rows stay untouched
    keys = [(b"k%d" % i) if i % 5 else ("ünï-%d\"" % i).encode("utf-8") for i in range(n_agg)]
    agg = rng.integers(0, n_agg - 2, size=n)
    values = []
    for r, a in enumerate(agg):
        u = rng.random()
        v = sdk_value(keys[a], int(rng.integers(-2**31, 2**31)))
        values.append(None if u < 0.15 else v[:-1] if u < 0.25 else b"\x1a" + v[1:] if u < 0.30 else v)
    res = run_and_compare(eng, SDK, values, keys, agg_idx=agg, n_agg=n_agg)
    status = res[1].cpu().numpy()
    winners = set({int(a): r for r, a in enumerate(agg)}.values())
    assert all((status[r] == DECODE_SKIPPED) == (r not in winners) for r in range(n))  # losers are never parsed
    rows = res[0].cpu().numpy()
    for r in winners:
        if values[r] is None:
            assert not rows[agg[r]].any()  # a tombstone: 64 zero bytes
    assert (rows[-2:] == SENTINEL).all()


# ---- both paths ---------------------------------------------------------------------------------------------------------------
def test_a_block_beyond_the_stage_parses_from_global_and_gives_the_staged_result(eng):
    long_key = b"L" * 20000
    n = 768
    keys = [b"m%03d-" % i + b"x" * 150 for i in range(n)]  # ~190 bytes a value: 256 of them are beyond the stage by their sum
    keys[300] = long_key                                   # ... and block 1 by this one alone
    rng = np.random.default_rng(9)
    values = [sdk_value(k, int(b)) for k, b in zip(keys, rng.integers(-10**9, 10**9, size=n))]
    values[17], values[299], values[301], values[767] = None, values[299][:-1], values[301] + b"\x12", None
    _, off = table(values)
    assert all(off[min(b + 256, n)] - off[b] > STAGE + 16 for b in range(0, n, 256))  # every block takes the global path
    whole = run_and_compare(eng, SDK, values, keys)
    # the same records in launches whose blocks fit the stage: 128 at a time, the long one alone
    rows = np.zeros((n, 64), dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    pieces = [(a, min(a + 128, 300)) for a in range(0, 300, 128)] + [(300, 301)] + [(a, min(a + 128, n)) for a in range(301, n, 128)]
    for a, b in pieces:
        _, o = table(values[a:b])
        assert o[-1] + 16 <= STAGE
        part = run_and_compare(eng, SDK, values[a:b], keys[a:b])
        rows[a:b], status[a:b] = part[0].cpu().numpy(), part[1].cpu().numpy()
    assert (whole[0].cpu().numpy() == rows).all() and (whole[1].cpu().numpy() == status).all()


# ---- alignment ----------------------------------------------------------------------------------------------------------------
def test_the_values_buffer_at_each_of_the_sixteen_start_alignments(eng):
    n = 300
    rng = np.random.default_rng(16)
    keys = [b"a%d" % i * (1 + i % 4) for i in range(n)]
    values = [cases.wrap(k, cases.counter_payload(k, int(c), i)) for i, (k, c) in enumerate(zip(keys, rng.integers(-1000, 1000, size=n)))]
    for r in rng.choice(n, size=n // 12, replace=False):
        values[r] = None if r % 2 else values[r][:-1]
    values[0], values[-1] = values[0][:-1], values[-1][:-1]  # damage at both ends of the buffer
    expect = host_expectation(COUNTER, values, keys)  # once: the same for every alignment
    for shift in range(16):
        run_and_compare(eng, COUNTER, values, keys, shift=shift, expect=expect, band=b"}" * 16)


# ---- guard band ---------------------------------------------------------------------------------------------------------------
def test_a_value_one_byte_short_never_borrows_the_next_records_first_byte(eng):
    # the payload ends in 0x0A, the tag byte every next value starts with: a parser that reads one byte beyond a value's
    # end would complete record r with record r + 1's first byte
    tmpl = JsonTemplate((b"balance=", (2, 0), b"\n"))
    n = 520
    keys = [b"g%d" % i for i in range(n)]
    full = [cases.wrap(k, b"balance=%d\n" % (i - 7)) for i, k in enumerate(keys)]
    assert all(v[-1] == 0x0A and v[0] == 0x0A for v in full)
    values = [v[:-1] if i % 2 == 0 else v for i, v in enumerate(full)]  # the last record (odd n - 1) is whole, so:
    values.append(full[0][:-1])                                        # ... one more short one, in front of the band
    keys.append(keys[0])
    band = b"\x0a\x12" * 32  # plausible tag bytes behind the last value
    for shift in (0, 5):
        res = run_and_compare(eng, tmpl, values, keys, shift=shift, band=band)
        status = res[1].cpu().numpy()
        assert (status[0::2] == DECODE_ENVELOPE).all() and (status[1::2] == DECODE_OK).all()
        rows = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
        assert list(rows["count"][1::2]) == [i - 7 for i in range(1, n, 2)]  # r + 1 decodes as itself


# ---- ambiguous Doubles ----------------------------------------------------------------------------------------------------------
def test_doubles_the_device_cannot_decide_are_settled_by_the_host_export_inside_their_envelopes(eng):
    n = 300
    keys = [b"acct-%d" % i for i in range(n)]
    at = (3, 255, 290)
    balance = {r: text.encode() for r, text in zip(at, cases.AMBIGUOUS_DOUBLES)}
    values = [cases.wrap(k, b'{"accountNumber":"acct-%d","accountOwner":"O \\u20ac %d","securityCode":"%04d","balance":%s}' % (i, i, i, balance.get(i, b"%d.5" % i)))
              for i, k in enumerate(keys)]
    res = run_and_compare(eng, BANK, values, keys)
    assert res[2] == (n, 0, 0, 3) and res.refused is None
    status = res[1].cpu().numpy()
    assert (status == DECODE_OK).all()  # AMBIGUOUS is transient: never left in the status array
    rows, spans = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1), res.spans.cpu().numpy()
    for r, text in zip(at, cases.AMBIGUOUS_DOUBLES):
        assert rows["balance"].view(np.uint64)[r] == np.float64(float(text)).view(np.uint64)
        (o0, l0), (o1, l1) = spans[r, 0], spans[r, 1]  # relative to the value, as the kernel reports the others
        assert values[r][o0:o0 + l0] == b"O \\u20ac %d" % r and values[r][o1:o1 + l1] == b"%04d" % r


# ---- a refused winner -----------------------------------------------------------------------------------------------------------
def test_a_refused_winner_leaves_its_row_and_everything_else_is_decoded(eng):
    keys = [b"k0", b"k1", b"k2", b"k3"]
    good = lambda a, b: sdk_value(keys[a], b)  # noqa: E731
    values = [good(0, 1), good(1, 2), good(2, 3)[:-2], good(2, 4) + b"\x0a\x00", good(3, 5), good(1, 6), None]
    agg = [0, 1, 2, 2, 3, 1, 0]
    res = run_and_compare(eng, SDK, values, keys, agg_idx=agg, n_agg=4)
    assert res[2] == (2, 1, 1, 0)
    assert "1 state value(s)" in res.refused and "record 3 " in res.refused and f"status {DECODE_ENVELOPE} " in res.refused
    rows = res[0].cpu().numpy()
    assert (rows[2] == SENTINEL).all() and not rows[0].any()
    assert list(rows.view(S.STATE_DTYPE).reshape(-1)["count"][[1, 3]]) == [6, 5]
    assert list(res[1].cpu().numpy()) == [DECODE_SKIPPED, DECODE_SKIPPED, DECODE_SKIPPED, DECODE_ENVELOPE, DECODE_OK, DECODE_OK, DECODE_OK]
    import torch

    d, o = table(values)
    with pytest.raises(ReplayError) as ei:  # ... or raised, when asked
        decode_states(eng, SDK, dev(d), dev(o), *(dev(x) for x in table(keys)), dev(np.asarray(agg, dtype=np.int64)),
                      out=torch.zeros((4, 64), dtype=torch.uint8, device="cuda"), raise_on_refused=True, envelope=PB)
    assert ei.value.status == -7  # SURGE_E_CORRUPT


# ---- round trips ------------------------------------------------------------------------------------------------------------------
def with_decode_base(e, algebra, fn):
    """fn() with the bytes the template does not name taken from the algebra's defaults, as a resuming store sets them"""
    defaults = algebra.to_c().default_state
    e._check(e._lib.surge_replay_set_decode_base(e._h, ctypes.byref(defaults)))
    try:
        return fn()
    finally:
        e._check(e._lib.surge_replay_set_decode_base(e._h, None))


def test_counter_states_survive_the_enveloped_encoder_and_the_decoder_byte_for_byte():
    from fixture_models import COUNTER_ALGEBRA, CountDecremented, CounterCommandModel, CountIncremented, NoOpEvent
    from surge_amd.log import KeyTable, pack_events

    n = 1200
    rng = np.random.default_rng(31)
    keys = [f"agg-{i:05d}" if i % 9 else f'k"{i}\\\n\x03é' for i in range(n)]
    model = CounterCommandModel()
    kt = KeyTable()
    for k in keys:
        kt.intern(k)
    events, seqs = [], [0] * n
    for a in rng.permutation(np.repeat(np.arange(n), rng.integers(0, 6, size=n))):
        seqs[a] += 1
        seq = seqs[a]
        kind = int(rng.integers(0, 3))
        events.append(NoOpEvent(keys[a], seq) if kind == 0 else (CountIncremented if kind == 1 else CountDecremented)(keys[a], int(rng.integers(-50, 50)), seq))
    log = pack_events(model, events, kt)
    with ReplayEngine(COUNTER_ALGEBRA) as e:
        e.load_csr(log.seg_off, log.events)
        e.fold()
        states = e.snapshot()
        present = (states["flags"] & S.STATE_PRESENT) != 0
        assert 0 < present.sum() < n
        kd, ko = (dev(x) for x in key_table_utf8(keys))
        d_out, d_off = encode_states(e, COUNTER, kd, ko, envelope=PB)
        res = with_decode_base(e, COUNTER_ALGEBRA, lambda: decode_states(e, COUNTER, d_out, d_off, kd, ko, envelope=PB))
    assert res[2] == (int(present.sum()), int(n - present.sum()), 0, 0) and res.refused is None
    got = res[0].cpu().numpy()
    want = np.frombuffer(states.tobytes(), dtype=np.uint8).reshape(n, 64).copy()
    want[~present] = 0  # no text, a null value: the canonical None
    assert (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:10]


def test_bank_account_states_and_their_strings_survive_the_enveloped_round_trip():
    import uuid

    from fixture_models import BA_CREATED, BA_UPDATED, BANK_ACCOUNT_ALGEBRA

    n = 1500
    rng = np.random.default_rng(21)
    keys = [str(uuid.UUID(int=int(x))) for x in rng.integers(0, 1 << 62, size=n)]
    owners = [f"Owner {i} \"q\" ünï \\ \n" if i % 7 == 0 else f"Jane Doe {i}" for i in range(n)]
    codes = ["" if i % 50 == 0 else f"{i % 10000:04d}" for i in range(n)]
    two = rng.random(n) < 0.5
    so = np.zeros(n + 1, np.int64)
    np.cumsum(1 + two.astype(np.int64), out=so[1:])
    ev = np.zeros(int(so[-1]), dtype=S.EVENT_DTYPE)
    ev["type"][so[:-1]] = BA_CREATED
    ev["type"][so[:-1][two] + 1] = BA_UPDATED
    kinds = rng.integers(0, 4, size=ev.shape[0])
    vals = np.select([kinds == 0, kinds == 1, kinds == 2],
                     [np.round(rng.random(ev.shape[0]) * 1e7) / 100, rng.random(ev.shape[0]) * 10.0 ** rng.integers(-12, 25, size=ev.shape[0]),
                      rng.choice([0.0, -0.0, 1e20, 1e-7, 5e-324, 1.7976931348623157e308, 0.1 + 0.2, 1e21, 100.0], size=ev.shape[0])],
                     default=rng.standard_normal(ev.shape[0]) * 1e3)
    ev["raw"] = vals.view(np.uint64)
    with ReplayEngine(BANK_ACCOUNT_ALGEBRA) as e:
        e.load_csr(so, ev)
        e.fold()
        states = e.snapshot()
        kd, ko = (dev(x) for x in key_table_utf8(keys))
        cols = [tuple(dev(x) for x in key_table_utf8(col)) for col in (owners, codes)]
        d_out, d_off = encode_states(e, BANK, kd, ko, strings=cols, envelope=PB)
        res = with_decode_base(e, BANK_ACCOUNT_ALGEBRA, lambda: decode_states(e, BANK, d_out, d_off, kd, ko, want_spans=True, envelope=PB))
        merged = [merge_state_strings(e, c, d_out, d_off, None, res[1], res.spans, n_agg=n) for c in (0, 1)]
        merged = [(m[0].cpu().numpy().tobytes(), m[1].cpu().tolist()) for m in merged]
    assert res[2] == (n, 0, 0, 0) and res.refused is None
    want = states.copy()
    minus_zero = want["balance"].view(np.uint64) == np.uint64(1 << 63)
    assert minus_zero.any()
    want["balance"][minus_zero] = 0.0  # the documented exception: -0.0 is written as 0
    got = res[0].cpu().numpy()
    want = np.frombuffer(want.tobytes(), dtype=np.uint8).reshape(n, 64)
    assert (got == want).all(), np.flatnonzero((got != want).any(axis=1))[:10]
    for (data, off), col in zip(merged, (owners, codes)):
        assert [data[off[a]:off[a + 1]] for a in range(n)] == [s.encode("utf-8") for s in col]
    # the spans point into the VALUE: the bytes between the quotes, behind the envelope's own bytes
    text, offs, spans = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy(), res.spans.cpu().numpy()
    for a in (0, 7, n - 1):
        v = text[offs[a]:offs[a + 1]]
        o0, l0 = spans[a, 0]
        assert v[0] == 0x0A and json.loads(b'"' + v[o0:o0 + l0] + b'"') == owners[a]


# ---- the wire path ----------------------------------------------------------------------------------------------------------------
def fresh_engine():
    e = ReplayEngine()
    e.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    e.fold()
    return e


def enveloped_topic(compression, seed=5, n_ids=300, n_records=1600, per_batch=90):
    """-> (list of batches' bytes, delivered (offset, key, value | None) in order): Counter states in envelopes, offset gaps as
    compaction leaves them, tombstones, ids that come back after one."""
    rng = np.random.default_rng(seed)
    ids = [k.encode("utf-8") for k in gen.ids_of(n_ids)]
    version = [0] * n_ids
    alive = [False] * n_ids
    batches, delivered, base = [], [], int(rng.integers(0, 1000))
    kept, delta = [], 0
    for _ in range(n_records):
        i = int(rng.integers(n_ids))
        delta += 1 + int(rng.integers(0, 3))  # gaps
        if alive[i] and rng.random() < 0.25:
            kept.append((delta, ids[i], None))
            alive[i] = False
        else:
            version[i] += 1
            kept.append((delta, ids[i], cases.wrap(ids[i], cases.counter_payload(ids[i], int(rng.integers(-10**6, 10**6)), version[i]))))
            alive[i] = True
        if len(kept) == per_batch:
            data, recs, base = gen.compacted_batch(base, kept, compression, tail_gap=int(rng.integers(0, 4)))
            batches.append(data)
            delivered += recs
            kept, delta = [], 0
    if kept:
        data, recs, base = gen.compacted_batch(base, kept, compression)
        batches.append(data)
        delivered += recs
    return batches, delivered


@pytest.mark.parametrize("compression", ["lz4", "none"])
@pytest.mark.parametrize("n_loads", [1, 3])
def test_enveloped_values_from_record_batches_to_resident_states(compression, n_loads):
    batches, delivered = enveloped_topic(compression)
    assert any(v is None for _, _, v in delivered)
    with fresh_engine() as e, DeviceDecoder(states=True) as d, EventsTopicIngest(frames=True, device_lz4=True) as g:
        totals = np.zeros(4, dtype=np.int64)
        for j in range(n_loads):
            g.feed(b"".join(batches[len(batches) * j // n_loads:len(batches) * (j + 1) // n_loads]))
            sec, arena = g.drain_sections()
            d.push_async([(sec, arena)])
            d.finish()
            totals += np.array(d.load_states_into(e, COUNTER, envelope=PB))
        keys = d.keys()
        got = e.device_state().cpu().numpy()
    last = {}
    for _, k, v in delivered:
        last[k.decode("utf-8")] = v
    assert keys == list(dict.fromkeys(k.decode("utf-8") for _, k, _ in delivered)) and got.shape[0] == len(keys)
    n_deleted = 0
    for i, k in enumerate(keys):
        if last[k] is None:
            assert not got[i].any(), k
            n_deleted += 1
        else:
            rc, st, _ = decode_state_host(COUNTER, last[k], k, envelope=PB)
            assert rc == DECODE_OK and got[i].tobytes() == st.tobytes(), k
    assert n_deleted >= 10 and totals[2] == 0 and totals[3] == 0
    if n_loads == 1:
        assert (int(totals[0]), int(totals[1])) == (len(keys) - n_deleted, n_deleted)


def test_a_damaged_enveloped_winner_is_named_by_its_topic_offset():
    val = lambda k, c: cases.wrap(k, cases.counter_payload(k, c, c))  # noqa: E731
    recs = [(1000, b"k0", val(b"k0", 1)), (1003, b"k1", val(b"k1", 2)), (1004, b"k2", val(b"k2", 3)), (1010, b"k3", val(b"k3", 4)[:-3]),  # a loser
            (1042, b"k2", val(b"k2", 9)[:2] + b"\x0a" + val(b"k2", 9)[2:]),  # the winner of k2: a byte too many in front of its id
            (1050, b"k3", val(b"k3", 8)), (1051, b"k4", None)]
    with fresh_engine() as e, DeviceDecoder(states=True) as d:
        d.push_records([k for _, k, _ in recs], [v or b"" for _, _, v in recs], [o for o, _, _ in recs])
        e.grow(5)
        e.device_state().fill_(SENTINEL)
        __import__("torch").cuda.synchronize()
        with pytest.raises(IngestError) as ei:
            d.load_states_into(e, COUNTER, envelope=PB)
        assert ei.value.status == -7 and "topic offset 1042" in str(ei.value)
        got = e.device_state().cpu().numpy()
        assert (got[2] == SENTINEL).all() and not got[4].any()  # the refused winner's row is untouched
        for i, (k, c) in ((0, (b"k0", 1)), (1, (b"k1", 2)), (3, (b"k3", 8))):
            assert got[i].tobytes() == decode_state_host(COUNTER, val(k, c), k, envelope=PB)[1].tobytes()
        d.push_records([b"k2"], [val(b"k2", 11)], [1060])  # the decoder goes on
        assert d.load_states_into(e, COUNTER, envelope=PB) == (1, 0, 0, 0)
        # the same bytes through the bare route are refused at their first byte: the envelope is the caller's to name
        d.push_records([b"k2"], [val(b"k2", 12)], [1061])
        with pytest.raises(IngestError) as ei:
            d.load_states_into(e, COUNTER)
        assert "status 1 " in str(ei.value)  # LITERAL


# ---- the store ----------------------------------------------------------------------------------------------------------------------
def test_an_sdk_sample_store_resumes_from_its_state_topic_and_folds_the_events_tail():
    """700 UUID-keyed aggregates of the Scala SDK sample.  Store A folds the head of every aggregate's deposits and publishes
    its states as the gateway stores them (the device encoder's envelope, the device framer's LZ4 batches on two partitions);
    a fresh store resumes from those bytes and folds the tail.  Every aggregate equals the sample's own fold over all of its
    events and a full refold, byte for byte, and is served in its stored form."""
    from fixture_models import SDK_SAMPLE_MODEL, MoneyDeposited, SdkEvent, SdkSampleBusinessLogic, sdk_sample_state_bytes
    from surge_amd.snapshot import BulkSnapshotPublisher
    from surge_amd.store import GpuReplayStateStore

    n = 700
    rng = np.random.default_rng(77)
    keys = [f"0c3f1d9e-7a55-4a5c-9d5e-{i:012x}" for i in range(n)]
    per_agg = [[MoneyDeposited(int(a)) for a in rng.integers(0, 2**31, size=int(k))] for k in rng.integers(0, 40, size=n)]
    n_head = [int(np.ceil(len(d) * rng.random())) for d in per_agg]
    for a in range(n - 30, n):
        n_head[a] = 0  # ids that first appear in the tail: the resident state grows for them
    order = rng.permutation(np.repeat(np.arange(n), [len(d) for d in per_agg]))
    seen = [0] * n
    head, tail = [], []
    for a in order:
        (head if seen[a] < n_head[a] else tail).append(SdkEvent(keys[a], per_agg[a][seen[a]]))
        seen[a] += 1
    want = {keys[a]: SDK_SAMPLE_MODEL.apply_events(None, per_agg[a]) for a in range(n)}
    assert sum(w is None for w in want.values()) >= 5 and len(tail) > 1000
    bl = SdkSampleBusinessLogic()
    stores, pub = [], None
    try:
        a_store = GpuReplayStateStore(bl)
        stores.append(a_store)
        a_store.restore(head)
        pub = BulkSnapshotPublisher(a_store.engine, a_store.keys.keys, 2, template=SDK, compression="lz4", device_compression=True, envelope=PB)
        topic = {p: bytes(b) for p, b in pub.publish().items()}
        assert len(topic) == 2
        records = [(k, a_store.get_aggregate_bytes(k)) for k in a_store.keys.keys]
        assert all(v == sdk_sample_state_bytes(k, SDK_SAMPLE_MODEL.apply_events(None, per_agg[keys.index(k)][:n_head[keys.index(k)]])) for k, v in records[:50])

        full = GpuReplayStateStore(bl)  # the one-shot fold of everything
        stores.append(full)
        full.restore(head + tail)
        full_rows = full.engine.snapshot()

        def check(store):
            rows = store.engine.snapshot()
            assert sorted(store.keys.keys) == sorted(full.keys.keys)
            for k in keys:
                got = store.get_aggregate(k)
                assert got == want[k] == full.get_aggregate(k), k
                if want[k] is None:
                    assert store.get_aggregate_bytes(k) is None
                else:
                    assert store.get_aggregate_bytes(k) == sdk_sample_state_bytes(k, want[k]), k
                    assert rows[store.keys.get(k)].tobytes() == full_rows[full.keys.get(k)].tobytes(), k  # all 64 bytes

        resumed = GpuReplayStateStore(bl)
        stores.append(resumed)
        counts = resumed.restore_from_state_topic([[topic.get(p) for p in range(2)]], n_partitions=2, template=SDK, envelope=PB, events_tail=tail)
        assert counts["refused"] == 0 and counts["rows_written"] == len(records) and counts["tombstones"] == 0
        check(resumed)

        by_records = GpuReplayStateStore(bl)
        stores.append(by_records)
        counts = by_records.restore_from_state_records(records, events_tail=tail, template=SDK, envelope=PB)
        assert counts["refused"] == 0 and counts["rows_written"] == len(records)
        check(by_records)

        bare = GpuReplayStateStore(bl)  # without the envelope named, the first byte is not the template's
        stores.append(bare)
        with pytest.raises(ReplayError) as ei:
            bare.restore_from_state_records(records, template=SDK)
        assert ei.value.status == -7 and "status 1 " in str(ei.value)
    finally:
        if pub is not None:
            pub.close()
        for s in stores:
            s.close()


# ---- the spelling -----------------------------------------------------------------------------------------------------------------
def test_an_unknown_envelope_spelling_is_refused_before_any_launch(eng):
    import torch

    from fixture_models import SdkSampleBusinessLogic
    from surge_amd.store import GpuReplayStateStore

    data, off = table([sdk_value(b"k", 1)])
    out = torch.full((1, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        decode_states(eng, SDK, dev(data), dev(off), out=out, envelope="nonsense")
    assert (out.cpu().numpy() == SENTINEL).all()
    with fresh_engine() as e, DeviceDecoder(states=True) as d:
        d.push_records([b"k"], [sdk_value(b"k", 1)], [0])
        with pytest.raises(ValueError):
            d.load_states_into(e, SDK, envelope="nonsense")
        assert d.state_result()[0].numel() == 1  # nothing was handed over
    store = GpuReplayStateStore(SdkSampleBusinessLogic())
    try:
        for call in (lambda: store.restore_from_state_records([("k", sdk_value(b"k", 1))], template=SDK, envelope="nonsense"),
                     lambda: store.restore_from_state_topic([b""], template=SDK, envelope="protobuf")):
            with pytest.raises(ValueError):
                call()
        assert not store._restored and len(store.keys) == 0
    finally:
        store.close()
