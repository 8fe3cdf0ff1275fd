"""The lenient reading mode of the device state decoder (``surge_replay_set_decode_mode``, ``state_decode_kernel<*, true>``):
reordered, spaced values with unknown members -> resident states, behind ``decode_states(lenient=True)`` and
``DeviceDecoder.load_states_into(lenient=True)``.

Every device input is first decoded by the host export (``surge_decode_json_state_lenient`` /
``surge_decode_protobuf_state_lenient``, pinned on ``json.loads`` by tests/test_state_lenient.py); the device must give the same
rows, statuses and spans.  Shapes are the smallest at which the kernel takes each of its paths: one block, a block edge, a
second and a third block, a block staged in LDS beside one whose span exceeds the 32 KiB stage, every 16-byte alignment of
the value buffer."""
import ctypes
import random

import numpy as np
import pytest

import number_text_cases as numbers
import state_lenient_cases as L
import state_topic_gen as gen
from surge_amd import schema as S
from surge_amd.encode import (DECODE_LITERAL, DECODE_OK, DECODE_SKIPPED, STRING_COLUMNS, JsonTemplate, decode_state_host, decode_states)
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine, ReplayError

pytestmark = pytest.mark.gpu

PB = "protobuf_state"
COUNTER, BANK, SDK = L.COUNTER, L.BANK, L.SDK
SENTINEL = 0xAB  # what the rows, and the bytes around the arrays the call writes, hold before it
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


def host_expectation(template, values, keys, agg_idx=None, n_agg=None, envelope="none", lenient=True):
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
        last[int(a)] = r
    written = tombs = refused = 0
    for a, r in last.items():
        value = values[r] or b""
        if not value:  # a tombstone, decided before anything of the value is looked at
            rows[a], status[r] = 0, DECODE_OK
            tombs += 1
            continue
        rc, st, sp = decode_state_host(template, value, None if keys is None else keys[a], envelope=envelope, lenient=lenient)
        status[r] = rc
        if rc == DECODE_OK:
            rows[a] = np.frombuffer(st.tobytes(), dtype=np.uint8)
            spans[r] = sp
            written += 1
        else:
            refused += 1
    return rows, status, (written, tombs, refused), spans


def run_and_compare(eng, template, values, keys, agg_idx=None, n_agg=None, shift=0, expect=None, band=b"", envelope="none", lenient=True):
    """Decode on the device through the C call itself — the value buffer starts ``shift`` bytes behind a 16-byte boundary and is
    followed by ``band``; one sentinel row lies in front of the states and two behind them, 64 sentinel bytes on either side of
    the status array and of the spans — and hold rows, statuses, spans, counts and the return code to the host export."""
    import torch

    data, off = table(values)
    buf = torch.zeros(shift + data.shape[0] + len(band) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if len(band):
        buf[shift + data.shape[0]:shift + data.shape[0] + len(band)].copy_(torch.from_numpy(np.frombuffer(band, dtype=np.uint8).copy()))
    d_values = buf[shift:shift + data.shape[0]]
    d_values.copy_(torch.from_numpy(data))
    d_off = dev(off)
    kd, ko = (None, None) if keys is None else (dev(x) for x in table(keys))
    n = len(values)
    n_agg = n if n_agg is None else n_agg
    d_agg = None if agg_idx is None else dev(np.asarray(agg_idx, dtype=np.int64))
    backing = torch.full((n_agg + 3, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    status_backing = torch.full((n + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    spans_backing = torch.full((n * 2 * STRING_COLUMNS + 16,), -1, dtype=torch.int64, device="cuda")
    out, d_status, d_spans = backing[1:n_agg + 1], status_backing[64:64 + n], spans_backing[8:8 + n * 2 * STRING_COLUMNS]
    d_spans.zero_()  # (a column the template does not name is never written: zeros, as the host export reports it)
    counts = (ctypes.c_int64 * 4)()
    t = template.to_c()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    fn = eng._lib.surge_replay_decode_protobuf_states if envelope == PB else eng._lib.surge_replay_decode_json_states
    with eng.reading_leniently(lenient):
        rc = fn(eng._h, ctypes.byref(t), ptr(d_values), ptr(d_off), n, ptr(kd), ptr(ko), ptr(d_agg), n_agg, ptr(out), ptr(d_status), ptr(d_spans),
                ctypes.byref(counts))
        message = (eng._lib.surge_replay_last_error(eng._h) or b"").decode() if rc else ""
    rows, status, want_counts, spans = expect or host_expectation(template, values, keys, agg_idx, n_agg, envelope, lenient)
    got_rows, got_status, got_spans = out.cpu().numpy(), d_status.cpu().numpy(), d_spans.cpu().numpy().reshape(n, STRING_COLUMNS, 2)
    assert (got_status == status).all(), [(int(r), int(got_status[r]), int(status[r])) for r in np.flatnonzero(got_status != status)[:10]]
    assert (got_rows == rows).all(), np.flatnonzero((got_rows != rows).any(axis=1))[:10]
    ok = (status == DECODE_OK) & np.array([bool(v) for v in values])
    assert (got_spans[ok] == spans[ok]).all(), np.flatnonzero((got_spans != spans).any(axis=(1, 2)) & ok)[:10]
    got_counts = tuple(int(c) for c in counts)
    assert got_counts[:3] == want_counts
    # nothing around the arrays the call writes is touched
    assert (backing[0].cpu().numpy() == SENTINEL).all() and (backing[n_agg + 1:].cpu().numpy() == SENTINEL).all()
    sb = status_backing.cpu().numpy()
    assert (sb[:64] == SENTINEL).all() and (sb[64 + n:] == SENTINEL).all()
    pb = spans_backing.cpu().numpy()
    assert (pb[:8] == -1).all() and (pb[8 + n * 2 * STRING_COLUMNS:] == -1).all()
    assert rc == (-7 if want_counts[2] else 0), (rc, message)  # SURGE_E_CORRUPT exactly when a winner was refused
    if want_counts[2]:
        first = int(np.flatnonzero((status != DECODE_OK) & (status != DECODE_SKIPPED))[0])
        assert f"{want_counts[2]} state value(s)" in message and f"record {first} " in message and f"status {int(status[first])} " in message, message
    return got_rows, got_status, got_counts, got_spans


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


def counter_text(key: bytes, count: int, version: int) -> bytes:
    return L.text_of([(b"aggregateId", b'"' + key + b'"'), (b"count", b"%d" % count), (b"version", b"%d" % version)])


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
def test_the_whole_corpus_in_one_launch_per_template(eng):
    groups = {}
    cases = L.corpus()
    cases += L.mutations([c for c in cases if c.status == L.OK and len(c.value) < 4000 and c.template is COUNTER][:60], 6)
    for c in cases:
        groups.setdefault(id(c.template), []).append(c)
    assert len(groups) == 3
    for group in groups.values():
        values, keys = [c.value for c in group], [c.key for c in group]
        _, off = table(values)
        if group[0].template is COUNTER:  # more than two blocks; one of them holds the 40 KB value and is read from global, the others are staged
            spans = [int(off[min(b + 256, len(values))] - off[b]) for b in range(0, len(values), 256)]
            assert len(spans) >= 3 and sum(s > STAGE for s in spans) == 1 and sum(s + 16 <= STAGE for s in spans) >= 2, spans
        _, status, counts, _ = run_and_compare(eng, group[0].template, values, keys)
        for c, st in zip(group, status):
            if c.status >= 0 and c.value:
                assert st == c.status, (c.name, st)
            elif c.status == L.REFUSED and c.value:
                assert st != DECODE_OK, c.name
        assert counts[3] == 0  # the corpus' Doubles are short: nothing is handed back to the host
        run_and_compare(eng, group[0].template, values, None)  # without key comparison


def test_the_envelope_instantiation_over_the_enveloped_corpus(eng):
    groups = {}
    cases = L.envelope_cases()
    cases += L.mutations([c for c in cases if c.status == L.OK and len(c.value) < 4000][:40], 6)
    for c in cases:
        groups.setdefault(id(c.template), []).append(c)
    assert len(groups) == 3 and sum(len(g) for g in groups.values()) > 256
    for group in groups.values():
        _, status, counts, _ = run_and_compare(eng, group[0].template, [c.value for c in group], [c.key for c in group], envelope=PB)
        for c, st in zip(group, status):
            if c.status >= 0:
                assert st == c.status, (c.name, st)
        assert counts[3] == 0
    sdk = next(g for g in groups.values() if g[0].template is SDK)
    run_and_compare(eng, SDK, [c.value for c in sdk], None, envelope=PB)


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_record_counts_around_a_block_with_losers_tombstones_and_refused_winners(eng, n):
    rng = random.Random(n)
    n_agg = max(1, n // 3) + 2  # the last two aggregates are never named: their rows stay untouched
    keys = [b"k%d" % i for i in range(n_agg)]
    agg = [rng.randrange(0, n_agg - 2) for _ in range(n)]
    winners = set({a: r for r, a in enumerate(agg)}.values())
    values = []
    for r, a in enumerate(agg):
        u = rng.random()
        v = L.rewritten(counter_text(keys[a], rng.randrange(-2 ** 31, 2 ** 31), r), rng)
        if r not in winners and u < 0.5:
            v = b'{"aggregateId":' + b"\xff\x00[" * rng.randrange(1, 9)  # a loser that would not parse: never looked at
        elif u < 0.15:
            v = None
        elif u < 0.25:
            v = v.rstrip(b" \t\r\n")[:-1]  # the closing brace gone
        elif u < 0.30:
            v = v.replace(b'"count"', b'"Count"')  # a field missing
        values.append(v)
    rows, status, counts, _ = run_and_compare(eng, COUNTER, values, keys, agg_idx=agg, n_agg=n_agg)
    assert all((status[r] == DECODE_SKIPPED) == (r not in winners) for r in range(n))  # losers are never parsed
    for r in winners:
        if values[r] is None:
            assert not rows[agg[r]].any()  # a tombstone: 64 zero bytes
        elif status[r] != DECODE_OK:
            assert status[r] in (L.SYNTAX, L.MISSING) and (rows[agg[r]] == SENTINEL).all()  # a refused winner leaves its row
    assert (rows[-2:] == SENTINEL).all()
    if n >= 255:
        assert counts[0] and counts[1] and counts[2]


# ---- both paths in one launch ---------------------------------------------------------------------------------------------------
def test_a_staged_block_and_a_block_beyond_the_stage_in_one_launch_give_what_they_give_alone(eng):
    rng = random.Random(9)
    n = 768
    keys = [b"m%03d" % i for i in range(n)]
    values = [L.rewritten(counter_text(k, rng.randrange(-10 ** 9, 10 ** 9), i), rng, unknown=(b"u", b"[]")) for i, k in enumerate(keys)]
    # block 0: small values, staged.  block 1: beyond the stage by one long unknown member.  block 2: beyond it by the sum of its values.
    values[300] = values[300][:values[300].index(b"{") + 1] + b'"blob":"' + b"y]}\\\\" * 7000 + b'",' + values[300][values[300].index(b"{") + 1:]
    for i in range(512, n):
        values[i] = values[i][:values[i].index(b"{") + 1] + b'"pad":[' + b",".join([b"null"] * 30) + b"]," + values[i][values[i].index(b"{") + 1:]
    values[17], values[299], values[301], values[767], values[600] = None, values[299].rstrip()[:-1], values[301] + b"x", None, values[600].replace(b'"version"', b'"v"')
    _, off = table(values)
    spans = [int(off[min(b + 256, n)] - off[b]) for b in range(0, n, 256)]
    assert spans[0] + 16 <= STAGE and spans[1] > STAGE + 16 and spans[2] > STAGE + 16, spans
    rows, status, _, _ = run_and_compare(eng, COUNTER, values, keys)
    assert status[299] == L.SYNTAX and status[301] == L.TRAILING and status[600] == L.MISSING and status[300] == DECODE_OK
    # the same records in launches whose blocks all fit the stage, the long one in a launch of its own (global)
    alone_rows, alone_status = np.zeros((n, 64), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    pieces = [(0, 256), (256, 300), (300, 301), (301, 512)] + [(a, min(a + 64, n)) for a in range(512, n, 64)]
    for a, b in pieces:
        _, o = table(values[a:b])
        assert (o[-1] + 16 <= STAGE) == (a != 300)
        part = run_and_compare(eng, COUNTER, values[a:b], keys[a:b])
        alone_rows[a:b], alone_status[a:b] = part[0], part[1]
    assert (rows == alone_rows).all() and (status == alone_status).all()


# ---- alignment ------------------------------------------------------------------------------------------------------------------
def test_the_values_buffer_at_each_of_the_sixteen_start_alignments(eng):
    n = 300
    rng = random.Random(16)
    keys = [b"a%d" % i * (1 + i % 4) for i in range(n)]
    values = [L.rewritten(counter_text(k, rng.randrange(-1000, 1000), i), rng) for i, k in enumerate(keys)]
    for r in rng.sample(range(n), n // 12):
        values[r] = None if r % 2 else values[r].rstrip()[:-1]
    values[0], values[-1] = values[0].rstrip()[:-1], values[-1].rstrip()[:-1]  # damage at both ends of the buffer
    expect = host_expectation(COUNTER, values, keys)  # once: the same for every alignment
    for shift in range(16):
        run_and_compare(eng, COUNTER, values, keys, shift=shift, expect=expect, band=b"}" * 16)


# ---- the value's end ------------------------------------------------------------------------------------------------------------
def test_a_value_one_byte_short_is_never_completed_by_the_next_records_first_byte(eng):
    # record 3 i lacks its closing brace; record 3 i + 1 IS a closing brace (and whitespace): a parser that reads one byte beyond
    # a value's end would complete the first with the second.  Record 3 i + 2 is whole and decodes as itself.
    n = 174
    keys, values = [], []
    for i in range(n):
        full = b'{"x":[%d],"balance":%d}' % (i, i - 7)
        values += [full[:-1], b"} ", b" " + full]
        keys += [b"g%d" % i] * 3
    band = b"}" * 64  # ... and behind the last value
    values.append(values[0])
    keys.append(keys[0])
    for shift in (0, 5):
        rows, status, _, _ = run_and_compare(eng, SDK, values, keys, shift=shift, band=band)
        assert (status[0::3] == L.SYNTAX).all() and (status[1::3] == L.SYNTAX).all() and (status[2::3] == DECODE_OK).all()
        got = rows.view(S.STATE_DTYPE).reshape(-1)
        assert list(got["count"][2::3]) == [i - 7 for i in range(n)]


# ---- a refused winner, counted and named ------------------------------------------------------------------------------------------
def test_a_refused_winner_leaves_its_row_and_everything_else_is_decoded(eng):
    import torch

    keys = [b"k0", b"k1", b"k2", b"k3"]
    good = lambda a, b: b' {"later":{"a":[1]},"balance" : %d }' % b  # noqa: E731
    values = [good(0, 1), good(1, 2), b"\xff{[", good(2, 4)[:-2] + b",}", good(3, 5), good(1, 6), None]
    agg = [0, 1, 2, 2, 3, 1, 0]
    rows, status, counts, _ = run_and_compare(eng, SDK, values, keys, agg_idx=agg, n_agg=4)
    assert counts == (2, 1, 1, 0)
    assert (rows[2] == SENTINEL).all() and not rows[0].any()
    assert list(rows.view(S.STATE_DTYPE).reshape(-1)["count"][[1, 3]]) == [6, 5]
    assert list(status) == [DECODE_SKIPPED, DECODE_SKIPPED, DECODE_SKIPPED, L.SYNTAX, DECODE_OK, DECODE_OK, DECODE_OK]
    d, o = table(values)
    with pytest.raises(ReplayError) as ei:  # ... raised, when asked
        decode_states(eng, SDK, dev(d), dev(o), *(dev(x) for x in table(keys)), dev(np.asarray(agg, dtype=np.int64)),
                      out=torch.zeros((4, 64), dtype=torch.uint8, device="cuda"), raise_on_refused=True, lenient=True)
    assert ei.value.status == -7 and "record 3 with status 12 " in str(ei.value)  # SURGE_E_CORRUPT, SYNTAX
    res = decode_states(eng, SDK, dev(d), dev(o), *(dev(x) for x in table(keys)), dev(np.asarray(agg, dtype=np.int64)),
                        out=torch.zeros((4, 64), dtype=torch.uint8, device="cuda"), lenient=True)
    assert res[2] == (2, 1, 1, 0) and "record 3 " in res.refused


# ---- ambiguous Doubles -------------------------------------------------------------------------------------------------------------
def test_doubles_the_device_cannot_decide_are_settled_by_the_lenient_host_export(eng):
    n = 300
    ties = numbers.long_texts()[:3]
    assert all(len(t) > 19 for t in ties)
    keys = [b"acct-%d" % i for i in range(n)]
    at = (3, 255, 290)
    balance = {r: text.encode() for r, text in zip(at, ties)}
    rng = random.Random(4)
    compact = [b'{"accountNumber":"acct-%d","accountOwner":"O \\u20ac %d","securityCode":"%04d","balance":%s}' % (i, i, i, balance.get(i, b"%d.5" % i)) for i in range(n)]
    values = [L.rewritten(v, rng) for v in compact]
    for envelope in ("none", PB):
        vs = [L.wrap(k, v) for k, v in zip(keys, values)] if envelope == PB else values
        rows, status, counts, spans = run_and_compare(eng, BANK, vs, keys, envelope=envelope)
        assert counts == (n, 0, 0, 3)
        assert (status == DECODE_OK).all()  # AMBIGUOUS is transient: never left in the status array
        got = rows.view(S.STATE_DTYPE).reshape(-1)
        for r, text in zip(at, ties):
            assert got["balance"].view(np.uint64)[r] == np.float64(float(text)).view(np.uint64)
            (o0, l0), (o1, l1) = spans[r, 0], spans[r, 1]  # relative to the value, as the kernel reports the others
            assert vs[r][o0:o0 + l0] == b"O \\u20ac %d" % r and vs[r][o1:o1 + l1] == b"%04d" % r
    # a strict handle refuses the same text at its first literal, and hands nothing back
    _, status, counts, _ = run_and_compare(eng, BANK, values[:8], keys[:8], lenient=False)
    assert counts[3] == 0 and (status != DECODE_OK).sum() >= 7  # (a seeded order can be the template's own: then only the unknown member refuses it)


# ---- the mode is the handle's, and goes back -----------------------------------------------------------------------------------------
def test_the_strict_mode_reads_as_before_on_the_same_handle_before_and_after(eng):
    reordered, compact = b'{"version":2,"count":1,"aggregateId":"a"}', b'{"aggregateId":"a","count":1,"version":2}'
    values, keys = [reordered, compact], [b"a", b"a"]
    for _ in range(2):
        _, status, _, _ = run_and_compare(eng, COUNTER, values, keys, lenient=False)
        assert list(status) == [DECODE_LITERAL, DECODE_OK]
        rows, status, _, _ = run_and_compare(eng, COUNTER, values, keys, lenient=True)
        assert list(status) == [DECODE_OK, DECODE_OK] and (rows[0] == rows[1]).all()
    assert not eng._reading_leniently
    with eng.reading_leniently():
        with eng.reading_leniently():  # blocks nest: the inner one does not end the outer one's mode
            pass
        _, status, _, _ = run_and_compare(eng, COUNTER, values, keys, lenient=False, expect=host_expectation(COUNTER, values, keys))
        assert list(status) == [DECODE_OK, DECODE_OK]
    assert eng._lib.surge_replay_set_decode_mode(eng._h, 2) == -1 and b"decode mode" in eng._lib.surge_replay_last_error(eng._h)
    assert eng._lib.surge_replay_set_decode_mode(eng._h, -1) == -1
    _, status, _, _ = run_and_compare(eng, COUNTER, values, keys, lenient=False)  # a refused setting changes nothing
    assert list(status) == [DECODE_LITERAL, DECODE_OK]


def test_a_template_the_mode_cannot_read_is_unsupported_and_nothing_is_written(eng):
    import torch

    flat = JsonTemplate((b"balance=", (2, 0), b"\n"))
    d, o = table([b"balance=1\n"])
    out = torch.full((1, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(ReplayError) as ei:
        decode_states(eng, flat, dev(d), dev(o), out=out, lenient=True)
    assert ei.value.status == -5 and "first literal" in str(ei.value) and "part 0" in str(ei.value)  # SURGE_E_UNSUPPORTED
    assert (out.cpu().numpy() == SENTINEL).all()
    assert decode_states(eng, flat, dev(d), dev(o), out=out)[2] == (1, 0, 0, 0)  # the strict mode reads it, and the mode went back


def test_a_v2_handle_takes_the_setting_and_refuses_the_decode_as_before():
    import torch

    from test_slots import LEDGER

    with ReplayEngine(LEDGER) as e:
        assert e._lib.surge_replay_set_decode_mode(e._h, 1) == 0
        d, o = table([b'{"balance":1}'])
        with pytest.raises(ReplayError) as ei:
            decode_states(e, SDK, dev(d), dev(o), out=torch.zeros((1, 64), dtype=torch.uint8, device="cuda"), lenient=True)
        assert ei.value.status == -5 and "ABI v1" in str(ei.value)


# ---- the wire path --------------------------------------------------------------------------------------------------------------
def fresh_engine():
    e = ReplayEngine()
    e.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
    e.fold()
    return e


def rewritten_topic(compression, seed=5, n_ids=300, n_records=1600, per_batch=90):
    """-> (list of batches' bytes, delivered (offset, key, rewritten value | None, compact value | None) in order): Counter states
    as ``state_topic_gen`` writes them, every value rewritten — reordered, spaced, one unknown member —, with the offset gaps
    compaction leaves, tombstones, and ids that come back after one."""
    from oracle import oracle

    rng = random.Random(seed)
    names = gen.ids_of(n_ids)
    ids = [k.encode("utf-8") for k in names]
    version, alive = [0] * n_ids, [False] * n_ids
    batches, delivered, base = [], [], rng.randrange(0, 1000)
    kept, compact, delta = [], [], 0

    def close(tail_gap):
        nonlocal base, kept, compact, delta, delivered
        data, recs, base = gen.compacted_batch(base, kept, compression, tail_gap=tail_gap)
        batches.append(data)
        delivered += [(o, k, v, c) for (o, k, v), c in zip(recs, compact)]
        kept, compact, delta = [], [], 0

    for _ in range(n_records):
        i = rng.randrange(n_ids)
        delta += 1 + rng.randrange(0, 3)  # gaps
        if alive[i] and rng.random() < 0.25:
            kept.append((delta, ids[i], None))
            compact.append(None)
            alive[i] = False
        else:
            version[i] += 1
            text = oracle.counter_state_json(names[i], rng.randrange(-10 ** 6, 10 ** 6), version[i])
            kept.append((delta, ids[i], L.rewritten(text, rng)))
            compact.append(text)
            alive[i] = True
        if len(kept) == per_batch:
            close(rng.randrange(0, 4))
    if kept:
        close(0)
    return batches, delivered


@pytest.mark.parametrize("compression,n_loads", [("lz4", 1), ("none", 3)])
def test_rewritten_values_from_record_batches_to_resident_states(compression, n_loads):
    batches, delivered = rewritten_topic(compression)
    assert any(v is None for _, _, v, _ in delivered)
    with fresh_engine() as e, DeviceDecoder(states=True) as d, EventsTopicIngest(frames=True, device_lz4=True) as g:
        totals = np.zeros(4, dtype=np.int64)
        for j in range(n_loads):
            g.feed(b"".join(batches[len(batches) * j // n_loads:len(batches) * (j + 1) // n_loads]))
            sec, arena = g.drain_sections()
            d.push_async([(sec, arena)])
            d.finish()
            totals += np.array(d.load_states_into(e, COUNTER, lenient=True))
        assert not e._reading_leniently
        keys = d.keys()
        got = e.device_state().cpu().numpy()
        # the same topic again through the strict mode: refused, as it has always been
        g.feed(batches[0])
        sec, arena = g.drain_sections()
        d.push_async([(sec, arena)])
        d.finish()
        with pytest.raises(IngestError) as ei:
            d.load_states_into(e, COUNTER)
        assert ei.value.status == -7
    last = {}
    for _, k, v, c in delivered:
        last[k.decode("utf-8")] = (v, c)
    assert keys == list(dict.fromkeys(k.decode("utf-8") for _, k, _, _ in delivered)) and got.shape[0] == len(keys)
    n_deleted = 0
    for i, k in enumerate(keys):
        v, c = last[k]
        if v is None:
            assert not got[i].any(), k
            n_deleted += 1
        else:
            rc, st, _ = decode_state_host(COUNTER, c, k, lenient=True)  # the compact text the value was rewritten from
            assert rc == DECODE_OK and got[i].tobytes() == st.tobytes(), k
            assert decode_state_host(COUNTER, c, k)[1].tobytes() == st.tobytes() and decode_state_host(COUNTER, v, k)[0] != DECODE_OK
    assert n_deleted >= 10 and totals[2] == 0 and totals[3] == 0
    if n_loads == 1:
        assert (int(totals[0]), int(totals[1])) == (len(keys) - n_deleted, n_deleted)
