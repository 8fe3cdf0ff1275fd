"""The device state decoder (``surge_replay_decode_json_states``) against the encoders it inverts, against the host
restatement of its parser (``surge_decode_json_state``), and behind ``GpuReplayStateStore.restore_from_state_records``.

Shapes are the smallest at which the kernel takes each of its paths: one block, a partial last block, several blocks, a
block span beyond the 32 KiB stage (parses from global), every 16-byte alignment of the value buffer."""
import ctypes
import json

import numpy as np
import pytest

from oracle import oracle
from surge_amd import schema as S
from surge_amd import synth
from surge_amd.encode import (DECODE_AMBIGUOUS, DECODE_OK, DECODE_SKIPPED, JP_I32, JsonTemplate, decode_state_host, decode_states, encode_states,
                              key_table_utf8)
from surge_amd.replay import ReplayEngine, ReplayError

pytestmark = pytest.mark.gpu

COUNTER, BANK = JsonTemplate.counter(), JsonTemplate.bank_account()
SENTINEL = 0xAB  # what the rows hold before a call: "untouched" is checkable


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def values_table(texts):
    """(uint8 data, int64 offsets) of record values; ``None`` / ``b""`` = a null value."""
    texts = [t or b"" for t in texts]
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return np.frombuffer(b"".join(texts), dtype=np.uint8).copy(), off


def sentinel_rows(n):
    import torch

    return torch.full((n, 64), SENTINEL, dtype=torch.uint8, device="cuda")


def host_expectation(template, texts, keys, agg_idx=None, n_agg=None):
    """What the call must leave behind, from the host decoder alone: (rows as uint8[n_agg, 64] over sentinel rows, status
    per record, counts)."""
    n = len(texts)
    agg_idx = list(range(n)) if agg_idx is None else list(agg_idx)
    n_agg = n if n_agg is None else n_agg
    rows = np.full((n_agg, 64), SENTINEL, dtype=np.uint8)
    status = np.full(n, DECODE_SKIPPED, dtype=np.uint8)
    last = {}
    for r, a in enumerate(agg_idx):
        last[a] = r
    written = tombs = refused = 0
    for a, r in last.items():
        text = texts[r] or b""
        if not text:
            rows[a], status[r] = 0, DECODE_OK
            tombs += 1
            continue
        rc, st, _ = decode_state_host(template, text, None if keys is None else keys[a])
        status[r] = rc
        if rc == DECODE_OK:
            rows[a] = np.frombuffer(st.tobytes(), dtype=np.uint8)
            written += 1
        else:
            refused += 1
    return rows, status, (written, tombs, refused)


def run_and_compare(eng, template, texts, keys, agg_idx=None, n_agg=None, shift=0, expect=None):
    """Decode on the device (value buffer starting ``shift`` bytes behind a 16-byte boundary) and hold rows, statuses, counts
    and the return code to the host decoder."""
    import torch

    data, off = values_table(texts)
    buf = torch.zeros(data.shape[0] + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d_values = buf[shift:shift + data.shape[0]]
    d_values.copy_(torch.from_numpy(data))
    kd, ko = (None, None) if keys is None else (dev(x) for x in key_table_utf8(keys))
    n_agg = len(texts) if n_agg is None else n_agg
    out = sentinel_rows(n_agg)
    res = decode_states(eng, template, d_values, dev(off), kd, ko, None if agg_idx is None else dev(np.asarray(agg_idx, dtype=np.int64)), out=out)
    rows, status, counts = expect or host_expectation(template, texts, keys, agg_idx, n_agg)
    got_rows, got_status = res[0].cpu().numpy(), res[1].cpu().numpy()
    assert (got_status == status).all(), np.flatnonzero(got_status != status)[:10]
    assert (got_rows == rows).all(), np.flatnonzero((got_rows != rows).any(axis=1))[:10]
    assert res[2][:3] == counts
    assert (res.refused is not None) == (counts[2] > 0)  # SURGE_E_CORRUPT exactly when a winner was refused
    if counts[2]:
        first = int(np.flatnonzero((status != DECODE_OK) & (status != DECODE_SKIPPED))[0])
        assert f"{counts[2]} state value(s)" in res.refused and f"record {first} " in res.refused, res.refused
    return res


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


def test_counter_states_survive_encode_then_decode():
    """The log of test_gpu_json_encoder_matches_play_json_text_of_the_counter_fixture: text from the device encoder, back
    through the device decoder with the identity mapping.  PRESENT aggregates get count / version / flags back; None and
    poisoned aggregates have no text (a null value) and come back None."""
    n = 5000
    rng = np.random.default_rng(11)
    keys = [f"agg-{i:05d}" for i in range(n)]
    keys[7], keys[8], keys[9], keys[10] = 'we"ird\\id', "tab\there\nnl", "ünï-✓-ключ", "\x01\x1f"
    lens = rng.integers(0, 12, size=n)
    so, ev = synth.csr_log(lens, 12, synth.STRESS_MIX)
    ev["raw"][(ev["type"] == S.EVT_INC) & (rng.random(ev.shape[0]) < 0.3)] = np.uint64(np.uint32(np.int32(-7)))
    with ReplayEngine() as e:
        e.load_csr(so, ev)
        e.fold()
        states = e.snapshot()
        kd, ko = (dev(x) for x in key_table_utf8(keys))
        d_out, d_off = encode_states(e, COUNTER, kd, ko)
        res = decode_states(e, COUNTER, d_out, d_off, kd, ko)
    got = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
    present = states["flags"] == S.STATE_PRESENT
    assert 0 < present.sum() < n and (states["flags"] & S.STATE_POISONED).any()
    for f in ("count", "version", "flags"):
        assert (got[f][present] == states[f][present]).all()
    assert not got[~present].tobytes().strip(b"\0")  # None and poisoned rows: the canonical None
    assert res[2] == (int(present.sum()), int(n - present.sum()), 0, 0) and res.refused is None
    assert (res[1].cpu().numpy() == DECODE_OK).all()


def test_bank_account_states_survive_encode_then_decode_with_the_owner_and_code_spans():
    import uuid

    from fixture_models import BANK_ACCOUNT_ALGEBRA, BA_CREATED, BA_UPDATED

    n = 20000  # the states of test_gpu_json_encoder_writes_bank_account_states_with_play_json_double_text
    rng = np.random.default_rng(21)
    keys = [str(uuid.UUID(int=int(x))) for x in rng.integers(0, 1 << 62, size=n)]
    owners = [f"Owner {i} \"q\" ünï" if i % 97 == 0 else f"Jane Doe {i}" for i in range(n)]
    codes = ["" if i % 50 == 0 else f"{i % 10000:04d}" for i in range(n)]
    two = rng.random(n) < 0.5
    so = np.zeros(n + 1, np.int64)
    np.cumsum(1 + two.astype(np.int64), out=so[1:])
    ev = np.zeros(int(so[-1]), dtype=S.EVENT_DTYPE)
    ev["type"][so[:-1]] = BA_CREATED
    ev["type"][so[:-1][two] + 1] = BA_UPDATED
    kinds = rng.integers(0, 6, size=ev.shape[0])
    vals = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4],
                     [np.round(rng.random(ev.shape[0]) * 1e7) / 100, rng.integers(-10 ** 6, 10 ** 6, size=ev.shape[0]).astype(np.float64),
                      rng.random(ev.shape[0]) * 10.0 ** rng.integers(-12, 25, size=ev.shape[0]), rng.standard_normal(ev.shape[0]) * 1e3,
                      rng.choice([0.0, -0.0, 1e20, 1e-7, 5e-324, 1.7976931348623157e308, 0.1 + 0.2, 1e21, 100.0], size=ev.shape[0])],
                     default=rng.integers(0, 0x7FF0000000000000, size=ev.shape[0], dtype=np.uint64).view(np.float64))
    ev["raw"] = vals.view(np.uint64)
    bad = rng.choice(ev.shape[0], size=25, replace=False)
    ev["raw"][bad] = rng.choice(np.array([0x7FF8000000000000, 0x7FF0000000000000, 0xFFF0000000000000], dtype=np.uint64), size=25)
    with ReplayEngine(BANK_ACCOUNT_ALGEBRA) as e:
        e.load_csr(so, ev)
        e.fold()
        states = e.snapshot()
        kd, ko = (dev(x) for x in key_table_utf8(keys))
        cols = [tuple(dev(x) for x in key_table_utf8(col)) for col in (owners, codes)]
        nonfinite = ~np.isfinite(states["balance"])
        assert 0 < nonfinite.sum() <= 25
        kind = dev(np.where(nonfinite, 0, 1).astype(np.uint8))  # the non-finite aggregates have no JSON text: filtered out
        e._check(e._lib.surge_replay_set_encode_filter(e._h, ctypes.c_void_p(kind.data_ptr())))
        d_out, d_off = encode_states(e, BANK, kd, ko, strings=cols)
        e._check(e._lib.surge_replay_set_encode_filter(e._h, None))
        res = decode_states(e, BANK, d_out, d_off, kd, ko, want_spans=True)
    got = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
    want_bits = states["balance"].view(np.uint64).copy()
    minus_zero = want_bits == np.uint64(1 << 63)
    assert minus_zero.any()
    want_bits[minus_zero] = 0  # the one exception: -0.0 is written as 0
    ok = ~nonfinite
    assert (got["balance"].view(np.uint64)[ok] == want_bits[ok]).all()
    assert (got["flags"][ok] == S.STATE_PRESENT).all() and not got[nonfinite].tobytes().strip(b"\0")
    assert res[2][:3] == (int(ok.sum()), int(nonfinite.sum()), 0) and res.refused is None
    text, offs, spans = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy(), res.spans.cpu().numpy()
    for a in np.flatnonzero(ok):
        v = text[offs[a]:offs[a + 1]]
        (o0, l0), (o1, l1) = spans[a, 0], spans[a, 1]
        assert json.loads(b'"' + v[o0:o0 + l0] + b'"') == owners[a] and json.loads(b'"' + v[o1:o1 + l1] + b'"') == codes[a], a


def damaged(text: bytes, kind: int, rng) -> bytes:
    pick = lambda options: options[int(rng.integers(len(options)))]  # noqa: E731
    if kind == 0:  # truncation
        return text[:int(rng.integers(1, len(text)))]
    if kind == 1:  # a wrong literal byte (the opening brace, or the field name's first letter)
        return (b"[" + text[1:]) if rng.random() < 0.5 else (text[:2] + b"X" + text[3:])
    if kind == 2:  # an integer / number that overflows or is none
        head, _, tail = text.rpartition(b":")
        return head + b":99999999999999999999" + tail[tail.index(b"}"):] if b"version" in text else head + b":1e" + tail[tail.index(b"}"):]
    if kind == 3:  # a bad escape inside the first string
        at = text.index(b'":"') + 3
        return text[:at] + pick([b"\\x", b"\\u12G4", b"\\ud800", b"\\"]) + text[at:]
    return text + pick([b" ", b"}", b"\x00", b"garbage"])  # trailing bytes


@pytest.mark.parametrize("which", ["counter", "bank_account"])
def test_device_and_host_agree_on_every_record_of_a_batch_with_damaged_values(eng, which):
    n = 3000
    rng = np.random.default_rng(5 if which == "counter" else 6)
    if which == "counter":
        keys = [f"agg-{i:05d}" if i % 9 else f'k"{i}\\\n\x03é' for i in range(n)]
        texts = [oracle.counter_state_json(k, int(c), int(v)) for k, c, v in zip(keys, rng.integers(-2**31, 2**31, size=n), rng.integers(-2**31, 2**31, size=n))]
        template = COUNTER
    else:
        keys = [f"acct-{i}" for i in range(n)]
        bal = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 20, size=n)
        texts = [f'{{"accountNumber":"{k}","accountOwner":{json.dumps("O " + chr(0x20ac) * (i % 3) + str(i), ensure_ascii=i % 2 == 0)},'
                 f'"securityCode":"{i % 10000:04d}","balance":{oracle.play_json_double_text(float(b))}}}'.encode() for i, (k, b) in enumerate(zip(keys, bal))]
        # one Double the device cannot decide (more than 19 digits): handed back, re-parsed by the host export, patched in
        texts[1234] = texts[1234].rpartition(b":")[0] + b":0.1000000000000000055511151231257827021181583404541015625}"
        template = BANK
    hit = rng.choice(n, size=n // 20, replace=False)  # about 5 %
    hit = hit[hit != 1234]
    for j, r in enumerate(hit):
        texts[r] = damaged(texts[r], j % 5, rng)
    res = run_and_compare(eng, template, texts, keys)
    assert res[2][2] >= len(hit) * 0.9 and res[2][3] == (1 if which == "bank_account" else 0)
    assert DECODE_AMBIGUOUS not in res[1].cpu().numpy()  # transient: never left in the status array
    # a key table that does not match is reported per record, too
    keys[3] = keys[3] + "x"
    run_and_compare(eng, template, texts, keys)
    run_and_compare(eng, template, texts, None)


@pytest.mark.parametrize("n,long_every", [(1, 0), (255, 0), (256, 0), (257, 0), (1500, 0), (1500, 3)])
def test_block_staging_at_every_alignment_and_the_fallback_for_spans_beyond_the_stage(eng, n, long_every):
    rng = np.random.default_rng(n * 7 + long_every)
    keys = [f"k{i}" * (1 + i % 5) for i in range(n)]
    if long_every:
        for i in range(0, n, long_every):
            keys[i] = ("\x02long\"" * 40) + str(i)  # ~500 bytes of escapes: 86 of them put a block's span beyond 32 KiB
    texts = [oracle.counter_state_json(k, int(c), i) for i, (k, c) in enumerate(zip(keys, rng.integers(-1000, 1000, size=n)))]
    for r in rng.choice(n, size=max(1, n // 16), replace=False):
        texts[r] = None if r % 2 else texts[r][:-1]  # null values and damage in every block, the last (partial) one included
    texts[-1] = texts[-1] if texts[-1] is None else texts[-1][:-1]
    if long_every:
        data, off = values_table(texts)
        spans = [off[min(b + 256, n)] - off[b] for b in range(0, n, 256)]
        assert max(spans) > 32 * 1024 + 16  # these blocks parse straight from global ...
    expect = host_expectation(COUNTER, texts, keys)  # once: the same for every alignment
    for shift in range(16):
        run_and_compare(eng, COUNTER, texts, keys, shift=shift, expect=expect)


MOCK_STATE = JsonTemplate((b'{"string":', "KEY", b',"int":', (JP_I32, 0), b"}"))  # MockState(string, int).toJsString


def test_the_last_record_per_aggregate_wins_in_the_reference_sequence(eng):
    # AggregateStateStoreKafkaStreamsSpec.scala:64-85: four keys piped in, then state1 again with another value
    keys = ["state1", "state2", "state3", "invalidValidation"]
    seq = [("state1", 1), ("state2", 2), ("state3", 3), ("invalidValidation", 1), ("state1", 3)]
    texts = [json.dumps({"string": k, "int": v}, separators=(",", ":")).encode() for k, v in seq]
    res = run_and_compare(eng, MOCK_STATE, texts, keys, agg_idx=[keys.index(k) for k, _ in seq], n_agg=4)
    rows = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
    assert list(rows["count"]) == [3, 2, 3, 1] and res[2] == (4, 0, 0, 0)
    assert list(res[1].cpu().numpy()) == [DECODE_SKIPPED, 0, 0, 0, 0]


def test_keep_last_against_log_compaction_on_a_fuzzed_topic_with_tombstones_and_re_created_ids(eng):
    from surge_amd.snapshot import StateRecord, compact

    n_agg, n_rec = 300, 2000
    rng = np.random.default_rng(77)
    keys = [f"agg-{i}" if i % 7 else f'a"{i}\\' for i in range(n_agg + 20)]  # the last 20 are never named: rows untouched
    agg = rng.integers(0, n_agg, size=n_rec)
    texts = [None if rng.random() < 0.10 else oracle.counter_state_json(keys[a], r, r + 1) for r, a in enumerate(agg)]
    # ids re-created after a tombstone, and ids whose last word is the tombstone
    for a in range(0, 40, 2):
        r0, r1 = n_rec + a, n_rec + a + 1
        agg = np.append(agg, [a, a])
        texts += [None, oracle.counter_state_json(keys[a], r0, r1)] if a % 4 else [oracle.counter_state_json(keys[a], r0, r1), None]
    res = run_and_compare(eng, COUNTER, texts, keys, agg_idx=agg, n_agg=n_agg + 20)
    table = compact(StateRecord("t", 0, keys[a], t) for a, t in zip(agg, texts))
    rows = res[0].cpu().numpy()
    for a, k in enumerate(keys):
        if k in table:
            rc, st, _ = decode_state_host(COUNTER, table[k], k)
            assert rc == DECODE_OK and rows[a].tobytes() == st.tobytes(), a
        elif a in set(agg.tolist()):
            assert rows[a].tobytes() == bytes(64), a  # deleted: the canonical None
        else:
            assert rows[a].tobytes() == bytes([SENTINEL]) * 64, a
    assert res[2][1] >= 10  # tombstones that won


def test_two_thousand_records_of_one_aggregate_and_a_malformed_loser(eng):
    n = 2000
    keys = ["only", "other"]
    texts = [oracle.counter_state_json("only", r, -r) for r in range(n)]
    texts[17] = b'{"aggregateId":"only","count":oops'  # a loser: never parsed, never reported
    res = run_and_compare(eng, COUNTER, texts, keys, agg_idx=[0] * n, n_agg=2)
    rows = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
    assert int(rows["count"][0]) == n - 1 and int(rows["version"][0]) == -(n - 1) and res[2] == (1, 0, 0, 0) and res.refused is None
    status = res[1].cpu().numpy()
    assert status[-1] == DECODE_OK and (status[:-1] == DECODE_SKIPPED).all()


def test_an_aggregate_index_out_of_range_is_refused_and_nothing_is_written(eng):
    keys = [f"k{i}" for i in range(8)]
    texts = [oracle.counter_state_json(keys[i % 8], i, i) for i in range(600)]
    data, off = values_table(texts)
    kd, ko = (dev(x) for x in key_table_utf8(keys))
    for bad_value in (8, -1, 1 << 40):
        agg = np.arange(600, dtype=np.int64) % 8
        agg[431] = bad_value
        out = sentinel_rows(8)
        with pytest.raises(ReplayError) as ei:
            decode_states(eng, COUNTER, dev(data), dev(off), kd, ko, dev(agg), out=out)
        assert ei.value.status == -1 and "d_agg_idx" in str(ei.value)
        assert (out.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ReplayError) as ei:  # the identity mapping needs a row per record
        decode_states(eng, COUNTER, dev(data), dev(off), None, None, None, out=sentinel_rows(8))
    assert ei.value.status == -1


def test_resume_from_state_records_plus_the_events_tail_equals_the_full_refold_and_the_oracle():
    """Counter model, 1500 Zipf aggregates, no throwing events.  Store A folds the first part of every aggregate's events and
    publishes its snapshot (tombstones for the aggregates that are still None); a fresh store resumes from those records
    and folds the rest.  Every byte of every row equals the one-shot fold of all events and the CPU oracle — and right
    after the load, before the tail, there is nothing to publish: the loaded states are the baseline."""
    import torch

    from fixture_models import CountDecremented, CounterBusinessLogic, CountIncremented, NoOpEvent
    from surge_amd.log import KeyTable, pack_events
    from surge_amd.snapshot import SnapshotWriter
    from surge_amd.store import GpuReplayStateStore

    n = 1500
    rng = np.random.default_rng(3)
    lens = np.minimum(synth.zipf_lengths(np.arange(n, dtype=np.int64), 3), 24) * (rng.random(n) < 0.9)
    ids = [f"agg-{i}" if i % 11 else f'q"{i}\\t\x05ü' for i in range(n)]
    owner = rng.permutation(np.repeat(np.arange(n), lens))  # offset order: the aggregates' events interleaved
    seq = np.zeros(n, dtype=np.int64)
    events = []
    for a in owner:
        seq[a] += 1
        k = int(rng.integers(0, 3))
        arg = int(rng.integers(-50, 50))
        events.append(NoOpEvent(ids[a], int(seq[a])) if k == 0 else (CountIncremented if k == 1 else CountDecremented)(ids[a], arg, int(seq[a])))
    first_part = np.ceil(lens * rng.random(n)).astype(np.int64)  # how many of an aggregate's events the snapshot holds (0: still None)
    first_part[-30:] = 0
    seen = np.zeros(n, dtype=np.int64)
    head, tail = [], []
    for a, e in zip(owner, events):
        seen[a] += 1
        (head if seen[a] <= first_part[a] else tail).append(e)
    known = [ids[a] for a in range(n - 30)]  # the last 30 ids first appear in the tail: the resident state grows for them
    bl = CounterBusinessLogic()
    model = bl.command_model()

    def key_table():
        kt = KeyTable()
        for k in known:
            kt.intern(k)
        return kt

    stores = []
    try:
        a_store = GpuReplayStateStore(bl)
        stores.append(a_store)
        a_store.restore_log(pack_events(model, head, key_table()))
        records = SnapshotWriter(a_store, 4).full_snapshot()
        assert len(records) == len(known) and any(r.value is None for r in records) and sum(r.value is not None for r in records) > 1000

        full = GpuReplayStateStore(bl)  # the one-shot fold of everything, same dense indices
        stores.append(full)
        full.keys = key_table()
        full.restore(head + tail)
        want = full.engine.snapshot()
        log = pack_events(model, head + tail, key_table())
        assert want.tobytes() == oracle.fold_csr(log.seg_off, log.events, None, model.event_algebra()).tobytes()

        resumed = GpuReplayStateStore(bl)
        stores.append(resumed)
        counts = resumed.restore_from_state_records(records, events_tail=tail)
        assert counts["refused"] == 0 and counts["rows_written"] + counts["tombstones"] == len(records)
        assert resumed.keys.keys == full.keys.keys
        assert resumed.engine.snapshot().tobytes() == want.tobytes()  # all 64 bytes of every row
        assert resumed.get_aggregate(ids[3]) == full.get_aggregate(ids[3])

        staged = GpuReplayStateStore(bl)  # the same in two steps, to look between them
        stores.append(staged)
        staged.restore_from_state_records(((r.key, r.value) for r in records))
        d_kind = torch.zeros(staged.engine.n_agg, dtype=torch.uint8, device="cuda")
        nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
        staged.engine._check(staged.engine._lib.surge_replay_snapshot_delta(staged.engine._h, ctypes.c_void_p(d_kind.data_ptr()), ctypes.byref(nv), ctypes.byref(nt), 0))
        assert (nv.value, nt.value) == (0, 0) and not d_kind.any()  # nothing to publish: what was loaded is what is published
        head_only = a_store.engine.snapshot()
        assert staged.engine.snapshot().tobytes() == head_only.tobytes()  # the load alone restores A's rows, defaults included
        staged.apply_events(tail)
        assert staged.engine.snapshot().tobytes() == want.tobytes()
    finally:
        for s in stores:
            s.close()
