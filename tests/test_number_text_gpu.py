"""-m gpu: the DEVICE compile of the number parser (surge_amd/csrc/f64_parse.h: section_kernel out of LDS and out of global
memory, the framed-records kernel, state_decode_kernel) and of the number writer (f64_text.h in the encoder kernels) at the
cases of tests/number_text_cases.py — ties, 19-digit significands at every exponent, the subnormal and overflow
boundaries, powers of two, the two-digit rule — and the two paths that hand a Double the device cannot decide back to
the host.  What is right: Python's ``float()`` / ``int()`` (correctly rounded), the host decoders (``EventJsonTemplate.decode``,
``decode_state_host``) for what is accepted and refused, and the host copy of the writer that tests/test_f64_text.py pins
on the oracle.  tests/test_number_text_cases.py holds the corpus to its claims (and the host parser to ``float()``) on the CPU.

The carriers are the smallest there are: an event value is ``{"v":<text>}``, a state value ``{"k":"<id>","v":<text>}``."""
import functools

import numpy as np
import pytest

import kafka_wire as kw
import number_text_cases as C
from oracle import oracle
from surge_amd import _native
from surge_amd import schema as S
from surge_amd.encode import (DECODE_AMBIGUOUS, DECODE_OK, DECODE_SKIPPED, JP_F64, JP_I32, JP_I64, JP_U32, JsonTemplate, decode_state_host, decode_states,
                              encode_states, key_table_utf8)
from surge_amd.ingest import ARG_F64, DeviceDecoder, EventJsonTemplate, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine

pytestmark = pytest.mark.gpu

EVENT = EventJsonTemplate("", [("", 0, "", "v", ARG_F64)])
STATE = JsonTemplate((b'{"k":', "KEY", b',"v":', (JP_F64, 16), b"}"))
BARE = JsonTemplate((b'{"v":', (JP_F64, 16), b"}"))
BANK = JsonTemplate.bank_account()
SENTINEL = 0xAB
LIMIT_TEXTS = [("1." + "0" * (n - 2), "1." + "0" * (n - 3) + "1") for n in (398, 399, 400, 401)]  # the dropped digits all zero | one of them not
MALFORMED = ["1.", "1e", "--1", "1.5.2", "1e5e5", "-", "+1", "1e+", "0x10", ".5"]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def event_value(text):
    return b'{"v":' + text.encode() + b"}"


def float_bits(texts):
    return np.array([C.bits_of(float(t)) for t in texts], dtype=np.uint64)


def record_key(i):
    return b"k%d:%d" % (i % 53, i)


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


# ---- events: the carriers ------------------------------------------------------------------------------------------------
def wire_of(texts, sizes):
    """Record batches of ``sizes[k % len(sizes)]`` records, every third one lz4; ``(wire, section bytes per batch)``."""
    batches, lens, at, k = [], [], 0, 0
    while at < len(texts):
        n = sizes[k % len(sizes)]
        recs = [(record_key(i), event_value(t)) for i, t in enumerate(texts[at:at + n], at)]
        lens.append(sum(len(kw.record(j, *r)) for j, r in enumerate(recs)))
        batches.append(kw.record_batch(at, recs, compression="lz4" if k % 3 == 1 else "none"))
        at += n
        k += 1
    return b"".join(batches), lens


def host_events(wire):
    with EventsTopicIngest() as g:
        g.feed(wire)
        agg, ev, off = g.drain_json(EVENT)
        return agg, ev, off, g.key_table().keys


def device_events_from_wire(wire, chunks=3):
    with EventsTopicIngest(frames=True, device_lz4=True) as g, DeviceDecoder(EVENT) as d:
        for c in range(chunks):  # a batch cut by a chunk's end is completed by the next feed
            g.feed(wire[c * len(wire) // chunks:(c + 1) * len(wire) // chunks])
            d.push_from(g)
        return results(d)


def device_events_from_records(texts, polls=2):
    with DeviceDecoder(EVENT) as d:
        for p in range(polls):
            lo, hi = p * len(texts) // polls, (p + 1) * len(texts) // polls
            d.push_records([record_key(i) for i in range(lo, hi)], [event_value(t) for t in texts[lo:hi]], list(range(lo, hi)))
        return results(d)


def results(d):
    agg, ev, off, n_keys = d.result()
    keys = d.keys()
    assert n_keys == len(keys)
    return agg.cpu().numpy(), ev.cpu().numpy().view(S.EVENT_DTYPE).reshape(-1), off.cpu().numpy(), keys, d.counters()


def check_events(got, host, texts, handed_back):
    agg, ev, off, keys, counters = got
    bits = ev["raw"].astype(np.uint64)
    want = float_bits(texts)
    assert bits.shape == want.shape
    bad = np.flatnonzero(bits != want)
    assert bad.size == 0, [(texts[i], hex(int(bits[i])), hex(int(want[i]))) for i in bad[:5]]
    assert keys == host[3] and agg.tobytes() == host[0].tobytes() and ev.tobytes() == host[1].tobytes() and off.tobytes() == host[2].tobytes()
    assert counters["doubles_parsed_on_host"] == handed_back and counters["records_delivered"] == len(texts)


@functools.lru_cache(maxsize=None)
def short_topic():
    """``decimal_texts()`` as a topic: batches for each of section_kernel's LDS classes (sections up to 8320 bytes, up to 16640,
    up to 64 KiB) and one beyond 64 KiB, which it parses out of global memory; and what the host decoder reads in it."""
    texts = C.decimal_texts()
    wire, lens = wire_of(texts, [150, 330, 64, 2200, 700, 1])
    assert min(lens) < 100 and sum(1 for n in lens if n <= 8320) > 5 and sum(1 for n in lens if 8320 < n <= 16640) > 5
    assert sum(1 for n in lens if 16640 < n <= 65536) > 5 and sum(1 for n in lens if n > 65536) >= 1
    return texts, wire, host_events(wire)


def test_the_record_kernel_parses_every_short_spelling_like_float_with_no_hand_back():
    """push_records in two polls: the parser over flat pointers, one lane per record."""
    texts, _, host = short_topic()
    check_events(device_events_from_records(texts), host, texts, 0)


def test_the_section_kernel_parses_every_short_spelling_like_float_out_of_lds_and_out_of_global_memory():
    """The wire path in three chunks, lz4 and plain batches: the parser over LDS pointers for the three staged classes, over a
    global pointer for the batch beyond 64 KiB."""
    texts, wire, host = short_topic()
    check_events(device_events_from_wire(wire), host, texts, 0)


def test_doubles_the_device_cannot_decide_are_patched_in_by_the_host_over_several_pushes_on_both_routes():
    """Every long spelling between ordinary records (eight of them for one long one), batches small and large: each push has
    its own list of handed-back records, the patch goes to the record's place in the grown result."""
    short = C.decimal_texts()[5::10]
    longs = C.long_texts()
    texts = []
    for i, t in enumerate(longs):
        texts += short[8 * i:8 * i + 8] + [t]
    texts += longs[:3]  # ... and three in a row at the very end
    wire, _ = wire_of(texts, [150, 40, 330, 1])
    host = host_events(wire)
    check_events(device_events_from_records(texts, polls=3), host, texts, len(longs) + 3)
    check_events(device_events_from_wire(wire, chunks=4), host, texts, len(longs) + 3)


def host_accepts(value):
    try:
        return EVENT.decode(value)
    except IngestError:
        return None


def check_one_by_one(texts, template=EVENT, value_of=event_value, payload_of=lambda t: C.bits_of(float(t))):
    """Each value in a push of its own behind a good record, through the records kernel and through the section kernel:
    what the host decoder refuses fails the push with CORRUPT and leaves the decoder exactly as it was — the same keys, the
    same results, usable, not poisoned; what it accepts decodes to the host's bytes and to ``payload_of``."""
    good = value_of("1.5") if template is EVENT else value_of("15")
    refused = accepted = 0
    with DeviceDecoder(template) as d, EventsTopicIngest(frames=True) as g:
        d.push_records([b"first:0"], [good])
        n, keys, offset = 1, ["first"], 1000
        for t in texts:
            value = value_of(t)
            try:
                want = template.decode(value)
            except IngestError:
                want = None
            for route in ("records", "wire"):
                def push():
                    if route == "records":
                        d.push_records([b"new-a:1", b"new-b:1"], [good, value], [offset, offset + 1])
                    else:
                        g.feed(kw.record_batch(offset, [(b"new-a:1", good), (b"new-b:1", value)]))
                        d.push_from(g)
                if want is None:
                    with pytest.raises(IngestError) as ei:
                        push()
                    assert ei.value.status == -7 and f"offset {offset + 1}" in str(ei.value), (t[:40], route, str(ei.value))
                    refused += 1
                else:
                    push()
                    n += 2
                    keys = list(dict.fromkeys(keys + ["new-a", "new-b"]))
                    ev = d.result()[1].cpu().numpy().view(S.EVENT_DTYPE).reshape(-1)
                    assert ev[-1].tobytes() == want.tobytes(), (t[:40], route)
                    assert int(ev[-1]["raw"]) == payload_of(t), (t[:40], route)
                    accepted += 1
                offset += 2
                assert d.keys() == keys and d.result()[0].shape[0] == n, (t[:40], route)  # a refused push interned and appended nothing
        d.push_records([b"last:0"], [good])  # still usable
        assert d.keys() == keys + ["last"] and d.result()[0].shape[0] == n + 1
    return accepted, refused


def test_a_number_of_400_bytes_is_refused_by_the_event_decoder_on_the_device_as_on_the_host():
    """The host refuses a number of 400 bytes or more before it parses (surge_parse_f64_json); so must the device, with an
    ordinary failed push — whether the digits it would drop are all zero (it could decide the value alone) or not (it would
    hand the record back, and the host would refuse what the device accepted)."""
    texts = [t for pair in LIMIT_TEXTS for t in pair]
    assert [len(t) for t in texts] == [398, 398, 399, 399, 400, 400, 401, 401]
    assert [host_accepts(event_value(t)) is not None for t in texts] == [True] * 4 + [False] * 4
    assert check_one_by_one(texts) == (8, 8)


def test_malformed_number_spellings_are_refused_by_the_event_decoder_on_the_device_as_on_the_host():
    accepted, refused = check_one_by_one(MALFORMED + ["1.0", "-1e5", "1E+2"])
    assert accepted == 6 and refused == 2 * len(MALFORMED)  # (the host refuses every one of them: tests/test_ingest_gpu.py pins the host parser)


def test_integer_spellings_at_the_edges_of_int_decode_on_the_device_as_on_the_host():
    from fixture_models import CounterBusinessLogic

    tmpl = CounterBusinessLogic().command_model().event_json_template()
    texts = sorted({t for kind in C.INT_RANGES for t in C.integer_texts(kind)})
    as_arg = lambda t: ('{"aggregateId":"a","incrementBy":%s,"sequenceNumber":7,"_type":"countIncremented"}' % t).encode()  # noqa: E731
    as_seq = lambda t: ('{"aggregateId":"a","incrementBy":15,"sequenceNumber":%s,"_type":"countIncremented"}' % t).encode()  # noqa: E731
    in_range = lambda t: C.int_or_none(t) is not None and -2 ** 31 <= C.int_or_none(t) < 2 ** 31  # noqa: E731
    n_ok = sum(in_range(t) for t in texts)
    assert n_ok >= 8 and len(texts) - n_ok >= 8
    # the argument travels as the low word of the payload, the sequence number in its own word: both are Python's int
    assert check_one_by_one(texts, tmpl, as_arg, lambda t: C.int_or_none(t) & 0xFFFFFFFF) == (2 * n_ok, 2 * (len(texts) - n_ok))
    assert check_one_by_one(texts, tmpl, as_seq, lambda t: 15) == (2 * n_ok, 2 * (len(texts) - n_ok))
    with DeviceDecoder(tmpl) as d:
        ok = [t for t in texts if in_range(t)]
        d.push_records([b"a:1"] * len(ok), [as_seq(t) for t in ok])
        ev = d.result()[1].cpu().numpy().view(S.EVENT_DTYPE).reshape(-1)
        assert ev["seq"].astype(np.int64).tolist() == [C.int_or_none(t) for t in ok]


# ---- states ------------------------------------------------------------------------------------------------------------
def values_table(texts):
    texts = [t or b"" for t in texts]
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return np.frombuffer(b"".join(texts), dtype=np.uint8).copy(), off


def host_expectation(template, texts, keys, agg_idx=None, n_agg=None):
    """What a call must leave behind, from the host decoder alone (the helper of tests/test_state_decode_gpu.py, with the STR
    spans of the values that decode): rows over sentinel rows, a status per record, counts, spans."""
    n = len(texts)
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
        text = texts[r] or b""
        if not text:
            rows[a], status[r] = 0, DECODE_OK
            tombs += 1
            continue
        rc, st, sp = decode_state_host(template, text, None if keys is None else keys[a])
        status[r] = rc
        if rc == DECODE_OK:
            rows[a] = np.frombuffer(st.tobytes(), dtype=np.uint8)
            spans[r] = sp
            written += 1
        else:
            refused += 1
    return rows, status, (written, tombs, refused), spans


def decode_and_compare(eng, template, texts, keys, agg_idx=None, n_agg=None, want_spans=False):
    import torch

    data, off = values_table(texts)
    kd, ko = (None, None) if keys is None else (dev(x) for x in key_table_utf8(keys))
    n_agg = len(texts) if n_agg is None else n_agg
    out = torch.full((n_agg, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    res = decode_states(eng, template, dev(data), dev(off), kd, ko, None if agg_idx is None else dev(np.asarray(agg_idx, dtype=np.int64)), out=out,
                        want_spans=want_spans)
    rows, status, counts, spans = host_expectation(template, texts, keys, agg_idx, n_agg)
    got_rows, got_status = res[0].cpu().numpy(), res[1].cpu().numpy()
    assert (got_status == status).all(), [(int(r), int(got_status[r]), int(status[r]), texts[r][:60]) for r in np.flatnonzero(got_status != status)[:5]]
    assert (got_rows == rows).all(), [(int(a), got_rows[a, 16:24].tobytes().hex(), rows[a, 16:24].tobytes().hex()) for a in np.flatnonzero((got_rows != rows).any(axis=1))[:5]]
    assert res[2][:3] == counts
    assert DECODE_AMBIGUOUS not in got_status  # transient: never left in the status array
    assert (res.refused is not None) == (counts[2] > 0)
    if counts[2]:
        first = int(np.flatnonzero((status != DECODE_OK) & (status != DECODE_SKIPPED))[0])
        assert f"{counts[2]} state value(s)" in res.refused and f"record {first} " in res.refused, res.refused
    if want_spans:
        ok = status == DECODE_OK
        assert (res.spans.cpu().numpy()[ok] == spans[ok]).all()
    return res, rows, status


@pytest.mark.parametrize("long_keys", [False, True], ids=["staged", "beyond the stage"])
def test_the_state_kernel_parses_every_short_spelling_like_float_with_no_hand_back(eng, long_keys):
    """state_decode_kernel out of its 32 KiB stage, and — with some 500-byte ids in every block — out of global memory."""
    texts = C.decimal_texts()
    n = len(texts)
    assert n % 256  # a partial last block
    keys = [f"k{i}" for i in range(n)]
    if long_keys:
        for i in range(0, n, 3):
            keys[i] = ("\x02long\"" * 40) + str(i)
    esc = lambda k: k.replace('"', '\\"').replace("\x02", "\\u0002")  # noqa: E731
    values = [b'{"k":"%s","v":%s}' % (esc(k).encode(), t.encode()) for k, t in zip(keys, texts)]
    if long_keys:
        off = values_table(values)[1]
        assert min(off[min(b + 256, n)] - off[b] for b in range(0, n - 256, 256)) > 32 * 1024 + 16
    res, rows, status = decode_and_compare(eng, STATE, values, keys)
    assert (status == DECODE_OK).all() and res[2] == (n, 0, 0, 0)  # not one Double handed back
    got = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)["balance"].view(np.uint64)
    want = float_bits(texts)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(texts[i], hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


def test_ambiguous_state_values_of_winners_losers_and_refused_winners_come_back_like_the_host_decodes_them(eng):
    """3 000 BankAccount records for 2 000 aggregates, one value in ten a Double of more than 19 digits: the device reports
    those AMBIGUOUS and the host settles them.  Some are losers (a later record of the aggregate wins: never parsed, never
    handed back, their value must not reach the row), some winners carry trailing bytes (the host refuses them: the row
    keeps the sentinel), and the aggregates named twice have an ambiguous record first, last, or both."""
    n_rec, n_agg = 3000, 2000
    rng = np.random.default_rng(31)
    longs, short = C.long_texts(), C.decimal_texts()[3::7]
    keys = [f"acct-{a}" for a in range(n_agg + 10)]  # the last ten are never named
    agg = np.concatenate([rng.permutation(n_agg), rng.integers(0, n_agg, size=n_rec - n_agg)])
    ambiguous = rng.random(n_rec) < 0.1
    garbage = ambiguous & (rng.random(n_rec) < 0.2)
    texts = []
    for r in range(n_rec):
        num = longs[r % len(longs)] if ambiguous[r] else short[r % len(short)]
        owner = f'O \\"{r}\\" \\u20ac' if r % 5 == 0 else f"Jane {r}"
        t = f'{{"accountNumber":"{keys[agg[r]]}","accountOwner":"{owner}","securityCode":"{r % 10000:04d}","balance":{num}}}'.encode()
        texts.append(t + (b" " if r % 2 else b"}") if garbage[r] else t)
    last = {}
    for r, a in enumerate(agg):
        last[int(a)] = r
    winners = np.zeros(n_rec, dtype=bool)
    winners[list(last.values())] = True
    assert (ambiguous & ~winners).sum() >= 30 and (ambiguous & winners & ~garbage).sum() >= 100 and (garbage & winners).sum() >= 20
    res, rows, status = decode_and_compare(eng, BANK, texts, keys, agg_idx=agg, n_agg=n_agg + 10, want_spans=True)
    assert res[2][3] == int((ambiguous & winners).sum())  # each ambiguous winner once, no loser
    assert res[2][2] == int((garbage & winners).sum())
    got = res[0].cpu().numpy()
    for r in np.flatnonzero(garbage & winners):
        assert got[agg[r]].tobytes() == bytes([SENTINEL]) * 64  # refused on the re-parse: the row is untouched
    for r in np.flatnonzero(ambiguous & winners & ~garbage):
        assert int(got[agg[r]].view(S.STATE_DTYPE)["balance"].view(np.uint64)[0]) == C.bits_of(float(longs[r % len(longs)]))
    assert (got[n_agg:] == SENTINEL).all()


def test_a_number_of_400_bytes_and_malformed_numbers_are_refused_by_the_state_decoder_on_the_device_as_on_the_host(eng):
    texts = [t for pair in LIMIT_TEXTS for t in pair] + MALFORMED + ["1.0", "-1e5"]
    values = [b'{"v":' + t.encode() + b"}" for t in texts]
    res, rows, status = decode_and_compare(eng, BARE, values, None)
    assert status[:4].tolist() == [DECODE_OK] * 4 and (status[4:8] != DECODE_OK).all()
    assert (status[8:8 + len(MALFORMED)] != DECODE_OK).sum() == len(MALFORMED) - 1  # (a leading '+' is read, as the parser's comment says)
    assert res[2][3] == 2  # the 398- and the 399-byte number with a digit the fast path drops
    got = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)["balance"].view(np.uint64)
    for i in np.flatnonzero(status == DECODE_OK):
        assert int(got[i]) == C.bits_of(float(texts[i])), texts[i][:40]


def test_integer_spellings_at_the_edges_of_each_type_decode_in_state_parts_on_the_device_as_on_the_host(eng):
    tmpl = JsonTemplate((b'{"a":', (JP_I32, 0), b',"b":', (JP_U32, 4), b',"c":', (JP_I64, 8), b"}"))
    values, want = [], []
    for field, kind in enumerate(("I32", "U32", "I64")):
        lo, hi = C.INT_RANGES[kind]
        for t in C.integer_texts(kind):
            parts = ["0", "0", "0"]
            parts[field] = t
            values.append(('{"a":%s,"b":%s,"c":%s}' % tuple(parts)).encode())
            v = C.int_or_none(t)
            want.append((field, v if v is not None and lo <= v <= hi else None))
    res, rows, status = decode_and_compare(eng, tmpl, values, None)
    got = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
    for i, (field, v) in enumerate(want):
        assert (status[i] == DECODE_OK) == (v is not None), values[i]  # accepted exactly when it is an integer of the type
        if v is not None:
            word = (int(got["count"][i]), int(got["version"].view(np.uint32)[i]), int(got["sum64"][i]))[field]
            assert word == v, values[i]


# ---- the writer --------------------------------------------------------------------------------------------------------
def test_the_encoder_kernels_write_every_double_like_the_host_copy_and_the_oracle_and_read_them_back():
    """``double_bits()`` as BankAccount balances (one Created event per aggregate: the payload is copied bit for bit), the
    aggregate count no multiple of the encoder's 256-lane blocks; both passes of the encoder (lengths, then text) run
    f64_play_json_text — Ryu, BigDecimal's layout, the two-digit rule's floating-point product and divisions."""
    from fixture_models import BANK_ACCOUNT_ALGEBRA, BA_CREATED

    cls = C.bit_classes()
    bits = C.double_bits()
    n = bits.shape[0]
    assert n % 256
    ev = np.zeros(n, dtype=S.EVENT_DTYPE)
    ev["type"], ev["raw"] = BA_CREATED, bits
    lib = _native.load()
    host_out = np.zeros(n * 26 + 1, np.uint8)
    host_off = np.zeros(n + 1, np.int64)
    total = lib.surge_format_f64_json_many(bits.ctypes.data, n, host_out.ctypes.data, host_out.nbytes, host_off.ctypes.data)
    with ReplayEngine(BANK_ACCOUNT_ALGEBRA) as e:
        e.load_csr(np.arange(n + 1, dtype=np.int64), ev)
        e.fold()
        assert e.snapshot()["balance"].view(np.uint64).tobytes() == bits.tobytes()
        ko = dev(np.zeros(n + 1, dtype=np.int64))
        d_out, d_off = encode_states(e, BARE, dev(np.zeros(0, np.uint8)), ko)
        res = decode_states(e, BARE, d_out, d_off)
    out, off = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy()
    assert off[0] == 0 and off[-1] == len(out) == total + 6 * n and (np.diff(off) == np.diff(host_off) + 6).all()  # {"v": and }
    host = host_out[:total].tobytes()
    at = 0
    for name, part in cls.items():
        check_oracle = name in ("powers of two", "powers of ten", "mantissas 1 to 5000")
        for a in range(at, at + part.shape[0]):
            text = out[off[a]:off[a + 1]]
            assert text[:5] == b'{"v":' and text[-1:] == b"}", (name, a, text)
            assert text[5:-1] == host[host_off[a]:host_off[a + 1]], (name, hex(int(bits[a])), text)
            if check_oracle:
                assert text[5:-1].decode() == oracle.play_json_double_text(float(bits[a:a + 1].view(np.float64)[0])), (name, hex(int(bits[a])), text)
        at += part.shape[0]
    assert at == n
    # ... and back through the device parser: the same bits, but for -0.0, which is written as 0
    want = bits.copy()
    assert (want == np.uint64(1 << 63)).any()
    want[want == np.uint64(1 << 63)] = 0
    got = res[0].cpu().numpy().view(S.STATE_DTYPE).reshape(-1)["balance"].view(np.uint64)
    assert (res[1].cpu().numpy() == DECODE_OK).all() and res[2] == (n, 0, 0, 0) and res.refused is None
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(want[i])), hex(int(got[i])), out[off[i]:off[i + 1]]) for i in bad[:5]]
