"""-m gpu: ``DeviceDecoder.push_records_async`` — the framed-records stage at block counts around its launch's 256 records, at
every alignment of a block's key bytes and of the values' base, over a sweep of sizes, at the keys and values it branches on — and
the slot queue with records pushes in it, also with one thread pushing while another finishes.  Every device result is held to
``records_push_cases.expected`` (the host decode of the same records with the test's own ids, offsets and first-delivered order),
and where the wire route can carry the records, to that route too; what is about the asynchronous call is also held to the
synchronous ``push_records``.  Every push is a few hundred records."""
import numpy as np
import pytest

import event_envelope_cases as env
import event_strings_cases as esc
import number_text_cases as numbers
import records_push_cases as C
from surge_amd.ingest import ARG_F64, ARG_I32, DeviceDecoder, EventJsonTemplate, EventsTopicIngest, IngestError

pytestmark = pytest.mark.gpu

E_STATE, E_CORRUPT = -2, -7
TYPED = EventJsonTemplate("t", [("a", 0, "", "v", ARG_I32), ("b", 1, "", "v", ARG_I32)])
ENVELOPED = EventJsonTemplate("", [("", 0, "", "v", ARG_I32)], envelope="protobuf_event")
DOUBLES = EventJsonTemplate("", [("", 0, "", "v", ARG_F64)])


def pushed_async(template, keys, values, offsets=None, as_arrays=False, states=False):
    """One asynchronous push on a fresh decoder, finished without the closing wait -> the result, and the counters."""
    with DeviceDecoder(template, states=states) as d:
        if as_arrays:
            d.push_records_async(C.arrays(keys), C.arrays(values), offsets)
        else:
            d.push_records_async(keys, values, offsets)
        assert d.pending == 1
        d.finish(wait=False)
        assert d.pending == 0
        return (C.state_result_of(d)[:4] if states else C.result_of(d)), d.counters()


def records(n, ids=37, length=lambda i: 0):
    keys = [b"id-%d:%d" % (i % ids, i) for i in range(n)]
    return keys, [C.value(i - n // 2, length(i)) for i in range(n)]


# ---- the kernel at its edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_a_push_of_n_records_is_what_the_host_decodes_and_what_the_wire_route_delivers(n):
    keys, values = records(n, length=lambda i: 0 if i % 3 else 20 + i % 50)
    offsets = [10 + 3 * i for i in range(n)]
    want = C.expected(C.EVENT, keys, values, offsets)
    got, counters = pushed_async(C.EVENT, keys, values, offsets, as_arrays=n % 2 == 0)
    assert got == want
    assert got == C.wire_result(C.EVENT, keys, values, offsets)
    assert counters["records_seen"] == n and counters["records_delivered"] == n


def test_the_spans_of_the_second_and_third_block_start_at_every_residue_and_so_do_the_values():
    """Key lengths chosen so that the key spans of blocks 1 and 2 start at each of the 16 residues of a 16-byte line, and the
    push's key bytes — where its values begin — take each of the 16 residues."""
    seen = [set(), set(), set()]
    with DeviceDecoder(C.EVENT) as d:
        known, all_want = [], ([], b"", [])
        for r in range(16):
            keys, values = records(520, ids=41, length=lambda i: 0 if i % 2 else 20 + (i * 7) % 40)
            key_bytes = lambda lo, hi: sum(len(k) for k in keys[lo:hi])  # noqa: E731
            for lo, hi, at, residue in ((0, 256, 5, r), (0, 512, 300, (r + 3) % 16), (0, 520, 515, (r + 11) % 16)):
                pad = (residue - key_bytes(lo, hi)) % 16
                keys[at] = b"z" * pad + keys[at]  # a longer id in front of the colon
                assert key_bytes(lo, hi) % 16 == residue
            for s, bound in zip(seen, (256, 512, 520)):
                s.add(key_bytes(0, bound) % 16)
            offsets = list(range(1000 * r, 1000 * r + 520))
            want = C.expected(C.EVENT, keys, values, offsets, known=known)
            d.push_records_async(keys, values, offsets)
            d.finish(wait=False)
            known = want[3]
            all_want = (all_want[0] + want[0], all_want[1] + want[1], all_want[2] + want[2])
        assert C.result_of(d) == (*all_want, known)
    assert all(s == set(range(16)) for s in seen)


@pytest.mark.parametrize("total", [24 << 10, 64 << 10])
def test_size_sweep_one_block_of_24_and_of_64_kib_and_each_a_byte_larger(total):
    """More sizes, nothing else: 256 records of ``total`` bytes and of one byte more in front of a small second block."""
    keys, values = C.one_block_of(total)
    tail_keys, tail_values = records(40)
    for extra in (0, 1):
        vals = values[:-1] + [C.value(255, len(values[-1]) + extra)]
        got, _ = pushed_async(C.EVENT, keys + tail_keys, vals + tail_values, as_arrays=True)
        assert got == C.expected(C.EVENT, keys + tail_keys, vals + tail_values)


def test_size_sweep_a_one_mebibyte_value_between_blocks_of_a_few_kilobytes():
    keys, values = records(700, length=lambda i: 0 if i % 4 else 20 + i % 30)
    values[300] = C.value(300, 1 << 20)
    got, _ = pushed_async(C.EVENT, keys, values, as_arrays=True)
    assert got == C.expected(C.EVENT, keys, values)


def test_keys_with_the_colon_at_either_end_without_one_empty_and_long_ids_and_the_flush_record():
    long_a, long_b = b"L" * 253 + b"ab", b"L" * 253 + b"bb"  # 255 bytes, different in byte 253
    keys = [b":first", b"last:", b"no-colon", b"", long_a + b":1", long_b + b":2", b"", long_a + b":3", b"last:again", b"::", b"", b"no-colon:9"]
    values = [C.value(i) for i in range(len(keys))]
    values[6], values[10] = b"", b""  # the producer's flush record: empty key AND empty value (records 3 has an empty key and a value)
    gaps = [5, 6, 7, 100, 101, 5000, 5001, 5002, 2 ** 40, 2 ** 40 + 1, 2 ** 40 + 7, 2 ** 40 + 8]
    want_ids = [b"", b"last", b"no-colon", long_a, long_b]
    for offsets in (None, gaps):
        want = C.expected(C.EVENT, keys, values, offsets)
        assert want[3] == want_ids and want[0] == [0, 1, 2, 0, 3, 4, 3, 1, 0, 2]
        assert want[2] == ([0, 1, 2, 3, 4, 5, 7, 8, 9, 11] if offsets is None else [gaps[i] for i in (0, 1, 2, 3, 4, 5, 7, 8, 9, 11)])
        for as_arrays in (False, True):
            got, counters = pushed_async(C.EVENT, keys, values, offsets, as_arrays=as_arrays)
            assert got == want
            assert counters == {"records_seen": 12, "records_delivered": 10, "flush_records_skipped": 2, "doubles_parsed_on_host": 0}
        assert C.wire_result(C.EVENT, keys, values, offsets) == want


def test_a_value_that_ends_with_its_blocks_span_and_one_that_ends_a_byte_short_of_it():
    """Record 255 is the last of block 0, record 256 the first of block 1 — and the last of the push: both values end exactly
    where a span ends.  Then record 255 loses its closing brace and record 256's value IS a closing brace: a decoder that read
    one byte past the value's length would accept 255 and name 256; the refusal names 255, nothing is delivered."""
    keys, values = records(257)
    offsets = list(range(500, 757))
    with DeviceDecoder(C.EVENT) as d:
        d.push_records_async(keys, values, offsets)
        d.finish(wait=False)
        good = C.result_of(d)
        assert good == C.expected(C.EVENT, keys, values, offsets)
        short = values[:255] + [values[255][:-1], b"}"]
        with pytest.raises(IngestError):
            C.EVENT.decode(short[255])
        d.push_records_async(keys, short, [o + 1000 for o in offsets])
        with pytest.raises(IngestError) as ei:
            d.finish(wait=False)
        assert ei.value.status == E_CORRUPT and "offset 1755)" in str(ei.value) and "record 255 " in str(ei.value), str(ei.value)
        assert C.result_of(d) == good and d.pending == 0


def test_the_state_instantiation_whole_key_ids_tombstones_and_the_gathered_values():
    n = 513
    keys = [(b"a:%d" % (i % 90)) if i % 3 else b"a" + b"%d" % (i % 7) for i in range(n)]  # "a:1" and "a" are two ids
    values = [b"" if i % 11 == 5 else b'{"count":%d,"pad":"%s"}' % (i, b"y" * (i % 37)) for i in range(n)]
    keys[400], values[400] = b"", b""  # a flush record
    offsets = [7 * i for i in range(n)]
    want = C.expected(None, keys, values, offsets, states=True)
    assert any(b":" in k for k in want[3]) and b"a1" in want[3] and b"a:1" in want[3]
    for as_arrays in (False, True):
        with DeviceDecoder(states=True) as d:
            (d.push_records_async(C.arrays(keys), C.arrays(values), offsets) if as_arrays else d.push_records_async(keys, values, offsets))
            d.finish(wait=False)
            agg, val, off, ids, val_off = C.state_result_of(d)
            assert (agg, val, off, ids) == want
            kept = [v for k, v in zip(keys, values) if k or v]
            assert val_off == np.concatenate([[0], np.cumsum([len(v) for v in kept])]).tolist()  # a tombstone: no bytes
            assert d.counters()["flush_records_skipped"] == 1
    with DeviceDecoder(states=True) as d:  # ... and the synchronous call gives the same
        d.push_records(keys, values, offsets)
        assert C.state_result_of(d)[:4] == want


@pytest.mark.parametrize("case", ["malformed event", "unknown type", "envelope id mismatch"])
def test_a_bad_record_fails_its_own_push_by_offset_commits_nothing_and_the_next_push_is_good(case):
    template = {"malformed event": C.EVENT, "unknown type": TYPED, "envelope id mismatch": ENVELOPED}[case]
    value_of = {"malformed event": lambda i, a: C.value(i), "unknown type": lambda i, a: b'{"t":"%s","v":%d}' % (b"ab"[i % 2:i % 2 + 1], i),
                "envelope id mismatch": lambda i, a: env.wrap(a, C.value(i))}[case]
    bad_of = {"malformed event": lambda a: b'{"v":', "unknown type": lambda a: b'{"t":"zzz","v":1}', "envelope id mismatch": lambda a: env.wrap(a + b"x", C.value(1))}[case]
    says = {"malformed event": "record 77 of the push", "unknown type": "names an event type the template does not know", "envelope id mismatch": "names another aggregateId"}[case]
    keys = [b"id-%d:%d" % (i % 23, i) for i in range(300)]
    good = [value_of(i, C.id_of(k)) for i, k in enumerate(keys)]
    with DeviceDecoder(template) as d:
        d.push_records_async(keys[:100], good[:100], list(range(100)))
        d.finish(wait=False)
        before = C.result_of(d)
        assert before == C.expected(template, keys[:100], good[:100])
        fresh = [b"never-seen-%d:1" % i for i in range(100)]  # ids only the failed push would have interned
        bad = [value_of(i, C.id_of(k)) for i, k in enumerate(fresh)]
        bad[77] = bad_of(C.id_of(fresh[77]))
        d.push_records_async(fresh, bad, list(range(100, 200)))
        with pytest.raises(IngestError) as ei:
            d.finish(wait=False)
        assert ei.value.status == E_CORRUPT and "(offset 177)" in str(ei.value) and says in str(ei.value), str(ei.value)
        assert C.result_of(d) == before and d.pending == 0
        d.push_records_async(keys[200:], good[200:], list(range(200, 300)))
        d.finish(wait=False)
        assert C.result_of(d) == C.expected(template, keys[:100] + keys[200:], good[:100] + good[200:], list(range(100)) + list(range(200, 300)))


def test_a_double_the_device_cannot_decide_is_handed_back_in_an_asynchronous_records_push():
    longs = numbers.long_texts()[:12]
    texts = []
    for i, t in enumerate(longs):
        texts += ["%d.5" % (i * 5 + j) for j in range(5)] + [t]
    keys = [b"k%d:%d" % (i % 9, i) for i in range(len(texts))]
    values = [b'{"v":' + t.encode() + b"}" for t in texts]
    with DeviceDecoder(DOUBLES) as d:
        half = len(texts) // 2
        d.push_records_async(keys[:half], values[:half], list(range(half)))
        d.push_records_async(C.arrays(keys[half:]), C.arrays(values[half:]), list(range(half, len(texts))))
        d.finish(wait=False)
        d.finish(wait=False)
        got = C.result_of(d)
        assert got == C.expected(DOUBLES, keys, values)
        raw = np.frombuffer(got[1], dtype=C.S.EVENT_DTYPE)["raw"].astype(np.uint64)
        assert raw.tolist() == [numbers.bits_of(float(t)) for t in texts]
        assert d.counters()["doubles_parsed_on_host"] == len(longs)


def test_enveloped_values_and_kept_event_strings_are_what_the_synchronous_call_gives():
    n = 300
    keys = [b"acct-%d:%d" % (i % 70, i) for i in range(n)]
    owner = lambda i: (b"owner \\\"%d\\\" \\u00e9" % i) if i % 4 else b""  # noqa: E731
    values = [env.wrap(C.id_of(k), esc.created(owner(i), b"%04d" % i, account=C.id_of(k), balance=b"%d.25" % i) if i % 3 == 0 else esc.updated(C.id_of(k), b"%d.5" % i))
              for i, k in enumerate(keys)]
    want = C.expected(esc.BANK_ENV, keys, values)
    results = []
    for mode in ("sync", "async lists", "async arrays"):
        with DeviceDecoder(esc.BANK_ENV, event_strings=esc.BANK_STRINGS) as d:
            for lo, hi in ((0, 130), (130, n)):
                if mode == "sync":
                    d.push_records(keys[lo:hi], values[lo:hi], list(range(lo, hi)))
                else:
                    pack = C.arrays if mode == "async arrays" else list
                    d.push_records_async(pack(keys[lo:hi]), pack(values[lo:hi]), list(range(lo, hi)))
            while d.pending:
                d.finish(wait=False)
            assert C.result_of(d) == want, mode
            cols = d.state_strings()
            results.append([None if c is None else (c[0].cpu().numpy().tobytes(), c[1].cpu().tolist()) for c in cols])
    assert results[0][0] is not None and results[0][1] is not None and b"owner" in results[0][0][0]
    assert results[1] == results[0] and results[2] == results[0]


# ---- the queue --------------------------------------------------------------------------------------------------------------------
def polls_of(n_polls, per_poll=150, ids=60):
    polls = []
    for p in range(n_polls):
        lo = p * per_poll
        keys = [b"p%d-%d:%d" % (p if i % 5 == 0 else 0, i % ids, i) for i in range(lo, lo + per_poll)]  # every poll brings ids of its own
        polls.append((keys, [C.value(i) for i in range(lo, lo + per_poll)], list(range(lo, lo + per_poll))))
    return polls


def joined(polls):
    return [k for p in polls for k in p[0]], [v for p in polls for v in p[1]], [o for p in polls for o in p[2]]


def test_five_records_pushes_in_flight_the_sixth_refused_and_the_results_in_push_order():
    polls = polls_of(6)
    with DeviceDecoder(C.EVENT) as d:
        for k, poll in enumerate(polls[:5]):
            d.push_records_async(*poll)
            assert d.pending == k + 1
        with pytest.raises(IngestError) as ei:
            d.push_records_async(*polls[5])
        assert ei.value.status == E_STATE and d.pending == 5
        with pytest.raises(IngestError) as ei:
            d.push_records(*polls[5])  # the synchronous call stays what it was: refused while anything is pending
        assert ei.value.status == E_STATE and "asynchronous pushes are pending" in str(ei.value) and d.pending == 5
        for k in range(5):
            d.finish(wait=False)
            assert d.pending == 4 - k
        assert C.result_of(d) == C.expected(C.EVENT, *joined(polls[:5]))  # (result_of: the one synchronise)
        with pytest.raises(IngestError) as ei:
            d.finish()
        assert ei.value.status == E_STATE
        d.push_records(*polls[5])
        assert C.result_of(d) == C.expected(C.EVENT, *joined(polls)) and d.stats()["pushes"] == 6


def test_a_wire_push_a_records_push_and_a_wire_push_in_flight_over_one_key_table():
    polls = polls_of(3)
    with EventsTopicIngest(frames=True) as g1, EventsTopicIngest(frames=True) as g3, DeviceDecoder(C.EVENT) as d:
        g1.feed(C.wire_of(*polls[0]))
        g3.feed(C.wire_of(*polls[2]))
        d.push_async(g1.drain_sections())
        d.push_records_async(*polls[1])
        d.push_async(g3.drain_sections())
        assert d.pending == 3
        for _ in range(3):
            d.finish(wait=False)
        want = C.expected(C.EVENT, *joined(polls))
        assert C.result_of(d) == want
        firsts = [want[3].index(C.id_of(p[0][0])) for p in polls]  # the ids each push brought are numbered in push order
        assert firsts == sorted(firsts) and d.stats()["pushes"] == 3


def test_the_callers_arrays_may_be_overwritten_as_soon_as_the_call_returns():
    polls = polls_of(3, per_poll=400)
    with DeviceDecoder(C.EVENT) as d:
        for keys, values, offsets in polls:
            (kd, ko), (vd, vo), of = C.arrays(keys), C.arrays(values), np.asarray(offsets, dtype=np.int64).copy()
            d.push_records_async((kd, ko), (vd, vo), of)
            for a in (kd, ko, vd, vo, of):
                a.view(np.uint8)[:] = 0xA5  # before the finish: the push has its own copy
        for _ in polls:
            d.finish(wait=False)
        assert C.result_of(d) == C.expected(C.EVENT, *joined(polls))


def test_the_middle_push_of_three_fails_and_the_table_and_the_result_hold_exactly_the_other_two():
    polls = polls_of(3)
    bad_values = list(polls[1][1])
    bad_values[60] = b'{"v":1'
    with DeviceDecoder(C.EVENT) as d:
        d.push_records_async(*polls[0])
        d.push_records_async(polls[1][0], bad_values, polls[1][2])
        d.push_records_async(*polls[2])
        d.finish(wait=False)
        with pytest.raises(IngestError) as ei:
            d.finish(wait=False)
        assert ei.value.status == E_CORRUPT and f"(offset {polls[1][2][60]})" in str(ei.value), str(ei.value)
        assert d.pending == 1
        d.finish(wait=False)
        want = C.expected(C.EVENT, *joined([polls[0], polls[2]]))
        assert C.result_of(d) == want and not any(k.startswith(b"p1-") for k in want[3])
        assert d.stats()["pushes"] == 2 and d.counters()["records_delivered"] == 300


def test_a_push_of_no_record_between_two_real_ones_takes_no_slot():
    polls = polls_of(2)
    with DeviceDecoder(C.EVENT) as d:
        d.push_records_async(*polls[0])
        assert d.pending == 1
        d.push_records_async([], [], [])
        d.push_records_async(C.arrays([]), C.arrays([]))
        assert d.pending == 1 and len(d._inflight) == 1
        d.push_records_async(*polls[1])
        assert d.pending == 2
        d.finish(wait=False)
        d.finish(wait=False)
        assert d.pending == 0 and d._inflight == []
        assert C.result_of(d) == C.expected(C.EVENT, *joined(polls)) and d.stats()["pushes"] == 2


def test_one_thread_pushes_records_while_another_finishes_them():
    """include/surge_ingest.h: ONE thread may enqueue pushes while ONE other finishes them.  The pushing thread takes a permit per
    push (four: one slot stays free), the finishing thread returns it behind each finish; thirty polls, results in push order."""
    import queue
    import threading

    polls = polls_of(30, per_poll=120)
    permits, pushed, errors = threading.Semaphore(4), queue.Queue(), []
    with DeviceDecoder(C.EVENT) as d:
        def pusher():
            try:
                for k, poll in enumerate(polls):
                    permits.acquire()
                    (d.push_records_async(C.arrays(poll[0]), C.arrays(poll[1]), poll[2]) if k % 2 else d.push_records_async(*poll))
                    pushed.put(k)
            except BaseException as e:  # handed to the test's thread
                errors.append(e)
            finally:
                pushed.put(None)

        t = threading.Thread(target=pusher, name="records-pusher")
        t.start()
        finished = 0
        while pushed.get() is not None:
            d.finish(wait=False)
            finished += 1
            permits.release()
        t.join()
        assert not errors and finished == 30 and d.pending == 0
        assert C.result_of(d) == C.expected(C.EVENT, *joined(polls)) and d.stats()["pushes"] == 30
