"""Start offsets and positions of the host framer (``surge_ingest_set_start_offset`` and its kin, ``include/surge_ingest.h``):
a consumer that seeks to offset ``s`` is sent the whole batch that contains ``s`` and must be handed the records from ``s`` on,
transactions read as ever.  Expected values are the writer's own record list (``start_offsets_gen.Topic``) filtered by
``offset >= s``; everything is exact."""
import ctypes
import struct

import numpy as np
import pytest

import kafka_wire as kw
import start_offsets_gen as gen
from surge_amd import _native
from surge_amd.ingest import (ARG_I32, FLOOR_DTYPE, SECTION_FLOORED, EventJsonTemplate, EventsTopicIngest, FramedFetches, IngestError,
                              PartitionedFramedFetches)

E_STATE = -2
CODECS = ("none", "lz4")
TOPICS = {c: gen.standard_topic(c) for c in CODECS}
TEMPLATE = EventJsonTemplate("_type", [("countIncremented", 1, "sequenceNumber", "incrementBy", ARG_I32)])


def json_value(n):
    return b'{"_type":"countIncremented","sequenceNumber":%d,"incrementBy":%d}' % (n, n % 7 + 1)


def drained(g):
    return [(o, k, v) for o, _, k, v in g.drain_records()]


@pytest.mark.parametrize("codec", CODECS)
def test_every_start_delivers_the_records_from_it_on(codec):
    t = TOPICS[codec]
    for s in gen.interesting_starts(t):
        with EventsTopicIngest(start_offset=s) as g:
            g.feed(t.bytes)
            want = t.delivered(s)
            assert g.ready == len(want), s
            assert drained(g) == want, s
            c, below = g.counters(), g.below_start()
            assert c["records_delivered"] == len(want), s
            # transactions are read as ever: the aborted records are the aborted records wherever the start lies
            assert c["records_aborted"] == 8 and c["control_batches"] == 2 and c["open_transactions"] == 0, s
            everything = t.delivered(-1)
            flush_below = 1 if 0 < s and 5 < s else 0
            assert below["records_dropped"] == (len(everything) - len(want) + flush_below if s > 0 else 0), s
            assert c["flush_records_skipped"] == 1 - flush_below, s
            assert g.position() == max(t.next_offset, s), s


@pytest.mark.parametrize("codec", CODECS)
def test_start_zero_and_minus_one_are_todays_output(codec):
    t = TOPICS[codec]
    with EventsTopicIngest() as plain:
        plain.feed(t.bytes)
        want, want_counters = plain.drain_records(), plain.counters()
    for s in (0, -1):
        with EventsTopicIngest(start_offset=s) as g:
            g.feed(t.bytes)
            assert g.drain_records() == want and g.counters() == want_counters
            assert g.below_start() == {"batches_discarded": 0, "records_dropped": 0}
    with EventsTopicIngest(frames=True, device_lz4=True) as plain, EventsTopicIngest(frames=True, device_lz4=True, start_offset=0) as g:
        plain.feed(t.bytes)
        g.feed(t.bytes)
        a, b = plain.drain_sections()[0], g.drain_sections()[0]
        assert a.tobytes() == b.tobytes() and g.take_floors().shape[0] == 0


def test_the_next_higher_offset_is_delivered_first_inside_a_compaction_gap():
    t = TOPICS["none"]
    with EventsTopicIngest(start_offset=35) as g:
        g.feed(t.bytes)
        assert drained(g)[0][0] == 40
    with EventsTopicIngest(start_offset=73) as g:  # the batch's last offset is a gap: its lastOffsetDelta still says 63
        g.feed(t.bytes)
        assert drained(g)[0][0] == 74


def test_a_transaction_that_straddles_the_start_commits_or_aborts_as_a_whole():
    t = TOPICS["lz4"]
    with EventsTopicIngest(start_offset=81) as g:  # inside the committed transaction: its first batch lies below
        g.feed(t.tail_bytes(81))  # (what the broker sends: from the batch that contains 81)
        assert [o for o, _, _ in drained(g)][:3] == [81, 82, 93]
    with EventsTopicIngest(start_offset=88) as g:  # inside the aborted one
        g.feed(t.tail_bytes(88))
        assert drained(g)[0][0] == 93 and g.counters()["records_aborted"] == 8
    with EventsTopicIngest(start_offset=78) as g:  # the marker has not arrived: nothing is stable
        g.feed(b"".join(b["bytes"] for b in t.batches[4:6]))
        assert g.ready == 0 and g.position() == 78  # in front of the open transaction, never below the start
        g.feed(t.batches[6]["bytes"])
        assert [o for o, _, _ in drained(g)] == [78, 79, 80, 81, 82]


@pytest.mark.parametrize("codec", CODECS)
def test_the_straddling_batch_cut_across_two_feeds(codec):
    t = TOPICS[codec]
    raw = t.bytes
    at = raw.index(t.batches[3]["bytes"]) + len(t.batches[3]["bytes"]) // 2
    with EventsTopicIngest(start_offset=44) as g:
        g.feed(raw[:at])
        assert g.ready == 0 and g.position() == 44
        g.feed(raw[at:])
        assert drained(g) == t.delivered(44)


def test_a_value_below_the_start_is_never_decoded():
    bad = gen.Topic().data([(b"a:0", json_value(0)), (b"a:1", b"{not json"), (b"a:2", json_value(2))]).data([(b"b:3", json_value(3))])
    with EventsTopicIngest(start_offset=2) as g:
        g.feed(bad.bytes)
        agg, ev, off = g.drain_json(TEMPLATE)
        assert off.tolist() == [2, 3] and agg.tolist() == [0, 1] and ev["seq"].tolist() == [2, 3]
        assert [k for k in g.key_table().keys] == ["a", "b"]
    with EventsTopicIngest(start_offset=1) as g:  # the same value AT the start fails the drain as ever
        g.feed(bad.bytes)
        with pytest.raises(IngestError, match="offset 1"):
            g.drain_json(TEMPLATE)
    with EventsTopicIngest(start_offset=2) as g:  # fixed16 likewise: a 9-byte value below the start
        g.feed(gen.Topic().data([(b"a:0", b"123456789"), (b"a:1", gen.fixed16(1, 1, 5)), (b"c:2", gen.fixed16(1, 2, 6))]).bytes)
        with pytest.raises(IngestError):
            EventsTopicIngest.drain_fixed16(_fed(gen.Topic().data([(b"a:0", b"123456789")]).bytes, 0))
        agg, ev, off = g.drain_fixed16()
        assert off.tolist() == [2] and agg.tolist() == [0] and g.key_table().keys == ["c"]  # the key below the start is not interned


def _fed(raw, start):
    g = EventsTopicIngest(start_offset=start)
    g.feed(raw)
    return g


def test_a_flush_record_below_and_at_the_start():
    t = TOPICS["none"]  # its flush record is offset 5
    for s, skipped in ((5, 1), (6, 0)):
        with EventsTopicIngest(start_offset=s) as g:
            g.feed(t.bytes)
            assert drained(g) == t.delivered(s)
            assert g.counters()["flush_records_skipped"] == skipped


@pytest.mark.parametrize("codec", CODECS)
def test_sections_carry_one_floored_section_and_the_floors_list_names_it(codec):
    t = TOPICS[codec]
    for s in gen.interesting_starts(t):
        with EventsTopicIngest(frames=True, device_lz4=True, device_crc=True, start_offset=s) as g:
            g.feed(t.bytes)
            secs, _ = g.drain_sections()
            floors = g.take_floors()
            want = [t.batches[i] for i in t.committed() if t.batches[i]["last"] >= s]
            assert secs["base_offset"].tolist() == [b["base"] for b in want], s
            flagged = np.flatnonzero(secs["codec"] & SECTION_FLOORED)
            straddles = [i for i, b in enumerate(want) if b["base"] < s <= b["last"]] if s > 0 else []
            assert flagged.tolist() == straddles, s
            assert floors["section"].tolist() == straddles and floors["first_offset"].tolist() == [s] * len(straddles) and (floors["part"] == 0).all(), s
            below = g.below_start()
            gone = [t.batches[i] for i in t.committed() if t.batches[i]["last"] < s] if s > 0 else []
            assert below["batches_discarded"] == len(gone) and below["records_dropped"] == sum(len(b["records"]) for b in gone), s
            assert g.counters()["records_delivered"] == sum(len(b["records"]) for b in want), s
            assert g.position() == max(t.next_offset, s), s


def test_each_refusal_of_the_start_offset_calls_says_what_is_wrong():
    lib = _native.load()
    with EventsTopicIngest(frames=True) as g:
        g.feed(TOPICS["none"].bytes)
        assert lib.surge_ingest_set_start_offset(g._h, 5) == E_STATE
        assert lib.surge_ingest_last_error(g._h) == b"surge_ingest_set_start_offset after the first feed"
    assert lib.surge_ingest_set_start_offset(None, 5) == -1 and lib.surge_ingest_last_error(None) == b"handle is NULL"
    with EventsTopicIngest(frames=True, start_offset=12) as g:
        g.feed(TOPICS["none"].bytes)
        g.drain_sections()
        got = ctypes.c_int64()
        assert lib.surge_ingest_take_floors(g._h, 0, None, ctypes.byref(got)) == -1 and got.value == 1  # too small: says what it needs
        assert b"floors table too small" in lib.surge_ingest_last_error(g._h)
        assert lib.surge_ingest_take_floors(g._h, -1, None, ctypes.byref(got)) == -1 and lib.surge_ingest_last_error(g._h) == b"bad argument"
        assert g.take_floors()["section"].tolist() == [0]  # (neither refusal took the list away)
    h = ctypes.c_void_p()
    assert lib.surge_ingest_group_create(1, 1, ctypes.byref(h)) == 0
    try:
        raw = TOPICS["none"].bytes
        starts = (ctypes.c_int64 * 1)(12)
        assert lib.surge_ingest_group_set_start_offsets(h, None) == -1
        assert lib.surge_ingest_group_set_start_offsets(h, starts) == 0
        data, lens = (ctypes.c_void_p * 1)(ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p)), (ctypes.c_int64 * 1)(len(raw))
        secs, n, slab = np.zeros(64, dtype=[("a", "<i8", 4)]), ctypes.c_int64(), ctypes.c_void_p()
        assert lib.surge_ingest_group_feed(h, data, lens, 1, None, 64, secs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), ctypes.byref(slab)) == 0
        assert lib.surge_ingest_group_set_start_offsets(h, starts) == E_STATE
        assert lib.surge_ingest_group_last_error(h) == b"surge_ingest_group_set_start_offsets after the first feed"
        got = ctypes.c_int64()
        assert lib.surge_ingest_group_take_floors(h, 0, None, ctypes.byref(got)) == -1 and got.value == 1
        assert b"floors table too small" in lib.surge_ingest_group_last_error(h)
    finally:
        lib.surge_ingest_group_destroy(h)


def test_the_floor_is_named_once_even_when_the_drain_is_split():
    t = TOPICS["none"]
    with EventsTopicIngest(frames=True, start_offset=12) as g:
        g.feed(t.bytes)
        seen = []
        while True:
            secs, _ = g.drain_sections(max_sections=1)
            if not secs.shape[0]:
                break
            seen.append((int(secs["base_offset"][0]), g.take_floors()["section"].tolist()))
        assert seen[0] == (10, [0]) and all(f == [] for _, f in seen[1:])


def test_a_group_of_four_partitions_with_four_starts():
    topics = [gen.standard_topic("lz4"), gen.standard_topic("none"), gen.standard_topic("lz4"), gen.standard_topic("none")]
    starts = [0, 12, 82, 158]
    fetch = [topics[0].bytes, topics[1].bytes, None, topics[3].bytes]  # partition 2 gets nothing in the first response
    later = [None, None, topics[2].tail_bytes(82), None]
    with PartitionedFramedFetches([fetch, later], 4, threads=2, overlap=False, device_crc=True, start_offsets=starts) as framed:
        items = list(framed)
        assert framed.positions() == [t.next_offset for t in topics]
        assert framed.below_start()["batches_discarded"] == sum(topics[p].batches[i]["last"] < starts[p] for p in (1, 3) for i in topics[p].committed())  # (partition 2 is sent nothing below its start)
    (secs, slab), (secs2, slab2) = items  # (destructures as the pair it always was)
    first = items[0]
    want = [[t.batches[i]["base"] for i in t.committed() if t.batches[i]["last"] >= s] for t, s in zip(topics, starts)]
    assert secs["base_offset"].tolist() == want[0] + want[1] + want[3]
    assert first.floors["part"].tolist() == [1, 3] and first.floors["first_offset"].tolist() == [12, 158]
    assert first.floors["section"].tolist() == [len(want[0]), len(want[0]) + len(want[1])]
    assert np.flatnonzero(secs["codec"] & SECTION_FLOORED).tolist() == first.floors["section"].tolist()
    assert first.positions == (159, 159, 82, 159)  # a partition without bytes stands at its start
    assert items[1].floors["part"].tolist() == [2] and items[1].floors["section"].tolist() == [0] and secs2["base_offset"].tolist() == want[2]
    # without start offsets the items are the plain pairs they were
    with PartitionedFramedFetches([fetch], 4, threads=2, overlap=False) as framed:
        assert type(next(iter(framed))) is tuple
    with FramedFetches([topics[1].bytes], overlap=False) as framed:
        assert type(next(iter(framed))) is tuple
    with FramedFetches([topics[1].bytes], overlap=False, start_offset=12) as framed:
        item = next(iter(framed))
        assert item.floors["section"].tolist() == [0] and item.positions == (159,) and item[0]["base_offset"][0] == 10


def test_set_start_offset_after_a_feed_is_refused():
    lib = _native.load()
    with EventsTopicIngest() as g:
        g.feed(TOPICS["none"].batches[0]["bytes"])
        with pytest.raises(IngestError) as e:
            g.set_start_offset(5)
        assert e.value.status == E_STATE
    h = ctypes.c_void_p()
    assert lib.surge_ingest_group_create(2, 1, ctypes.byref(h)) == 0
    try:
        starts = (ctypes.c_int64 * 2)(4, 0)
        assert lib.surge_ingest_group_set_start_offsets(h, starts) == 0
        raw = TOPICS["none"].bytes
        data = (ctypes.c_void_p * 2)(ctypes.cast(ctypes.c_char_p(raw), ctypes.c_void_p), None)
        lens = (ctypes.c_int64 * 2)(len(raw), 0)
        secs = np.zeros(64, dtype=[("a", "<i8", 4)])
        n, slab = ctypes.c_int64(), ctypes.c_void_p()
        assert lib.surge_ingest_group_feed(h, data, lens, 1, None, 64, secs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), ctypes.byref(slab)) == 0
        assert lib.surge_ingest_group_set_start_offsets(h, starts) == E_STATE
        floors = np.zeros(2, dtype=FLOOR_DTYPE)
        got = ctypes.c_int64()
        assert lib.surge_ingest_group_take_floors(h, 0, None, ctypes.byref(got)) == -1 and got.value == 1  # too small: says what it needs
        assert lib.surge_ingest_group_take_floors(h, 2, floors.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)) == 0
        assert (got.value, int(floors["part"][0]), int(floors["section"][0]), int(floors["first_offset"][0])) == (1, 0, 0, 4)
    finally:
        lib.surge_ingest_group_destroy(h)


@pytest.mark.parametrize("codec", CODECS)
def test_positions_after_each_feed_and_never_past_an_open_transaction(codec):
    t = TOPICS[codec]
    with EventsTopicIngest() as g:
        assert g.position() == 0
        for k, b in enumerate(t.batches, 1):
            g.feed(b["bytes"])
            g.drain_records()
            assert g.position() == t.position(k), k
    assert t.position(5) == 74 and t.position(6) == 74 and t.position(7) == 84  # (the writer's own expectation is not vacuous)
    with EventsTopicIngest(frames=True, device_lz4=True) as g:
        for k, b in enumerate(t.batches, 1):
            g.feed(b["bytes"])
            g.drain_sections()
            assert g.position() == t.position(k), k
    with EventsTopicIngest() as g:  # what is decided but not drained yet is still to be delivered: the position waits for it
        g.feed(t.bytes)
        assert g.position() == 0
        g.drain_records(max_records=2)
        assert g.position() == 2


def small_transactional_topic(codec):
    t = gen.Topic(codec)
    v = lambda n: gen.fixed16(1, n, n)  # noqa: E731
    t.data([(b"a:0", v(0)), (b"b:1", v(1))])
    t.data([(b"a:2", v(2)), (b"", b""), (b"c:4", v(4))], pid=5)
    t.data([(b"d:5", v(5))])  # another producer's batch between the transaction and its marker
    t.data([(b"b:6", v(6)), (b"b:7", v(7))], pid=5)
    t.marker(5, kw.COMMIT)
    t.data([(b"e:9", v(9)), (b"e:10", v(10))], pid=6).marker(6, kw.ABORT)
    t.data([(b"a:12", v(12)), (b"f:13", v(13)), (b"f:14", v(14))], gone={1})
    return t


@pytest.mark.parametrize("codec", CODECS)
def test_consume_to_a_position_then_start_there_delivers_the_topic_exactly_once(codec):
    t = small_transactional_topic(codec)
    whole = t.delivered()
    for frames in (False, True):
        for cut in range(len(t.batches) + 1):
            with EventsTopicIngest(frames=frames, device_lz4=frames) as g:
                g.feed(b"".join(b["bytes"] for b in t.batches[:cut]))
                first = _offsets(g, t, frames, 0)
                p = g.position()
            assert p == t.position(cut)
            with EventsTopicIngest(frames=frames, device_lz4=frames, start_offset=p) as g:
                g.feed(t.tail_bytes(p))
                second = _offsets(g, t, frames, p)
            assert first + second == [o for o, _, _ in whole], (frames, cut, p)


def _offsets(g, t, frames, start):
    """The offsets a drain delivers; in FRAMES mode the handed-out sections' records from the floor on (what the device keeps)."""
    if not frames:
        return [o for o, _, _ in drained(g)]
    secs, _ = g.drain_sections()
    by_base = {b["base"]: b for b in t.batches}
    return [o for base in secs["base_offset"].tolist() for o, k, v in by_base[base]["records"] if o >= start and not (k == b"" and v == b"")]


def test_prefixes_and_mutations_of_a_straddling_topic_under_asan_and_ubsan(tmp_path):
    """tests/cpp/start_offsets_prefixes.cpp: every prefix and seeded mutations of a small straddling topic with every start of the
    list above, through the host drains, the FRAMES drain and a group, built with -fsanitize=address,undefined — a stand-alone
    program, nothing of it is loaded into this process."""
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "start_offsets_prefixes")
    srcs = [os.path.join(root, "tests", "cpp", "start_offsets_prefixes.cpp")] + [os.path.join(root, "surge_amd", "csrc", f)
                                                                                  for f in ("ingest.cpp", "ingest_group.cpp", "crc32c.cpp", "lz4_frame.cpp", "event_decode.cpp", "f64_text.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(root, "include")] + srcs + ["-pthread", "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]
