"""-m gpu: snappy sections through the device decoder (surge_amd/csrc/ingest_snappy.hip: the plan and snappy_parse_kernel, in
front of the LZ4 stage's exec pass) against the host decoder and the writer's own output (tests/snappy_cases.py).

The named cases are one-record sections of the state topic's shape pushed into a STATE decoder: it hands back every byte of
key and value, so every literal and copy of a case is seen.  The topics of many records go through an events decoder of
16-byte values.  Every test that means to exercise the kernel asserts the route counters — device chunks = the chunks built,
host sections = 0 — so a fallback cannot hide a failure."""
import functools
import random
import struct

import numpy as np
import pytest

import kafka_wire as kw
import snappy_cases as sc
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError, PartitionedFramedFetches

pytestmark = pytest.mark.gpu

corpus = functools.lru_cache(maxsize=None)(sc.cases)
MODES = ("by copy", "by copy, device crc", "in place", "in place, device crc")


@pytest.fixture(scope="module")
def states():
    with DeviceDecoder(states=True) as d:
        yield d


@pytest.fixture(scope="module")
def events():
    with DeviceDecoder(None) as d:
        yield d


def routes(d):
    s = d.route_stats()
    return s["snappy_device_chunks"], s["snappy_host_sections"]


def push_wire(d, wire, mode="by copy", start_offset=None):
    """One fetch of one partition framed by the host, compressed sections left as they are on the wire, in one push."""
    crc = mode.endswith("device crc")
    if mode.startswith("by copy"):
        with EventsTopicIngest(frames=True, device_lz4=True, device_crc=crc, start_offset=start_offset) as g:
            g.feed(wire)
            return d.push_from(g)
    with PartitionedFramedFetches(iter([[wire]]), 1, threads=1, hold=1, overlap=False, device_crc=crc, device_lz4=True, in_place=True) as framed:
        (secs, slab), = list(framed)
        d.push(secs, slab)
        return secs.shape[0]


def pushed(d, wire, chunks, host_sections=0, **how):
    """... with the route counters held to what the test built."""
    before = routes(d)
    n = push_wire(d, wire, **how)
    after = routes(d)
    assert (after[0] - before[0], after[1] - before[1]) == (chunks, host_sections), (before, after)
    return n


def state_records(d):
    """[(offset, key, value)] a state decoder holds, and cleared."""
    agg, values, value_off, offsets, n_keys = d.state_result()
    keys = d.keys()
    assert n_keys == len(keys)
    v, vo = values.cpu().numpy().tobytes(), value_off.cpu().numpy().tolist()
    out = [(int(o), keys[int(a)].encode(), v[vo[i]:vo[i + 1]]) for i, (a, o) in enumerate(zip(agg.cpu().numpy(), offsets.cpu().numpy()))]
    d.clear()
    return out


def host_records(wire):
    with EventsTopicIngest() as g:
        g.feed(wire)
        return [(o, k, v) for o, _, k, v in g.drain_records()]


def one_chunk_sections(base, c, sections):
    """The case's records as one batch per way of wrapping its stream, offsets from ``base``: [(wire, chunks)]."""
    return [(sc.batch(base + 10 * i, c.records, section), chunks) for i, (section, chunks) in enumerate(sections)]


# ---- the named cases, each a one-chunk section in a push of its own ------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in corpus()])
def test_a_named_case_decodes_to_the_writers_output(states, name):
    (c,) = [c for c in corpus() if c.name == name]
    assert sc.model_uncompress(c.stream) == c.output
    small = len(c.output) <= sc.DEVICE_CHUNK_MAX - 16
    wraps = [(sc.frame([c.stream]), 1), (c.stream, 1), (sc.frame([sc.overlong_preamble(c)]), 1), (sc.frame([sc.empty_chunk(), c.stream]), 2)]
    if len(c.output) % 16 == 0:
        wraps.append((sc.frame([c.stream, sc.empty_chunk()]), 2))
    for k, (wire, chunks) in enumerate(one_chunk_sections(1000, c, wraps if small else wraps[:3])):
        want = [(1000 + 10 * k + i, key, value) for i, (key, value, *_) in enumerate(c.records)]
        assert pushed(states, wire, chunks) == 1
        assert state_records(states) == want, (name, k)
        assert host_records(wire) == want, (name, k)


def words(rng, n):
    """``n`` bytes of text that compresses into short copies and literals, as JSON does."""
    vocab = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 9))) for _ in range(60)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(vocab) + (b'":"' if rng.random() < 0.2 else b" ") + (b"%d" % rng.randrange(1000) if rng.random() < 0.3 else b"")
    return bytes(out[:n])


def sized_record(key, size, rng):
    """[(key, value)] whose records section is exactly ``size`` bytes."""
    n = size - 30
    for _ in range(8):
        raw = kw.record(0, key, bytes(n))
        if len(raw) == size:
            return [(key, words(rng, n))]
        n += size - len(raw)
    raise AssertionError(size)


def test_one_chunk_per_lds_class_of_the_exec_pass(states):
    """Chunks of greedy-compressed text whose output is exactly a class's capacity (8, 16, 24, 32, 48, 64 KiB) and, below 64 KiB,
    one byte more (the next class); each holds copies, so each is listed for the exec pass."""
    rng = random.Random(31)
    for cap in sc.EXEC_CLASS_CAPS:
        wires, want = [], []
        for j, size in enumerate((cap, cap + 1) if cap < 65536 else (cap,)):
            recs = sized_record(b"class-%d" % size, size, rng)
            stream = sc.greedy_block(sc.records_section(recs))
            assert sum(1 for e in sc.count_elements(stream)[1] if e.kind) > 100
            wires.append(sc.batch(size + j, recs, sc.frame([stream])))
            want.append((size + j, recs[0][0], recs[0][1]))
        assert pushed(states, b"".join(wires), len(wires)) == len(wires)
        assert state_records(states) == want, cap
        assert host_records(b"".join(wires)) == want


@pytest.mark.parametrize("size, chunks", [(32768, 1), (32769, 2), (65536, 2), (65537, 3)])
def test_sections_of_32_kib_chunks_whose_last_chunk_is_full_or_one_byte_long(states, size, chunks):
    rng = random.Random(size)
    recs = sized_record(b"section-%d" % size, size, rng)
    section = sc.compress_section(sc.records_section(recs))
    assert len(sc.model_section(section)) == size
    n_chunks, p = 0, 16
    while p < len(section):
        p += 4 + struct.unpack(">i", section[p:p + 4])[0]
        n_chunks += 1
    assert n_chunks == chunks
    wire = sc.batch(5, recs, section)
    assert pushed(states, wire, chunks) == 1
    assert state_records(states) == [(5, recs[0][0], recs[0][1])] == host_records(wire)


def test_a_raw_block_at_64_kib_goes_to_the_device_and_one_byte_above_it_through_the_host(states):
    rng = random.Random(33)
    for size, chunks, host in ((65536, 1, 0), (65537, 0, 1)):
        recs = sized_record(b"raw-%d" % size, size, rng)
        wire = sc.batch(7, recs, sc.greedy_block(sc.records_section(recs)))
        assert pushed(states, wire, chunks, host) == 1
        assert state_records(states) == [(7, recs[0][0], recs[0][1])] == host_records(wire)


def test_chunks_off_the_16_byte_grid_and_chunks_above_64_kib_go_through_the_host_and_give_the_same_records(states):
    rng = random.Random(34)
    recs = sized_record(b"odd-chunks", 5000, rng)
    big = sized_record(b"big-chunk", 150000, rng)
    wire = sc.batch(0, recs, sc.compress_section(sc.records_section(recs), chunk=1000)) + sc.batch(1, big, sc.compress_section(sc.records_section(big), chunk=70000))
    assert pushed(states, wire, 0, 2) == 2
    assert state_records(states) == [(0, recs[0][0], recs[0][1]), (1, big[0][0], big[0][1])] == host_records(wire)
    # ... and in one push with a section the device takes: 16-byte grid, the last chunk short
    grid = sized_record(b"grid-chunks", 5000, rng)
    wire += sc.batch(2, grid, sc.compress_section(sc.records_section(grid), chunk=1008))
    assert pushed(states, wire, 5, 2) == 3
    assert [o for o, _, _ in state_records(states)] == [0, 1, 2]


# ---- topics of many records through an events decoder -----------------------------------------------------------------------------
def event16(rng):
    return struct.pack("<iiQ", rng.randrange(3), rng.randrange(1 << 31), rng.getrandbits(64))


def event_topic(seed, codecs, n_batches=9, block=sc.greedy_block, chunk=sc.CHUNK, per_batch=(1, 400)):
    """(wire, ids, events, chunks): batches of 16-byte events under keys <id>:<offset>, batch b written with codecs[b % len(codecs)];
    every fourth a committed transaction, one an aborted one.  chunks: snappy chunks written, of the batches delivered."""
    rng = random.Random(seed)
    wire, ids, events, off, chunks = [], [], [], 0, 0
    for b in range(n_batches):
        n = rng.randrange(*per_batch)
        recs = [(b"agg-%d-%s:%d" % (rng.randrange(50), b"x" * rng.randrange(40), off + i), event16(rng)) for i in range(n)]
        tx = dict(transactional=True, producer_id=40 + b, base_sequence=0) if b % 4 == 3 else {}
        codec = codecs[b % len(codecs)]
        aborted = b == 7
        if codec == "snappy":
            section = sc.compress_section(sc.records_section(recs), chunk=chunk, block=block)
            wire.append(sc.batch(off, recs, section, **tx))
            chunks += 0 if aborted else -(-len(sc.records_section(recs)) // chunk)
        else:
            wire.append(kw.record_batch(off, recs, compression=codec, **tx))
        if not aborted:
            ids += [(k.split(b":")[0], off + i) for i, (k, _) in enumerate(recs)]
            events += [v for _, v in recs]
        off += n
        if tx:
            wire.append(kw.control_batch(off, 40 + b, 0 if aborted else 1))
            off += 1
    return b"".join(wire), ids, events, chunks


def event_results(d):
    agg, ev, off, n_keys = d.result()
    keys = d.keys()
    assert n_keys == len(keys)
    out = agg.cpu().numpy().tolist(), ev.cpu().numpy().tobytes(), off.cpu().numpy().tolist(), keys
    d.clear()
    return out


def check_events(got, ids, events, keys_before=()):
    agg, ev, off, keys = got
    order = list(dict.fromkeys(list(keys_before) + [i.decode() for i, _ in ids]))
    assert off == [o for _, o in ids]
    assert ev == b"".join(events)
    assert keys == order and agg == [order.index(i.decode()) for i, _ in ids]


def check_host(wire, ids, events):
    with EventsTopicIngest() as g:
        g.feed(wire)
        agg, ev, off = g.drain_fixed16()
        keys = g.key_table().keys
    check_events((agg.tolist(), ev.tobytes(), off.tolist(), keys), ids, events)


@pytest.mark.parametrize("mode", MODES)
def test_a_snappy_topic_by_copy_and_in_place_with_the_crc_on_the_host_and_on_the_device(mode):
    wire, ids, events, chunks = event_topic(41, ["snappy"], chunk=4096)
    with DeviceDecoder(None) as d:
        pushed(d, wire, chunks, mode=mode)
        check_events(event_results(d), ids, events)
    check_host(wire, ids, events)


def test_one_push_of_uncompressed_lz4_and_snappy_sections_interleaved(events):
    wire, ids, events_, chunks = event_topic(42, ["none", "lz4", "snappy"], n_batches=12, chunk=2048)
    assert chunks > 4
    known = events.keys()
    pushed(events, wire, chunks)
    check_events(event_results(events), ids, events_, known)
    check_host(wire, ids, events_)


def test_a_topic_written_by_pyarrows_snappy_in_32_kib_chunks():
    pytest.importorskip("pyarrow")
    wire, ids, events, chunks = event_topic(43, ["snappy"], n_batches=5, block=sc.arrow_block(), per_batch=(900, 1400))
    assert chunks >= 8  # (batches of 40 - 60 KB: two chunks each)
    with DeviceDecoder(None) as d:
        pushed(d, wire, chunks)
        check_events(event_results(d), ids, events)
    check_host(wire, ids, events)


def test_several_parts_in_one_push_and_several_pushes_in_flight():
    topics = [event_topic(50 + p, ["snappy", "lz4"], n_batches=5, chunk=1024) for p in range(3)]
    with DeviceDecoder(None) as d:
        framers = [EventsTopicIngest(frames=True, device_lz4=True, device_crc=True) for _ in topics]
        try:
            before = routes(d)
            parts = []
            for g, (wire, _, _, _) in zip(framers, topics):
                g.feed(wire)
                parts.append(g.drain_sections())
            d.push_async(parts[:2])
            d.push_async(parts[2])
            d.finish()
            d.finish()
            assert routes(d) == (before[0] + sum(t[3] for t in topics), before[1])
            ids = [i for t in topics for i in t[1]]
            check_events(event_results(d), ids, [e for t in topics for e in t[2]])
        finally:
            for g in framers:
                g.close()


def test_a_floored_push_passes_over_the_records_below_the_start_offset():
    wire, ids, events, chunks = event_topic(44, ["snappy"], n_batches=3, chunk=4096, per_batch=(200, 300))
    start = ids[7][1]  # inside the first batch: its section travels whole, with a floor
    keep = [k for k, (_, o) in enumerate(ids) if o >= start]
    with DeviceDecoder(None) as d:
        pushed(d, wire, chunks, start_offset=start)  # (no batch lies below the start as a whole: every chunk built is decoded)
        check_events(event_results(d), [ids[k] for k in keep], [events[k] for k in keep])
        assert d.below_floor() == 7


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def good_push_follows(d):
    c = corpus()[0]
    assert push_wire(d, sc.batch(0, c.records, sc.frame([c.stream]))) == 1
    assert state_records(d) == [(0, c.records[0][0], c.records[0][1])]


@pytest.mark.parametrize("name", sorted(sc.refusals()))
def test_a_refusal_fails_its_push_as_corrupt_commits_nothing_and_leaves_the_decoder_good(states, name):
    section, status = sc.refusals()[name]
    recs = [(b"never-delivered", b"v")]
    # Who refuses.  What is wrong with an ELEMENT (a tag or literal past the input, an offset, output that misses the preamble) only
    # the decode finds: on the device route snappy_parse_kernel ("bad snappy chunk in the batch at ...", from stage 2's first wait),
    # on the host route the plan's host decoder.  The framing and the preambles are the plan's to read on either route ("... (the
    # section at ...)") — a preamble that no block of its size can reach (more than 32 x) among them.
    element = sc.TAG_PAST_INPUT <= status <= sc.OUTPUT_SHORT
    if name.startswith("framing"):
        by_kernel = [name in ("framing: a bad block in the second chunk", "framing: an offset that reaches into the chunk in front")]  # (the chunk in front: 16 bytes)
        assert by_kernel[0] == element
    else:
        reached = element and sc.read_varint(section)[0] <= 32 * len(section)
        by_kernel = [reached, reached, reached, False]
        by_kernel = [b for b, w in zip(by_kernel, [section, b"x", b"x", b"x"]) if w]
    # a raw block: as it is, as a section's only chunk, behind an empty chunk (the device's second chunk) and behind a chunk off the
    # 16-byte grid (the host's)
    wraps = [section] if name.startswith("framing") else [section, sc.frame([section]), sc.frame([sc.empty_chunk(), section]), sc.frame([corpus()[0].stream, section])]
    wraps = [w for w in wraps if w]  # (a section of no bytes at all is the framer's to refuse: there is no arena to push)
    for k, wrapped in enumerate(wraps):
        keys_before, pushes_before = states.keys(), states.stats()["pushes"]
        with pytest.raises(IngestError) as ei:
            push_wire(states, sc.batch(7000 + k, recs, wrapped))
        assert ei.value.status == -7 and "snappy" in str(ei.value) and f"base offset {7000 + k}" in str(ei.value), (name, k, str(ei.value))
        assert (f"bad snappy chunk in the batch at base offset {7000 + k}" in str(ei.value)) == by_kernel[k], (name, k, str(ei.value))
        assert (f"(the section at base offset {7000 + k})" in str(ei.value)) == (not by_kernel[k]), (name, k, str(ei.value))
        assert states.keys() == keys_before and states.stats()["pushes"] == pushes_before and state_records(states) == []
        good_push_follows(states)


def test_seeded_mutations_are_refused_or_decode_to_what_the_model_says(states):
    """One mutated chunk per push.  Where the model decoder refuses the chunk the push is CORRUPT; where it decodes it, the push
    does what a push of the SAME bytes written uncompressed does (the records may well be damaged: that is the record stage's to say)."""
    streams = [(c.name, c.stream) for c in corpus() if len(c.stream) < 3000]
    refused = decoded = 0
    for name, data in sc.mutations(streams, per_stream=2, seed=123):
        recs = [(b"mutated", b"v")]
        try:
            plain = sc.model_uncompress(data)
        except sc.Refused:
            plain = None
        if plain is not None and len(plain) > sc.DEVICE_CHUNK_MAX:
            continue

        def outcome(wire):
            try:
                push_wire(states, wire)
            except IngestError as e:
                assert e.status == -7, str(e)
                return "corrupt", "snappy" in str(e)
            return state_records(states), False

        got = outcome(sc.batch(0, recs, sc.frame([data])))
        if plain is None:
            assert got == ("corrupt", True), name
            refused += 1
        else:
            want = outcome(kw.record_batch(0, recs, compression="lz4", codec_override=0, compressor=lambda r: plain))
            assert got == want, name
            decoded += 1
        states.clear()
    assert refused > 5 and decoded > 5
    good_push_follows(states)
