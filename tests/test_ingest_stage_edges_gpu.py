"""-m gpu: the device decoder's LZ4 stage (surge_amd/csrc/ingest_lz4.hip) and CRC-32C stage (ingest_crc.hip) at the edges
their code branches on, with inputs made for them by tests/lz4_seqgen.py (tests/test_lz4_seqgen.py holds those inputs to
liblz4, to the host decoder and to the shapes they are named for — on the CPU).

What is right is the test's own source list: the ids in first-seen order, the 16-byte events, the offsets.  The designed
repetition lies in the ids (and the events) — the bytes the decoder hands back.  What it does not hand back are record
headers: the header values of random bytes that tune a section's length are seen only through the records behind them
(a lost or added byte moves those), so no section here ENDS in one — the last record of a sized, an LDS-class or a padded
block has no headers, and only the closing byte of its empty header list is beyond what a test can see.  The host decoder
is asked afterwards only."""
import functools
import struct

import numpy as np
import pytest

import lz4_seqgen as G
from surge_amd.ingest import SECTION_CRC_PENDING, SECTION_CRC_WIRE, DeviceDecoder, EventsTopicIngest, IngestError, PartitionedFramedFetches

pytestmark = pytest.mark.gpu


def named(topic, err):
    """The failing batch's case, looked up by the base offset the error names."""
    text = str(err)
    at = text.find("base offset ")
    if at < 0:
        return text
    base = int(text[at + 12:].split()[0].rstrip(".,:;)"))
    return f"{text} [{topic.names[base] if base < topic.n else '?'}]"


def results(d):
    agg, ev, off, n_keys = d.result()
    keys = d.keys()
    assert n_keys == len(keys)
    return agg.cpu().numpy(), ev.cpu().numpy().tobytes(), off.cpu().numpy(), keys


def decode(topic, pushes=1, device_crc=False):
    """The topic's wire bytes through host framing and the device decoder, LZ4 frames left to the GPU, in ``pushes`` feeds
    cut anywhere (a cut batch is completed by the next feed)."""
    wire = topic.wire
    with EventsTopicIngest(frames=True, device_lz4=True, device_crc=device_crc) as g, DeviceDecoder(None) as d:
        for k in range(pushes):
            g.feed(wire[k * len(wire) // pushes:(k + 1) * len(wire) // pushes])
            try:
                d.push_from(g)
            except IngestError as e:
                raise AssertionError(named(topic, e)) from e
        return results(d)


def check(topic, got):
    agg, ev, off, keys = got
    assert off.shape[0] == topic.n, (off.shape[0], topic.n)
    assert off.tolist() == list(range(topic.n))
    want = topic.event_bytes()
    if ev != want:
        bad = [j for j in range(topic.n) if ev[16 * j:16 * j + 16] != want[16 * j:16 * j + 16]]
        raise AssertionError(f"{len(bad)} events differ, the first is record {bad[0]} [{topic.names[bad[0]]}]")
    if keys != topic.keys():
        bad = [a for a, (x, y) in enumerate(zip(keys, topic.keys())) if x != y]
        first = topic.ids.index(topic.keys()[bad[0]].encode()) if bad else -1
        raise AssertionError(f"{len(keys)} keys for {len(topic.keys())}; the first that differs is key {bad[:1]} [{topic.names[first] if bad else ''}]")
    assert agg.tolist() == topic.agg().tolist()


def check_host(topic):
    with EventsTopicIngest() as g:
        g.feed(topic.wire)
        agg, ev, off = g.drain_fixed16()
        keys = g.key_table().keys
    assert keys == topic.keys() and ev.tobytes() == topic.event_bytes() and agg.tolist() == topic.agg().tolist() and off.tolist() == list(range(topic.n))


@functools.lru_cache(maxsize=None)
def forced():
    out = G.forced_topics()
    out.update(G.full_block_topics())
    return out


padded = functools.lru_cache(maxsize=None)(G.padded_topics)
crc_topic = functools.lru_cache(maxsize=None)(G.crc_topic)


# ---- a: random parses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", G.FUZZ_SEEDS)
def test_random_parses_of_periodic_ids_decode_to_the_source_records(seed):
    """About 150 KB of records per seed, every batch one frame whose blocks are RANDOM valid parses: any earlier occurrence
    as the match's source, any length up to the longest, literal runs drawn around the thresholds of pass 1 — overlapping
    matches below and above period 64, matches of 256 | 257 | more bytes, runs of 0 | 12 | 13 | 15 | 270 and more literals,
    continued lengths (tests/test_lz4_seqgen.py counts them).  In one push and in three."""
    t = G.fuzz_topic(seed)
    for pushes in (1, 3):
        check(t, decode(t, pushes))
    check_host(t)


@pytest.mark.parametrize("seed", G.MAPPED_SEEDS)
def test_random_parses_for_the_mapped_route_decode_to_the_source_records(seed):
    """The same records parsed at random out of what lz4_exec_kernel expands through its byte map — short matches that do not
    overlap, from sources inside the 64-byte output window (dependency rounds) and below it, groups of 64 sequences that lie
    across a multiple of 2048 (the map wraps): the route a topic of compressed text goes, and a freely drawn parse almost never."""
    t = G.fuzz_topic(seed, mapped=True)
    for pushes in (1, 3):
        check(t, decode(t, pushes))
    check_host(t)


# ---- b: forced sequence edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["literal runs", "match lengths", "window ends", "256 and 257", "block ends", "chains", "overlaps below 64", "overlaps from 64",
                                  "group spans", "match to the end", "offset 65532"])
def test_stated_parses_at_the_decoders_thresholds_decode_to_the_source_records(name):
    """One frame per case, the cases of a kind in one push (a failure names the case):
    literal runs 11 .. 16 in front of a match (12 is the last a simple header of pass 1 holds); match lengths around one and
    two extension bytes; headers that start in the last four bytes of a 64-byte window of the compressed block, simple ones
    and ones for the slow path; matches of 256 (mapped) and 257 bytes (sequence by sequence); a last match whose header lies 16 .. 20 bytes before the
    block's end (16: the window a lane of pass 1 loads ends exactly there); chains of back-to-back short
    matches that read what the match before them wrote, inside one 64-byte output window; overlapping matches of every
    period with lengths around 64 and far above; groups of 64 sequences that span 2048 | 2049 bytes and groups whose map
    wraps; full 64 KiB blocks whose last match ends at the block's end, with the largest offset such a block can hold."""
    t = forced()[name]
    check(t, decode(t))
    check_host(t)


# ---- c: size classes ---------------------------------------------------------------------------------------------------------
def test_blocks_that_fill_a_size_class_exactly_and_by_one_byte_more_decode_to_the_source_records():
    """Decoded sizes C, C + 1 and C + 2 for the capacities 8192 .. 49152 of lz4_exec_kernel's launches, and 65535 | 65536 |
    65537 | 65538 | 65545 (two blocks), each a frame of random parses whose section was tuned to the size.  Every section
    ends with a record without headers: its event's 16 bytes and the one byte of its empty header list are the block's last
    bytes (that one byte is the only one no output of the decoder shows), so the event ends with the class's last byte at
    C + 1, lies across the capacity at C + 2, and across the two blocks at 65538 and 65545."""
    t = G.size_class_topic()
    for pushes in (1, 3):
        check(t, decode(t, pushes))
    check_host(t)


# ---- d: LDS classes of pass 1 -----------------------------------------------------------------------------------------------
def test_blocks_on_either_side_of_the_parse_kernels_lds_classes_at_every_skew_decode_to_the_source_records():
    """All-literal blocks of random bytes with skew + n_in + 48 == 6656 | 6657 | 16448 | 16449 for every skew 0 .. 15 of the
    block's first byte (fillers put each block there: tests/test_lz4_seqgen.py checks the layout), in one push: the last
    block a launch of lz4_parse_kernel stages in its LDS, and the first that belongs to the next."""
    t = G.lds_class_topic()
    check(t, decode(t))
    check_host(t)


# ---- e: the compressed path of lz4_block_kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one padded block", "stored block, padded block"])
def test_a_block_of_exactly_64_kib_of_compressed_bytes_decodes_to_the_source_records(name):
    """A legal frame no writer here produces: 19-byte and 275-byte sequences that do not shrink pad the block to a
    COMPRESSED size of 65536 — the planner gives it to lz4_block_kernel, whose compressed path nothing else runs.  liblz4
    reads both frames (tests/test_lz4_seqgen.py), so the device delivers their records."""
    t = padded()[name]
    check(t, decode(t))
    check_host(t)


# ---- f: CRC-32C length and alignment sweep ----------------------------------------------------------------------------------
def push_in_place(wire, d):
    """One fetch of one partition, received into the group's slab and framed where it lies."""
    with PartitionedFramedFetches(iter([[wire]]), 1, threads=1, hold=1, overlap=False, device_crc=True, device_lz4=True, in_place=True) as framed:
        (secs, slab), = list(framed)
        assert np.all(secs["codec"] == SECTION_CRC_WIRE)
        d.push(secs, slab)
        return secs.shape[0]


@pytest.mark.parametrize("mode", ["pending", "wire"])
def test_the_device_crc_accepts_sections_of_every_length_remainder_and_alignment(mode):
    """One uncompressed batch of random bytes per length: every length from the smallest record to 160, and for one, two
    and three 4 KiB tiles every length whose remainder mod 4096 lies at 0 .. 8, 60 .. 68 (a lane's 64-byte piece) or
    4088 .. 4095 — counted over the bytes the device checksums: the section (PENDING: the host passes on the register after
    the header) or the 40 covered header bytes and the section (WIRE: in-place framing, the register starts at ~0).  Four
    pushes per mode, the filler in front 0 .. 3 bytes longer: every section at each alignment.  A kernel that drops or
    misplaces one byte refuses a good batch."""
    for shift in range(4):
        t = crc_topic(40 if mode == "wire" else 0, shift)
        with DeviceDecoder(None) as d:
            try:
                if mode == "wire":
                    assert push_in_place(t.wire, d) == len(t.batches)
                else:
                    with EventsTopicIngest(frames=True, device_lz4=True, device_crc=True) as g:
                        g.feed(t.wire)
                        secs, arena = g.drain_sections()
                        assert secs.shape[0] == len(t.batches) and np.all(secs["codec"] == SECTION_CRC_PENDING)
                        d.push(secs, arena)
            except IngestError as e:
                raise AssertionError(f"shift {shift}: {named(t, e)}") from e
            check(t, results(d))
        check_host(t)


def test_the_device_crc_of_a_batch_framed_in_place_refuses_one_damaged_byte_wherever_it_lies():
    """WIRE mode: the shortest batch and batches of one, two and three tiles whose checksummed length has remainder 0, 1,
    4095 or 64 mod 4096; one byte damaged per push — the section's first and last byte, the bytes on either side of every
    4 KiB boundary counted from the section's end (where the kernel cuts its tiles), a covered header byte, the crc field.
    Every damaged push fails with SURGE_E_CORRUPT, names the device check and the batch, delivers and interns nothing; the
    undamaged batch goes through the same decoder afterwards."""
    t = crc_topic(40, 0)
    spans = [t.lengths[0] + 40, 128, 4096, 8192, 12288, 4097, 8193, 4095, 8191, 12287, 4160, 8256]
    picked = [b for b in t.batches[1:] if len(b) - 21 in spans]
    assert len(picked) == len(spans)
    fetches, plan = [], []
    for batch in picked:
        n = len(batch)
        spots = {61, n - 1, 30 + 10 * (n % 2), 18}
        for cut in range(n - 4096, 21, -4096):
            spots |= {cut - 1, cut}
        for at in sorted(spots):
            bad = bytearray(batch)
            bad[at] ^= 0x40
            fetches += [bytes(bad), batch]
            plan += [(batch, at), (batch, None)]
    assert 60 <= len(fetches) // 2 <= 140
    seen = ["seen"]
    with DeviceDecoder(None) as d, PartitionedFramedFetches(iter([[f] for f in fetches]), 1, threads=1, hold=1, overlap=False, device_crc=True, device_lz4=True,
                                                            in_place=True) as framed:
        d.push_records([b"seen:1"], [G.event(1, 1, 1)])  # the table holds a key
        d.clear()
        done = 0
        for (batch, at), (secs, slab) in zip(plan, framed):
            (base,), (n,) = struct.unpack_from(">q", batch, 0), struct.unpack_from(">i", batch, 57)
            assert secs.shape[0] == 1 and int(secs["codec"][0]) == SECTION_CRC_WIRE and int(secs["base_offset"][0]) == base
            if at is not None:
                with pytest.raises(IngestError) as err:
                    d.push(secs, slab)
                assert err.value.status == -7, (base, at, str(err.value))
                assert "CRC-32C mismatch (verified on the device)" in str(err.value) and f"base offset {base}" in str(err.value), (at, str(err.value))
                assert d.keys() == seen and d.result()[0].shape[0] == 0
            else:
                d.push(secs, slab)
                agg, ev, off, keys = results(d)
                seen = list(dict.fromkeys(seen + [i.decode() for i in t.ids[base:base + n]]))
                assert off.tolist() == list(range(base, base + n)) and ev == b"".join(t.events[base:base + n]) and keys == seen
                d.clear()
            done += 1
        assert done == len(plan)
