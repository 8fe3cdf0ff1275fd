"""The snappy reader on the host (surge_amd/csrc/snappy_block.h, its exports in snappy_frame.cpp) and codec 2 through the host
framer: against the test's own element writer and model decoder (tests/snappy_cases.py), against pyarrow's bundled snappy in
both directions, every refusal by name, and the batches through EventsTopicIngest and a partition group."""
import ctypes
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import kafka_wire as kw
import snappy_cases as sc
from surge_amd import _native
from surge_amd.ingest import EventsTopicIngest, IngestError, PartitionedFramedFetches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


@pytest.fixture(scope="module")
def corpus():
    return sc.cases()


def product(lib, fn, data, cap):
    """(bytes or None, status) of one of the two decompress exports at capacity ``cap``."""
    dst = ctypes.create_string_buffer(max(cap, 1))
    status = ctypes.c_int32(-1)
    got = getattr(lib, fn)(data, len(data), dst, cap, ctypes.byref(status))
    if got >= 0:
        assert status.value == 0
        return dst.raw[:got], 0
    assert got in (-6, -7) and (got == -6) == (status.value == sc.NO_SPACE), (got, status.value)
    return None, status.value


def expect_of(section):
    try:
        return sc.model_section(section), 0
    except sc.Refused as r:
        return None, r.status


# ---- the writer's streams --------------------------------------------------------------------------------------------------------
def test_the_cases_hold_the_elements_they_mean_to_exercise(corpus):
    by_name = {c.name: sc.count_elements(c.stream)[1] for c in corpus}

    def lits(name):
        return [(e.length, e.header) for e in by_name[name] if e.kind == 0]

    def copies(name):
        return [(e.kind, e.length, e.offset) for e in by_name[name] if e.kind]

    for n, header in ((1, 1), (60, 1), (61, 2), (256, 2), (257, 3)):
        assert (n, header) in lits(f"literal of {n}")
    assert {(5, 5), (5, 4), (6, 3), (1, 2)} <= set(lits("small lengths spelled in 1 2 3 and 4 extension bytes"))
    assert {(1, 4, 2047), (1, 11, 2047), (1, 4, 1), (1, 11, 1)} <= set(copies("copy-1 lengths 4 and 11 at offsets 1 and 2047"))
    assert {(2, 1, 2048), (2, 64, 2048), (2, 1, 1), (2, 64, 1)} <= set(copies("copy-2 lengths 1 and 64 at offsets 1 and 2048"))
    assert {(4, 40, 300), (4, 9, 1), (4, 64, 345)} <= set(copies("copy-4 with an offset below 65536"))
    assert {(2, 64, 1), (2, 63, 2), (2, 64, 3), (2, 64, 63), (1, 11, 10)} <= set(copies("the period is the data: offsets 1 2 3 and M - 1"))
    kinds = [e.kind for e in by_name["a copy behind a copy and a literal behind a literal"]]
    assert any(a and b for a, b in zip(kinds, kinds[1:])) and any(a == 0 and b == 0 for a, b in zip(kinds, kinds[1:]))
    assert by_name["ends with a literal"][-1].kind == 0 and by_name["ends with a copy exactly at its preamble"][-1].kind == 2
    first = by_name["an offset that reaches the chunk's first byte"]
    at = 0
    for e in first:
        if e.kind and e.offset == at:
            break
        at += e.length
    else:
        raise AssertionError("no copy whose offset is its own position")
    for width in (1, 2, 3):
        (case,) = [c for c in corpus if c.name == f"a preamble of {width} byte" + ("s" if width > 1 else "")]
        assert len(sc.varint(len(case.output))) == width
    span = [e for e in by_name["64 consecutive copies spanning more than 2048 bytes"]]
    pos, ends = 0, []
    for e in span:
        pos += e.length
        if e.kind:
            ends.append(pos)
    assert len(ends) >= 64 and ends[63] - ends[0] > 2048
    assert [(e.kind, e.length) for e in by_name["a chunk of 65536 bytes that is one literal"]] == [(0, 65536)]
    assert [(e.kind, e.length, e.offset) for e in by_name["a copy of offset 65535 that ends at 65536"]] == [(0, 65535, 0), (2, 1, 65535)]
    assert max(e.length for e in by_name["long literals that leave their window"] if e.kind == 0) > 128
    assert sum(1 for e in by_name["a dense chain of short elements"] if e.kind) >= 400


def test_the_product_decodes_every_hand_built_stream_to_the_writers_output(lib, corpus):
    for c in corpus:
        assert sc.model_uncompress(c.stream) == c.output == sc.records_section(c.records), c.name
        want = ctypes.c_int32(-1)
        assert lib.surge_snappy_uncompressed_length(c.stream, len(c.stream), ctypes.byref(want)) == len(c.output) and want.value == 0
        assert product(lib, "surge_snappy_uncompress", c.stream, len(c.output)) == (c.output, 0), c.name
        assert product(lib, "surge_snappy_uncompress", c.stream, len(c.output) + 7) == (c.output, 0), c.name
        assert product(lib, "surge_snappy_uncompress", c.stream, len(c.output) - 1) == (None, sc.NO_SPACE), c.name
        longer = sc.overlong_preamble(c)
        assert len(longer) == len(c.stream) + 1 and product(lib, "surge_snappy_uncompress", longer, len(c.output)) == (c.output, 0), c.name
    empty = sc.empty_chunk()
    assert empty == b"\x00" and product(lib, "surge_snappy_uncompress", empty, 0) == (b"", 0)
    assert product(lib, "surge_snappy_uncompress", b"\x80\x80\x00", 0) == (b"", 0)  # the empty block, over-long


def test_pyarrows_snappy_reads_the_hand_built_streams_and_the_product_reads_pyarrows_blocks(lib, corpus):
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("snappy")
    for c in corpus:
        assert codec.decompress(c.stream, decompressed_size=len(c.output), asbytes=True) == c.output, c.name
    rng = random.Random(5)
    texts = [b"", b"a", b"ab" * 40000, rng.randbytes(70000), b"".join(b'{"aggregateId":"agg-%d","count":%d}' % (i % 97, i) for i in range(4000))]
    for text in texts:
        block = codec.compress(text, asbytes=True)
        assert product(lib, "surge_snappy_uncompress", block, len(text)) == (text, 0)
        assert product(lib, "surge_snappy_frame_decompress", block, len(text)) == (text, 0)  # one raw block is a section too
        framed = sc.compress_section(text, block=sc.arrow_block())
        status = ctypes.c_int32(-1)
        assert lib.surge_snappy_frame_bound(framed, len(framed), ctypes.byref(status)) == len(text) and status.value == 0
        assert product(lib, "surge_snappy_frame_decompress", framed, len(text)) == (text, 0)


def test_every_refusal_by_name(lib):
    names = set()
    for name, (section, status) in sc.refusals().items():
        cap = 1 << 16
        assert product(lib, "surge_snappy_frame_decompress", section, cap) == (None, status), name
        if not name.startswith("framing"):
            assert product(lib, "surge_snappy_uncompress", section, cap) == (None, status), name
        text = lib.surge_snappy_status_name(status).decode()
        assert "snappy" in text, text
        names.add(status)
    assert names == set(range(sc.PREAMBLE_TRUNCATED, sc.TRAILING_BYTES + 1))  # one named input, at least, per refusal
    assert len({lib.surge_snappy_status_name(s) for s in range(sc.TOO_LARGE + 1)}) == sc.TOO_LARGE + 1
    # bad arguments are not refusals of the input
    assert lib.surge_snappy_uncompress(None, 0, None, 0, None) == -1 and lib.surge_snappy_frame_decompress(b"\x00", 1, None, 4, None) == -1
    assert lib.surge_snappy_frame_bound(b"\x00", -1, None) == -1


def test_the_frame_reader_on_framed_and_raw_sections_of_one_to_three_chunks(lib, corpus):
    small = [c for c in corpus if len(c.output) < 4000]
    for k in (1, 2, 3):
        for take in (small[:k], small[3:3 + k], small[-k:]):
            section = sc.frame([c.stream for c in take])
            want = b"".join(c.output for c in take)
            assert sc.model_section(section) == want
            status = ctypes.c_int32(-1)
            assert lib.surge_snappy_frame_bound(section, len(section), ctypes.byref(status)) == len(want)
            assert product(lib, "surge_snappy_frame_decompress", section, len(want)) == (want, 0)
            assert product(lib, "surge_snappy_frame_decompress", section, len(want) - 1) == (None, sc.NO_SPACE)
    with_empty = sc.frame([small[0].stream, sc.empty_chunk(), small[1].stream, sc.empty_chunk()])
    assert product(lib, "surge_snappy_frame_decompress", with_empty, 1 << 16) == (small[0].output + small[1].output, 0)
    assert product(lib, "surge_snappy_frame_decompress", sc.frame([]), 16) == (b"", 0)  # the header alone: an empty section
    for c in small[:4]:  # without the magic: one raw block
        assert product(lib, "surge_snappy_frame_decompress", c.stream, len(c.output)) == (c.output, 0)


def test_seeded_mutations_decode_as_the_model_says_or_are_refused_with_its_status(lib, corpus):
    streams = [(c.name, c.stream) for c in corpus if len(c.stream) < 20000]
    framed = [("framed " + c.name, sc.frame([c.stream, corpus[0].stream])) for c in corpus[:6]]
    seen = set()
    for name, data in sc.mutations(streams + framed, per_stream=6):
        want = expect_of(data)
        assert product(lib, "surge_snappy_frame_decompress", data, 1 << 17) == want, name
        seen.add(want[1])
    assert {0, sc.OUTPUT_SHORT, sc.OFFSET_BEYOND_OUTPUT, sc.LITERAL_PAST_INPUT} <= seen


# ---- record batches with codec 2 through the host framer ------------------------------------------------------------------------
def topic(rng, codec_section, n_batches=9):
    """(plain wire, snappy wire, records delivered): data batches of 1 .. 120 records, every third transactional — one of those
    aborted — closed by markers; codec_section(records section) -> the compressed section."""
    plain, snap, delivered, off = [], [], [], 0
    for b in range(n_batches):
        recs = [(b"agg-%d:%d" % (rng.randrange(40), off + i), rng.randbytes(rng.randrange(0, 300)) if i % 7 else b"x" * rng.randrange(900)) for i in range(rng.randrange(1, 121))]
        kwargs = dict(transactional=True, producer_id=7 + b, base_sequence=0) if b % 3 == 2 else {}
        plain.append(kw.record_batch(off, recs, **kwargs))
        snap.append(sc.batch(off, recs, codec_section(sc.records_section(recs)), **kwargs))
        aborted = b == 5
        if not aborted:
            delivered += [(off + i, k, v) for i, (k, v) in enumerate(recs)]
        off += len(recs)
        if kwargs:
            marker = kw.control_batch(off, 7 + b, 0 if aborted else 1)
            plain.append(marker)
            snap.append(marker)
            off += 1
    return b"".join(plain), b"".join(snap), delivered


WRITERS = {
    "framed 32 KiB chunks": lambda s: sc.compress_section(s),
    "framed 1000-byte chunks": lambda s: sc.compress_section(s, chunk=1000),
    "one raw block": sc.greedy_block,
}


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_snappy_batches_through_the_host_route_equal_the_same_records_uncompressed(writer):
    plain, snap, delivered = topic(random.Random(11), WRITERS[writer])
    got = []
    for wire in (plain, snap):
        with EventsTopicIngest() as g:
            g.feed(wire)
            got.append((g.drain_records(), g.counters()))
    assert [(o, k, v) for o, _, k, v in got[1][0]] == delivered
    assert got[0][0] == got[1][0]
    a, b = got[0][1], got[1][1]
    assert b["bytes_decompressed"] > 0 and a["bytes_decompressed"] == 0
    assert {k: v for k, v in a.items() if k != "bytes_decompressed"} == {k: v for k, v in b.items() if k != "bytes_decompressed"}
    assert b["records_aborted"] > 0 and b["control_batches"] == 3


def test_pyarrow_written_batches_through_the_host_route():
    pytest.importorskip("pyarrow")
    plain, snap, delivered = topic(random.Random(12), lambda s: sc.compress_section(s, block=sc.arrow_block()))
    with EventsTopicIngest() as g:
        g.feed(snap)
        assert [(o, k, v) for o, _, k, v in g.drain_records()] == delivered


def section_bytes(item):
    sections, address = item
    return [(int(s["base_offset"]), int(s["n_records"]), int(s["codec"]) & 0xFF, ctypes.string_at(address + int(s["byte_off"]), int(s["byte_len"]))) for s in sections]


def test_a_frames_mode_framer_decompresses_on_the_host_or_leaves_the_section_as_it_is_on_the_wire():
    plain, snap, _ = topic(random.Random(13), WRITERS["framed 1000-byte chunks"])
    out = {}
    for name, wire, flags in (("plain", plain, {}), ("host", snap, {}), ("wire", snap, dict(device_lz4=True)), ("wire+crc", snap, dict(device_lz4=True, device_crc=True))):
        with EventsTopicIngest(frames=True, **flags) as g:
            g.feed(wire)
            out[name] = section_bytes(g.drain_sections())
    assert out["host"] == out["plain"] and all(c == 0 for _, _, c, _ in out["host"])
    assert [(o, n) for o, n, _, _ in out["wire"]] == [(o, n) for o, n, _, _ in out["plain"]]
    for (_, _, codec, sec), (_, _, _, raw) in zip(out["wire"], out["plain"]):
        assert codec == 2 and sc.model_section(sec) == raw
    assert [s[:3] for s in out["wire+crc"]] == [s[:3] for s in out["wire"]]


def test_a_partition_group_grows_its_slices_for_host_side_snappy_and_delivers_the_same_sections():
    rng = random.Random(14)
    parts = [topic(rng, WRITERS["framed 32 KiB chunks"], n_batches=6) for _ in range(3)]
    # text that compresses well: the first trial's slices (the feed's own size) do not hold what the host decompresses into them
    recs = [(b"k:%d" % i, b"abcdefgh" * 400) for i in range(40)]
    parts.append((kw.record_batch(0, recs), sc.batch(0, recs, sc.compress_section(sc.records_section(recs))), None))
    got = {}
    for name, which, flags in (("plain", 0, dict(device_lz4=False)), ("host", 1, dict(device_lz4=False)), ("wire", 1, dict(device_lz4=True, device_crc=False))):
        with PartitionedFramedFetches([[p[which] for p in parts]], n_partitions=4, threads=2, overlap=False, **flags) as framed:
            got[name] = [section_bytes(item) for item in framed]
            got[name + " counters"] = framed.counters()
    assert got["host"] == got["plain"]
    assert got["host counters"]["bytes_decompressed"] > got["plain counters"]["bytes_decompressed"] == 0
    assert all(c == 2 for _, _, c, _ in got["wire"][0])
    assert [sc.model_section(s) for _, _, _, s in got["wire"][0]] == [s for _, _, _, s in got["plain"][0]]


def test_a_bad_snappy_batch_fails_the_feed_with_the_refusals_own_words(lib):
    recs = [(b"k:0", b"v")]
    for name, (section, status) in sc.refusals().items():
        with EventsTopicIngest() as g:
            with pytest.raises(IngestError) as ei:
                g.feed(sc.batch(0, recs, section))
            assert ei.value.status == -7 and "snappy" in str(ei.value), name
            # (the framer sizes its buffer by the preambles first, and there a preamble that no block of its size can reach — an
            # element gives at most 64 bytes for 3 — is refused as short before anything is decoded)
            if not name.startswith("framing") and status > sc.PREAMBLE_TOO_LARGE and sc.read_varint(section)[0] > 32 * len(section):
                status = sc.OUTPUT_SHORT
            assert lib.surge_snappy_status_name(status).decode() in str(ei.value), name
            assert g.ready == 0


def test_in_place_framing_refuses_snappy_without_the_device_flag_and_gzip_and_zstd_stay_unsupported():
    recs = [(b"k:0", b"v")]
    for codec in (1, 4):
        for flags in ({}, dict(frames=True), dict(frames=True, device_lz4=True)):
            with EventsTopicIngest(**flags) as g:
                with pytest.raises(IngestError) as ei:
                    g.feed(kw.record_batch(0, recs, codec_override=codec))
                assert ei.value.status == -5 and "codec not supported" in str(ei.value) and "snappy" in str(ei.value)
    wire = sc.batch(0, recs, sc.compress_section(sc.records_section(recs)))
    with PartitionedFramedFetches([[wire]], n_partitions=1, threads=1, overlap=False, device_lz4=False, in_place=True) as framed:
        assert section_bytes(next(framed))[0][3] == sc.records_section(recs)  # (in_place needs device_lz4: without it the group frames by copy)


def test_the_exports_are_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "surge_ingest.h")).read()
    for name in _native.SNAPPY_EXPORTS:
        assert name + "(" in header and name in _native.SNAPPY_H
    assert "surge_device_decoder_route_stats(" in header
    assert {"snappy_frame.cpp", "ingest_snappy.hip"} <= set(_native.SOURCES)
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in _native.SNAPPY_EXPORTS + ("surge_device_decoder_route_stats",):
        assert f" T {name}\n" in nm, name


# ---- the sanitizer run -----------------------------------------------------------------------------------------------------------
def test_no_prefix_or_mutation_makes_the_reader_read_or_write_outside_its_buffers_under_asan_and_ubsan(tmp_path, corpus):
    """tests/cpp/snappy_prefixes.cpp: every corpus stream (raw and framed), every prefix of it, every named refusal and the seeded
    mutations, each in a malloc of exactly its length and decoded into one of exactly the capacity tried, through the exports
    built with -fsanitize=address,undefined — a stand-alone program that reads the corpus from a file; nothing of it is loaded
    into this process."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    whole = [(c.stream, 0, len(c.output)) for c in corpus]
    whole += [(sc.frame([c.stream, sc.empty_chunk(), corpus[1].stream]), 0, len(c.output) + len(corpus[1].output)) for c in corpus[:8]]
    whole += [(section, status, 1 << 12) for section, status in sc.refusals().values()]
    mutated = sc.mutations([(c.name, c.stream) for c in corpus if len(c.stream) < 20000] + [("framed", sc.frame([c.stream for c in corpus[:3]]))], per_stream=8, seed=7)
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        for section, status, out_len in whole:
            f.write(struct.pack("<BBII", 1, status, len(section), out_len) + section)
        for _, section in mutated:
            f.write(struct.pack("<BBII", 0, 0xFF, len(section), 1 << 17) + section)
    exe = str(tmp_path / "snappy_prefixes")
    srcs = [os.path.join(ROOT, "tests", "cpp", "snappy_prefixes.cpp"), os.path.join(ROOT, "surge_amd", "csrc", "snappy_frame.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in (build.stderr or "").lower() or "ubsan" in (build.stderr or "").lower()):
        pytest.skip("no AddressSanitizer / UBSan runtime next to g++")
    assert build.returncode == 0, build.stderr[-3000:]
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "PASS" in res.stdout and "Sanitizer" not in res.stderr, res.stdout[-1500:] + res.stderr[-4000:]
