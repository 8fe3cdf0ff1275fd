"""tests/lz4_blockgen.py on the CPU: the inputs of tests/test_frame_lz4_edges_gpu.py have the sizes they are said to have and
are what the host writer AND the independent test-side writer frame them as (which pins the host writer, the GPU tests'
expected value, on kafka_wire for values beyond 8 KiB and 1 MiB); every named case REACHES the edge it is named for --
shown on wave_compress, the CPU restatement of the device compressor's scheme: without this the GPU tests could pass
without testing anything --; and the scheme's output, like the host compressor's, is a valid LZ4 block."""
import numpy as np
import pytest

import kafka_wire as kw
import lz4_blockgen as g

TS = 1_700_000_000_000


def model_blocks(name):
    """[(block, compressed or None)] over every block of every section of a case."""
    _, _, sections = g.case(name)
    return [(b, g.wave_compress(b)) for s in sections for b in g.blocks_of(s)]


def sequences(name):
    return [q for _, c in model_blocks(name) if c is not None for q in g.walk_sequences(c)]


def host_sections(records, max_records=1):
    """The host writer's records sections and its bytes for the records in one partition."""
    from surge_amd.snapshot import RecordBatchWriter

    inp, _ = g.section([v for _, v in records], [k for k, _ in records])
    with RecordBatchWriter(1, max_records, 1 << 30) as w:
        w.append(*inp, TS)
        data, nrec, _ = w.partition_bytes(0)
    assert nrec == len(records)
    return [r for _, r in g.walk_batches(data)], data


# ---- 1: sizes, and the two writers ----------------------------------------------------------------------------------
def test_sections_have_the_stated_sizes():
    for name in ("block_sizes_zeros", "block_sizes_period7"):
        assert [len(s) for s in g.case(name)[2]] == g.BLOCK_SIZES
    assert g.PAIR_SIZES == [65] and all(n in g.BLOCK_SIZES + g.PAIR_SIZES for n in [8, 12, 13, 64, 80, 4096, 4097, 65536, 65537, 131072, 131074])
    for fill in (g.zeros, g.periodic(g.PERIOD7)):
        assert len(g.pair_for_section_size(65, fill)[1]) == 65
    with pytest.raises(ValueError):
        g.value_for_section_size(65, g.zeros)  # a body of 63 bytes gives 64, of 64 bytes 66
    for n in (8, 64, 66, 8193, 8195, 8196, (1 << 20) + 2, (1 << 20) + 5, (1 << 20) + 6):  # on either side of the prefix steps
        assert len(kw.record(0, b"k", g.value_for_section_size(n, g.zeros))) == n
    assert [len(s) for s in g.case("block_ends")[2]] == [n for n in g.END_SIZES for _ in range(5)]
    assert [len(s) for s in g.case("far_offsets")[2]] == [n for n in g.FAR_SIZES for _ in range(3)]
    assert {len(s) for s in g.case("mixed_frames")[2]} == {5 * g.BLOCK + 30000}
    recs, parts = g.case_many_partitions()
    assert sorted({len(kw.record(0, k, v)) for k, v in recs}) == [8, 300 * 1024] and parts == list(range(64))
    # a section is head + value + 0x00: below 1 MiB at most 10 bytes of head beside the key
    for name in g.CASES:
        for (k, v), s in zip(*g.case(name)[::2]):
            assert s.endswith(v + b"\0") and len(s) - len(v) - len(k) - 1 <= 10


@pytest.mark.parametrize("name", sorted(g.CASES))
def test_a_representative_of_every_case_is_framed_alike_by_the_host_writer_and_the_test_side_writer(name):
    records, _, sections = g.case(name)
    order = sorted(range(len(records)), key=lambda i: len(sections[i]))
    pick = sorted({order[0], order[len(order) // 2], 0, len(records) - 1})[:3]  # the smallest, the median, the first, capped by size below
    pick = [i for i in pick if len(sections[i]) <= 140000] or [order[0]]
    host, data = host_sections([records[i] for i in pick])
    assert host == [sections[i] for i in pick]
    assert data == b"".join(kw.record_batch(j, [records[i]], base_timestamp=TS, producer_epoch=-1) for j, i in enumerate(pick))


@pytest.mark.parametrize("lengths,per_batch", [
    (range(8170, 8200), 70),                           # bodies around 8192: the record's length prefix goes to 3 bytes
    ([(1 << 20) - 15, (1 << 20) - 14, (1 << 20) - 13], 70),  # bodies around 2^20: it goes to 4
    ([100_000, 65536 * 3 + 1, 8192], 2),
])
def test_the_host_writer_frames_large_values_as_the_test_side_writer_does(lengths, per_batch):
    rng = np.random.default_rng(len(lengths))
    records = [(b"key-%d" % i, g.rnd(rng, L)) for i, L in enumerate(lengths)]
    sizes = {next(i for i, b in enumerate(kw.record(0, k, v)) if b < 0x80) + 1 for k, v in records}  # bytes of the length prefix
    assert len(sizes) > 1 or per_batch == 2, sizes  # the sweep crosses a step of the length prefix
    _, data = host_sections(records, per_batch)
    assert data == b"".join(kw.record_batch(s, records[s:s + per_batch], base_timestamp=TS, producer_epoch=-1) for s in range(0, len(records), per_batch))


# ---- 2: every case reaches its edge ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block_sizes_zeros", "block_sizes_period7"])
def test_block_sizes_store_what_must_be_stored_and_compress_the_rest(name):
    blocks = model_blocks(name)
    assert all(c is None for b, c in blocks if len(b) <= 12) and sum(len(b) <= 12 for b, _ in blocks) == 5 + 6
    assert sorted(len(b) for b, c in blocks if len(b) <= 4) == [1, 1, 2, 2, 3, 4]  # the last blocks of 65537 .. 65540, 131073, 131074
    assert all(c is not None and len(c) < len(b) for b, c in blocks if len(b) >= 64)
    sizes = {len(b) for b, _ in blocks}
    assert {64, 75, 76, 4096, 4097, 65535, 65536} <= sizes  # one window / two, both hash tables, a full block
    for fill in (g.zeros, g.periodic(g.PERIOD7)):
        sec = g.pair_for_section_size(65, fill)[1]
        assert g.wave_compress(sec) is not None
    # last windows with 1, 2, .. active lanes: n - 11 positions may start a match
    assert {(n - 11) % 64 for n in sizes | set(g.PAIR_SIZES) if 13 <= n <= 80} >= set(range(2, 64))


def test_literal_runs_reach_every_class_of_length_bytes():
    records, _, sections = g.case("literal_runs")
    n_plain = len(g.LITERAL_LENGTHS)
    lb = [{q[3] for q in g.walk_sequences(g.wave_compress(s))} for s in sections]
    assert {0, 1, 2, 64, 65} <= set().union(*lb[:n_plain])
    assert {0, 1, 2, 64, 65} <= set().union(*lb[n_plain:])
    lits = {q[0] for s in sections[:n_plain] for q in g.walk_sequences(g.wave_compress(s))[:1]}
    assert {64, 256, 320, 16320, 16384} <= lits and sum(x % 64 != 0 for x in lits) <= 2  # steps of 64: the window (but for a chance repeat)
    primed = {q[0] for s in sections[n_plain:] for q in g.walk_sequences(g.wave_compress(s))}
    assert {14, 15, 269, 270, 16334} <= primed and any(x >= 16335 for x in primed)  # ... and byte by byte behind a match


@pytest.mark.parametrize("name,offset", [("match_lengths_byte", 1), ("match_lengths_period3", 3), ("match_lengths_period64", 64)])
def test_match_lengths_reach_every_class_of_length_bytes(name, offset):
    seqs = sequences(name)
    assert {0, 1, 2, 64, 65} <= {q[4] for q in seqs} and {273, 274} <= {q[2] for q in seqs}
    long = [q for q in seqs if q[2] >= 270]
    assert long and all(q[1] % offset == 0 and q[1] < 64 + offset for q in long)  # overlapping copies of the pattern
    assert len({q[2] for q in seqs} & set(range(16339 - 20, 16339 + 20))) >= 30 and {16338, 16339} <= {q[2] for q in seqs}  # across the 64 / 65 step


def test_whole_blocks_are_one_match_with_257_length_bytes():
    blocks = model_blocks("whole_blocks")
    whole = [(b, c) for b, c in blocks if b in (bytes(g.BLOCK), b"\xff" * g.BLOCK)]
    assert len(whole) == 4
    for b, c in whole:
        seqs = g.walk_sequences(c)
        assert [(q[1], q[2], q[4]) for q in seqs] == [(1, g.BLOCK - 6, 257), (0, 0, 0)] and seqs[0][0] == 1 and seqs[1][0] == 5


def test_block_ends_reach_the_limits_of_the_end_rules():
    _, _, sections = g.case("block_ends")
    for i, n in enumerate(g.END_SIZES):
        at12, at11, at13, z40, z100 = [g.wave_compress(s) for s in sections[5 * i:5 * i + 5]]
        assert (n - 11) % 64 in (1, 32, 63)
        size, matches, last = g.walk_block(at12)
        assert matches == [(n - 12, 7)] and last == 5 and len(at12) == n - 2  # starts at n - 12, ends at n - 5
        assert at11 is None                                                   # no match may start at n - 11
        size, matches, last = g.walk_block(at13)
        assert matches == [(n - 13, 7)] and last == 6
        for c in (z40, z100):
            assert c is not None
            size, matches, last = g.walk_block(c)
            assert size == n and last == 5 and sum(matches[-1]) == n - 5      # cut at n - 5


def test_far_offsets_reach_the_candidate_at_position_0_and_the_largest_offset():
    _, _, sections = g.case("far_offsets")
    for i, n in enumerate(g.FAR_SIZES):
        rzr, copy64, copy12 = [g.walk_sequences(g.wave_compress(s)) for s in sections[3 * i:3 * i + 3]]
        assert max(q[1] for q in rzr) > n - 200
        assert n - 64 in {q[1] for q in copy64}   # a match at n - 64 whose candidate is position 0
        assert n - 12 in {q[1] for q in copy12}   # ... and at n - 12: no offset of a block of n bytes is larger
    assert 65524 in {q[1] for q in g.walk_sequences(g.wave_compress(sections[-1]))}


@pytest.mark.parametrize("r_len", [300, 2000, 60000])
def test_the_stored_decision_is_crossed_byte_by_byte(r_len):
    blocks = model_blocks(f"stored_decision_{r_len}")
    assert len(blocks) == len(g.STORED_K) + (len(g.STORED_K_RECENT) if r_len == 60000 else 0)
    saved = [None if c is None else len(b) - len(c) for b, c in blocks]
    assert None in saved and any(s is not None for s in saved)
    assert all(s is None or s > 0 for s in saved)
    # a stored block whose neighbour in the sweep is compressed, and saves at most 3 bytes
    assert any(a is None and b is not None and b <= 3 for a, b in zip(saved, saved[1:]))


def test_binary_values_hold_every_byte_value_and_compress():
    records, _, sections = g.case("binary")
    assert set(b"".join(sections)) == set(range(256))
    assert any(min(v) >= 0x80 for _, v in records)
    assert all(c is not None for _, c in model_blocks("binary")[:6])
    assert sum(c is not None for _, c in model_blocks("binary")) >= 40


def test_protobuf_state_is_the_protobuf_runtimes_state_message():
    """message State { string aggregateId = 1; bytes payload = 2; }: the bytes surge_amd/encode.py's "protobuf_state"
    envelope is held to (tests/test_gpu_parity.py), from Google's encoder."""
    pytest.importorskip("google.protobuf")
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    fd = descriptor_pb2.FileDescriptorProto(name="lz4_blockgen_state.proto", syntax="proto3")
    m = fd.message_type.add(name="State")
    F = descriptor_pb2.FieldDescriptorProto
    m.field.add(name="aggregateId", number=1, type=F.TYPE_STRING, label=F.LABEL_OPTIONAL)
    m.field.add(name="payload", number=2, type=F.TYPE_BYTES, label=F.LABEL_OPTIONAL)
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    State = message_factory.GetMessageClass(pool.FindMessageTypeByName("State"))
    for key, payload in [(b"acct-7", bytes(range(256)) * 3), (b"k" * 127, b"\xff" * 127), (b"k" * 128, b"\x80" * 20000)]:
        assert g.protobuf_state(key, payload) == State(aggregateId=key.decode(), payload=payload).SerializeToString()
    records = g.case("binary")[0]
    assert sum(v == g.protobuf_state(k, State.FromString(v).payload) and State.FromString(v).aggregateId == k.decode() for k, v in records[6:]) == 40


def test_mixed_frames_put_compressed_blocks_of_every_size_modulo_8_behind_stored_ones():
    _, _, sections = g.case("mixed_frames")
    rem = set()
    for s in sections:
        comp = [g.wave_compress(b) for b in g.blocks_of(s)]
        assert [c is None for c in comp] == [True, False, True, False, True, False]
        rem |= {len(c) % 8 for c in comp if c is not None}
    assert rem == set(range(8))
    recs, _ = g.case_many_partitions()
    big = [kw.record(0, k, v) for k, v in recs if v]
    assert len(big) == 22 and all([g.wave_compress(b) is None for b in g.blocks_of(s)] == [True, False, True, False, True] for s in big[:4])
    assert sum(len(kw.record(0, k, v)) for k, v in recs) < 7 << 20


# ---- 3: valid output, and the one size condition --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(g.CASES))
def test_the_scheme_and_the_host_compressor_write_valid_blocks_and_the_scheme_compresses_what_compresses_well(name):
    pa = g.pa_lz4()
    for b, c in model_blocks(name):
        hc = g.host_compress(b)
        assert g.block_decode(hc) == b
        if c is not None:
            assert len(c) < len(b) and g.block_decode(c) == b
            size, matches, last = g.walk_block(c)
            assert size == len(b) and last >= 5 and all(start <= size - 12 for start, _ in matches)
        if 2 * len(hc) < len(b):  # the one size condition: what the host compressor halves, the scheme compresses
            assert c is not None, (name, len(b), len(hc))
        if pa is not None:
            for body in (hc, c):
                if body is not None and len(body) <= g.BLOCK:  # (the host compressor's output of a random block is longer than a frame's block may be)
                    assert g.lz4_decompress(g.frame_of_blocks([(False, body)]), len(b)) == b
    if pa is not None:  # kafka_wire's own frame of a whole section
        s = g.case(name)[2][-1]
        assert g.lz4_decompress(kw.lz4_frame(s), len(s)) == s


def test_what_the_host_writers_own_compressor_halves_the_scheme_compresses():
    """The size condition as the GPU tests state it: against RecordBatchWriter(compression="lz4"), whose frames the
    test-side walkers must be able to walk."""
    from surge_amd.snapshot import RecordBatchWriter

    recs, parts = g.case_many_partitions()
    inputs = [(1, g.case(name)[1]) for name in sorted(g.CASES)] + [(64, g.section([v for _, v in recs], [k for k, _ in recs], parts, 64)[0])]
    halved = 0
    for n_part, inp in inputs:
        with RecordBatchWriter(n_part, 1) as w, RecordBatchWriter(n_part, 1, compression="lz4") as wz:
            w.append(*inp, TS)
            wz.append(*inp, TS)
            for p in range(n_part):
                raw, lz = g.walk_batches(w.partition_bytes(p)[0]), g.walk_batches(wz.partition_bytes(p)[0])
                assert len(raw) == len(lz) > 0
                for (_, records), (_, frame) in zip(raw, lz):
                    blocks, src = g.walk_frame(frame), g.blocks_of(records)
                    assert len(blocks) == len(src)
                    for (stored, body), s in zip(blocks, src):
                        if not stored and 2 * len(body) < len(s):
                            halved += 1
                            assert g.wave_compress(s) is not None, (len(s), len(body))
    assert halved > 1000


def test_the_scheme_stores_and_splits_as_the_kernel_header_says():
    assert g.wave_compress(b"") is None and g.wave_compress(bytes(12)) is None
    assert g.block_decode(g.wave_compress(bytes(13))) == bytes(13)  # pure zeros: position 0 is the candidate
    rng = np.random.default_rng(1)
    assert g.wave_compress(g.rnd(rng, 5000)) is None
    b = bytes(4096) + b"x"
    assert g.hash_log_for(4096) == 11 and g.hash_log_for(4097) == 13
    assert g.block_decode(g.wave_compress(b)) == b and g.block_decode(g.wave_compress(b, 11)) == b
