"""-m gpu: the device LZ4 compressor and framer (frame_lz4_block_kernel, frame_lz4_pack_kernel in
surge_amd/csrc/frame_lz4.hip) at the edges they branch on: hand-built blocks from tests/lz4_blockgen.py, whose CPU test
(tests/test_lz4_blockgen.py) has shown on a restatement of the kernel's scheme that every case reaches the edge it is
named for.  What the CPU cannot show is what the wave does: the ballots, the one-wave barrier, the strided length writes,
the unaligned 8-byte copies.

Every test frames its input with DeviceFramer(compression="lz4") and with the host writer, uncompressed, and holds the
device's output to check_against_uncompressed: the host writer's batches and header fields, the CRC of the compressed
batch, the block count, the end rules, stored if and only if not smaller, and -- the assertion that matters -- liblz4's
decompression of every frame equal to the host writer's records.  Then the case's own checks, on the device's own blocks.

Sizes: no ratio is asserted on hand-built blocks (a wave misses the repeat that begins inside a window of new content: 1.19 x
the host compressor on ``64 random bytes + zeros + the same 64 bytes``); every test prints device bytes over
RecordBatchWriter(compression="lz4") bytes (profiles/frame_lz4_edges.json).  The one size condition: a block the host
compressor brings below half its input comes out of the device compressed."""
import numpy as np
import pytest

import lz4_blockgen as g
from lz4_blockgen import BLOCK, check_against_uncompressed, device_frames, host_frames, walk_batches, walk_block, walk_frame, walk_sequences

pytestmark = pytest.mark.gpu

pa = pytest.importorskip("pyarrow")  # liblz4 as Apache Arrow bundles it: the pin every test here rests on
if not pa.Codec.is_available("lz4"):
    pytest.skip("this pyarrow build has no LZ4 frame codec", allow_module_level=True)

TS = 1_700_000_000_000


def publish(name, inp, sections=None, n_part=1, max_records=1):
    """The routine of every test here, for one publish.  Returns ``{partition: [[(stored, body, source block)] per batch]}``
    of the device's output, and the device's bytes."""
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    with RecordBatchWriter(n_part, max_records) as w, RecordBatchWriter(n_part, max_records, compression="lz4") as wz, \
            DeviceFramer(n_part, 0, max_records, compression="lz4") as f:
        exp = host_frames(w, inp, TS)
        got = device_frames(f, inp, TS)
        host = host_frames(wz, inp, TS)
        assert f.records == int(np.count_nonzero(inp[0])) and f.uncompressed_bytes == sum(len(v) for v in exp.values())
        assert list(f.next_offsets()) == [w.partition_bytes(p)[2] for p in range(n_part)]
    check_against_uncompressed(got, exp)
    out = {}
    for p in exp:
        records = [r for _, r in walk_batches(exp[p])]
        if sections is not None and n_part == 1 and max_records == 1:
            assert records == sections  # the host writer frames the case as the test-side writer does
        dev = [walk_frame(fr) for _, fr in walk_batches(got[p])]
        hst = [walk_frame(fr) for _, fr in walk_batches(host[p])]
        assert len(dev) == len(hst) == len(records)
        out[p] = []
        for r, db, hb in zip(records, dev, hst):
            src = g.blocks_of(r)
            assert len(db) == len(hb) == len(src)
            for (d_stored, d_body), (h_stored, h_body), s in zip(db, hb, src):
                if not h_stored and 2 * len(h_body) < len(s):  # the one size condition
                    assert not d_stored and len(d_body) < len(s), (name, len(s), len(h_body), len(d_body))
            out[p].append([(st, body, s) for (st, body), s in zip(db, src)])
    d, h = sum(map(len, got.values())), sum(map(len, host.values()))
    print(f"lz4-edges {name}: device {d} bytes, host {h} bytes, ratio {d / h:.4f}")
    return out, got


def run_case(name):
    _, inp, sections = g.case(name)
    out, got = publish(name, inp, sections)
    return out[0], got


def sequences(batches):
    return [q for blocks in batches for stored, body, _ in blocks if not stored for q in walk_sequences(body)]


def read_back(got, inp):
    """The project's host decoder reads the device's batches: keys and values of the input, offsets from 0."""
    from surge_amd.ingest import EventsTopicIngest

    kind, part, keys, key_off, vals, val_off = inp
    for p, data in got.items():
        with EventsTopicIngest() as ing:  # CRC, framing, LZ4 and varints are checked by the reader
            ing.feed(data)
            recs = ing.drain_records()
        idx = [a for a in range(len(kind)) if kind[a] and part[a] == p]
        assert [r[0] for r in recs] == list(range(len(idx)))
        for (_, _, k, v), a in zip(recs, idx):
            assert k == keys[key_off[a]:key_off[a + 1]].tobytes()
            assert v == (vals[val_off[a]:val_off[a + 1]].tobytes() if kind[a] == 1 else None)


# ---- block sizes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fill", [("block_sizes_zeros", g.zeros), ("block_sizes_period7", g.periodic(g.PERIOD7))])
def test_blocks_of_every_size_are_stored_or_compressed_as_their_size_asks(name, fill):
    batches, _ = run_case(name)
    pair, pair_section = g.pair_for_section_size(65, fill)  # no one record has a section of 65 bytes
    inp, _ = g.section([v for _, v in pair], [k for k, _ in pair])
    out, _ = publish(name + "_65", inp, max_records=2)
    assert [s for blocks in out[0] for _, _, s in blocks] == [pair_section]
    blocks = [b for bl in batches + out[0] for b in bl]
    assert sorted({len(s) for bl in batches + out[0] for s in [b"".join(x[2] for x in bl)]}) == sorted(g.BLOCK_SIZES + g.PAIR_SIZES)
    assert sum(len(s) <= 12 for _, _, s in blocks) == 11 and all(stored for stored, _, s in blocks if len(s) <= 12)
    assert sorted(len(s) for _, _, s in blocks if len(s) <= 4) == [1, 1, 2, 2, 3, 4]  # the last blocks of 65537 .. 65540, 131073, 131074
    for stored, body, s in blocks:
        if len(s) >= 64:
            assert not stored and len(body) < len(s), len(s)


# ---- literal runs ---------------------------------------------------------------------------------------------------
def test_literal_runs_of_every_class_of_length_bytes():
    batches, _ = run_case("literal_runs")
    n_plain = len(g.LITERAL_LENGTHS)
    assert {0, 1, 2, 64, 65} <= {q[3] for q in sequences(batches[:n_plain])}
    assert {0, 1, 2, 64, 65} <= {q[3] for q in sequences(batches[n_plain:])}
    assert {16320, 16384} <= {q[0] for q in sequences(batches[:n_plain])}  # 64 and 65 length bytes, the step of the strided write


# ---- match lengths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", [("match_lengths_byte", 1), ("match_lengths_period3", 3), ("match_lengths_period64", 64)])
def test_matches_of_every_class_of_length_bytes_and_their_read_back(name, offset):
    batches, got = run_case(name)
    seqs = sequences(batches)
    assert {0, 1, 2, 64, 65} <= {q[4] for q in seqs}
    assert any(16319 <= q[2] < 16339 for q in seqs) and any(16339 <= q[2] < 16359 for q in seqs)  # either side of the 65th length byte
    long = [q for q in seqs if q[2] >= 270]
    assert long and all(q[1] % offset == 0 for q in long)  # copies of the pattern onto itself
    assert any(q[1] < q[2] for q in long)                  # overlapping
    read_back(got, g.case(name)[1])


def test_whole_blocks_of_one_byte_value_are_one_match_with_257_length_bytes():
    batches, got = run_case("whole_blocks")
    whole = [(stored, body, s) for blocks in batches for stored, body, s in blocks if s in (bytes(BLOCK), b"\xff" * BLOCK)]
    assert len(whole) == 4
    for stored, body, s in whole:
        assert not stored
        seqs = walk_sequences(body)
        assert [(q[1], q[2], q[4]) for q in seqs] == [(1, BLOCK - 6, 257), (0, 0, 0)] and seqs[1][0] == 5
    read_back(got, g.case("whole_blocks")[1])


# ---- end of block ---------------------------------------------------------------------------------------------------
def test_matches_at_the_limits_of_the_end_rules():
    batches, _ = run_case("block_ends")
    for i, n in enumerate(g.END_SIZES):
        (at12,), (at11,), (at13,), (z40,), (z100,) = batches[5 * i:5 * i + 5]
        assert not at12[0] and walk_block(at12[1])[1:] == ([(n - 12, 7)], 5) and len(at12[1]) == n - 2  # starts at n - 12, ends at n - 5
        assert at11[0]                                                                                  # no match may start at n - 11
        assert not at13[0] and walk_block(at13[1])[1:] == ([(n - 13, 7)], 6)
        for stored, body, s in (z40, z100):
            assert not stored
            size, matches, last = walk_block(body)
            assert size == n and last == 5 and sum(matches[-1]) == n - 5                                # cut at n - 5


# ---- far offsets and position 0 -------------------------------------------------------------------------------------
def test_far_offsets_and_the_candidate_at_position_0():
    batches, _ = run_case("far_offsets")
    for i, n in enumerate(g.FAR_SIZES):
        rzr, copy64, copy12 = [walk_sequences(blocks[0][1]) for blocks in batches[3 * i:3 * i + 3]]
        assert not any(blocks[0][0] for blocks in batches[3 * i:3 * i + 3])
        assert max(q[1] for q in rzr) > n - 200
        assert n - 64 in {q[1] for q in copy64}  # the candidate is position 0: nobody inserted it, the table starts as zeros
        assert n - 12 in {q[1] for q in copy12}  # no offset of a block of n bytes is larger
    assert 65524 in {q[1] for q in walk_sequences(batches[-1][0][1])}


# ---- the stored decision --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_len", [300, 2000, 60000])
def test_the_stored_decision_within_a_byte_or_two_of_equality(r_len):
    batches, _ = run_case(f"stored_decision_{r_len}")
    saved = [None if stored else len(s) - len(body) for blocks in batches for stored, body, s in blocks]
    assert len(saved) == len(g.STORED_K) + (len(g.STORED_K_RECENT) if r_len == 60000 else 0)
    assert None in saved and any(x is not None for x in saved)
    assert all(x is None or x > 0 for x in saved)  # no compressed block is as long as its input
    print(f"lz4-edges stored_decision_{r_len}: bytes saved per block of the sweep (None = stored): {saved}")
    assert any(a is None and b is not None and b <= 3 for a, b in zip(saved, saved[1:]))


# ---- binary content -------------------------------------------------------------------------------------------------
def test_binary_values_of_all_256_byte_values():
    batches, got = run_case("binary")
    assert sum(not stored for blocks in batches for stored, _, _ in blocks) >= 40
    assert not any(stored for blocks in batches[:6] for stored, _, _ in blocks)
    read_back(got, g.case("binary")[1])


def test_protobuf_state_is_what_the_encoders_envelope_writes():
    """lz4_blockgen.protobuf_state, which the binary case builds its states with, against surge_amd/encode.py's
    "protobuf_state" envelope on the device, for a few Counter aggregates."""
    import torch

    from oracle import oracle
    from surge_amd import schema as S
    from surge_amd import synth
    from surge_amd.encode import JsonTemplate, encode_states, key_table_utf8
    from surge_amd.replay import ReplayEngine

    keys = ["acct-0", "k" * 127, "k" * 128, "ключ-✓" * 40]
    so, ev = synth.csr_log(np.full(len(keys), 2), 41, synth.STRESS_MIX)
    ev["type"][:] = S.EVT_INC
    with ReplayEngine() as eng:
        eng.load_csr(so, ev)
        eng.fold()
        states = eng.snapshot()
        data, off = key_table_utf8(keys)
        d_out, d_off = encode_states(eng, JsonTemplate.counter(), torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda(), envelope="protobuf_state")
        out, offs = d_out.cpu().numpy().tobytes(), d_off.cpu().numpy()
    for a, key in enumerate(keys):
        assert int(states[a]["flags"]) == S.STATE_PRESENT
        payload = oracle.counter_state_json(key, int(states[a]["count"]), int(states[a]["version"]))
        assert out[offs[a]:offs[a + 1]] == g.protobuf_state(key.encode(), payload)


# ---- mixed frames ---------------------------------------------------------------------------------------------------
def test_frames_of_stored_and_compressed_blocks_at_every_size_modulo_8():
    batches, got = run_case("mixed_frames")
    rem = set()
    for blocks in batches:
        assert [stored for stored, _, _ in blocks] == [True, False, True, False, True, False]
        rem |= {len(body) % 8 for stored, body, _ in blocks if not stored}
    assert rem == set(range(8))
    read_back(got, g.case("mixed_frames")[1])


def test_both_size_classes_in_one_block_table_over_64_partitions():
    records, parts = g.case_many_partitions()
    inp, _ = g.section([v for _, v in records], [k for k, _ in records], parts, 64)
    out, got = publish("many_partitions", inp, n_part=64)
    assert sorted(out) == list(range(64))
    for p in range(64):
        (blocks,) = out[p]
        if p % 3 == 0:
            assert [stored for stored, _, _ in blocks] == [True, False, True, False, True] and len(blocks[-1][2]) > g.SMALL
        else:
            assert [(stored, len(s)) for stored, _, s in blocks] == [(True, 8)]
    read_back(got, inp)


# ---- read back by the project's decoders ----------------------------------------------------------------------------
def test_identical_events_are_read_back_by_the_device_lz4_decoder_as_by_the_host_decoder():
    """20 000 identical fixed-16 events of one aggregate, keyed <id>:<seq> as tests/test_frame_lz4_gpu.py's event16_input
    keys them: record after record repeats the one before it but for its offsetDelta and the digits of its key, the
    densest run of short-offset matches the compressor can hand the device decoder.  Driven as
    test_lz4_batches_are_read_back_by_the_device_lz4_decoder_as_by_the_host_decoder drives the two decoders."""
    from surge_amd import schema as S
    from surge_amd.ingest import READ_COMMITTED, DeviceDecoder, EventsTopicIngest
    from surge_amd.snapshot import DeviceFramer

    n = 20000
    ev = np.zeros(1, dtype=S.EVENT_DTYPE)
    ev["type"], ev["seq"], ev["raw"] = S.EVT_INC, 1, 3
    inp, _ = g.section([ev.tobytes()] * n, [b"acct-00007:%d" % j for j in range(n)])
    with DeviceFramer(1, compression="lz4") as f:
        got = device_frames(f, inp, 5)
        uncompressed = f.uncompressed_bytes
    (wire,) = got.values()
    frames = [walk_frame(frame) for _, frame in walk_batches(wire)]
    assert len(frames) == 2 and all(len(blocks) > 2 and not any(stored for stored, _ in blocks) for blocks in frames)
    seqs = [q for blocks in frames for _, body in blocks for q in walk_sequences(body)]
    assert sum(0 < q[1] < 64 for q in seqs) > n // 2  # most records are a match at the distance of one record
    print(f"lz4-edges identical_events: device {len(wire)} bytes of {uncompressed} uncompressed")
    with EventsTopicIngest(READ_COMMITTED) as ing:
        ing.feed(wire)
        host = ing.drain_fixed16()
        host_keys = ing.key_table().keys
    with EventsTopicIngest(READ_COMMITTED, frames=True, device_lz4=True) as ing, DeviceDecoder(None) as d:
        ing.feed(wire)
        d.push_from(ing)
        agg, evd, off, n_keys = d.result()
        dev = (agg.cpu().numpy(), evd.cpu().numpy().view(S.EVENT_DTYPE).reshape(-1), off.cpu().numpy())
        dev_keys = d.keys()
    assert n_keys == len(dev_keys) == 1 and dev_keys == host_keys
    assert host[0].shape[0] == n
    for h, d_ in zip(host, dev):
        assert h.shape == d_.shape and h.tobytes() == d_.tobytes()
