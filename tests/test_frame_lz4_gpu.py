"""-m gpu: the LZ4 mode of the device framer (surge_device_framer_set_compression, frame_lz4_block_kernel in
surge_amd/csrc/frame_lz4.hip).  Its output is not the host compressor's byte for byte, so it is held to what it has
to be instead: the batches of the host writer's UNCOMPRESSED output for the same input (cuts, offsets, header fields),
each records section one LZ4 frame that liblz4 (as Apache Arrow bundles it) decompresses to the host writer's records,
whose compressed blocks obey the block format's end rules, about as small as the host compressor's, and read by the
project's own host and device decoders."""
import struct
import uuid

import numpy as np
import pytest

from lz4_blockgen import BLOCK, check_against_uncompressed, walk_batches, walk_frame

pytestmark = pytest.mark.gpu

pa = pytest.importorskip("pyarrow")  # liblz4 as Apache Arrow bundles it: the pin every test here rests on
if not pa.Codec.is_available("lz4"):
    pytest.skip("this pyarrow build has no LZ4 frame codec", allow_module_level=True)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def random_input(rng, n, n_part, key_max, val_max, p_skip=0.5, p_tomb=0.1, key_min=0):
    """tests/test_frame_gpu.py's shapes: random printable keys and values (nothing for LZ4 to find: stored blocks)."""
    p_tomb = min(p_tomb, 1 - p_skip)
    kind = rng.choice([0, 1, 2], size=n, p=[p_skip, max(0.0, 1 - p_skip - p_tomb), p_tomb]).astype(np.uint8)
    part = rng.integers(0, n_part, size=n).astype(np.int32)
    klen = rng.integers(key_min, key_max + 1, size=n)
    vlen = np.where(kind == 1, rng.integers(0, val_max + 1, size=n), 0)
    key_off = np.zeros(n + 1, np.int64); np.cumsum(klen, out=key_off[1:])
    val_off = np.zeros(n + 1, np.int64); np.cumsum(vlen, out=val_off[1:])
    keys = rng.integers(32, 127, size=max(int(key_off[-1]), 1)).astype(np.uint8)
    vals = rng.integers(32, 127, size=max(int(val_off[-1]), 1)).astype(np.uint8)
    return kind, part, keys, key_off, vals, val_off


def text_input(rng, keys, values, n_part, p_skip=0.0, p_tomb=0.02):
    """Given keys and values (bytes each); the values of skipped aggregates and tombstones are left out, as the filtered
    encoder leaves them out."""
    n = len(keys)
    p_tomb = min(p_tomb, 1 - p_skip)
    kind = rng.choice([0, 1, 2], size=n, p=[p_skip, max(0.0, 1 - p_skip - p_tomb), p_tomb]).astype(np.uint8)
    part = rng.integers(0, n_part, size=n).astype(np.int32)
    values = [v if k == 1 else b"" for v, k in zip(values, kind)]
    key_off = np.zeros(n + 1, np.int64); np.cumsum([len(k) for k in keys], out=key_off[1:])
    val_off = np.zeros(n + 1, np.int64); np.cumsum([len(v) for v in values], out=val_off[1:])
    kb = np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy()
    vb = np.frombuffer(b"".join(values) or b"\0", np.uint8).copy()
    return kind, part, kb, key_off, vb, val_off


def counter_input(rng, n, n_part, p_skip=0.0):
    keys = [b"agg-%07d" % i for i in rng.permutation(10 * n)[:n]]
    values = [b'{"aggregateId":"%s","count":%d,"version":%d}' % (k, rng.integers(-500, 500), rng.integers(1, 3000)) for k in keys]
    return text_input(rng, keys, values, n_part, p_skip)


def bank_input(rng, n, n_part, p_skip=0.0):
    ids = [str(uuid.UUID(bytes=rng.bytes(16), version=4)).encode() for _ in range(n)]
    values = [b'{"accountNumber":"%s","accountOwner":"owner-%d","securityCode":"%04d","balance":%s}'
              % (k, rng.integers(0, 5000), rng.integers(0, 10000), repr(round(float(rng.random() * 1e5), 2)).encode()) for k in ids]
    return text_input(rng, ids, values, n_part, p_skip)


def event16_input(rng, n, n_part, n_ids=300):
    """Records the device decoder accepts without a template: key <id>:<seq>, value one 16-byte surge_event16."""
    from surge_amd import schema as S

    ev = np.zeros(n, dtype=S.EVENT_DTYPE)
    ev["type"] = rng.choice([S.EVT_INC, S.EVT_DEC, S.EVT_NOOP], size=n)
    ev["seq"] = np.arange(1, n + 1)
    ev["raw"] = rng.integers(1, 9, size=n).astype(np.uint64)
    keys = [b"acct-%05d:%d" % (rng.integers(0, n_ids), j) for j in range(n)]
    values = [ev[j:j + 1].tobytes() for j in range(n)]
    return text_input(rng, keys, values, n_part, p_skip=0.0, p_tomb=0.0)


# ---- the two writers ------------------------------------------------------------------------------------------------
def host_frames(writer, inp, ts):
    kind, part, keys, key_off, vals, val_off = inp
    writer.reset()
    writer.append(kind, part, keys, key_off, vals, val_off, ts)
    out = {}
    for p in range(writer.n_partitions):
        data, nrec, _ = writer.partition_bytes(p)
        if nrec:
            out[p] = data
    return out


def host_next_offsets(writer):
    return [writer.partition_bytes(p)[2] for p in range(writer.n_partitions)]


def device_frames(framer, inp, ts):
    import torch

    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a).to(dev) for a in inp]
    torch.cuda.synchronize(dev)
    return {p: bytes(v) for p, v in framer.frame(*t, timestamp_ms=ts).items()}


# ---- 1, 2: same batches, same records, block rules ------------------------------------------------------------------
RANDOM_SHAPES = [
    (0, 3, 0, 0, 8, 40), (1, 1, 0, 0, 8, 40), (500, 4, 0, 0, 12, 120), (5000, 7, 1, 0, 5, 30), (5000, 3, 3, 0, 5, 30),
    (6000, 2, 70, 0, 20, 60), (6000, 5, 0, 300, 10, 90), (6000, 1, 0, 5000, 3, 50), (40000, 2, 0, 0, 13, 100),
    (30000, 1, 0, 0, 2, 61), (30000, 1, 20000, 1 << 30, 1, 3), (200000, 64, 0, 0, 13, 100),
]


@pytest.mark.parametrize("n,n_part,max_records,max_bytes,key_max,val_max", RANDOM_SHAPES)
def test_lz4_batches_of_random_text_are_the_host_writers_batches(n, n_part, max_records, max_bytes, key_max, val_max):
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(n + 31 * n_part + max_records + max_bytes)
    with RecordBatchWriter(n_part, max_records, max_bytes) as w, DeviceFramer(n_part, 0, max_records, max_bytes, compression="lz4") as f:
        for publish in range(3):
            inp = random_input(rng, n, n_part, key_max, val_max, p_skip=[0.5, 0.9, 0.0][publish])
            exp = host_frames(w, inp, 1_700_000_000_000 + publish)
            got = device_frames(f, inp, 1_700_000_000_000 + publish)
            check_against_uncompressed(got, exp)
            assert f.records == int(np.count_nonzero(inp[0]))
            assert f.uncompressed_bytes == sum(len(v) for v in exp.values())
            assert list(f.next_offsets()) == host_next_offsets(w)


@pytest.mark.parametrize("make,n,n_part,max_records,max_bytes", [
    (counter_input, 30000, 3, 0, 0),          # 10 000 records = about 0.7 MB per batch: a dozen blocks each
    (counter_input, 20000, 1, 1 << 20, 1 << 30),  # one batch of everything
    (counter_input, 3000, 64, 0, 0),          # many partitions, small batches: the small size class
    (bank_input, 12000, 2, 0, 0),
    (bank_input, 6000, 1, 1 << 20, 1 << 30),
])
def test_lz4_batches_of_state_text_are_the_host_writers_batches_and_about_as_small(make, n, n_part, max_records, max_bytes):
    """Device bytes <= 1.05 x the host compressor's (RecordBatchWriter(compression="lz4")) on compressible records.
    Where the cap comes from: a lane-for-lane CPU simulation of the wave's match finder stayed within 1.033 x of the host
    compressor with the smallest hash table considered (12 bits); a compressor that stores everything, or loses half its
    matches, is far outside."""
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(n + n_part)
    with RecordBatchWriter(n_part, max_records, max_bytes) as w, RecordBatchWriter(n_part, max_records, max_bytes, compression="lz4") as wz, \
            DeviceFramer(n_part, 0, max_records, max_bytes, compression="lz4") as f:
        dev_total = host_total = 0
        multi_block = False
        for publish in range(3):
            inp = make(rng, n, n_part, p_skip=[0.0, 0.8, 0.3][publish])
            exp = host_frames(w, inp, 1_700_000_000_000 + publish)
            got = device_frames(f, inp, 1_700_000_000_000 + publish)
            n_comp, _ = check_against_uncompressed(got, exp)
            assert n_comp > 0
            multi_block |= any(len(r) > 2 * BLOCK for data in exp.values() for _, r in walk_batches(data))
            assert list(f.next_offsets()) == host_next_offsets(w)
            dev_total += sum(len(v) for v in got.values())
            host_total += sum(len(v) for v in host_frames(wz, inp, 1_700_000_000_000 + publish).values())
        assert multi_block or n_part == 64
        print(f"device lz4 {dev_total} bytes, host lz4 {host_total} bytes, ratio {dev_total / host_total:.4f}")
        assert dev_total <= 1.05 * host_total, (dev_total, host_total)


# ---- 4: the project's readers ---------------------------------------------------------------------------------------
def test_lz4_batches_are_read_back_by_the_host_decoder():
    from surge_amd.ingest import EventsTopicIngest
    from surge_amd.snapshot import DeviceFramer

    for make, n in ((lambda r, n, p: random_input(r, n, p, 9, 70, p_skip=0.3, key_min=1), 3000), (lambda r, n, p: counter_input(r, n, p, 0.1), 25000)):
        rng = np.random.default_rng(3)
        n_part = 3
        kind, part, keys, key_off, vals, val_off = inp = make(rng, n, n_part)
        with DeviceFramer(n_part, compression="lz4") as f:
            got = device_frames(f, inp, 123)
        seen = 0
        for p, data in got.items():
            with EventsTopicIngest() as g:  # CRC, framing, LZ4 and varints are checked by the reader
                g.feed(data)
                recs = g.drain_records()
            idx = [a for a in range(n) if kind[a] and part[a] == p]
            assert len(recs) == len(idx)
            for (offset, _, k, v), a in zip(recs, idx):
                assert k == keys[key_off[a]:key_off[a + 1]].tobytes()
                assert v == (vals[val_off[a]:val_off[a + 1]].tobytes() if kind[a] == 1 else None)
            assert [r[0] for r in recs] == list(range(len(idx)))
            seen += len(recs)
        assert seen == int(np.count_nonzero(kind))


def test_lz4_batches_are_read_back_by_the_device_lz4_decoder_as_by_the_host_decoder():
    """Driven the way tests/test_ingest_gpu.py's both_decoders(device_lz4=True) drives the two decoders."""
    from surge_amd import schema as S
    from surge_amd.ingest import READ_COMMITTED, DeviceDecoder, EventsTopicIngest
    from surge_amd.snapshot import DeviceFramer

    rng = np.random.default_rng(17)
    n_part = 2
    inp = event16_input(rng, 40000, n_part)  # about 0.7 MB of records per partition, batches of 10 000: multi-block frames
    with DeviceFramer(n_part, compression="lz4") as f:
        got = device_frames(f, inp, 5)
    assert sorted(got) == [0, 1]
    for p, wire in got.items():
        assert any(len(walk_frame(frame)) > 2 for _, frame in walk_batches(wire))
        with EventsTopicIngest(READ_COMMITTED) as g:
            g.feed(wire)
            host = g.drain_fixed16()
            host_keys = g.key_table().keys
        with EventsTopicIngest(READ_COMMITTED, frames=True, device_lz4=True) as g, DeviceDecoder(None) as d:
            g.feed(wire)
            d.push_from(g)
            agg, ev, off, n_keys = d.result()
            dev = (agg.cpu().numpy(), ev.cpu().numpy().view(S.EVENT_DTYPE).reshape(-1), off.cpu().numpy())
            dev_keys = d.keys()
        assert n_keys == len(dev_keys) and dev_keys == host_keys
        assert host[0].shape[0] == int(np.count_nonzero(inp[1] == p))
        for h, g_ in zip(host, dev):
            assert h.shape == g_.shape and h.tobytes() == g_.tobytes()


# ---- 5: switching and errors ----------------------------------------------------------------------------------------
def test_switching_codecs_keeps_the_logs_and_errors_advance_nothing():
    from surge_amd import _native
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(9)
    n_part = 3
    with RecordBatchWriter(n_part) as w, DeviceFramer(n_part) as f:
        for publish, codec in enumerate(["none", "lz4", "none"]):
            f.set_compression(codec)
            inp = counter_input(rng, 4000, n_part, p_skip=0.2)
            exp = host_frames(w, inp, 1000 + publish)
            got = device_frames(f, inp, 1000 + publish)
            if codec == "none":
                assert got == exp  # today's guarantee: the host writer's bytes
            else:
                check_against_uncompressed(got, exp)
                assert sum(map(len, got.values())) < sum(map(len, exp.values()))
            assert list(f.next_offsets()) == host_next_offsets(w)
        # codec 1 (gzip) is refused and the codec stays what it was
        f.set_compression("lz4")
        assert _native.load().surge_device_framer_set_compression(f._h, 1) == -1
        with pytest.raises(ValueError):
            f.set_compression("gzip")
        inp = counter_input(rng, 4000, n_part, p_skip=0.2)
        exp = host_frames(w, inp, 2000)
        check_against_uncompressed(device_frames(f, inp, 2000), exp)
        # a partition out of range in LZ4 mode: an error, nothing advanced
        before = f.next_offsets().copy()
        kind, part = inp[0], inp[1].copy()
        part[np.nonzero(kind)[0][7]] = n_part
        with pytest.raises(RuntimeError):
            device_frames(f, (kind, part) + inp[2:], 2001)
        assert list(f.next_offsets()) == list(before)
        inp = counter_input(rng, 4000, n_part, p_skip=0.2)
        exp = host_frames(w, inp, 2002)
        check_against_uncompressed(device_frames(f, inp, 2002), exp)
        assert list(f.next_offsets()) == host_next_offsets(w)


# ---- 6: the publisher -----------------------------------------------------------------------------------------------
def test_publisher_with_device_compression_publishes_what_the_host_compressor_route_publishes():
    from surge_amd import schema as S
    from surge_amd.ingest import EventsTopicIngest
    from surge_amd.replay import ReplayEngine
    from surge_amd.snapshot import BulkSnapshotPublisher, StateRecord, compact

    n, n_part = 6000, 2  # about 3000 records of 60 bytes per partition: frames of several blocks
    keys = [f"agg-{i:05d}" for i in range(n)]

    def run(device_compression):
        rng = np.random.default_rng(5)
        lens = rng.integers(0, 9, size=n)
        so = np.zeros(n + 1, np.int64); np.cumsum(lens, out=so[1:])
        ne = int(so[-1])
        ev = S.make_events(rng.choice([S.EVT_INC, S.EVT_DEC, S.EVT_NOOP, S.EVT_DELETE], size=ne, p=[.6, .2, .1, .1]),
                           rng.integers(1, 1000, size=ne), rng.integers(-50, 50, size=ne))
        records, codecs = [], set()

        def ingest(batches):
            for p in sorted(batches):
                data = bytes(batches[p])
                codecs.update(struct.unpack(">h", h[21:23])[0] for h, _ in walk_batches(data))
                with EventsTopicIngest() as g:
                    g.feed(data)
                    records.extend((p, off, k, v) for off, _, k, v in g.drain_records())

        with ReplayEngine() as eng:
            eng.load_csr(so, ev)
            eng.fold()
            pub = BulkSnapshotPublisher(eng, keys, n_part, compression="lz4", device_compression=device_compression)
            try:
                assert (pub.framer is not None) == device_compression
                ingest(pub.publish())
                first = dict(pub.timings)
                touched = rng.choice(n, size=400, replace=False)
                be = S.make_events([S.EVT_DELETE if j % 5 == 0 else S.EVT_INC for j in range(400)], rng.integers(1000, 2000, size=400),
                                   rng.integers(1, 9, size=400))
                eng.append_events(touched.astype(np.int64), be)
                ingest(pub.publish())
                touched = rng.choice(n, size=300, replace=False)
                eng.append_events(touched.astype(np.int64), S.make_events([S.EVT_INC] * 300, rng.integers(2000, 3000, size=300), rng.integers(1, 9, size=300)))
                ingest(pub.publish_async().result())
            finally:
                pub.close()
        assert codecs == {3}
        return records, first

    dev, t_dev = run(True)
    host, _ = run(False)
    assert len(dev) > 4000 and any(v is None for _, _, _, v in dev)
    assert dev == host  # the same records per partition, in the same order, at the same offsets
    as_records = lambda rs: [StateRecord("state", p, k.decode(), v) for p, _, k, v in rs]  # noqa: E731
    assert compact(as_records(dev)) == compact(as_records(host))
    assert t_dev["device_framing_copy_crc_ms"] > 0 and 0 < t_dev["record_batch_bytes"] < t_dev["uncompressed_bytes"]
