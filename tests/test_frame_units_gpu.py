"""-m gpu: the device framer across its units (surge_amd/csrc/device_framer.hip: the steps of a publish and the commit rule;
frame_internal.h: the one scan path and its scratch rule, the owned buffers; frame_lz4.hip: the LZ4 step) where
tests/test_frame_gpu.py, test_frame_edges_gpu.py and test_frame_lz4_gpu.py do not go: ONE framer whose buffers and scan scratch
grow in one publish and are larger than needed in the next, empty publishes between real ones, every refusal of the size
kernel followed by a publish that has to be right, and a codec switch at a larger size than the buffers have seen.

Uncompressed output is held to the host writer's bytes, partition by partition; LZ4 output to check_against_uncompressed
(tests/lz4_blockgen.py); both to the host writer's next offsets and uncompressed size after every publish."""
import ctypes

import numpy as np
import pytest

from lz4_blockgen import check_against_uncompressed, device_frames, pa_lz4
from test_frame_gpu import make_input

pytestmark = pytest.mark.gpu

NEEDS_LZ4 = pytest.mark.skipif(pa_lz4() is None, reason="no pyarrow with the LZ4 frame codec: nothing to hold LZ4 output to")
CODECS = ["none", pytest.param("lz4", marks=NEEDS_LZ4)]
TS = 1_700_000_000_000
E_RANGE = -6


def make_records(rng, codec, n, n_part, p_skip=0.0):
    """Counter state text where the output is compressed (blocks that shrink), random text otherwise."""
    if codec == "lz4":
        from test_frame_lz4_gpu import counter_input

        return counter_input(rng, n, n_part, p_skip)
    return make_input(rng, n, n_part, 12, 90, p_skip=p_skip)


def host_publish(w, inp, ts):
    """lz4_blockgen.host_frames and the next offsets of every partition with ONE flush: RecordBatchWriter.partition_bytes
    flushes every partition each time it is asked for one, which at 65 536 partitions is 20 s per publish."""
    w.reset()
    w.append(*inp, ts)
    w._check(w._lib.surge_snapshot_writer_flush(w._h))
    frames, nxt = {}, []
    data, ln, nrec, next_offset = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    for p in range(w.n_partitions):
        w._check(w._lib.surge_snapshot_writer_partition(w._h, p, ctypes.byref(data), ctypes.byref(ln), ctypes.byref(nrec), ctypes.byref(next_offset)))
        if nrec.value:
            frames[p] = ctypes.string_at(data, ln.value)
        nxt.append(next_offset.value)
    return frames, nxt


def publish_and_check(w, f, inp, ts):
    """One publish through both writers; the device's output, counts and offsets against the host writer's."""
    exp, exp_next = host_publish(w, inp, ts)
    got = device_frames(f, inp, ts)
    if f.compression == "none":
        assert sorted(got) == sorted(exp)
        for p in exp:
            assert got[p] == exp[p], (p, len(got[p]), len(exp[p]))
    else:
        check_against_uncompressed(got, exp)
    assert f.records == int(np.count_nonzero(inp[0]))
    assert f.uncompressed_bytes == sum(len(v) for v in exp.values())
    assert list(f.next_offsets()) == exp_next
    return exp


def raw_frame(f, inp, ts):
    """surge_device_framer_frame itself, arrays of `inp` that are None passed as NULL: (rc, spans, records, batches)."""
    import torch

    dev = torch.device("cuda:0")
    t = [None if a is None else torch.from_numpy(a).to(dev) for a in inp]
    torch.cuda.synchronize(dev)
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    data, offs = ctypes.c_void_p(), ctypes.c_void_p()
    nrec, nbat = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = f._lib.surge_device_framer_frame(f._h, len(inp[0]), *[ptr(x) for x in t], ts, ctypes.byref(data), ctypes.byref(offs), ctypes.byref(nrec),
                                          ctypes.byref(nbat))
    spans = np.ctypeslib.as_array(ctypes.cast(offs, ctypes.POINTER(ctypes.c_int64)), shape=(f.n_partitions + 1,)).copy()
    return rc, spans, nrec.value, nbat.value


@pytest.mark.parametrize("codec", CODECS)
def test_scan_scratch_and_buffers_grow_and_shrink_in_use_on_one_framer(codec):
    """65 536 partitions and 3 records: the two scans over the partitions are far longer than everything sized by the records,
    so the scratch that select, sort and the record scans left is too small for them (scan_in_place waits and grows); then
    20 000 records over those partitions (the sort's scratch and every per-record buffer grow), then 3 again (everything is
    larger than needed, and what the large publish left in the buffers must not show)."""
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(65536)
    n_part = 65536
    with RecordBatchWriter(n_part) as w, DeviceFramer(n_part, compression=codec) as f:
        for publish, n in enumerate([3, 20000, 3]):
            exp = publish_and_check(w, f, make_records(rng, codec, n, n_part), TS + publish)
            assert sum(map(len, exp.values())) > 0


@pytest.mark.parametrize("codec", CODECS)
def test_empty_publishes_between_real_ones(codec):
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(2)
    n_part = 5
    with RecordBatchWriter(n_part) as w, DeviceFramer(n_part, compression=codec) as f:
        publish_and_check(w, f, make_records(rng, codec, 700, n_part, p_skip=0.3), TS)
        before = list(f.next_offsets())
        assert sum(before) > 0
        for ts, empty in ((TS + 1, make_input(rng, 0, n_part, 12, 90)), (TS + 2, make_input(rng, 300, n_part, 12, 90, p_skip=1.0))):
            assert not np.count_nonzero(empty[0])
            assert device_frames(f, empty, ts) == {}
            assert f.records == 0 and f.batches == 0 and f.uncompressed_bytes == 0
            assert list(f.next_offsets()) == before
            rc, spans, n_rec, n_bat = raw_frame(f, empty, ts)
            assert rc == 0 and not spans.any() and (n_rec, n_bat) == (0, 0)
            assert list(f.next_offsets()) == before
        publish_and_check(w, f, make_records(rng, codec, 700, n_part, p_skip=0.3), TS + 3)


def negative_key_span(inp):
    kind, part, keys, key_off, vals, val_off = inp
    a = int(np.nonzero(kind)[0][3])
    key_off = key_off.copy()
    key_off[a + 1] = key_off[a] - 1  # (read by the size kernel alone, which refuses the publish: no key is fetched through it)
    return kind, part, keys, key_off, vals, val_off


def value_without_offsets(inp):
    assert (inp[0] == 1).any()
    return inp[:4] + (inp[4], None)


def keys_without_bytes(inp):
    assert (np.diff(inp[3])[inp[0] != 0] > 0).any()
    return inp[:2] + (None,) + inp[3:]


@pytest.mark.parametrize("codec", CODECS)
def test_every_refusal_of_the_size_kernel_leaves_the_framer_usable(codec):
    """A negative key span, a value aggregate without value offsets, key bytes without a key table: refused with nothing
    advanced and no partition given a span, and the next publish is the host writer's.  (The two refusals the other tests
    make — a partition out of range in both codecs, an unknown kind uncompressed — are not repeated here; none of these
    three is made elsewhere.)"""
    import torch

    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(3)
    n_part = 4
    with RecordBatchWriter(n_part) as w, DeviceFramer(n_part, compression=codec) as f:
        publish_and_check(w, f, make_records(rng, codec, 900, n_part, p_skip=0.2), TS)
        for i, spoil in enumerate((negative_key_span, value_without_offsets, keys_without_bytes)):
            good = make_records(rng, codec, 900, n_part, p_skip=0.2)
            bad = spoil(good)
            before = list(f.next_offsets())
            t =[None if a is None else torch.from_numpy(a).to("cuda:0") for a in bad]
            with pytest.raises(RuntimeError):
                f.frame(*t, timestamp_ms=TS + 10 * i)
            assert list(f.next_offsets()) == before
            rc, spans, n_rec, n_bat = raw_frame(f, bad, TS + 10 * i)
            assert rc == E_RANGE and not spans.any() and (n_rec, n_bat) == (0, 0)
            assert f._lib.surge_device_framer_uncompressed_bytes(f._h) == 0
            assert list(f.next_offsets()) == before
            publish_and_check(w, f, good, TS + 10 * i + 1)


@NEEDS_LZ4
def test_buffers_survive_a_codec_switch_at_a_larger_size():
    """A small uncompressed publish, then an LZ4 and an uncompressed one of some 300 000 bytes of batches: the buffers of the
    uncompressed framing are regrown by the LZ4 publish, those of the LZ4 step sized by it, and all of them used again at
    that size by the codec they were not grown under."""
    from surge_amd.snapshot import DeviceFramer, RecordBatchWriter

    rng = np.random.default_rng(4)
    n_part = 3
    with RecordBatchWriter(n_part) as w, DeviceFramer(n_part) as f:
        for publish, (codec, n) in enumerate([("none", 40), ("lz4", 5000), ("none", 5000)]):
            f.set_compression(codec)
            exp = publish_and_check(w, f, make_records(rng, "lz4", n, n_part), TS + publish)
            assert n == 40 or sum(map(len, exp.values())) >= 300_000
