"""-m gpu: ``surge_replay_partition_hash_utf8_device`` — the shard map straight from UTF-8 ids in device memory
(``partition_hash_utf8_kernel``, csrc/shard_utf8.hip).  What every id must give is the host export's answer (the same routine,
``csrc/shard_utf8.h``, held against the UTF-16 route by tests/test_shard_utf8.py) and, for the corpus, ``shard_utf8_cases.expected``
itself.  The sizes around the kernel's LDS stage are taken from the kernel's own constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shard_utf8_cases as cases
import start_offsets_gen as sgen
from surge_amd import _native, kafka
from surge_amd.ingest import DeviceDecoder
from surge_amd.replay import ReplayEngine, ReplayError

pytestmark = pytest.mark.gpu

GUARD = -77
E_INVALID, E_CORRUPT = -1, -7
_SRC = open(os.path.join(_native.CSRC, "shard_utf8.hip")).read()
BLOCK = int(re.search(r"constexpr int kShBlock = (\d+);", _SRC).group(1))
STAGE = eval(re.search(r"constexpr int kShStageBytes = ([0-9* ]+);", _SRC).group(1))  # noqa: S307  (digits, blanks and '*' only)


@pytest.fixture(scope="module")
def eng():
    with ReplayEngine() as e:
        yield e


@pytest.fixture(scope="module")
def corpus():
    return [raw for _, raw in cases.corpus()]


def on_device(eng, data, off, n_partitions, cut, align=0):
    """One launch over ``data`` / ``off`` (numpy, host): ``(partitions, first_bad)``.  The arena starts ``align`` bytes behind a
    16-byte boundary and ends with its last id; the output lies between guard values, which must still stand."""
    n = off.shape[0] - 1
    whole = torch.zeros(16 + align + data.size, dtype=torch.uint8, device="cuda")
    base = (-whole.data_ptr()) % 16 + align
    d_data = whole[base:base + data.size]
    d_data.copy_(torch.from_numpy(data))
    assert data.size == 0 or d_data.data_ptr() % 16 == align % 16
    buf = torch.full((n + 64,), GUARD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    first_bad = -1
    try:
        eng.partition_hash_utf8_device(d_data, torch.from_numpy(off).cuda(), n_partitions, buf[32:32 + n], up_to_colon=cut)
    except ReplayError as e:  # some id is malformed: the others were hashed all the same
        assert e.status == E_CORRUPT and e.first_bad >= 0
        first_bad = e.first_bad
    got = buf.cpu().numpy()
    assert (got[:32] == GUARD).all() and (got[32 + n:] == GUARD).all()
    return got[32:32 + n], first_bad


def on_host(data, off, n_partitions, cut):
    out = kafka.partition_for_utf8(data, off, n_partitions, up_to_colon=cut)
    bad = np.nonzero(out == -1)[0]
    return out, (int(bad[0]) if bad.size else -1)


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("n_partitions", cases.N_PARTITIONS)
def test_the_corpus_in_one_launch(eng, corpus, n_partitions, cut):
    data, off = cases.table(corpus)
    want, want_first = on_host(data, off, n_partitions, cut)
    assert (want == cases.expected(corpus, n_partitions, cut)).all() and want_first >= 0
    got, first_bad = on_device(eng, data, off, n_partitions, cut)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert first_bad == want_first
    if n_partitions == 64:  # the status, as the wrapper raises it
        out = torch.full((len(corpus),), GUARD, dtype=torch.int32, device="cuda")
        with pytest.raises(ReplayError) as ei:
            eng.partition_hash_utf8_device(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda(), n_partitions, out, up_to_colon=cut)
        assert ei.value.status == E_CORRUPT and ei.value.first_bad == want_first
        assert f"{int((want == -1).sum())} of {len(corpus)} ids" in str(ei.value)
        assert (out.cpu().numpy() == want).all()  # every other id was hashed all the same


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_counts_around_a_workgroup(eng, corpus, n):
    ids = [corpus[(7 * i + n) % len(corpus)] for i in range(n)]
    data, off = cases.table(ids)
    want, want_first = on_host(data, off, 7, True)
    got, first_bad = on_device(eng, data, off, 7, True)
    assert (got == want).all() and first_bad == want_first


def test_every_alignment_of_the_arena(eng, corpus):
    data, off = cases.table(corpus)
    want, want_first = on_host(data, off, 64, False)
    for align in range(16):
        got, first_bad = on_device(eng, data, off, 64, False, align=align)
        assert (got == want).all() and first_bad == want_first, align


def filled(corpus, total, n=BLOCK):
    """``n`` ids of ``total`` bytes in all: corpus ids, the last one padded with a well-formed tail to make the sum."""
    ids = [corpus[(5 * i + 3) % len(corpus)][:40] for i in range(n - 1)]
    rest = total - sum(len(k) for k in ids)
    assert rest >= 0
    tail = ("zé€\U0001f600" * (rest // 10 + 1)).encode()[:rest]
    return ids + [tail]  # (where the cut splits a character the id is malformed: the host export says which it is)


@pytest.mark.parametrize("align", [0, 15])
def test_spans_just_under_and_just_over_the_stage(eng, corpus, align):
    """A workgroup's span is staged when it fits the stage counted from the 16-byte boundary in front of it: the last size
    that fits, the first that does not, and their neighbours — with another workgroup behind it that takes the other path."""
    fits = STAGE - align
    for total in (fits - 1, fits, fits + 1, fits + 17):
        ids = filled(corpus, total) + corpus[:BLOCK + 1]
        data, off = cases.table(ids)
        assert off[BLOCK] == total
        want, want_first = on_host(data, off, 7, True)
        got, first_bad = on_device(eng, data, off, 7, True, align=align)
        assert (got == want).all() and first_bad == want_first, total


@pytest.mark.parametrize("well_formed", [True, False])
def test_a_40_kb_id_between_short_ones(eng, corpus, well_formed):
    assert 40 * 1024 > STAGE
    body = ("abé€\U0001f600" * ((40 * 1024 - 1) // 11)).encode()  # 11 bytes a round: characters of every length, whole
    long_id = body + b"x" * (40 * 1024 - 1 - len(body)) + (b"!" if well_formed else b"\xc3")
    assert len(long_id) == 40 * 1024
    ids = corpus[:300] + [long_id] + corpus[:300]  # the long id's workgroup reads global memory, the ones around it stage
    data, off = cases.table(ids)
    want, want_first = on_host(data, off, 2**31 - 1, False)
    assert (want[300] >= 0) == well_formed
    got, first_bad = on_device(eng, data, off, 2**31 - 1, False, align=5)
    assert (got == want).all() and first_bad == want_first


def test_no_id_and_refused_arguments_leave_the_output_alone(eng):
    lib = _native.load()
    data, off = cases.table([b"abc", b"de"])
    d_data, d_off = torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda()
    out = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
    eng.partition_hash_utf8_device(d_data, d_off[:1], 4, out[:0])  # n = 0
    fb = ctypes.c_int64(GUARD)
    assert lib.surge_replay_partition_hash_utf8_device(eng._h, None, None, 0, 4, 0, None, ctypes.byref(fb)) == 0 and fb.value == -1
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for args in ((p(d_data), p(d_off), 2, 0, 1, p(out)), (p(d_data), p(d_off), -1, 4, 1, p(out)), (None, p(d_off), 2, 4, 1, p(out)),
                 (p(d_data), None, 2, 4, 1, p(out)), (p(d_data), p(d_off), 2, 4, 1, None)):
        fb = ctypes.c_int64(GUARD)
        assert lib.surge_replay_partition_hash_utf8_device(eng._h, *args, ctypes.byref(fb)) == E_INVALID and fb.value == GUARD
    assert lib.surge_replay_partition_hash_utf8_device(None, p(d_data), p(d_off), 2, 4, 1, p(out), None) == E_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    with pytest.raises(ValueError):
        eng.partition_hash_utf8_device(d_data, d_off, 4, out[:1])  # an output shorter than the ids never reaches the library
    eng.partition_hash_utf8_device(d_data, d_off, 4, out[1:3])
    assert out.cpu().numpy().tolist() == [GUARD] + kafka.partition_for_keys(["abc", "de"], 4).tolist() + [GUARD]


def test_the_rows_of_a_decoder_s_key_table_as_it_grows(eng):
    """The table the kernel is for: ``DeviceDecoder.device_key_table()``.  Rows [0, n0) first; then a push interns new ids — the
    arena grows and may move — and only rows [n0, n1) are hashed, through the offsets' slice from n0 on."""
    first = ["agg-%d" % i for i in range(300)] + ["é-ключ", "smile-\U0001f600", "x" * 200, "a"]
    later = ["born-later-%d-€" % i for i in range(3000)] + ["\U0010ffff", "z"]

    def deliver(d, ids, at):
        d.push_records([k.encode() + b":%d" % i for i, k in enumerate(ids)], [sgen.fixed16(1, i + 1, 1) for i in range(len(ids))], list(range(at, at + len(ids))))
        d.clear()

    with DeviceDecoder(None) as d:
        deliver(d, first, 0)
        d_keys, d_key_off = d.device_key_table()
        n0 = int(d_key_off.numel()) - 1
        assert n0 == len(first)
        part = torch.full((len(first) + len(later),), GUARD, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.partition_hash_utf8_device(d_keys, d_key_off, 64, part[:n0], up_to_colon=True)
        deliver(d, later + first[:5], n0)  # (ids the table holds already intern nothing)
        d_keys, d_key_off = d.device_key_table()
        n1 = int(d_key_off.numel()) - 1
        assert n1 == len(first) + len(later)
        eng.partition_hash_utf8_device(d_keys, d_key_off[n0:], 64, part[n0:n1], up_to_colon=True)
        keys = d.keys()
        assert keys == first + later
        data, off = cases.table([k.encode() for k in keys])
        want, _ = on_host(data, off, 64, True)
        assert (part.cpu().numpy() == want).all() and (want == kafka.partition_for_keys(keys, 64, up_to_colon=True)).all()
