"""``store_recovery._sniff_value_kind`` — CPU-only: it decides which device decoder a whole topic gets, from the first
deliverable record of the framed sections.  The topics are written by the independent test-side writer
(``tests/native/wire_writer.c``) and framed by the product's host framer (``EventsTopicIngest(frames=True)``), so the walk
sees real sections at a real arena address."""
import ctypes

import numpy as np
import pytest

import topic_gen
from surge_amd.ingest import EventsTopicIngest
from surge_amd.store_recovery import _sniff_value_kind

FIXED = bytes(range(1, 17))  # a 16-byte fixed event (its first byte is not ``{``)
JSON = b'{"type":"inc","aggregateId":"a","incrementBy":1,"sequenceNumber":1}'
BRACE16 = b'{"a":1,"b":234}\n'  # JSON text that happens to be 16 bytes long
FLUSH = (b"", b"")  # the producer's flush record
assert len(FIXED) == 16 and len(BRACE16) == 16


def batch(records, base_offset=0, lz4=False):
    L = topic_gen.wire_lib()
    keys, vals = b"".join(k for k, _ in records), b"".join(v for _, v in records)
    ko = np.cumsum([0] + [len(k) for k, _ in records]).astype(np.int64)
    vo = np.cumsum([0] + [len(v) for _, v in records]).astype(np.int64)
    k, v = np.frombuffer(keys + b"\0", np.uint8), np.frombuffer(vals + b"\0", np.uint8)
    out = ctypes.create_string_buffer(4096 + 3 * (len(keys) + len(vals)) + 64 * len(records))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    n = L.surge_test_wire_batch(out, base_offset, len(records), None, p(k), p(ko), p(v), p(vo), None, topic_gen.WIRE_LZ4 if lz4 else 0, -1, 0, -1, 0)
    assert n > 0
    return out.raw[:n]


def sniff(*batches, device_lz4=False):
    """-> (what the sniffer says, the sections it was given)"""
    with EventsTopicIngest(frames=True, device_lz4=device_lz4) as g:
        g.feed(b"".join(batches))
        sections, arena = g.drain_sections()
        return _sniff_value_kind(sections, arena), sections


@pytest.mark.parametrize("value, kind", [(FIXED, "fixed16"), (JSON, "json"), (BRACE16, "json")])
@pytest.mark.parametrize("flush_in_front", [False, True])
def test_the_first_deliverable_value_names_the_kind(value, kind, flush_in_front):
    records = [FLUSH] * flush_in_front + [(b"a:1", value), (b"b:1", FIXED), (b"c:1", JSON)][: 3 - flush_in_front]
    got, sections = sniff(batch(records))
    assert sections.shape[0] == 1 and int(sections[0]["n_records"]) == len(records)
    assert got == kind


def test_a_batch_of_one_flush_record_is_passed_over_for_the_batch_behind_it():
    got, sections = sniff(batch([FLUSH]), batch([(b"a:1", FIXED), (b"b:1", FIXED)], base_offset=1))
    assert got == "fixed16" and int(sections["n_records"].sum()) == 3  # (the flush record is in what was walked)
    got, _ = sniff(batch([FLUSH]), batch([(b"a:1", JSON), (b"b:1", FIXED)], base_offset=1))
    assert got == "json"


@pytest.mark.parametrize("value, kind", [(FIXED, "fixed16"), (JSON, "json")])
def test_an_lz4_section_kept_as_a_frame_is_peeked_through_the_host_decoder(value, kind):
    records = [FLUSH, (b"a:1", value), (b"b:1", value)]
    got, sections = sniff(batch(records, lz4=True), device_lz4=True)
    assert sections.shape[0] == 1 and int(sections[0]["codec"]) & 0xFF == 3  # still the frame: the GPU would decompress it
    assert got == kind
    got, sections = sniff(batch(records, lz4=True))  # (decompressed by the framer: the same answer from the plain section)
    assert int(sections[0]["codec"]) & 0xFF != 3 and got == kind


def test_no_deliverable_record_is_none():
    got, sections = sniff(batch([FLUSH, FLUSH]), batch([FLUSH], base_offset=2))
    assert got is None and int(sections["n_records"].sum()) == 3
    got, sections = sniff(b"")
    assert got is None and sections.shape[0] == 0
