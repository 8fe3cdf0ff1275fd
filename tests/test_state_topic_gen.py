"""Pins the state-topic generator (``tests/state_topic_gen.py``) on what exists without the state-mode decoder: the HOST
decoder reads its partitions — LZ4 and uncompressed, compaction gaps, transactions, an aborted one, the leading flush record,
headers, tombstones — and returns the generator's own record lists; ``snapshot.compact`` of those is the table the GPU tests
expect.  The conditions those tests rely on are asserted here, on the CPU reference alone."""
import json

import pytest

import state_topic_gen as gen
from surge_amd.ingest import EventsTopicIngest
from surge_amd.snapshot import StateRecord, compact


@pytest.fixture(scope="module")
def topics():
    return {c: gen.make_topic(compression=c) for c in ("lz4", "none")}


def host_records(data):
    with EventsTopicIngest() as g:
        g.feed(data)
        got = [(o, k, v) for o, _, k, v in g.drain_records()]
        return got, g.counters()


@pytest.mark.parametrize("compression", ["lz4", "none"])
def test_the_host_decoder_returns_the_generators_own_records(topics, compression):
    flush = aborted = 0
    for units in topics[compression]:
        data, want = gen.concat(units)
        got, counters = host_records(data)
        assert [r for r in got if not (r[1] == b"" and r[2] == b"")] == want  # offsets with their gaps, null values as None
        flush += counters["flush_records_skipped"] + sum(1 for r in got if r[1] == b"" and r[2] == b"")
        aborted += counters["records_aborted"]
        assert counters["open_transactions"] == 0 and counters["control_batches"] > 5
        offs = [o for o, _, _ in want]
        assert offs == sorted(set(offs)) and any(b - a > 1 for a, b in zip(offs, offs[1:]))  # gaps
        # fetch by fetch (three slices of the units) the same records arrive
        fed = []
        with EventsTopicIngest() as g:
            for part in gen.split(units, 3):
                g.feed(gen.concat(part)[0])
                fed += [(o, k, v) for o, _, k, v in g.drain_records() if not (k == b"" and v == b"")]
        assert fed == want
    assert flush == 1 and aborted > 20


def test_both_compressions_carry_the_same_records(topics):
    for a, b in zip(topics["lz4"], topics["none"]):
        assert gen.concat(a)[1] == gen.concat(b)[1]
        assert len(gen.concat(a)[0]) < len(gen.concat(b)[0])


def test_the_topic_has_what_the_gpu_tests_rely_on(topics):
    records = [r for units in topics["lz4"] for r in gen.concat(units)[1]]
    assert 1900 <= len(records) <= 2200
    tombstones = sum(1 for _, _, v in records if v is None)
    assert tombstones >= 0.1 * len(records)
    assert all(v is None or len(v) > 0 for _, _, v in records)  # no empty non-null value: the state decoder refuses those
    state, recreated = {}, set()
    for _, k, v in records:
        if v is not None and k in state and state[k] is None:
            recreated.add(k)
        state[k] = v
    assert len(recreated) >= 20
    assert sum(1 for v in state.values() if v is None) >= 20
    keys = {k.decode() for k in state}
    assert "a" in keys and "a:b" in keys and sum(":" in k for k in keys) >= 5
    assert any(json.dumps(k, ensure_ascii=False) != '"' + k + '"' for k in keys)  # ids that need JSON escaping
    table = compact(StateRecord("state", 0, k.decode(), v) for _, k, v in records)
    assert table == {k.decode(): v for k, v in state.items() if v is not None}
    for k, v in table.items():
        assert json.loads(v)["aggregateId"] == k
