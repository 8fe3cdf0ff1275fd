"""-m gpu: the protocol of the device decoder's host object — what result parity does not see.  The slot queue's refusals
(include/surge_ingest.h: "Up to five pushes may be unfinished at a time (SURGE_E_STATE beyond that, and from push /
push_records while any is)", "A push_async that fails occupies no slot"), that a call refused for the decoder's mode leaves
the decoder as it was, and the accounting behind ``counters()`` / ``stats()``.

Where the header gives no figure — the key table's slot counts, the hash function in use — the expected values are what
the library reported for these inputs before the host object was split into units (commit 5d6f4c9), recorded once on an
MI355X: they are literals, not derived from the code under test.  The shapes launch the smallest grids the kernels have."""
import numpy as np
import pytest

import kafka_wire as kw
from surge_amd import schema as S
from surge_amd.encode import JsonTemplate
from surge_amd.ingest import DeviceDecoder, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -2  # SURGE_E_INVALID, SURGE_E_STATE
SLOTS = 5                    # "Up to five pushes may be unfinished at a time"


def event(seq):
    e = np.zeros(1, dtype=S.EVENT_DTYPE)
    e["type"], e["seq"], e["raw"] = S.EVT_INC, seq, 1
    return e.tobytes()


def refused(status, call, *args, **kw_):
    with pytest.raises(IngestError) as ei:
        call(*args, **kw_)
    assert ei.value.status == status, str(ei.value)


# ---- 1: the slot queue ---------------------------------------------------------------------------------------------------
def test_the_slot_queue_takes_five_pushes_and_refuses_what_the_header_says_it_refuses():
    # a fixed-16 topic of 4 batches x 3 records over 5 ids, framed once
    recs = [(f"id{r % 5}:{r}".encode(), event(r)) for r in range(12)]
    wire = b"".join(kw.record_batch(3 * b, recs[3 * b:3 * b + 3]) for b in range(4))
    first_seen = list(dict.fromkeys(k.split(b":")[0].decode() for k, _ in recs))
    want_agg = [first_seen.index(k.split(b":")[0].decode()) for k, _ in recs]

    def snapshot(d):
        agg, ev, off, n_keys = d.result()
        return agg.cpu().tolist(), ev.cpu().numpy().tobytes(), off.cpu().tolist(), n_keys, d.keys()

    with EventsTopicIngest(frames=True) as g, DeviceDecoder(None) as d:
        g.feed(wire)
        sections, arena = g.drain_sections()
        assert [(int(s["base_offset"]), int(s["n_records"])) for s in sections] == [(0, 3), (3, 3), (6, 3), (9, 3)]
        for k in range(SLOTS):
            d.push_async((sections, arena))
            assert d.pending == k + 1
        refused(E_STATE, d.push_async, (sections, arena))  # the sixth
        assert d.pending == SLOTS
        refused(E_STATE, d.push, sections, arena)  # results are appended in push order: nothing synchronous overtakes
        refused(E_STATE, d.push_records, [b"x:1"], [event(1)], [0])
        refused(E_STATE, d.reserve, 100, 1000)
        assert d.pending == SLOTS
        for k in range(SLOTS):
            d.finish()
            assert d.pending == SLOTS - 1 - k
        done = snapshot(d)
        assert done == (want_agg * SLOTS, b"".join(v for _, v in recs) * SLOTS, list(range(12)) * SLOTS, 5, first_seen)
        assert d.stats()["pushes"] == SLOTS and d.counters()["records_delivered"] == 12 * SLOTS
        refused(E_STATE, d.finish)  # nothing is pending
        assert snapshot(d) == done and d.pending == 0
        bad = sections.copy()
        bad["byte_len"][1] = -1
        refused(E_INVALID, d.push_async, (bad, arena))
        assert d.pending == 0  # a push_async that fails occupies no slot
        d.push(sections, arena)
        assert d.stats()["pushes"] == SLOTS + 1 and d.pending == 0
        assert snapshot(d)[2] == list(range(12)) * (SLOTS + 1)


# ---- 2: a call refused for the decoder's mode changes nothing ----------------------------------------------------------------
def test_a_call_of_the_other_mode_is_refused_and_leaves_the_decoder_as_it_was():
    """That these calls return SURGE_E_STATE is pinned beside the calls themselves
    (test_state_topic_gpu.py::test_the_two_kinds_of_decoder_refuse_each_others_hand_over); here: the keep-strings setter on an
    events decoder, and that every refusal leaves the delivered records, the pending result and the key table alone."""
    counter = JsonTemplate.counter()
    with ReplayEngine() as eng:
        eng.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
        eng.fold()
        with DeviceDecoder(None) as d:
            d.push_records([b"a:1", b"b:1", b"a:2"], [event(1), event(1), event(2)], [7, 8, 9])
            held = lambda: (d.counters(), d.result()[2].cpu().tolist(), d.keys())
            before = held()
            assert before[1:] == ([7, 8, 9], ["a", "b"]) and before[0]["records_delivered"] == 3
            assert d._lib.surge_device_decoder_keep_strings(d._h, 1) == E_STATE
            refused(E_STATE, d.state_result)
            refused(E_STATE, d.load_states_into, eng, counter)
            assert held() == before
        with DeviceDecoder(states=True) as d:
            d.push_records([b"a", b"b", b"a"], [b'{"x":1}', b'{"x":2}', b""], [7, 8, 9])
            held = lambda: (d.counters(), d.state_result()[3].cpu().tolist(), d.state_result()[1].cpu().numpy().tobytes(), d.keys())
            before = held()
            assert before[1:] == ([7, 8, 9], b'{"x":1}{"x":2}', ["a", "b"]) and before[0]["records_delivered"] == 3
            refused(E_STATE, d.result)
            refused(E_STATE, d.fold_into, eng, wait=True)
            refused(E_STATE, d.fold_into, eng, wait=False)
            refused(E_STATE, d.stage_into, eng)
            assert held() == before


# ---- 3: accounting ---------------------------------------------------------------------------------------------------------
# the key table's slot count behind each of the three pushes below, and behind reserve(5000, ...) on a fresh decoder
TABLE_SLOTS = (2048, 2048, 4096)
TABLE_SLOTS_RESERVED = 16384


def test_counters_and_stats_after_each_of_three_pushes():
    def records(ids, n, flush_at=()):
        out = [(f"{ids[r % len(ids)]}:{r}".encode(), event(r)) for r in range(n)]
        for at in flush_at:
            out[at] = (b"", b"")  # the producer's flush record
        return out

    old = [f"agg-{i}" for i in range(300)]
    new = [f"new-{i}" for i in range(1000)]
    pushes = [records(old, 700, flush_at=(5, 650)), records(old, 700), records(new, 1000)]
    seen = delivered = skipped = 0
    with DeviceDecoder(None) as d:
        for k, recs in enumerate(pushes):
            d.push_records([key for key, _ in recs], [v for _, v in recs], list(range(seen, seen + len(recs))))
            flush = sum(1 for key, _ in recs if not key)
            seen, delivered, skipped = seen + len(recs), delivered + len(recs) - flush, skipped + flush
            st = d.stats()
            print(f"decoder accounting, push {k + 1}:", st)
            assert d.counters() == {"records_seen": seen, "records_delivered": delivered, "flush_records_skipped": skipped, "doubles_parsed_on_host": 0}
            assert st == {**d.counters(), "hash_reseeds": 0, "table_slots": TABLE_SLOTS[k], "pushes": k + 1, "hash_function": 0}
        assert (seen, delivered, skipped) == (2400, 2398, 2)
        ids = list(dict.fromkeys(key.split(b":")[0].decode() for recs in pushes for key, _ in recs if key))  # first delivered, first numbered
        assert len(ids) == 1300 and d.keys() == ids
    with DeviceDecoder(None) as d:
        d.reserve(5000, 5000 * 8)
        print("decoder accounting, reserve(5000):", d.stats())
        assert d.stats()["table_slots"] == TABLE_SLOTS_RESERVED and d.stats()["pushes"] == 0


# ---- 4: the reads between pushes refuse in a fixed order ---------------------------------------------------------------------
def test_every_read_of_the_key_table_is_refused_while_a_push_is_pending():
    """include/surge_ingest.h: the lookups, the key order, the range and the key gather need every push finished
    (SURGE_E_STATE).  The pending test comes before anything a read decides from its arguments: ``lookup`` of no id at all is
    refused too while a push is pending, and is an empty answer once it is finished."""
    import torch

    recs = [(b"id0:0", event(0)), (b"id1:1", event(1)), (b"id0:2", event(2))]
    with EventsTopicIngest(frames=True) as g, DeviceDecoder(None) as d:
        g.feed(kw.record_batch(0, recs))
        sections, arena = g.drain_sections()
        d.push_async((sections, arena))
        assert d.pending == 1
        refused(E_STATE, d.lookup, [])
        refused(E_STATE, d.lookup, [b"id0"])
        refused(E_STATE, d.key_order)
        refused(E_STATE, d.range_rows)
        refused(E_STATE, d.gather_keys, torch.zeros(1, dtype=torch.int64, device="cuda"))
        assert d.pending == 1
        d.finish()
        none = d.lookup([])
        assert none.dtype == np.int64 and none.shape == (0,)
        assert d.range_rows().cpu().tolist() == [0, 1]
        assert d.key_order().cpu().tolist() == [0, 1]
