"""The string fields of events on the device (``DeviceDecoder(event_strings=...)``, ``surge_amd/csrc/ingest_strings.hip``): the
select / list / spans / gather passes behind a push's interning and the merge of what they keep, against the host export
(``EventJsonTemplate.string_spans``) plus a Python dict in which the last naming event of an aggregate wins.

The expectation is never the device's: a record's strings are the host export's spans unescaped by ``unescape_json_string``
(pinned against ``json.loads`` in tests/test_event_strings.py).  Shapes are the smallest at which the kernels branch: 64 lanes a
wave and 256 records a block of the select (-1, +0, +1, the second and third block), 256 pending records a block of the merge
with more and fewer than its 32 KiB stage, 16-byte pieces of the gather at every source and destination residue, the record
stage's three LDS classes (8320, 16640, 65536 bytes a section) and a section beyond them."""
import uuid

import numpy as np
import pytest

import event_strings_cases as esc
import kafka_wire as kw
import state_strings_gen as gen
from surge_amd import schema as S
from surge_amd.encode import JsonTemplate, unescape_json_string
from surge_amd.ingest import EVENT_STRING_OK, DeviceDecoder, EventsTopicIngest, IngestError
from surge_amd.replay import ReplayEngine

pytestmark = pytest.mark.gpu

BANK, STRINGS = esc.BANK, esc.BANK_STRINGS
OWNERS = [o.encode("utf-8") for o in gen.OWNERS]


def raw_of(text: bytes, ascii_only=False) -> bytes:
    """the still-escaped JSON spelling of a string"""
    import json

    return json.dumps(text.decode("utf-8"), ensure_ascii=ascii_only).encode("utf-8")[1:-1]


def created(key: bytes, owner: bytes, code: bytes = b"0042", ascii_only=False) -> bytes:
    return esc.created(raw_of(owner, ascii_only), raw_of(code), account=key)


def expect_into(table, records, rule="bank", floor=None):
    """the host export over ``(offset, key, value)`` records in topic order: table[(id, column)] = the last naming event's string"""
    template, strings = esc.RULES[rule]
    for off, key, value in records:
        if floor is not None and off < floor:
            continue
        rc, spans, status = template.string_spans(strings, value)
        assert rc == 0, (key, value)
        for c in range(4):
            if status[c] == EVENT_STRING_OK:
                o, n = spans[c]
                table[(key.split(b":", 1)[0], c)] = unescape_json_string(value[o:o + n])
    return table


def column_of(col):
    data, off = col[0].cpu().numpy().tobytes(), col[1].cpu().tolist()
    assert off[0] == 0 and off == sorted(off) and off[-1] == len(data)
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def check_columns(d, table, named=(0, 1)):
    keys = [k.encode("utf-8") for k in d.keys()]
    cols = d.state_strings()
    for c in range(4):
        if c not in named:
            assert cols[c] is None, c
            continue
        got = column_of(cols[c])
        assert len(got) == len(keys)
        want = [table.get((k, c), b"") for k in keys]
        assert got == want, (c, [(k, g, w) for k, g, w in zip(keys, got, want) if g != w][:3])
    return keys


def batches(records, compression, per_batch):
    """``(offset, key, value)`` records with consecutive offsets -> record batches of ``per_batch`` records"""
    out = b""
    for s in range(0, len(records), per_batch):
        chunk = records[s:s + per_batch]
        out += kw.record_batch(chunk[0][0], [(k, v) for _, k, v in chunk], compression=compression)
    return out


def push_wire(d, data, start=None):
    with EventsTopicIngest(frames=True, device_lz4=True) as g:
        if start is not None:
            g.set_start_offset(start)
        g.feed(data)
        assert d.push_from(g) > 0


def topic(n, pattern, first_offset=0, salt=0):
    """n records over n // 3 + 1 accounts; ``pattern`` says which are BankAccountCreated (the others BankAccountUpdated)"""
    recs = []
    for i in range(n):
        key = b"acct-%d" % ((i * 7 + salt) % (n // 3 + 1))
        sel = {"none": False, "all": True, "one in 64": i % 64 == 17, "last lane": i % 64 == 63}[pattern]
        owner = OWNERS[(i + salt) % len(OWNERS)] + b" %d" % i
        value = created(key, owner, b"" if i % 5 == 0 else b"%04d" % i, ascii_only=i % 3 == 0 and b"\xf0" not in owner) if sel else esc.updated(key, b"%d.25" % i)
        recs.append((first_offset + i, key, value))
    return recs


# ---- 1: one push, the select's and the gather's shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_a_push_of_n_records_keeps_the_strings_the_host_export_finds(n):
    for j, pattern in enumerate(("none", "all", "one in 64", "last lane")):
        recs = topic(n, pattern)
        with DeviceDecoder(BANK, event_strings=STRINGS) as d:
            if j % 2:
                d.push_records([k for _, k, _ in recs], [v for _, _, v in recs], [o for o, _, _ in recs])
            else:
                push_wire(d, batches(recs, ("lz4", "none")[(n + j) % 2 == 0], 250))
            n_sel = sum(b"Created" in v for _, _, v in recs)
            pend = d.event_strings_pending()
            assert pend["records"] == n_sel and pend["merges"] == 0
            if n_sel:
                off = pend["value_off"].cpu().tolist()
                sel = [(o, k, v) for o, k, v in recs if b"Created" in v]
                assert off == np.concatenate([[0], np.cumsum([len(v) for _, _, v in sel])]).tolist()  # topic order, CSR offsets
                assert pend["values"][:off[-1]].cpu().numpy().tobytes() == b"".join(v for _, _, v in sel)
                keys = d.keys()
                assert [keys[r].encode() for r in pend["rows"].cpu().tolist()] == [k for _, k, _ in sel]
            check_columns(d, expect_into({}, recs))
            assert d.event_strings_pending()["records"] == 0 and d.event_strings_pending()["merges"] == (1 if n_sel else 0)


def test_every_source_alignment_and_destination_residue_of_the_gather_with_guard_bytes_behind_the_compact_buffer():
    import torch

    # values of 100 + (i * 7) % 48 bytes: sources and destinations walk through every residue mod 16, pieces of every shape
    recs = []
    for i in range(300):
        key = b"a%03d" % i
        base = len(created(key, b""))
        recs.append((i, key, created(key, b"o" * (100 + (i * 7) % 48 - base) + b"", b"%04d" % i)))
    keys = [k for _, k, _ in recs]
    values = [v for _, _, v in recs]
    cut = 240
    src = np.cumsum([0] + [len(v) for v in values[:cut - 1]]) + sum(len(k) for k in keys[:cut])  # push_records stages the keys, then the values
    assert set((src % 16).tolist()) == set(range(16))
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        d.push_records(keys[:cut], values[:cut], list(range(cut)))  # (allocates the compact buffer with room to spare)
        pend = d.event_strings_pending()
        used = pend["bytes"]
        assert pend["capacity"] > used + sum(len(v) for v in values[cut:]) + 64, "the second push must fit where the guards are"
        pend["values"][used:] = 0xA5
        torch.cuda.synchronize()
        d.push_records(keys[cut:], values[cut:], list(range(cut, 300)))
        after = d.event_strings_pending()
        assert after["capacity"] == pend["capacity"] and after["records"] == 300
        off = after["value_off"].cpu().tolist()
        assert set(o % 16 for o in off[:cut]) == set(range(16)) and set(o % 16 for o in off[cut:-1]) == set(range(16))
        buf = after["values"].cpu().numpy()
        assert buf[:off[-1]].tobytes() == b"".join(values) and (buf[off[-1]:] == 0xA5).all()  # nothing behind the last value was written
        check_columns(d, expect_into({}, recs))


def test_a_block_of_pending_records_beyond_the_merges_stage_and_sections_of_every_lds_class():
    # sections of ~5, ~12, ~40 and ~84 KiB: the record stage's three LDS classes and the global path; 420-byte values, so a
    # block of 256 pending records holds 100 KiB (the merge's LDS stage is 32 KiB: it reads them from global memory)
    recs, sizes = [], (12, 28, 95, 200)
    for i in range(sum(sizes)):
        key = b"big-%d" % (i % 150)
        owner = ((gen.OWNERS[i % len(gen.OWNERS)] + "|") * 60)[:300].encode("utf-8")
        recs.append((i, key, created(key, owner if b"\xf0" not in owner else b"plain %d " % i * 30, b"c%d" % i)))
    for compression in ("none", "lz4"):
        data, at = b"", 0
        for n in sizes:
            data += kw.record_batch(at, [(k, v) for _, k, v in recs[at:at + n]], compression=compression)
            at += n
        with EventsTopicIngest(frames=True, device_lz4=True) as g, DeviceDecoder(BANK, event_strings=STRINGS) as d:
            g.feed(data)
            sections, arena = g.drain_sections()
            if compression == "none":
                lens = sections["byte_len"].tolist()
                assert lens[0] <= 8320 < lens[1] <= 16640 < lens[2] <= 65536 < lens[3]
            d.push(sections, arena)
            assert d.event_strings_pending()["bytes"] > 3 * 32 * 1024
            check_columns(d, expect_into({}, recs))


def test_the_last_value_of_a_section_and_of_a_records_push_and_every_accepted_case_of_the_corpus():
    cases = [c for c in esc.accepted_cases() if c.rule == "bank" and not c.name.startswith("dumped")]
    recs = [(i, b"case-%d" % i, c.value) for i, c in enumerate(cases)]
    recs.append((len(recs), b"last", created(b"last", b"the last value ends where the staged bytes end")))
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        d.push_records([k for _, k, _ in recs], [v for _, _, v in recs], [o for o, _, _ in recs])
        check_columns(d, expect_into({}, recs))
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        push_wire(d, batches(recs, "none", 40))
        check_columns(d, expect_into({}, recs))


def test_enveloped_events_and_the_two_class_rule():
    env = [c for c in esc.envelope_cases() if not c.refused and len(c.key) < 1000]
    recs = [(i, c.key, c.value) for i, c in enumerate(env)]
    with DeviceDecoder(esc.BANK_ENV, event_strings=STRINGS) as d:
        push_wire(d, batches(recs, "lz4", 7))
        check_columns(d, expect_into({}, recs, "bank_env"))
    two = [c for c in esc.position_cases() if c.rule == "two" and not c.refused]
    # one aggregate: class a sets column 0, class b replaces it and sets column 2, class c keeps both
    recs = [(0, b"x:1", two[0].value), (1, b"y:1", two[0].value), (2, b"x:2", two[1].value), (3, b"x:3", two[2].value)]
    with DeviceDecoder(esc.TWO, event_strings=esc.TWO_STRINGS) as d:
        push_wire(d, batches(recs, "none", 4))
        table = expect_into({}, recs, "two")
        assert table == {(b"x", 0): b"L\n", (b"x", 2): b"", (b"y", 0): b"Ann"}
        check_columns(d, table, named=(0, 2))


# ---- 2: across pushes -----------------------------------------------------------------------------------------------------------
def test_across_pushes_the_last_created_wins_an_updated_keeps_and_new_ids_extend(monkeypatch):
    monkeypatch.setenv("SURGE_INGEST_EVENT_STRINGS_PENDING", "100")  # (read when the decoder is armed)
    monkeypatch.setenv("SURGE_INGEST_DEBUG_WEAK_HASH", "1")          # (read at create: ids collide until the first re-seed)
    first = topic(300, "all")                      # 101 accounts, each created three times: 300 pending > 100, merged at the push's end
    second = topic(90, "none", 300) + [(390, b"acct-5", created(b"acct-5", b"replaced \xe2\x82\xac", b""))]
    third = [(400 + i, b"new-%d" % i, created(b"new-%d" % i, OWNERS[i % len(OWNERS)], b"n%d" % i)) for i in range(700)]  # 700 new ids: the table grows
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        table = {}
        push_wire(d, batches(first, "lz4", 100))
        assert d.event_strings_pending()["merges"] == 1 and d.event_strings_pending()["records"] == 0  # the bound was crossed
        assert d.stats()["hash_reseeds"] >= 1
        check_columns(d, expect_into(table, first))
        slots = d.stats()["table_slots"]
        push_wire(d, batches(second, "none", 50))
        assert d.event_strings_pending()["records"] == 1
        check_columns(d, expect_into(table, second))                   # read between pushes ...
        assert table[(b"acct-5", 0)] == "replaced €".encode() and table[(b"acct-5", 1)] == b""
        push_wire(d, batches(third, "lz4", 250))
        assert d.stats()["table_slots"] > slots
        keys = check_columns(d, expect_into(table, third))            # ... and again after more pushes
        assert len(keys) == 101 + 700 and d.event_strings_pending()["merges"] >= 3
        # clear drops what is pending and not merged: the id is interned, its strings stay empty; merged columns stay
        push_wire(d, batches([(2000, b"dropped", created(b"dropped", b"never merged"))], "none", 1))
        assert d.event_strings_pending()["records"] == 1
        d.clear()
        assert d.event_strings_pending()["records"] == 0
        keys = check_columns(d, table)
        assert keys[-1] == b"dropped"


# ---- 3: refusals ----------------------------------------------------------------------------------------------------------------
REFUSED = [c for c in esc.refused_cases() if c.rule == "bank"]


@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_a_refused_record_fails_its_push_by_offset_and_leaves_the_columns_as_they_were(case):
    good = [(10 + i, b"g%d" % (i % 4), created(b"g%d" % (i % 4), OWNERS[i])) for i in range(8)]
    bad = [(100, b"h0", created(b"h0", b"fine")), (101, b"bad", case.value), (102, b"h1", created(b"h1", b"also fine"))]
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        push_wire(d, batches(good, "none", 8))
        table = expect_into({}, good)
        check_columns(d, table)
        with pytest.raises(IngestError) as ei:
            push_wire(d, batches(bad, "lz4", 3))
        assert ei.value.status == -7 and "offset 101)" in str(ei.value), str(ei.value)
        assert d.n_keys == 4 and d.event_strings_pending()["records"] == 0  # nothing of the push is kept, no key of it interned
        check_columns(d, table)
        after = [(200, b"bad", created(b"bad", b"now it is fine"))]
        push_wire(d, batches(after, "none", 1))
        check_columns(d, expect_into(table, after))


REFUSED_ENV = [c for c in esc.refused_cases() if c.rule == "bank_env"]


@pytest.mark.parametrize("case", REFUSED_ENV, ids=[c.name for c in REFUSED_ENV])
def test_a_refused_enveloped_record_fails_its_push_by_offset_and_leaves_the_columns_as_they_were(case):
    wrap = esc.eec.wrap
    good = [(10 + i, b"g%d" % (i % 4), wrap(b"g%d" % (i % 4), created(b"g%d" % (i % 4), OWNERS[i]))) for i in range(8)]
    bad = [(100, b"h0", wrap(b"h0", created(b"h0", b"fine"))), (101, b"a", case.value), (102, b"h1", wrap(b"h1", created(b"h1", b"also fine")))]
    with DeviceDecoder(esc.BANK_ENV, event_strings=STRINGS) as d:
        push_wire(d, batches(good, "lz4", 8))
        table = expect_into({}, good, "bank_env")
        check_columns(d, table)
        with pytest.raises(IngestError) as ei:
            push_wire(d, batches(bad, "none", 3))
        assert ei.value.status == -7 and "offset 101)" in str(ei.value), str(ei.value)
        if case.name == "an enveloped refusal":  # the envelope and the event are good: it is the string walk behind sp_envelope_spans that refuses
            assert "string" in str(ei.value)
        assert d.n_keys == 4 and d.event_strings_pending()["records"] == 0
        check_columns(d, table)
        after = [(200, b"a", wrap(b"a", created(b"a", b"now it is fine")))]
        push_wire(d, batches(after, "none", 1))
        check_columns(d, expect_into(table, after, "bank_env"))


def test_guard_bytes_behind_the_columns_survive_every_merge():
    """The bytes buffer and the offsets buffer the next merge writes, filled with 0xA5 over their whole capacity before it: behind
    the column's total and behind its key count + 1 offsets nothing is written — through both buffers of a column, a column that
    grows, and a merge with nothing pending that only extends the column to new ids."""
    import torch

    pushes = [topic(300, "all"), topic(200, "all", 300, salt=5) + [(500 + i, b"late-%d" % i, created(b"late-%d" % i, OWNERS[i % len(OWNERS)] * 9, b"")) for i in range(300)],
              [(900 + i, b"only-updated-%d" % i, esc.updated(b"only-updated-%d" % i)) for i in range(70)], topic(64, "last lane", 1000)]
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        table = {}
        for k, recs in enumerate(pushes):
            push_wire(d, batches(recs, ("lz4", "none")[k % 2], 100))
            assert d.event_strings_pending()["records"] == sum(b"Created" in v for _, _, v in recs)
            nxt = [d.event_strings_next_column(c) for c in range(4)]
            assert nxt[2] is None and nxt[3] is None
            n_keys = d.n_keys
            for c in (0, 1):
                assert nxt[c][1].numel() >= (n_keys + 1) * 8
                nxt[c][0][:] = 0xA5
                nxt[c][1][:] = 0xA5
            torch.cuda.synchronize()
            cols = d.state_strings()
            expect_into(table, recs)
            for c in (0, 1):
                utf8, off = cols[c]
                total = int(off[-1].item())
                assert off.data_ptr() == nxt[c][1].data_ptr() and int(off.numel()) == n_keys + 1
                assert total == 0 or utf8.data_ptr() == nxt[c][0].data_ptr()
                assert total <= nxt[c][0].numel()
                assert bool((nxt[c][0][total:] == 0xA5).all()) and bool((nxt[c][1][(n_keys + 1) * 8:] == 0xA5).all())
            check_columns(d, table)
            assert d.event_strings_next_column(0) is None and d.event_strings_next_column(1) is None  # up to date: the next merge has nothing to write


# ---- 4: the default path ----------------------------------------------------------------------------------------------------------
def test_a_decoder_that_was_not_armed_gives_the_same_events_keys_and_counters_and_no_columns():
    recs = topic(600, "one in 64") + topic(300, "all", 600, salt=3)
    data = batches(recs, "lz4", 200)
    got = []
    for armed in (False, True):
        with DeviceDecoder(BANK, event_strings=STRINGS if armed else None) as d:
            push_wire(d, data)
            agg, ev, off, n_keys = d.result()
            got.append((agg.cpu().numpy().copy(), ev.cpu().numpy().copy(), off.cpu().numpy().copy(), n_keys, d.keys(), d.counters(), d.stats()))
            if not armed:
                with pytest.raises(IngestError) as ei:
                    d.state_strings()
                assert ei.value.status == -2
                with pytest.raises(IngestError):
                    d.event_strings_pending()
                with pytest.raises(IngestError) as ei:  # arming comes before the first push
                    d.keep_event_strings(STRINGS)
                assert ei.value.status == -2
    plain, armed = got
    assert all((a == b).all() for a, b in zip(plain[:3], armed[:3])) and plain[3:] == armed[3:]
    with DeviceDecoder() as fixed, pytest.raises(IngestError) as ei:  # 16-byte events: no template, no strings
        fixed.keep_event_strings(STRINGS)
    assert ei.value.status == -2
    with pytest.raises(ValueError):
        DeviceDecoder(event_strings=STRINGS)
    with pytest.raises(IngestError) as ei:  # strings that do not validate against the decoder's template
        DeviceDecoder(BANK, event_strings=esc.TWO_STRINGS)
    assert ei.value.status == -1


# ---- 5: a floored push ------------------------------------------------------------------------------------------------------------
def test_a_created_event_below_the_floor_contributes_nothing():
    recs = [(50, b"low", created(b"low", b"below the floor")), (51, b"both", created(b"both", b"below")), (52, b"low", esc.updated(b"low")),
            (53, b"both", created(b"both", b"above")), (54, b"high", created(b"high", b"only above", b""))]
    with DeviceDecoder(BANK, event_strings=STRINGS) as d:
        push_wire(d, batches(recs, "lz4", 5), start=52)
        assert d.below_floor() == 2 and d.event_strings_pending()["records"] == 2
        table = expect_into({}, recs, floor=52)
        assert (b"low", 0) not in table and table[(b"both", 0)] == b"above"
        assert check_columns(d, table) == [b"low", b"both", b"high"]


# ---- 6: a state decoder that kept its strings goes on as an events decoder ----------------------------------------------------------
def test_a_continued_state_decoder_merges_the_tails_strings_into_the_restored_columns():
    units, table = gen.make_topic(compression="lz4")
    state_template = JsonTemplate.bank_account()
    live = [k for k in table if table[k]]
    gone = [k for k in table if table[k] is None]
    assert len(gone) >= 3
    fresh = [str(uuid.UUID(int=99000 + i)) for i in range(5)]
    tail = [(i, k.encode(), created(k.encode(), b"tail owner %d \xc3\xa9" % i, b"t%d" % i)) for i, k in enumerate(live[:4] + gone[:3] + fresh)]
    tail += [(len(tail), live[5].encode(), esc.updated(live[5].encode()))]
    ingests = [EventsTopicIngest(frames=True, device_lz4=True) for _ in units]
    try:
        with ReplayEngine() as e, DeviceDecoder(states=True, keep_strings=True) as d:
            e.load_csr(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE))
            e.fold()
            with pytest.raises(IngestError) as ei:  # a state decoder reads no events
                d.keep_event_strings(STRINGS)
            assert ei.value.status == -2
            parts = []
            for g, part in zip(ingests, units):
                g.feed(gen.concat(part)[0])
                parts.append(g.drain_sections())
            d.push_async(parts)
            d.finish()
            assert d.load_states_into(e, state_template)[2] == 0
            d.continue_as_events(BANK)
            d.keep_event_strings(STRINGS)
            want = {}
            for k, t in table.items():
                want[(k.encode(), 0)], want[(k.encode(), 1)] = ((t[0].encode(), t[1].encode()) if t else (b"", b""))
            check_columns(d, want)  # the restored columns, before any event
            push_wire(d, batches(tail, "lz4", 6))
            keys = check_columns(d, expect_into(want, tail))
            assert len(keys) == len(table) + len(fresh)
            assert want[(gone[0].encode(), 0)].startswith(b"tail owner") and want[(live[5].encode(), 0)] == table[live[5]][0].encode()
            with pytest.raises(IngestError) as ei:  # armed once
                d.keep_event_strings(STRINGS)
            assert ei.value.status == -2
    finally:
        for g in ingests:
            g.close()
