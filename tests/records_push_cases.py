"""Shared builder of the framed-records push tests (``test_records_push_abi.py``, ``test_records_push_gpu.py``,
``test_store_consumer_records_gpu.py``): polls of ``(key, value, offset)`` records, and the three pins every device
result is held to.

The pins
  * the HOST decode of the same records — ``EventJsonTemplate.decode_keyed`` (``surge_event_json_decode_keyed``) per value, 16-byte
    values as they are — with the test's own lists for ids, offsets and first-delivered order (``expected``);
  * the WIRE route over the same records (``wire_result``: ``kafka_wire`` batches, host framing, ``DeviceDecoder.push``);
  * the synchronous ``push_records`` where the test is about the asynchronous call.

The values are the smallest JSON events there are, ``{"v":<int>}``, which a member the template does not name (``"p":"xxx"``, skipped
by the decoder) pads to any length from 15 bytes on."""
import numpy as np

import kafka_wire as kw
from surge_amd import schema as S
from surge_amd.ingest import ARG_I32, DeviceDecoder, EventJsonTemplate, EventsTopicIngest

EVENT = EventJsonTemplate("", [("", 0, "", "v", ARG_I32)])
BLOCK = 256  # records per block of the record stage's launch


def value(n: int, length: int = 0) -> bytes:
    """``{"v":n}``, padded to ``length`` bytes (0: as short as it is) by a member the template does not name."""
    short = b'{"v":%d}' % n
    if not length or length == len(short):
        return short
    frame = b'{"v":%d,"p":""}' % n
    assert length >= len(frame), (length, len(frame))
    return frame[:-2] + b"x" * (length - len(frame)) + b'"}'


def event16(seq: int, arg: int = 1) -> bytes:
    e = np.zeros(1, dtype=S.EVENT_DTYPE)
    e["type"], e["seq"], e["raw"] = S.EVT_INC, seq, np.uint64(np.uint32(np.int32(arg)))
    return e.tobytes()


def arrays(items):
    """A list of ``bytes`` as the ``(data_uint8, off_int64)`` pair ``push_records`` takes (own copies: a test may overwrite them)."""
    off = np.zeros(len(items) + 1, dtype=np.int64)
    if items:
        np.cumsum([len(x) for x in items], out=off[1:])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), off


def id_of(key: bytes, states: bool = False) -> bytes:
    return key if states else key.split(b":", 1)[0]


def expected(template, keys, values, offsets=None, known=(), states=False):
    """What a decoder that knows the ids ``known`` delivers for these records: ``(agg, events bytes, offsets, ids)`` — flush
    records (empty key and value) left out, ids numbered in first-delivered order behind ``known``.  Events mode: every value
    through the host decoder (a ``None`` template: the 16 bytes themselves); state mode: ``events`` is the values joined."""
    ids = list(known)
    index = {k: i for i, k in enumerate(ids)}
    agg, out, offs = [], [], []
    for r, (k, v) in enumerate(zip(keys, values)):
        if not k and not v:
            continue
        a = id_of(k, states)
        if a not in index:
            index[a] = len(ids)
            ids.append(a)
        agg.append(index[a])
        offs.append(r if offsets is None else offsets[r])
        if states or template is None:
            out.append(v)
        else:
            out.append(template.decode_keyed(a, v).tobytes())
    return agg, b"".join(out), offs, ids


def result_of(d):
    """An events decoder's result in the shape of ``expected`` (synchronises: a ``finish(wait=False)`` leaves it in stream order)."""
    import torch

    torch.cuda.synchronize()
    agg, ev, off, n_keys = d.result()
    ids = [k.encode() for k in d.keys()]
    assert n_keys == len(ids)
    return agg.cpu().tolist(), ev.cpu().numpy().tobytes(), off.cpu().tolist(), ids


def state_result_of(d):
    import torch

    torch.cuda.synchronize()
    agg, val, val_off, off, n_keys = d.state_result()
    ids = [k.encode() for k in d.keys()]
    assert n_keys == len(ids)
    return agg.cpu().tolist(), val.cpu().numpy().tobytes(), off.cpu().tolist(), ids, val_off.cpu().tolist()


def wire_of(keys, values, offsets=None, per_batch=200, compression="none") -> bytes:
    """The same records as uncompressed record batches: a new batch at every gap of the offsets and every ``per_batch`` records."""
    offsets = list(range(len(keys))) if offsets is None else list(offsets)
    out, start = [], 0
    for r in range(1, len(keys) + 1):
        if r == len(keys) or offsets[r] != offsets[r - 1] + 1 or r - start == per_batch:
            out.append(kw.record_batch(offsets[start], list(zip(keys[start:r], values[start:r])), compression=compression))
            start = r
    return b"".join(out)


def wire_result(template, keys, values, offsets=None):
    """The wire route's result for the same records on a fresh decoder."""
    with EventsTopicIngest(frames=True) as g, DeviceDecoder(template) as d:
        g.feed(wire_of(keys, values, offsets))
        d.push_from(g)
        return result_of(d)


def one_block_of(total: int, n: int = BLOCK):
    """``n`` records (one block of the launch) whose keys and values are ``total`` bytes together: keys of 16 bytes, the values
    sharing the rest."""
    assert n <= BLOCK
    keys = [b"%014d:%d" % (i, i % 10) for i in range(n)]
    assert all(len(k) == 16 for k in keys)
    v_total = total - 16 * n
    lens = [v_total // n] * n
    lens[-1] += v_total - sum(lens)
    values = [value(i, L) for i, L in enumerate(lens)]
    assert sum(len(k) for k in keys) + sum(len(v) for v in values) == total
    return keys, values
