"""GPU-side state encoders: fixed 64-byte states -> the plugin's serialized text, in bulk.

``encode_states`` publishes a whole snapshot (10 M aggregates ≈ 1 GB of JSON) without a per-aggregate host loop;
``encode_rows`` writes the same text for a list of rows in query order — the read seam's bytes for a batch of ids
(``GpuReplayStateStore.get_aggregate_bytes_many``; a store with a host key table still serves single reads through the
plugin's own ``writeState``).  The
text shape is declared as a template; ``JsonTemplate.counter()`` is the Counter fixture's play-json form
``{"aggregateId":"<id>","count":N,"version":N}``
(``modules/command-engine/scaladsl/src/test/scala/surge/scaladsl/TestBoundedContext.scala:15-16,127-129``);
``JsonTemplate.bank_account()`` is the surge-docs BankAccount's
``{"accountNumber":"<uuid>","accountOwner":"..","securityCode":"..","balance":<Double>}``
(``modules/surge-docs/src/test/scala/docs/command/BankAccountCommandModel.scala:19-23``, written by
``BankAccountSurgeModel.scala:26-28``): the Double as play-json writes it, the two strings from side columns.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Sequence, Tuple, Union

import numpy as np

from . import _native
from .replay import ReplayEngine, ReplayError

JP_LITERAL, JP_KEY, JP_I32, JP_U32, JP_I64, JP_F64, JP_STR = 0, 1, 2, 3, 4, 5, 6
STRING_COLUMNS = 4
MAX_PARTS = 16


class _CPart(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("field_offset", ctypes.c_uint32), ("lit_off", ctypes.c_uint32),
                ("lit_len", ctypes.c_uint32)]


class CJsonTemplate(ctypes.Structure):
    _fields_ = [("n_parts", ctypes.c_uint32), ("part", _CPart * MAX_PARTS), ("literals", ctypes.c_uint8 * 256)]


@dataclass(frozen=True)
class JsonTemplate:
    """Parts are ``bytes`` literals, the string ``"KEY"``, ``(kind, state_byte_offset)`` tuples, or ``(JP_STR, column)``."""

    parts: Sequence[Union[bytes, str, Tuple[int, int]]]

    @staticmethod
    def counter() -> "JsonTemplate":
        return JsonTemplate((b'{"aggregateId":', "KEY", b',"count":', (JP_I32, 0), b',"version":', (JP_I32, 4), b"}"))

    @staticmethod
    def bank_account() -> "JsonTemplate":
        """play-json's ``Json.format[BankAccount]``: fields in case-class order; ``balance`` is the v1 state's f64 at byte 16."""
        return JsonTemplate((b'{"accountNumber":', "KEY", b',"accountOwner":', (JP_STR, 0), b',"securityCode":', (JP_STR, 1),
                             b',"balance":', (JP_F64, 16), b"}"))

    def to_c(self) -> CJsonTemplate:
        t = CJsonTemplate()
        if not 1 <= len(self.parts) <= MAX_PARTS:
            raise ValueError(f"a template has 1..{MAX_PARTS} parts")
        t.n_parts = len(self.parts)
        pool = 0
        for i, p in enumerate(self.parts):
            if isinstance(p, bytes):
                if pool + len(p) > 256:
                    raise ValueError("literal pool exceeds 256 bytes")
                t.part[i].kind, t.part[i].lit_off, t.part[i].lit_len = JP_LITERAL, pool, len(p)
                for b in p:
                    t.literals[pool] = b
                    pool += 1
            elif p == "KEY":
                t.part[i].kind = JP_KEY
            else:
                t.part[i].kind, t.part[i].field_offset = int(p[0]), int(p[1])
        return t


def play_json_double(x: float) -> str:
    """The text play-json writes for a Scala ``Double`` (``surge_format_f64_json``: the library's host copy of the
    conversion its GPU encoder uses).  Raises ``ValueError`` for NaN / infinities, as ``BigDecimal(NaN)`` throws."""
    buf = ctypes.create_string_buffer(32)
    n = _native.load().surge_format_f64_json(int(np.float64(x).view(np.uint64)), buf, 32)
    if n == 0:
        raise ValueError(f"{x!r} is not a JSON number (play-json: NumberFormatException)")
    return buf.raw[:n].decode("ascii")


def key_table_utf8(keys: Sequence[Union[str, bytes]], slack: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Ids packed for the device: ``(their UTF-8 bytes, n + 1 int64 offsets)``.  ``bytes`` ids are taken as they stand;
    ``slack``: that many readable zero bytes behind the last id (``DeviceDecoder.lookup_device`` asks for 16)."""
    try:
        enc = [k.encode("utf-8") for k in keys]
    except AttributeError:  # (some are bytes already)
        enc = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum([len(e) for e in enc], out=off[1:])
    data = np.zeros(int(off[-1]) + slack, dtype=np.uint8)
    data[: int(off[-1])] = np.frombuffer(b"".join(enc), dtype=np.uint8)
    return data, off


def encode_states(engine: ReplayEngine, template: JsonTemplate, d_keys_utf8, d_key_off, capacity_hint: int = 0,
                  envelope: str = "none", strings=()):
    """Encode every resident aggregate.  Returns ``(out, out_off)`` CUDA tensors: aggregate ``a``'s text is
    ``out[out_off[a]:out_off[a+1]]`` (empty for None / poisoned aggregates).

    ``envelope="protobuf_state"`` wraps each value in the multilanguage module's ``State{aggregateId, payload}``
    message (``multilanguage-protocol.proto:7-10``; what ``GenericSurgeCommandBusinessLogic.scala:36-39`` stores),
    with the template text as the payload.  ``strings``: up to four ``(d_utf8, d_off)`` side string columns for
    ``(JP_STR, column)`` parts.  Raises ``ReplayError`` (UNSUPPORTED) after encoding everything else when some aggregate
    holds a NaN / infinite Double (no JSON number exists; those aggregates get zero bytes)."""
    import torch

    wrapped = check_envelope(envelope)
    lib = _native.load()
    fn = lib.surge_replay_encode_protobuf_state if wrapped else lib.surge_replay_encode_json
    n = engine.n_agg
    dev = d_key_off.device
    for c in range(STRING_COLUMNS):
        col = strings[c] if c < len(strings) else None
        engine._check(lib.surge_replay_set_encode_strings(
            engine._h, c, ctypes.c_void_p(col[0].data_ptr()) if col is not None and col[0].numel() else None,
            ctypes.c_void_p(col[1].data_ptr()) if col is not None else None))
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    cap = int(capacity_hint) if capacity_hint else max(64, 2 * int(d_keys_utf8.numel()) + 64 * n + sum(2 * int(c[0].numel()) for c in strings if c is not None))
    t = template.to_c()
    for _ in range(2):
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        total = ctypes.c_int64(0)
        rc = fn(
            engine._h, ctypes.byref(t), ctypes.c_void_p(d_keys_utf8.data_ptr()) if d_keys_utf8.numel() else None,
            ctypes.c_void_p(d_key_off.data_ptr()), ctypes.c_void_p(d_out.data_ptr()), cap,
            ctypes.c_void_p(d_off.data_ptr()), ctypes.byref(total))
        if rc == 0:
            return d_out[: total.value], d_off
        if rc == -6 and total.value > cap:  # SURGE_E_RANGE: retry with the exact size
            cap = total.value
            continue
        msg = lib.surge_replay_last_error(engine._h)
        raise ReplayError(rc, msg.decode() if msg else "")
    raise RuntimeError("encode_states: unreachable")


#: ``SURGE_READ_*`` (``include/surge_replay.h``): what a slot of ``encode_rows`` stands for
READ_MISS, READ_VALUE, READ_NONE, READ_POISONED, READ_NOT_A_NUMBER = 0, 1, 2, 3, 4


def encode_rows(engine: ReplayEngine, template: JsonTemplate, d_keys_utf8, d_key_off, d_rows, envelope: str = "none", strings=(), capacity_hint: int = 0):
    """Encode the aggregates ``d_rows`` names (an ``int64`` CUDA tensor; ``-1``: a miss), in that order
    (``surge_replay_encode_json_rows`` / ``_protobuf_state_rows``): the read seam's bytes for a batch of ids, composed on the
    device.  ``d_keys_utf8`` / ``d_key_off``: the key table the rows index (``DeviceDecoder.device_key_table()``); ``envelope`` and
    ``strings`` as in ``encode_states``.  Returns ``(out, out_off, kind)`` CUDA tensors: slot ``q``'s text is
    ``out[out_off[q]:out_off[q+1]]`` and ``kind[q]`` one of ``READ_*`` (zero bytes unless ``READ_VALUE``).  The encode filter is
    not consulted.  A buffer that is too small is retried once with the exact size, as in ``encode_states``; a row outside
    ``[-1, n_agg)`` raises ``ReplayError`` (INVALID); a row that holds a NaN / infinite Double raises it (UNSUPPORTED) after
    everything else was encoded."""
    import torch

    wrapped = check_envelope(envelope)
    lib = _native.load()
    fn = lib.surge_replay_encode_protobuf_state_rows if wrapped else lib.surge_replay_encode_json_rows
    n = int(d_rows.numel())
    dev = d_rows.device
    for c in range(STRING_COLUMNS):
        col = strings[c] if c < len(strings) else None
        engine._check(lib.surge_replay_set_encode_strings(
            engine._h, c, ctypes.c_void_p(col[0].data_ptr()) if col is not None and col[0].numel() else None,
            ctypes.c_void_p(col[1].data_ptr()) if col is not None else None))
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    cap = int(capacity_hint) if capacity_hint else max(64, 128 * n)  # (a guess: the first pass says what the rows need)
    t = template.to_c()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    for _ in range(2):
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        total = ctypes.c_int64(0)
        rc = fn(engine._h, ctypes.byref(t), ptr(d_keys_utf8), ctypes.c_void_p(d_key_off.data_ptr()), ptr(d_rows), n, ctypes.c_void_p(d_out.data_ptr()), cap,
                ctypes.c_void_p(d_off.data_ptr()), ptr(kind), ctypes.byref(total))
        if rc == 0:
            return d_out[: total.value], d_off, kind
        if rc == -6 and total.value > cap:  # SURGE_E_RANGE: retry with the exact size
            cap = total.value
            continue
        msg = lib.surge_replay_last_error(engine._h)
        raise ReplayError(rc, msg.decode() if msg else "")
    raise RuntimeError("encode_rows: unreachable")


# ---- the way back: serialized state values -> fixed 64-byte states -----------------------------------------------------
#: ``SURGE_STATE_DECODE_*`` (``include/surge_replay.h``)
DECODE_STATUS = {0: "OK", 1: "LITERAL", 2: "STRING", 3: "ESCAPE", 4: "KEY_MISMATCH", 5: "INT", 6: "RANGE", 7: "NUMBER", 8: "TRAILING",
                 9: "AMBIGUOUS", 10: "SURROGATE", 11: "ENVELOPE", 255: "SKIPPED"}
DECODE_OK, DECODE_LITERAL, DECODE_STRING, DECODE_ESCAPE, DECODE_KEY_MISMATCH, DECODE_INT, DECODE_RANGE = 0, 1, 2, 3, 4, 5, 6
DECODE_NUMBER, DECODE_TRAILING, DECODE_AMBIGUOUS, DECODE_SURROGATE, DECODE_SKIPPED = 7, 8, 9, 10, 255
DECODE_ENVELOPE = 11
DECODE_SYNTAX, DECODE_MISSING = 12, 13  # the lenient mode's own
DECODE_STATUS.update({12: "SYNTAX", 13: "MISSING"})
ENVELOPES = ("none", "protobuf_state")


def check_envelope(envelope) -> bool:
    """``True`` for the protobuf ``State`` envelope, ``False`` for bare text; the spellings are ``encode_states``'."""
    if envelope not in ENVELOPES:
        raise ValueError(f"unknown envelope {envelope!r}")
    return envelope == "protobuf_state"


class DecodedStates(tuple):
    """``(states, status, counts)`` of ``decode_states``; ``.spans`` holds the STR parts' raw spans, ``.refused`` the
    message of the call when winners were refused (``None`` otherwise)."""

    spans = None
    refused = None


def decode_state_host(template: JsonTemplate, value: bytes, key=None, envelope: str = "none", lenient: bool = False):
    """One serialized state value on the host (``surge_decode_json_state``: the parser the device kernel runs;
    ``envelope="protobuf_state"``: ``surge_decode_protobuf_state``, the value is the multilanguage module's
    ``State{aggregateId, payload}`` message around the template's text, field 1 is compared with ``key`` byte for byte and the
    spans are relative to the whole value).  Returns
    ``(status, state, spans)``: a ``SURGE_STATE_DECODE_*`` status, the state (a one-element ``STATE_DTYPE`` array, zeros
    unless the status is 0) and ``spans[c] = (offset, length)`` of STR column ``c``'s still-escaped bytes.  ``key``
    (``str`` or UTF-8 ``bytes``): the id the KEY string must equal; ``None``: not compared.  ``lenient``: the lenient reading
    mode (``surge_decode_json_state_lenient`` / ``surge_decode_protobuf_state_lenient``: members in any order, whitespace,
    unknown members skipped); a template it cannot read raises ``ValueError``."""
    from .schema import STATE_DTYPE

    lib = _native.load()
    if lenient:
        fn = lib.surge_decode_protobuf_state_lenient if check_envelope(envelope) else lib.surge_decode_json_state_lenient
    else:
        fn = lib.surge_decode_protobuf_state if check_envelope(envelope) else lib.surge_decode_json_state
    t = template.to_c()
    value = bytes(value)
    kb = None if key is None else (key.encode("utf-8") if isinstance(key, str) else bytes(key))
    state = np.zeros(1, dtype=STATE_DTYPE)
    span = (ctypes.c_int64 * (2 * STRING_COLUMNS))()
    rc = fn(ctypes.byref(t), value, len(value), kb, -1 if kb is None else len(kb), state.ctypes.data_as(ctypes.c_void_p), span)
    if rc == -5:  # SURGE_E_UNSUPPORTED
        raise ValueError("the lenient mode reads templates of the shape {\"<name>\": value ,\"<name>\": value ... } with distinct names: not this one")
    if rc < 0:
        raise ValueError(("surge_decode_json_state" if envelope == "none" else "surge_decode_protobuf_state") + ": bad argument or inconsistent template")
    return rc, state, [(span[2 * c], span[2 * c + 1]) for c in range(STRING_COLUMNS)]


def decode_states(engine: ReplayEngine, template: JsonTemplate, d_values, d_value_off, d_keys_utf8=None, d_key_off=None, d_agg_idx=None,
                  out=None, want_spans: bool = False, raise_on_refused: bool = False, envelope: str = "none", lenient: bool = False):
    """Decode state-topic record values on the device (``surge_replay_decode_json_states``; ``envelope="protobuf_state"``:
    ``surge_replay_decode_protobuf_states``, every value is a ``State{aggregateId, payload}`` message around the template's
    text and the spans are relative to the whole value): record ``r``'s text is
    ``d_values[d_value_off[r]:d_value_off[r+1]]`` (empty = tombstone) and names aggregate ``d_agg_idx[r]`` (``None``: aggregate
    ``r``); per aggregate the last record wins.  ``out``: the ``n_agg x 64`` byte CUDA tensor the rows go to (rows nothing
    names, and rows whose winner does not decode, keep what they hold) — ``None``: a fresh all-None tensor of one row per
    record (identity) or per key.  Returns ``(states, status, counts)``: the tensor, one ``SURGE_STATE_DECODE_*`` byte per
    record (CUDA) and ``counts = (rows written, tombstones, winners refused, Doubles re-parsed on the host)``; ``.spans`` of
    the result is the ``n_records x 4 x 2`` int64 CUDA tensor of STR spans when ``want_spans``.  Winners that do not decode
    are reported in ``counts`` (and ``.refused``), or raised as ``ReplayError`` (CORRUPT) with ``raise_on_refused``; any
    other failure raises.  ``lenient``: the call reads in the lenient mode (``ReplayEngine.reading_leniently``)."""
    import torch

    lib = _native.load()
    fn = lib.surge_replay_decode_protobuf_states if check_envelope(envelope) else lib.surge_replay_decode_json_states
    n = int(d_value_off.numel()) - 1
    dev = d_value_off.device
    if out is None:
        n_agg = n if d_agg_idx is None else (int(d_key_off.numel()) - 1 if d_key_off is not None else None)
        if n_agg is None:
            raise ValueError("decode_states: with d_agg_idx and no key table, pass `out` (it defines the aggregate count)")
        out = torch.zeros((n_agg, 64), dtype=torch.uint8, device=dev)
    n_agg = int(out.numel()) // 64
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    spans = torch.zeros((n, STRING_COLUMNS, 2), dtype=torch.int64, device=dev) if want_spans else None
    counts = (ctypes.c_int64 * 4)()
    t = template.to_c()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    with engine.reading_leniently(lenient):
        rc = fn(
            engine._h, ctypes.byref(t), ptr(d_values), ctypes.c_void_p(d_value_off.data_ptr()), n, ptr(d_keys_utf8),
            ctypes.c_void_p(d_key_off.data_ptr()) if d_key_off is not None else None, ptr(d_agg_idx), n_agg, ctypes.c_void_p(out.data_ptr()),
            ptr(status), ptr(spans), ctypes.byref(counts))
        msg = (lib.surge_replay_last_error(engine._h) or b"").decode() if rc else ""  # (before the mode is reset)
    res = DecodedStates((out, status, tuple(int(c) for c in counts)))
    res.spans = spans
    if rc == -7 and not raise_on_refused:  # SURGE_E_CORRUPT: everything else was decoded; counts[2] says how many were not
        res.refused = msg
        return res
    if rc:
        raise ReplayError(rc, msg)
    return res


# ---- the STR parts of decoded values, kept: spans -> side string columns ------------------------------------------------
def unescape_json_string(raw: bytes) -> bytes:
    """The bytes between the quotes of a JSON string -> its UTF-8 (``surge_unescape_json_string``: the routine the device
    runs on the spans ``decode_states(want_spans=True)`` reports).  Raises ``ValueError`` naming the ``SURGE_STATE_DECODE_*``
    status for a raw control byte, a bare quote, an unknown escape, a surrogate or a text that ends inside an escape."""
    raw = bytes(raw)
    lib = _native.load()
    n = lib.surge_unescape_json_string(raw, len(raw), None, 0)
    if n < 0:
        raise ValueError(f"not the body of a JSON string: {DECODE_STATUS.get(-n, -n)}")
    out = ctypes.create_string_buffer(max(int(n), 1))
    lib.surge_unescape_json_string(raw, len(raw), out, n)
    return out.raw[:n]


def merge_state_strings(engine: ReplayEngine, column: int, d_values=None, d_value_off=None, d_agg_idx=None, d_status=None, d_spans=None,
                        prev=None, n_agg: int = None, capacity_hint: int = 0):
    """String column ``column`` of the decoded records merged into the column so far (``surge_replay_merge_state_strings``).
    ``d_values`` / ``d_value_off`` / ``d_agg_idx`` as ``decode_states`` took them, ``d_status`` / ``d_spans`` as it left them
    (``res[1]``, ``res.spans``); ``prev``: the ``(d_utf8, d_off)`` column so far or ``None``; ``n_agg``: the aggregates the
    new column covers (default: the engine's).  Per aggregate the winning OK record's unescaped string (empty for a
    tombstone), else the previous string, else empty.  Without records (``d_value_off=None``) the column is extended to
    ``n_agg``.  Returns ``(d_utf8, d_off)`` CUDA tensors, ready for ``encode_states(strings=...)``."""
    import torch

    lib = _native.load()
    n_agg = engine.n_agg if n_agg is None else int(n_agg)
    n_rec = 0 if d_value_off is None else int(d_value_off.numel()) - 1
    n_prev = 0 if prev is None else int(prev[1].numel()) - 1
    dev = torch.device("cuda", engine.device)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None  # noqa: E731
    d_off = torch.empty(n_agg + 1, dtype=torch.int64, device=dev)
    cap = int(capacity_hint) if capacity_hint else (int(prev[0].numel()) if prev is not None else 0) + (int(d_values.numel()) if d_values is not None else 0)
    for _ in range(2):
        d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        total = ctypes.c_int64(0)
        rc = lib.surge_replay_merge_state_strings(
            engine._h, int(column), ptr(d_values), ptr(d_value_off) if n_rec else None, n_rec, ptr(d_agg_idx) if n_rec else None,
            ptr(d_status), ptr(d_spans), ptr(prev[0]) if prev is not None else None, ptr(prev[1]) if prev is not None else None, n_prev, n_agg,
            ctypes.c_void_p(d_out.data_ptr()), cap, ctypes.c_void_p(d_off.data_ptr()), ctypes.byref(total))
        if rc == 0:
            return d_out[: total.value], d_off
        if rc == -6 and total.value > cap:  # SURGE_E_RANGE: retry with the exact size
            cap = total.value
            continue
        msg = lib.surge_replay_last_error(engine._h)
        raise ReplayError(rc, msg.decode() if msg else "")
    raise RuntimeError("merge_state_strings: unreachable")
