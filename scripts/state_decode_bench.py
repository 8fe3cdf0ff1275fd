"""Resuming from serialized states: the device decoder against the per-aggregate host loop, in one process.

    python scripts/state_decode_bench.py [n_aggregates=2000000] [pairs=3] > profiles/state_decode.json

For the Counter and the BankAccount fixture: n PRESENT states are folded into an engine and written as state-topic values by
the device encoder (its time is reported beside the decoder's: the same states, the other direction).  Then two routes
to the same resident states alternate, ``pairs`` times each after a warm-up:

* ``device``: the values (already on the device, as a fetch leaves them) through ``encode.decode_states`` into the
  engine's resident state — ``surge_replay_decode_json_states``, key comparison on;
* ``host``: what ``store.restore(prior=...)`` does for the same job — intern every id, ``model.state_to_fixed`` per aggregate
  in Python, one H2D copy of the rows (``load_csr(init_state)`` + ``fold``).  Its input is the dict of aggregate OBJECTS: the
  JSON text -> object step a real resume needs first (``read_state`` per record) is not charged to it.

Both end in the same 64-byte rows (checked).  One JSON line: per fixture the times of every repeat, medians, the spread
between repeats of a route, aggregates/s, and whether the device route wins by more than either spread in every pair."""
import json
import os
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import torch  # noqa: E402

from surge_amd import schema as S  # noqa: E402
from surge_amd.encode import JsonTemplate, decode_states, encode_states, key_table_utf8  # noqa: E402
from surge_amd.log import KeyTable  # noqa: E402
from surge_amd.replay import ReplayEngine  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fixture(name: str, n: int):
    """(model, template, keys, aggregates by key, string columns, the fixed states)"""
    from fixture_models import BankAccount, BankAccountCommandModel, CounterBusinessLogic, State

    rng = np.random.default_rng(1)
    if name == "counter":
        model = CounterBusinessLogic().command_model()
        keys = [f"agg-{i:08d}" for i in range(n)]
        counts, versions = rng.integers(-10**6, 10**6, size=n), rng.integers(1, 10**5, size=n)
        prior = {k: State(k, int(c), int(v)) for k, c, v in zip(keys, counts, versions)}
        return model, JsonTemplate.counter(), keys, prior, ()
    model = BankAccountCommandModel()
    keys = [str(uuid.UUID(int=i * 7919 + 1)) for i in range(n)]
    owners, codes = [f"Jane Doe {i}" for i in range(n)], [f"{i % 10000:04d}" for i in range(n)]
    balances = np.round(rng.random(n) * 1e9) / 100
    prior = {k: BankAccount(uuid.UUID(k), o, c, float(b)) for k, o, c, b in zip(keys, owners, codes, balances)}
    return model, JsonTemplate.bank_account(), keys, prior, (owners, codes)


def host_route(model, prior, engine):
    """The body of GpuReplayStateStore.restore(prior=...) with no events: seconds, and the rows it produced."""
    t0 = time.perf_counter()
    keys = KeyTable()
    for k in prior:
        keys.intern(k)
    init = np.zeros(len(keys), dtype=S.STATE_DTYPE)
    for k, agg in prior.items():
        init[keys.index[k]] = model.state_to_fixed(agg)[0]
    engine.load_csr(np.zeros(len(keys) + 1, dtype=np.int64), np.zeros(0, dtype=S.EVENT_DTYPE), init)
    engine.fold()
    engine.synchronize()
    return time.perf_counter() - t0


def run(name: str, n: int, pairs: int) -> dict:
    model, template, keys, prior, columns = fixture(name, n)
    algebra = model.event_algebra()
    with ReplayEngine(algebra) as eng, ReplayEngine(algebra) as host_eng:
        host_route(model, dict(list(prior.items())[:10000]), host_eng)  # warm-up (Python only: nothing of it is compiled)
        t_host_first = host_route(model, prior, eng)                     # ... and the states every later step works on
        want = eng.snapshot()
        kd, ko = (dev(x) for x in key_table_utf8(keys))
        cols = [tuple(dev(x) for x in key_table_utf8(c)) for c in columns]
        enc = []
        for _ in range(pairs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_out, d_off = encode_states(eng, template, kd, ko, strings=cols)
            torch.cuda.synchronize()
            enc.append(time.perf_counter() - t0)
        text_bytes = int(d_out.numel())
        rows = eng.device_state()
        runs = {"device": [], "host": [t_host_first]}
        for i in range(pairs + 1):
            rows.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = decode_states(eng, template, d_out, d_off, kd, ko, out=rows)  # returns when the rows stand
            dt = time.perf_counter() - t0
            assert res[2][0] == n and res.refused is None, res[2]
            if i:
                runs["device"].append(dt)
            if 0 < i < pairs:
                runs["host"].append(host_route(model, prior, host_eng))
        got = rows.cpu().numpy().view(S.STATE_DTYPE).reshape(-1)
        same = all((got[f] == want[f]).all() for f in ("count", "version", "flags")) and (got["balance"].view(np.uint64) == want["balance"].view(np.uint64)).all()
    out = {"aggregates": n, "text_bytes": text_bytes, "rows_equal_the_host_route": bool(same)}
    for route, ts in runs.items():
        out[route] = {"seconds": ts, "median_s": float(np.median(ts)), "spread_s": max(ts) - min(ts), "aggregates_per_s": n / float(np.median(ts))}
    out["encoder"] = {"seconds": enc[1:], "median_s": float(np.median(enc[1:])), "aggregates_per_s": n / float(np.median(enc[1:]))}
    spread = max(out["device"]["spread_s"], out["host"]["spread_s"])
    out["device_wins_by_more_than_either_spread_in_every_pair"] = all(h - d > spread for h, d in zip(runs["host"], runs["device"]))
    out["host_over_device_median"] = out["host"]["median_s"] / out["device"]["median_s"]
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print(json.dumps({"pairs": pairs, "host_route": "store.restore(prior=...): intern + state_to_fixed per aggregate + one H2D copy; JSON parsing not charged",
                      "counter": run("counter", n, pairs), "bank_account": run("bank_account", n, pairs)}))
