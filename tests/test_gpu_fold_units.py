"""-m gpu: the three run-time compiled programs (v1 flat, v1 lanes, v2 slots) share one module cache (csrc/rtc_module.hip).

One small log for every test: 130 aggregates (two full 64-lane groups and a partial one) of 0..40 events (lanes cross a
16-event tile, some rows are empty) and one aggregate of 100 events, which SURGE_REPLAY_CHUNK_T=16 makes CHUNKED and
TILED cut.  Event types 0..3 mean something to the built-in v1 schema and to the TwoCounters slot schema alike.  States
are compared with the CPU oracle byte for byte, as tests/test_gpu_parity.py does.  The `detail` texts are the ones the
library reported before its module caches became one; behind "by " it names whichever libhiprtc (or disk cache) served."""
import numpy as np
import pytest

from oracle import oracle
from surge_amd import schema as S
from surge_amd.replay import ReplayEngine
from test_slots import TWO_COUNTERS

pytestmark = pytest.mark.gpu

FLAT_COMPILED = "flat kernel compiled for the op table by "
LANES_COMPILED = "lane kernels compiled for the op table; "
SLOTS_COMPILED = "compiled by "
DISABLED = "disabled by SURGE_REPLAY_RTC=0"
FLAT_DISABLED = "v1 schema, ahead-of-time kernels interpret the op table: " + DISABLED
LANES_DISABLED = "lane kernels ahead of time (" + DISABLED + "); " + FLAT_DISABLED


@pytest.fixture(scope="module")
def log():
    rng = np.random.default_rng(11)
    lens = np.arange(130, dtype=np.int64) % 41
    lens[77] = 100
    so = np.zeros(131, np.int64)
    np.cumsum(lens, out=so[1:])
    n = int(so[-1])
    ev = np.zeros(n, dtype=S.EVENT_DTYPE)
    ev["type"] = rng.choice([0, 1, 2, 3], size=n, p=[0.1, 0.45, 0.44, 0.01])
    ev["seq"] = rng.integers(-(1 << 31), 1 << 31, size=n)
    ev["raw"] = (rng.integers(-(1 << 31), 1 << 31, size=n).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    exp = {"v1": oracle.fold_csr(so, ev).tobytes(), "v2": oracle.fold_csr_v2(so, ev, TWO_COUNTERS).tobytes()}
    for e in exp.values():
        assert len(e) == 130 * 64
    return so, ev, exp


@pytest.fixture(autouse=True)
def cut_at_16(monkeypatch):
    monkeypatch.setenv("SURGE_REPLAY_CHUNK_T", "16")
    monkeypatch.delenv("SURGE_REPLAY_RTC", raising=False)
    monkeypatch.delenv("SURGE_REPLAY_RTC_LANES", raising=False)


def folds(eng, log, algos, want):
    so, ev, exp = log
    eng.load_csr(so, ev)
    for algo in algos:
        eng.fold(algo)
        assert eng.stats().last_algo == algo
        assert eng.snapshot().tobytes() == exp[want], f"algo {algo} differs from the oracle"
    if S.ALGO_CHUNKED in algos:
        assert eng.layout_info().cut_aggregates > 0  # the 100-event aggregate, and every other row past 16 events


def three_kinds(monkeypatch, log):
    """(kernel_info of) a v1 handle folding FLAT, a v1 handle with the lane kernels opted in folding SORTED and CHUNKED, a
    v2 handle folding SLOTS and TILED — every state held to the oracle on the way."""
    infos = {}
    with ReplayEngine() as flat:
        folds(flat, log, (S.ALGO_FLAT,), "v1")
        infos["flat"] = flat.kernel_info()
        monkeypatch.setenv("SURGE_REPLAY_RTC_LANES", "1")
        with ReplayEngine() as lanes:
            folds(lanes, log, (S.ALGO_SORTED, S.ALGO_CHUNKED), "v1")
            infos["lanes"] = lanes.kernel_info()
            with ReplayEngine(TWO_COUNTERS) as slots:
                folds(slots, log, (S.ALGO_SLOTS, S.ALGO_TILED), "v2")
                infos["slots"] = slots.kernel_info()
    return infos


def test_three_programs_share_one_module_cache(monkeypatch, log):
    infos = three_kinds(monkeypatch, log)
    assert all(i["specialised"] for i in infos.values()), infos
    assert infos["flat"]["detail"].startswith(FLAT_COMPILED) and len(infos["flat"]["detail"]) > len(FLAT_COMPILED)
    assert infos["lanes"]["detail"].startswith(LANES_COMPILED + FLAT_COMPILED)
    assert infos["slots"]["detail"].startswith(SLOTS_COMPILED) and len(infos["slots"]["detail"]) > len(SLOTS_COMPILED)


def test_a_second_handle_with_the_same_op_table_is_a_cache_hit(log):
    with ReplayEngine() as first, ReplayEngine() as second:
        folds(first, log, (S.ALGO_FLAT,), "v1")
        a = first.kernel_info()
        folds(second, log, (S.ALGO_FLAT,), "v1")
        b = second.kernel_info()
    assert a["specialised"] and b["specialised"]
    # the module's own figure, handed out again: two compiles (or two loads from the disk cache) would not take the same time
    assert b["compile_ms"] == a["compile_ms"] and a["compile_ms"] > 0.0
    assert b["detail"] == a["detail"] and a["detail"].startswith(FLAT_COMPILED)


def test_with_run_time_compilation_off_all_three_fall_back_to_the_ahead_of_time_kernels(monkeypatch, log):
    monkeypatch.setenv("SURGE_REPLAY_RTC", "0")
    infos = three_kinds(monkeypatch, log)
    assert not any(i["specialised"] for i in infos.values()), infos
    assert all(i["compile_ms"] == 0.0 for i in infos.values())
    assert infos["flat"]["detail"] == FLAT_DISABLED
    assert infos["lanes"]["detail"] == LANES_DISABLED
    assert infos["slots"]["detail"] == DISABLED
