"""The host framer's trace (tests/ingest_trace.py) over a host-only build of the library: the same in two fresh processes, and it
reaches every message the framer's units (surge_amd/csrc: ingest.cpp, ingest_group.cpp, ingest_internal.h, crc32c.cpp) can hand to a
caller."""
import os
import re
import subprocess
import sys

import pytest

import ingest_trace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 1

FRAMER_UNITS = ("ingest.cpp", "ingest_group.cpp", "ingest_internal.h", "crc32c.cpp")

# Messages no caller can provoke from outside, each with the reason.  Everything else in the framer's units that reads like a message
# (a string literal with a space in it) must appear in the trace: a new message without a case in ingest_trace.py fails.
UNREACHABLE = {
    "out of host memory": "an allocation has to fail",
    "out of host memory while decoding": "an allocation has to fail",
    "out of host memory for the group's slab": "an allocation has to fail",
    "the partitions' carried sections outgrew the room surge_ingest_group_receive_buffer left for them":
        "cannot happen: nothing is fed between receive_buffer and the feed that checks it",
    "the group's slice for this partition is full":
        "only a group's member reports it, and the group answers it by running the feed again with four times the room, up to 256 x: "
        "an LZ4 block expands at most 255 x, so the last trial always fits and the message never leaves the group",
}


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    lib = ingest_trace.build_host_library(str(tmp_path_factory.mktemp("ingest_trace") / "libsurge_host.so"))
    cmd = [sys.executable, os.path.join(HERE, "ingest_trace.py"), lib, str(SEED)]
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for _ in range(2)]
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    return [out for out, _ in outs]


def source_messages():
    src = ""
    for unit in FRAMER_UNITS:
        with open(os.path.join(ROOT, "surge_amd", "csrc", unit)) as f:
            src += re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S) + "\n"
    # (preprocessor lines and static_asserts speak to the compiler, not to a caller)
    lines = [ln for ln in src.split("\n") if not ln.lstrip().startswith(("#", "static_assert"))]
    found = []
    for ln in lines:
        code, in_str, k = [], False, 0
        while k < len(ln):  # cut the // comment off, minding string literals
            if ln[k] == "\\" and in_str:
                k += 2
                continue
            if ln[k] == '"':
                in_str = not in_str
            elif not in_str and ln.startswith("//", k):
                break
            k += 1
        code = ln[:k]
        found += re.findall(r'"((?:[^"\\]|\\.)*)"', code)
    return sorted({m for m in found if " " in m.strip() and len(re.findall(r"[A-Za-z]", m)) >= 2})


def test_two_fresh_processes_print_the_same_trace(traces):
    a, b = traces
    assert a == b
    assert a.count("\n") > 2000 and " rc=0 " in a and " rc=-7 " in a


def test_the_trace_reaches_every_message_the_framer_can_return(traces):
    messages = source_messages()
    assert len(messages) >= 35, messages  # (the collection itself works: the framer's units held 42 when this was written)
    for m in UNREACHABLE:
        assert m in messages, f"{m!r} is listed as unreachable but none of {FRAMER_UNITS} holds it any longer"
    missing = [m for m in messages if m not in UNREACHABLE and m not in traces[0]]
    assert not missing, missing
