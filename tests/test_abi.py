"""The C-ABI shared library: builds, loads, exports exactly what include/surge_replay.h declares,
and fails loudly (no CPU fallback) when there is no GPU."""
import ctypes
import os
import re

import pytest

from surge_amd import _native
from surge_amd.schema import CSchema, DEFAULT_ALGEBRA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name="surge_replay.h", prefix="surge_(?:replay|format)_"):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]*)\s*\(", text)))


def test_library_builds_for_gfx950_and_loads():
    path = _native.build()
    assert os.path.exists(path)
    lib = _native.load()
    assert lib is not None


def test_exports_match_the_header():
    lib = _native.load()
    declared = header_symbols()
    assert declared == sorted(_native.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in surge_replay.h but not exported"


def test_ingest_exports_match_their_header():
    lib = _native.load()
    declared = header_symbols("surge_ingest.h", "surge_(?:ingest|event_json|crc32c|lz4|xxh32|device_decoder|parse_f64|replay_append_decoded|replay_stage_decoded)")
    assert declared == sorted(_native.INGEST_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in surge_ingest.h but not exported"


def test_snapshot_writer_exports_match_their_header():
    lib = _native.load()
    declared = header_symbols("surge_snapshot.h", "surge_(?:snapshot_writer|device_framer)")
    assert declared == sorted(_native.SNAPSHOT_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in surge_snapshot.h but not exported"


def test_make_lib_builds_the_same_library_as_the_python_build(tmp_path):
    """`make lib` is the recipe INTEGRATION.md gives JNI / C / C++ hosts.  It reads the same source list as
    _native.build() (surge_amd/csrc/SOURCES) and its output exports every symbol the three headers declare."""
    import shutil
    import subprocess

    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("make / hipcc not present")
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "surge_amd/csrc/SOURCES" in mk and re.search(r"^SRC\s*:=.*SOURCES", mk, re.M), "the Makefile must take its sources from csrc/SOURCES"
    for src in _native.SOURCES:
        assert os.path.exists(os.path.join(_native.CSRC, src))
    lib = str(tmp_path / "libsurge_replay_make.so")
    res = subprocess.run(["make", "-j8", "lib", "LIB=" + lib, "OBJ=" + str(tmp_path / "obj")], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (surge_[a-z0-9_]+)", nm))
    missing = [n for n in _native.EXPORTS + _native.INGEST_EXPORTS + _native.SNAPSHOT_EXPORTS if n not in exported]
    assert not missing, f"`make lib` output lacks {missing}"


def test_a_libhiprtc_candidate_that_fails_to_load_does_not_take_the_process_down():
    """a dlopen failure used to call dlerror() twice and build a std::string from NULL.  A process with
    a wrong SURGE_HIPRTC_LIBRARY must survive the failed candidate and go on to the next one."""
    import subprocess
    import sys

    code = (
        "import ctypes\n"
        "from surge_amd import _native\n"
        "lib = _native.load()\n"
        "from tests.test_slots import LEDGER\n"
        "sc = LEDGER.to_c(); n = ctypes.c_int64(0)\n"
        "rc = lib.surge_replay_compile_schema_v2(ctypes.byref(sc), b'gfx950', None, 0, ctypes.byref(n))\n"
        "print('RC', rc, n.value)\n"
    )
    env = dict(os.environ, SURGE_HIPRTC_LIBRARY="/nonexistent/libhiprtc.so", SURGE_REPLAY_CACHE="0")  # (a cache hit would not load libhiprtc at all)
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr  # 139 = the segfault
    assert "RC 0 " in res.stdout or "RC -" in res.stdout, res.stdout + res.stderr


def test_compiled_code_objects_are_kept_on_disk_and_a_damaged_file_is_compiled_again(tmp_path, monkeypatch):
    """the 0.6 - 1 s hiprtc compile of a schema's kernels is paid once per machine — the code object is
    stored under SURGE_REPLAY_CACHE_DIR keyed by the text compiled, the target and the runtime's version; a file that does not
    check out (truncated, flipped byte) is ignored and rewritten; SURGE_REPLAY_CACHE=0 turns the cache off."""
    import time

    from tests.test_slots import LEDGER

    lib = _native.load()
    sc = LEDGER.to_c()
    monkeypatch.setenv("SURGE_REPLAY_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("SURGE_REPLAY_CACHE", raising=False)

    def compile_once():
        n = ctypes.c_int64(0)
        t0 = time.perf_counter()
        rc = lib.surge_replay_compile_schema_v2(ctypes.byref(sc), b"gfx950", None, 0, ctypes.byref(n))
        if rc != 0:
            pytest.skip("no libhiprtc here")
        buf = ctypes.create_string_buffer(n.value)
        assert lib.surge_replay_compile_schema_v2(ctypes.byref(sc), b"gfx950", buf, n.value, ctypes.byref(n)) == 0
        return buf.raw[: n.value], time.perf_counter() - t0

    first, t_first = compile_once()
    files = sorted(tmp_path.glob("*.co"))
    assert len(files) == 1 and files[0].read_bytes()[24:] == first and files[0].read_bytes()[:8] == b"SRGCO1\0\0"
    again, t_again = compile_once()
    assert again == first and t_again < t_first / 3  # served from the file
    blob = bytearray(files[0].read_bytes())
    blob[len(blob) // 2] ^= 1
    files[0].write_bytes(bytes(blob))
    assert compile_once()[0] == first and files[0].read_bytes()[24:] == first  # compiled again, stored again
    files[0].write_bytes(bytes(blob[:100]))
    assert compile_once()[0] == first and files[0].read_bytes()[24:] == first
    monkeypatch.setenv("SURGE_REPLAY_CACHE", "0")
    files[0].unlink()
    assert compile_once()[0] == first and not list(tmp_path.glob("*.co"))
    monkeypatch.delenv("SURGE_REPLAY_CACHE")
    # the cache only lives in a directory that is this user's own and nobody else's to write — a directory others can
    # write to, or a symbolic link to one, is not used at all (a planted <key>.co would be loaded as GPU code unseen by hiprtc);
    # neither is a cached FILE that is a link or writable by others
    shared = tmp_path / "shared"
    shared.mkdir()
    shared.chmod(0o777)
    monkeypatch.setenv("SURGE_REPLAY_CACHE_DIR", str(shared))
    assert compile_once()[0] == first and not list(shared.glob("*.co"))
    link = tmp_path / "link"
    private = tmp_path / "private"
    private.mkdir(mode=0o700)
    link.symlink_to(private)
    monkeypatch.setenv("SURGE_REPLAY_CACHE_DIR", str(link))
    assert compile_once()[0] == first and not list(private.glob("*.co"))
    monkeypatch.setenv("SURGE_REPLAY_CACHE_DIR", str(private))
    assert compile_once()[0] == first
    (stored,) = list(private.glob("*.co"))
    assert stored.stat().st_mode & 0o077 == 0
    planted = bytearray(stored.read_bytes())
    stored.chmod(0o666)  # somebody else could have written it: not trusted, compiled again (and replaced by a private file)
    assert compile_once()[0] == first and list(private.glob("*.co"))[0].stat().st_mode & 0o022 == 0


def test_default_schema_matches_python_mirror():
    lib = _native.load()
    s = CSchema()
    assert lib.surge_replay_default_schema(ctypes.byref(s)) == 0
    mine = DEFAULT_ALGEBRA.to_c()
    assert bytes(s) == bytes(mine)


def test_bad_schema_is_rejected_before_touching_a_device():
    lib = _native.load()
    s = DEFAULT_ALGEBRA.to_c()
    s.state_size = 32
    h = ctypes.c_void_p()
    assert lib.surge_replay_create(ctypes.byref(s), 0, ctypes.byref(h)) == -5  # SURGE_E_UNSUPPORTED
    assert b"64-byte" in lib.surge_replay_last_error(None)
    s = DEFAULT_ALGEBRA.to_c()
    s.desc[0] = 1 << 20
    assert lib.surge_replay_create(ctypes.byref(s), 0, ctypes.byref(h)) == -5


def test_no_gpu_means_loud_failure_not_a_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("this box has a GPU; the no-device path is covered on the build container")
    from surge_amd.replay import ReplayEngine, ReplayError

    with pytest.raises(ReplayError) as ei:
        ReplayEngine()
    assert ei.value.status == -3  # SURGE_E_DEVICE


def test_product_code_never_touches_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use oracle/."""
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|liboracle|surge_fold_oracle|\boracle_[a-z_]+\s*\(", re.M)
    pkg = os.path.join(ROOT, "surge_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not pat.search(text), f"{f}: product code must not import, link or call the oracle"


def _build_c_demo(tmp_path):
    import subprocess

    exe = str(tmp_path / "c_host_demo")
    lib_dir = os.path.join(ROOT, "surge_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_host_demo.c"),
           "-L" + lib_dir, "-lsurge_replay", "-Wl,-rpath," + lib_dir, "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env)


def test_plain_c_host_links_and_fails_loudly_without_a_gpu(tmp_path):
    """The boundary is a C ABI: a C99 program with no Python/torch in the process links and runs it."""
    import torch

    _native.build()
    res = _build_c_demo(tmp_path)
    if torch.cuda.is_available():
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 2 and "no CPU fallback" in res.stdout


@pytest.mark.gpu
def test_plain_c_host_replays_the_reference_known_answers(tmp_path):
    res = _build_c_demo(tmp_path)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("PASS") == 8 and "FAIL" not in res.stdout


def _build_cpp_demo(tmp_path):
    import subprocess

    exe = str(tmp_path / "cpp_host_demo")
    lib_dir = os.path.join(ROOT, "surge_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cpp_host_demo.cpp"),
           "-L" + lib_dir, "-lsurge_replay", "-Wl,-rpath," + lib_dir, "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env)


def test_cpp_host_mirror_compiles_and_partitions_like_the_reference(tmp_path):
    """include/surge_replay.hpp (the compiled-language mirror of the plugin traits) builds warning-free; its
    partitioner (CPU entry point) reproduces the pinned stringHash answers; the store fails loudly without a GPU."""
    import torch

    _native.build()
    res = _build_cpp_demo(tmp_path)
    assert res.stdout.count("PASS") >= 4 and "FAIL" not in res.stdout, res.stdout + res.stderr
    if torch.cuda.is_available():
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 2 and "no CPU fallback" in res.stdout


@pytest.mark.gpu
def test_cpp_host_mirror_serves_get_aggregate_bytes_from_the_gpu_fold(tmp_path):
    res = _build_cpp_demo(tmp_path)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL PASS" in res.stdout and res.stdout.count("PASS  ") == 11 and "FAIL" not in res.stdout


def _build_jni_harness(tmp_path):
    import subprocess

    exe = str(tmp_path / "jni_harness")
    lib_dir = os.path.join(ROOT, "surge_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "jni_mock"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "integration", "jni", "surge_replay_jni.c"), os.path.join(ROOT, "tests", "jni_mock", "jni_harness.c"),
           "-L" + lib_dir, "-lsurge_replay", "-Wl,-rpath," + lib_dir, "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([exe], capture_output=True, text=True, env=env)


def test_jni_shim_compiles_and_turns_a_missing_gpu_into_an_ioexception(tmp_path):
    """N4: integration/jni/surge_replay_jni.c, compiled unchanged against a stand-in jni.h (no JDK here) and driven
    by a fake JNIEnv: the host-side partitioner answers, and create() without a GPU leaves a pending IOException."""
    import torch

    _native.build()
    res = _build_jni_harness(tmp_path)
    assert "FAIL" not in res.stdout and res.stdout.count("PASS  ") >= 4, res.stdout + res.stderr
    if torch.cuda.is_available():
        assert res.returncode == 0, res.stdout + res.stderr
    else:
        assert res.returncode == 2 and "no CPU fallback" in res.stdout


@pytest.mark.gpu
def test_jni_shim_replays_the_reference_known_answers_through_direct_buffers(tmp_path):
    res = _build_jni_harness(tmp_path)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL PASS" in res.stdout and res.stdout.count("PASS  ") == 26 and "FAIL" not in res.stdout


def test_the_fake_jnienv_harness_drives_every_jni_export():
    import re

    shim = open(os.path.join(ROOT, "integration", "jni", "surge_replay_jni.c")).read()
    harness = open(os.path.join(ROOT, "tests", "jni_mock", "jni_harness.c")).read()
    scala = open(os.path.join(ROOT, "integration", "scala", "NativeReplay.scala")).read()
    exports = re.findall(r"Java_surge_replay_gpu_NativeReplay_(\w+)\(", shim)
    assert len(exports) >= 19 and len(set(exports)) == len(exports)
    for name in exports:
        assert harness.count(f"Java_surge_replay_gpu_NativeReplay_{name}(env") >= 1, f"{name} is never called by the harness"
        assert re.search(rf"@native def {name}\(", scala), f"{name} has no @native declaration in NativeReplay.scala"


def test_device_framer_fails_loudly_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("this box has a GPU; the no-device path is covered on the build container")
    from surge_amd.snapshot import DeviceFramer

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceFramer(4)


def test_a_v1_schema_compiles_its_flat_kernel_for_gfx950_without_a_gpu_and_a_narrow_schema_to_fewer_vector_instructions(tmp_path):
    """surge_replay_compile_schema: the flat fold kernel's own device source (csrc/fold_flat_device.h) compiled by hiprtc with
    the schema's op table as compile-time masks — what a v1 handle runs from its first flat fold on.  Checkable on a build
    machine; and the point of it is visible in the code objects: the Counter fixture's schema (count and version only)
    compiles to fewer vector instructions than the built-in schema that uses every field — although every segment end
    carries a longer store (the untouched fields come from the defaults or the prior state) — and to half the cross-lane
    shuffles (the untouched fields are not in the scan)."""
    import shutil
    import subprocess

    from fixture_models import COUNTER_ALGEBRA

    lib = _native.load()
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    valu = {}
    for name, algebra in (("default", DEFAULT_ALGEBRA), ("counter", COUNTER_ALGEBRA)):
        sc = algebra.to_c()
        n = ctypes.c_int64()
        assert lib.surge_replay_compile_schema(ctypes.byref(sc), b"gfx950", None, 0, ctypes.byref(n)) == 0, lib.surge_replay_last_error(None).decode()
        buf = ctypes.create_string_buffer(n.value)
        assert lib.surge_replay_compile_schema(ctypes.byref(sc), b"gfx950", buf, n.value, ctypes.byref(n)) == 0
        assert buf.raw[:4] == b"\x7fELF" and b"surge_v1_flat8" in buf.raw and b"surge_v1_flat16" in buf.raw
        assert lib.surge_replay_compile_schema(ctypes.byref(sc), b"gfx950", buf, 16, ctypes.byref(n)) == -1  # too small
        if os.path.exists(objdump):
            co = tmp_path / f"{name}.co"
            co.write_bytes(buf.raw[: n.value])
            asm = subprocess.run([objdump, "-d", str(co)], capture_output=True, text=True, check=True).stdout
            body = asm[asm.index("<surge_v1_flat16>:"):]
            notes = subprocess.run([os.path.join(os.path.dirname(objdump), "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
            assert "surge_v1_flat16" in notes and not re.search(r"\.(private_segment_fixed_size|vgpr_spill_count):\s+[1-9]", notes), "the compiled flat kernel spills"
            ops = [l.split()[0] for l in body.splitlines() if l.split()[:1]]
            valu[name] = (sum(1 for o in ops if o.startswith("v_")), sum(1 for o in ops if o.startswith("ds_bpermute")))
    if valu:
        assert valu["counter"][0] < 0.9 * valu["default"][0] and valu["counter"][1] < 0.6 * valu["default"][1], valu
    bad = DEFAULT_ALGEBRA.to_c()
    bad.state_size = 48
    assert lib.surge_replay_compile_schema(ctypes.byref(bad), b"gfx950", None, 0, ctypes.byref(n)) != 0


def test_no_kernel_of_the_library_spills_to_scratch(tmp_path):
    """The code objects inside libsurge_replay.so (llvm-objdump --offloading), kernel by kernel from their metadata notes: a
    kernel of this library that starts to spill registers to scratch memory loses its place on the roofline silently — this
    fails loudly instead.  (Until round 5 fold_chunked_kernel<16> was the tolerated exception: 256 VGPRs, 10 of them spilled —
    loop-invariant load addresses the compiler hoisted three times over; kept as kClasses opaque bases it needs 204 and no
    scratch.)  rocPRIM's kernels are the library's own business."""
    import shutil
    import subprocess

    tools = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{tools}/llvm-objdump") and os.path.exists(f"{tools}/llvm-readelf")):
        pytest.skip("no llvm-objdump / llvm-readelf")
    shutil.copy(_native.build(), tmp_path / "lib.so")
    subprocess.run([f"{tools}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    objects = sorted(p for p in os.listdir(tmp_path) if p.endswith("gfx950"))
    assert len(objects) >= 8, objects  # one per translation unit with device code
    kernels = {}
    for name in objects:
        notes = subprocess.run([f"{tools}/llvm-readelf", "--notes", name], cwd=tmp_path, capture_output=True, text=True, check=True).stdout
        cur = None
        for line in notes.splitlines():
            m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_spill_count|vgpr_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = kernels.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = int(m.group(2))
    ours = {k: v for k, v in kernels.items() if "rocprim" not in k and "private_segment_fixed_size" in v}
    assert len(ours) >= 70, len(ours)
    for hot in ("fold_sorted_pf_kernelILi16", "fold_sorted_kernelILi16", "fold_rows_kernelILi8", "fold_tiled_kernelILi2", "fold_kernelILi1ELi16", "section_kernel", "lz4_exec_kernel"):
        assert any(hot in k for k in ours), hot
    spilling = {k: v for k, v in ours.items() if v["private_segment_fixed_size"] or v.get("vgpr_spill_count", 0)}
    assert not spilling, spilling
    chunked = [v for k, v in ours.items() if "fold_chunked_kernelILi16" in k]
    assert chunked and all(v["vgpr_count"] <= 256 for v in chunked), chunked
    # The register budgets the resident-wave counts of DESIGN §3 / §6e rest on (a kernel that outgrows its budget keeps its
    # results and silently loses waves per CU): 16-event lane kernels two waves per SIMD (<= 256), 8-event ones three
    # (<= 168); the record kernel's three narrow workgroup sizes six waves per SIMD (<= 80: 8 batches per CU), its 256-lane
    # one five (<= 96); the LZ4 passes 24 / 8 waves per CU by their LDS, which 96 registers do not undercut.
    budgets = (("fold_sorted_pf_kernelILi16", 256), ("fold_sorted_pf_kernelILi8", 168), ("fold_chunked_kernelILi8", 168), ("section_kernelILi64", 80),
               ("section_kernelILi128", 80), ("section_kernelILi192", 80), ("section_kernelILi256", 96), ("lz4_exec_kernel", 96), ("lz4_parse_kernel", 96))
    for name, limit in budgets:
        hit = [v["vgpr_count"] for k, v in ours.items() if name in k]
        assert hit and max(hit) <= limit, (name, hit, limit)


def test_the_lane_kernels_compile_for_a_v1_schema_without_a_gpu_and_without_scratch(tmp_path, monkeypatch):
    """The V1_LANES program (SORTED / CHUNKED / ROWS compiled for one op table; opt-in, SURGE_REPLAY_RTC_LANES=1) builds for
    gfx950 on a machine without a GPU; its code object lands in the disk cache.  None of its kernels touches scratch, the
    8-event sorted walk fits four waves per SIMD (<= 128 VGPRs) and the Counter fixture's schema compiles to well under half
    the vector instructions of the built-in one (count and version are all its walk carries)."""
    import subprocess

    from fixture_models import COUNTER_ALGEBRA

    tools = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{tools}/llvm-objdump") and os.path.exists(f"{tools}/llvm-readelf")):
        pytest.skip("no llvm-objdump / llvm-readelf")
    lib = _native.load()
    monkeypatch.setenv("SURGE_REPLAY_RTC_LANES", "1")
    valu = {}
    for name, algebra in (("default", DEFAULT_ALGEBRA), ("counter", COUNTER_ALGEBRA)):
        cache = tmp_path / name
        cache.mkdir()
        monkeypatch.setenv("SURGE_REPLAY_CACHE_DIR", str(cache))
        sc, n = algebra.to_c(), ctypes.c_int64()
        assert lib.surge_replay_compile_schema(ctypes.byref(sc), b"gfx950", None, 0, ctypes.byref(n)) == 0, lib.surge_replay_last_error(None).decode()
        found = False
        for co in sorted(cache.glob("*.co")):
            elf = tmp_path / (co.name + ".elf")
            elf.write_bytes(co.read_bytes()[24:])
            notes = subprocess.run([f"{tools}/llvm-readelf", "--notes", str(elf)], capture_output=True, text=True, check=True).stdout
            if "surge_v1_sorted16" not in notes:
                continue
            found = True
            for k in ("surge_v1_sorted8", "surge_v1_sorted16", "surge_v1_chunked8", "surge_v1_chunked16", "surge_v1_rows8", "surge_v1_rows16"):
                assert k in notes, k
            assert not re.search(r"\.(private_segment_fixed_size|vgpr_spill_count):\s+[1-9]", notes), "a compiled lane kernel spills"
            regs = dict(re.findall(r"\.name:\s+(surge_v1_\w+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", notes))
            assert int(regs["surge_v1_sorted8"]) <= 128 and int(regs["surge_v1_sorted16"]) <= 256 and int(regs["surge_v1_chunked16"]) <= 256, regs
            asm = subprocess.run([f"{tools}/llvm-objdump", "-d", str(elf)], capture_output=True, text=True, check=True).stdout
            body = asm[asm.index("<surge_v1_sorted16>:"):asm.index("<surge_v1_sorted32>:")]
            valu[name] = sum(1 for l in body.splitlines() if l.split()[:1] and l.split()[0].startswith("v_"))
        assert found, list(cache.iterdir())
    assert valu["counter"] < 0.75 * valu["default"], valu
