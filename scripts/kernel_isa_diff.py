#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code in two directories of hipcc objects (the evidence a refactor that only
moves kernels between translation units leaves with its change): every __global__ kernel of OLD has to exist in exactly one
object of NEW with the same instructions (llvm-objdump -d; addresses, encodings and the pc-relative distance to a table in
.rodata stripped) and the same vgpr / sgpr / LDS /
scratch figures in the code object's metadata.  Kernels are matched by demangled name with namespaces stripped, so a move
into a named namespace is not a difference.

    kernel_isa_diff.py OLD_DIR NEW_DIR [--may-differ SUBSTRING ...] [--gone SUBSTRING ...] [--renamed OLD=NEW ...]

Exit status 0 when every kernel outside --may-differ / --gone is identical; a kernel of --may-differ may not need more VGPRs
or scratch than before.  The diff of a kernel that differs is printed with register numbers and branch distances masked (an
argument that goes away renumbers the registers behind it: that is not the change one wants to read)."""
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def plain(names):
    out = run("c++filt", *names).split("\n")[:len(names)] if names else []
    return [re.sub(r"\b(?:\w+::)+|\(anonymous namespace\)::", "", n) for n in out]


def kernels_of(obj_dir):
    """{plain name: (object, instruction lines, metadata dict)} over every object of the directory"""
    found = {}
    for obj in sorted(glob.glob(os.path.join(obj_dir, "*.o"))):
        with tempfile.TemporaryDirectory() as tmp:
            link = os.path.join(tmp, os.path.basename(obj))
            os.symlink(os.path.abspath(obj), link)
            run(f"{LLVM}/llvm-objdump", "--offloading", link, cwd=tmp)
            for co in glob.glob(os.path.join(tmp, "*gfx950")):
                syms = run(f"{LLVM}/llvm-readelf", "-sW", co)
                kds = list(dict.fromkeys(m.group(1) for m in re.finditer(r"\s(\S+)\.kd$", syms, re.M)))  # (.dynsym and .symtab list them both)
                notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
                meta = {}
                for entry in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
                    name = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
                    if name:
                        meta[name.group(1)] = {k: int(re.search(rf"\{k}:\s+(\d+)", entry).group(1)) for k in META}
                body, cur = {}, None
                for line in run(f"{LLVM}/llvm-objdump", "-d", co).split("\n"):
                    head = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                    if head:
                        cur = body.setdefault(head.group(1), [])
                    elif cur is not None and line.startswith("\t") and line.strip() != "...":  # ("...": zero padding behind a section's last kernel)
                        text = re.sub(r"\s+", " ", line.split("//")[0]).strip()
                        if cur and cur[-1].startswith("s_getpc_b64"):  # the distance to a table in .rodata: an address like any other
                            text = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", text)
                        cur.append(text)
                for sym, name in zip(kds, plain(kds)):
                    found.setdefault(("rocprim:: " if "rocprim" in sym else "") + name, []).append((os.path.basename(obj), body[sym], meta[sym]))
    return found


def main(argv):
    args, may_differ, gone, renamed, mode = [], [], [], [], None
    for a in argv:
        if a in ("--may-differ", "--gone", "--renamed"):
            mode = {"--may-differ": may_differ, "--gone": gone, "--renamed": renamed}[a]
        elif mode is not None:
            mode.append(a)
        else:
            args.append(a)
    old, new = kernels_of(args[0]), kernels_of(args[1])
    for was, now in (r.split("=") for r in renamed):
        old = {k.replace(was, now): v for k, v in old.items()}
    bad, library = 0, {}
    for name in sorted(set(old) | set(new)):
        short = name if len(name) < 110 else name[:107] + "..."
        if name not in new or name not in old:
            expected = name in old and any(g in name for g in gone)
            bad += 0 if expected else 1
            print(f"{'gone     ' if name in old else 'NEW      '} {short}" + ("" if expected or name not in old else "   <-- MISSING"))
            continue
        if len(new[name]) != 1 or len(old[name]) != 1:
            bad += 1
            print(f"AMBIGUOUS {short}: in {[o for o, _, _ in old[name]]} and {[o for o, _, _ in new[name]]}")
            continue
        (o_obj, o_ins, o_meta), (n_obj, n_ins, n_meta) = old[name][0], new[name][0]
        same = o_ins == n_ins and o_meta == n_meta
        figures = " ".join(f"{k[1:].split('_')[0]}={o_meta[k]}" + ("" if o_meta[k] == n_meta[k] else f"->{n_meta[k]}") for k in META)
        if same and name.startswith("rocprim:: "):  # the library's instantiations: counted, not listed
            library[(o_obj, n_obj)] = library.get((o_obj, n_obj), 0) + 1
            continue
        print(f"{'identical' if same else 'DIFFERS  '} {short}\n          {o_obj} -> {n_obj}: {len(o_ins)} -> {len(n_ins)} instructions, {figures}")
        if not same:
            allowed = any(m in name for m in may_differ)
            grew = n_meta[".vgpr_count"] > o_meta[".vgpr_count"] or n_meta[".private_segment_fixed_size"] > o_meta[".private_segment_fixed_size"]
            bad += 0 if allowed and not grew else 1
            def mask(ins):
                return [re.sub(r"\b([sv])(\d+|\[\d+:\d+\])", r"\1#", re.sub(r"^(s_c?branch\w*) \d+$", r"\1 #", i)) for i in ins]
            raw = sum(1 for d in difflib.ndiff(o_ins, n_ins) if d[0] in "+-")
            print(f"            {raw} lines differ as they are; with register numbers and branch distances masked:")
            for d in difflib.unified_diff(mask(o_ins), mask(n_ins), "old", "new", lineterm="", n=1):
                print("            " + d)
    for (o_obj, n_obj), n in library.items():
        print(f"identical {n} kernels of rocPRIM, {o_obj} -> {n_obj}")
    print(f"{len(old)} kernels in {args[0]}, {len(new)} in {args[1]}: " + ("OK" if bad == 0 else f"{bad} unexpected difference(s)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
