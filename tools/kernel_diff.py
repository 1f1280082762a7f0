#!/usr/bin/env python3
"""Compares the gfx950 kernels of two builds of the library, kernel by kernel: the disassembled instruction text
(addresses and encodings stripped, branch targets renamed to labels numbered in order of appearance) and the metadata a
launch depends on (vgpr_count, sgpr_count, private_segment_fixed_size, group_segment_fixed_size).  A refactor that is
meant to leave the device code alone shows `identical` for every kernel; nothing needs timing then.

    tools/build_prev.sh                          # the parent's library, next to the current one
    python tools/kernel_diff.py lightmotif_amd/csrc/liblightmotif_hip_prev.so lightmotif_amd/csrc/liblightmotif_hip.so

Prints one line per kernel (`identical`, or `differs` with what differs), kernels found on one side only, and a summary;
exit status 1 when anything differs or is missing.  Needs no GPU."""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from kernel_regs import code_objects  # noqa: E402

META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def llvm_tool(name: str) -> str:
    """the LLVM tool that belongs to the hipcc in use: <rocm>/bin/hipcc -> <rocm>/lib/llvm/bin/<name>"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = Path(hipcc).resolve().parent.parent / "lib" / "llvm" / "bin" / name
    if not exe.exists():
        raise RuntimeError(f"{name} not found next to {hipcc} ({exe})")
    return str(exe)


def metadata(elf: Path) -> dict[str, dict[str, int]]:
    notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", str(elf)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.finditer(r"- \.agpr_count:.*?(?=\n\s+- \.agpr_count:|\namdhsa\.target|\Z)", notes, re.S):
        b = block.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", b)
        out[g("name").group(1)] = {k: int(g(k).group(1)) for k in META}
    return out


def instructions(elf: Path, names: set[str]) -> dict[str, list[str]]:
    """kernel -> its instructions as text.  A branch target `<kernel+0x1c4>` becomes `L<n>`, n counting the distinct
    targets of the kernel in order of first use, so that code which merely moved compares equal."""
    dis = subprocess.run([llvm_tool("llvm-objdump"), "-d", "--mcpu=gfx950", str(elf)], capture_output=True, text=True, check=True).stdout
    out: dict[str, list[str]] = {}
    cur, labels = None, {}
    for line in dis.split("\n"):
        m = re.match(r"[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            labels = {}
            if cur:
                out[cur] = []
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        text = line.split("//")[0].strip()  # `//` starts the address and the encoding
        if not text:
            continue
        text = re.sub(r"<[^>]+>", lambda t: "L%d" % labels.setdefault(t.group(0), len(labels)), text)
        # the numeric form of a branch offset sits before its <symbol+offset>; drop it, the label says it all
        text = re.sub(r"\b\d+\s+(L\d+)$", r"\1", text)
        out[cur].append(re.sub(r"\s+", " ", text))
    # What follows a kernel's last instruction is the code object's fill up to the next symbol or, behind the LAST kernel of a
    # translation unit, to the end of the section (`s_nop 0`, and `...` for zero bytes): it changes with the kernel's
    # neighbours, not with the kernel, so a kernel that moved to another unit would otherwise never compare equal.
    for text in out.values():
        while text and text[-1] in ("s_nop 0", "..."):
            text.pop()
    return out


def kernels(lib: Path) -> dict[str, tuple[dict[str, int], list[str]]]:
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(code_objects(lib.read_bytes())):
            f = Path(td) / f"co{i}.elf"
            f.write_bytes(co)
            meta = metadata(f)
            text = instructions(f, {n for n in meta})
            for name, md in meta.items():
                if name in out:
                    raise RuntimeError(f"{lib}: kernel {name} in two code objects")
                out[name] = (md, text.get(name, []))
    return out


def demangle(names: list[str]) -> list[str]:
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(.*", "", n).replace("void ", "") for n in r[:len(names)]]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--quiet", action="store_true", help="print only the kernels that differ or are missing, and the summary")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    names = sorted(set(old) | set(new))
    short = dict(zip(names, demangle(names)))
    same = differ = missing = 0
    for n in sorted(names, key=lambda n: short[n]):
        if n not in old or n not in new:
            missing += 1
            print(f"{'only in new' if n in new else 'only in old':12s} {short[n]}")
            continue
        (mo, to), (mn, tn) = old[n], new[n]
        what = [f"{k} {mo[k]} -> {mn[k]}" for k in META if mo[k] != mn[k]]
        if to != tn:
            first = next((i for i, (x, y) in enumerate(zip(to, tn)) if x != y), min(len(to), len(tn)))
            what.append(f"instructions {len(to)} -> {len(tn)}, first difference at {first}")
        if what:
            differ += 1
            print(f"{'differs':12s} {short[n]}: " + "; ".join(what))
        else:
            same += 1
            if not a.quiet:
                print(f"{'identical':12s} {short[n]}  ({len(tn)} instructions)")
    print(f"{len(names)} kernels: {same} identical, {differ} differ, {missing} on one side only")
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
