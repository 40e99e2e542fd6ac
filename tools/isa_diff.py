#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of liblamslide_hip.so the same?  (A host-side refactor must leave them so; no GPU needed.)

Compares per kernel symbol, not per file (two builds of one source differ as files): the sets of symbol names, every symbol's
instruction text (tools/isa_scan.py: disassemble + parse; the s_nop padding behind a kernel's last instruction is not part of it) and
the kernels' resource notes (registers, LDS, scratch ...).

Usage: tools/isa_diff.py A.so B.so   -> one line per difference, exit status 1 if there is any."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_scan


def notes_by_object(so_path):
    """[[(kernel symbol, its metadata lines), ...] of one code object, ...] from llvm-readelf --notes of the extracted code objects: one per
    translation unit, in link order (lam_slide_amd/_lib.py UNITS)"""
    with tempfile.TemporaryDirectory() as td:
        dst = os.path.join(td, "lib.so")
        with open(so_path, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(isa_scan.LLVM, "llvm-objdump"), "--offloading", dst], check=True, capture_output=True, cwd=td)
        objs = sorted((f for f in os.listdir(td) if "gfx950" in f), key=lambda f: int(f.split(".")[2]))  # lib.so.<bundle index>.hipv4-...
        texts = [subprocess.run([os.path.join(isa_scan.LLVM, "llvm-readelf"), "--notes", os.path.join(td, obj)], check=True, capture_output=True,
                                text=True).stdout for obj in objs]
    keep = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
            "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")
    out = []
    for text in texts:
        out.append([])
        for block in text.split(".agpr_count:")[1:]:  # (the first key of every kernel's entry)
            fields = dict(re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + block))
            out[-1].append((fields["symbol"], {k: fields.get(k) for k in keep}))
    return out


def notes(so_path):
    """{kernel symbol: its metadata lines} of the whole library"""
    return {sym: fields for obj in notes_by_object(so_path) for sym, fields in obj}


def code_text(insts):
    """A kernel's instruction text without the padding behind it: the s_nop lines after its last instruction fill the code object's
    section up to its alignment behind whichever kernel comes last in a unit, so they move when kernels move between units."""
    text = [i.text for i in insts]
    while text and insts[len(text) - 1].op == "s_nop":
        text.pop()
    return text


def main():
    a, b = sys.argv[1], sys.argv[2]
    ka, kb = (isa_scan.parse(isa_scan.disassemble(p)) for p in (a, b))
    bad = [f"only in {a}: {n}" for n in sorted(set(ka) - set(kb))] + [f"only in {b}: {n}" for n in sorted(set(kb) - set(ka))]
    bad += [f"instructions differ: {n}" for n in sorted(set(ka) & set(kb)) if code_text(ka[n]) != code_text(kb[n])]
    na, nb = notes(a), notes(b)
    bad += [f"resource notes differ: {n}" for n in sorted(set(na) | set(nb)) if na.get(n) != nb.get(n)]
    print("\n".join(bad) if bad else f"{len(ka)} symbols, {len(na)} kernels with notes: instruction text and resource notes equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
