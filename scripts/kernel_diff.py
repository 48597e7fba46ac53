"""Compare the gfx950 kernels of two builds, kernel by kernel.

    python scripts/kernel_diff.py OLD_BUILD_DIR NEW_BUILD_DIR      (two build/csrc directories)

For every *.o present in both directories the gfx950 code object is unbundled and, per kernel:
the kernels only in one side are listed; the common ones are compared in instruction text
(llvm-objdump -d without addresses and encodings) and in their metadata note (llvm-readelf --notes:
register and spill counts, LDS / scratch / kernarg sizes, the workgroup size limit). Whole objects
are not compared: kernels are emitted in the order host code first names them, which a rewritten
launcher changes while every kernel stays the same.

Exit 1 on any difference other than a kernel missing on the new side.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_mfma_exec import FUNC, OBJDUMP, code_object  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
CXXFILT = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
          ".max_flat_workgroup_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def metadata(co):
    """-> {kernel symbol without .kd: {field: value}} from the code object's metadata note."""
    out, cur = {}, {}
    for line in run(READELF, "--notes", co).splitlines():
        m = re.match(r"\s*(?:- )?(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if key in FIELDS:
            cur[key] = val
        elif key == ".symbol":          # one per kernel; the keys of a kernel's map are sorted
            cur[".symbol"] = val
        elif key == ".wavefront_size":  # the last key of a kernel's map
            if cur.get(".symbol", "").endswith(".kd"):
                out[cur.pop(".symbol")[:-3]] = cur
            cur = {}
    return out


def instructions(co, kernels):
    """-> {kernel: [instruction text]} of the kernel entry points in the disassembly."""
    out, fn = {}, None
    for line in run(OBJDUMP, "-d", "--mcpu=gfx950", co).splitlines():
        m = FUNC.match(line)
        if m:
            fn = m.group(1) if m.group(1) in kernels else None
            if fn:
                out[fn] = []
        elif fn and line.strip():
            out[fn].append(re.sub(r"^\s*[0-9a-f]+:\s+", "", line.split("//")[0]).strip())
    return out


def kernels_of(obj, tmp):
    sub = tempfile.mkdtemp(dir=tmp)
    co = code_object(obj, sub)
    meta = metadata(co)
    return meta, instructions(co, meta)


def demangle(names):
    """-> {symbol: readable name without the argument list} (the symbol itself without a c++filt)."""
    out = run(CXXFILT, *names).splitlines() if names and CXXFILT else names
    return {k: re.sub(r"^void |\(.*$", "", v) for k, v in zip(names, out)}


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"instruction {i}: '{x}' -> '{y}'"
    return f"{len(a)} -> {len(b)} instructions"


def main(old_dir, new_dir):
    olds = {f for f in os.listdir(old_dir) if f.endswith(".o")}
    news = {f for f in os.listdir(new_dir) if f.endswith(".o")}
    for f in sorted(olds ^ news):
        print(f"{f}: only in the {'old' if f in olds else 'new'} build (not compared)")
    common = gone = added = differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(olds & news):
            try:
                (mo, io), (mn, inn) = kernels_of(os.path.join(old_dir, f), tmp), kernels_of(os.path.join(new_dir, f), tmp)
            except RuntimeError:            # host-only object: no gfx950 bundle
                continue
            both = sorted(set(mo) & set(mn))
            name = demangle(sorted(set(mo) | set(mn)))
            bad = []
            for k in both:
                if io[k] != inn[k]:
                    bad.append(f"   differs in instructions: {name[k]}: {first_diff(io[k], inn[k])}")
                if mo[k] != mn[k]:
                    d = ", ".join(f"{x} {mo[k].get(x)} -> {mn[k].get(x)}" for x in FIELDS if mo[k].get(x) != mn[k].get(x))
                    bad.append(f"   differs in metadata: {name[k]}: {d}")
            only_old, only_new = sorted(set(mo) - set(mn)), sorted(set(mn) - set(mo))
            print(f"{f}: {len(both)} common kernels, {len(both) - len({b.split(': ')[1] for b in bad})} identical; "
                  f"{len(only_old)} only old, {len(only_new)} only new")
            for k in only_old:
                print(f"   only old: {name[k]}")
            for k in only_new:
                print(f"   only new: {name[k]}")
            print("\n".join(bad), end="\n" if bad else "")
            common += len(both)
            gone += len(only_old)
            added += len(only_new)
            differ += len({b.split(": ")[1] for b in bad})
    print(f"total: {common} common kernels, {differ} differ; {gone} only in the old build, {added} only in the new build")
    return 1 if differ or added else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
