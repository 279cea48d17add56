#!/usr/bin/env python3
"""Per-kernel resources of a built kernel object, from its metadata only (not
shipped).

  tools/kernel_resources.py isa-l_amd/build/ec_kernels.o > table.tsv
  tools/kernel_resources.py NEW.o --against OLD.o

The object is a HIP host object (its gfx950 code object is unbundled from
.hip_fatbin) or a code object. One row per kernel, sorted by name, from the
amdhsa.kernels note (llvm-readelf --notes): VGPRs, SGPRs, private segment
(scratch) bytes, LDS bytes, SGPR and VGPR spills, and the waves per SIMD the
VGPRs allow: floor(512 / VGPRs rounded up to 8), at most 8.

--against prints the kernels only one object has and every kernel that gained
scratch, gained VGPR spills or lost a wave per SIMD, and exits 1 if there are
any.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
FIELDS = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("scratch", "private_segment_fixed_size"),
          ("lds", "group_segment_fixed_size"), ("sgpr_spill", "sgpr_spill_count"), ("vgpr_spill", "vgpr_spill_count"))


def run(*args, **kw):
    return subprocess.run(args, check=True, capture_output=True, text=True, **kw).stdout


def notes(path):
    """The notes of the gfx950 code object in (or at) path."""
    if ".hip_fatbin" not in run(f"{LLVM}/llvm-readelf", "-S", "-W", path):
        return run(f"{LLVM}/llvm-readelf", "--notes", path)
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", path, os.path.join(d, "tmp.o"))
        run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
        return run(f"{LLVM}/llvm-readelf", "--notes", co)


def waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def kernels(path):
    """{demangled name: {field: value}} of every kernel of the object."""
    rows, cur, in_kernels = {}, None, False
    for line in notes(path).splitlines():
        if re.match(r"\s*amdhsa\.kernels:", line):
            in_kernels = True
        elif re.match(r"\s*amdhsa\.\w+:", line):
            in_kernels = False
        if not in_kernels:
            continue
        # a kernel's own keys sit at one indent; its arguments' deeper
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if m.group(2) == "name":
            rows[m.group(3).strip("'\"")] = cur
        else:
            cur[m.group(2)] = m.group(3)
    names = sorted(rows)
    try:
        plain = run("c++filt", input="\n".join(names)).splitlines()
    except FileNotFoundError:
        print("kernel_resources: no c++filt here: the kernel column holds mangled names and will not "
              "compare with a table that holds demangled ones", file=sys.stderr)
        plain = names
    out = {}
    for mangled, name in zip(names, plain):
        # the template arguments tell the instantiations apart: drop the rest
        name = name.replace("(anonymous namespace)::", "").removeprefix("void ")
        name = name[:name.rfind(">(") + 1] if ">(" in name else name.split("(")[0]
        r = {short: int(rows[mangled].get(key, 0)) for short, key in FIELDS}
        r["waves"] = waves(r["vgpr"])
        out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("object")
    ap.add_argument("--against", metavar="OLD", help="compare with this object instead of printing the table")
    args = ap.parse_args()
    new = kernels(args.object)
    cols = [short for short, _ in FIELDS] + ["waves"]
    if not args.against:
        print("\t".join(cols + ["kernel"]))
        for name, r in sorted(new.items()):
            print("\t".join(str(r[c]) for c in cols) + "\t" + name)
        return 0
    old = kernels(args.against)
    bad = [f"only in {which}: {n}" for which, a, b in (("OLD", old, new), ("NEW", new, old)) for n in sorted(a.keys() - b.keys())]
    for name in sorted(old.keys() & new.keys()):
        o, n = old[name], new[name]
        why = [f"{c} {o[c]} -> {n[c]}" for c in ("scratch", "vgpr_spill") if n[c] > o[c]]
        if n["waves"] < o["waves"]:
            why.append(f"waves {o['waves']} -> {n['waves']} (vgpr {o['vgpr']} -> {n['vgpr']})")
        if why:
            bad.append(f"{name}: " + ", ".join(why))
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {len(bad)} findings")
    for b in bad:
        print(b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
