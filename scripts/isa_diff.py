"""Per-kernel comparison of the gfx950 device code of two sets of hipcc objects: the proof that a
move-only change left every kernel alone, whichever object a kernel now lives in.

    python scripts/isa_diff.py OLD.o[,OLD2.o,...] NEW1.o[,NEW2.o,...]

Per kernel symbol: the instruction stream with its encodings (llvm-objdump -d, addresses
stripped; branch targets are symbol-relative) and the resources in the code object's metadata
(VGPR / AGPR / SGPR counts, spills, LDS and scratch bytes, workgroup size, kernarg size).
Lists the kernels only one side has; exits 1 if a common kernel differs or the new side adds one.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "group_segment_fixed_size", "private_segment_fixed_size", "max_flat_workgroup_size",
          "kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernels(obj, tmp):
    """{symbol: (instruction lines, {resource: value})} of one host object's gfx950 code object."""
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    if ".hip_fatbin" not in run(f"{LLVM}/llvm-readelf", "-S", obj):
        return {}   # a host-only unit
    run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj)
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}",
        f"--output={co}")
    res = {}
    for blk in run(f"{LLVM}/llvm-readelf", "--notes", co).split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            res[name.group(1)] = {f: int(m.group(1)) for f in FIELDS
                                  for m in [re.search(rf"\.{f}:\s+(\d+)", blk)] if m}
    out, cur = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), ([], res.get(m.group(1), {})))[0]
        elif cur is not None and "//" in line:
            cur.append(re.sub(r"// [0-9A-F]+:", "//", line).strip())
    return out


def load(arg):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in arg.split(","):
            for k, v in kernels(obj, tmp).items():
                assert k not in out, f"{k} defined twice in {arg}"
                out[k] = v
    return out


a, b = load(sys.argv[1]), load(sys.argv[2])
bad = 0
for k in sorted(set(a) - set(b)):
    print("only in old:", k)
for k in sorted(set(b) - set(a)):
    print("only in NEW:", k)
    bad += 1
for k in sorted(set(a) & set(b)):
    (ia, ra), (ib, rb) = a[k], b[k]
    if ra != rb:
        print("resources differ:", k, {f: (ra.get(f), rb.get(f)) for f in FIELDS if ra.get(f) != rb.get(f)})
        bad += 1
    if ia != ib:
        first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
        print(f"code differs: {k}: {len(ia)} vs {len(ib)} instructions, first at {first}:")
        print("   old:", ia[first] if first < len(ia) else "<end>")
        print("   new:", ib[first] if first < len(ib) else "<end>")
        bad += 1
print(f"{len(a)} old / {len(b)} new kernels, {len(set(a) & set(b))} common, {bad} differences")
sys.exit(1 if bad else 0)
