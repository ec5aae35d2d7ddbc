"""Instruction counts by mnemonic class in the compiler's assembly of the kernels whose demangled name contains FILTER, split by the
loop depth of the basic block (the compiler's "Loop Header ... Depth=" comments).  In the fused persistent kernels depth <= 1 is once
per launch / per TR iteration, depth >= 2 is inside the trip loop (the static count of the loop's blocks: the blocks of the first trip
and of a refresh trip are in it -- `--blocks` lists every block of depth >= 2 with its own counts, to tell the steady-state path apart).
Classes: quarter-rate integer VALU (32-bit multiplies, v_mad_u64_u32 and kin), v_cndmask, v_mov, fp64 VALU, other VALU, buffer loads,
buffer stores, LDS (ds_), scalar.
Where the compiler does not see the trip loop as a loop of its own (the fused launch: the trip loop is entered at two places, and all
of it is reported at the depth of the loop over the TR iterations), `--range FIRST:LAST` sums the blocks from label FIRST up to, not
including, label LAST in the order of the file; the option may be given several times and the ranges are added up.  The labels are read
off the assembly by hand: a trip's steady-state path is the chain of blocks from the target of the loop's back edge to that back edge.
A block that is only fallen into carries no label: the compiler's `; %bb.N:` comment in front of it is read as the label .LBB<f>_N, so such a
block can begin or end a range too.
usage: python tools/isa_trip_counts.py FILE.hip|FILE.s FILTER [--blocks] [--range FIRST:LAST ...]"""
import os, re, subprocess, sys, tempfile

CLASSES = ["qint", "cndmask", "mov", "fp64", "valu_other", "buf_load", "buf_store", "lds", "scalar"]


def classify(mn):
    if mn.startswith("buffer_load"):
        return "buf_load"
    if mn.startswith("buffer_store"):
        return "buf_store"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith("s_"):
        return "scalar"
    if not mn.startswith("v_"):
        return None
    if re.match(r"v_(mul_lo_[ui]32|mul_hi_[ui]32|mad_[ui]64_[ui]32)", mn):
        return "qint"
    if mn.startswith("v_cndmask"):
        return "cndmask"
    if mn.startswith("v_mov_b32") or mn.startswith("v_mov_b64") or mn.startswith("v_accvgpr"):
        return "mov"
    if "_f64" in mn:
        return "fp64"
    return "valu_other"


def assembly(path):
    if path.endswith(".s"):
        return open(path).read().split("\n")
    tmp = tempfile.mkdtemp()
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result",
                    "-I", inc, "-c", os.path.abspath(path), "-o", os.path.join(tmp, "x.o"), "-save-temps"], cwd=tmp, check=True, capture_output=True)
    asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")][0]
    return open(os.path.join(tmp, asm)).read().split("\n")


def fmt(c):
    return "  ".join("%s %d" % (k, c.get(k, 0)) for k in CLASSES)


def main():
    lines = assembly(sys.argv[1]); flt = sys.argv[2]; per_block = "--blocks" in sys.argv[3:]
    ranges = [a.split(":") for k, a in enumerate(sys.argv) if k > 0 and sys.argv[k - 1] == "--range"]
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1; continue
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        if flt in name:
            depth, label = 0, "entry"
            by_depth, blocks = {}, []
            # a block that is only fallen into has no label of its own: the compiler's "; %bb.N:" comment stands for .LBB<f>_N
            fn = next((m.group(1) for l in lines[i:j] for m in [re.match(r"^\.LBB(\d+)_\d+:", l)] if m), "0")
            for k in range(i, j):
                l = re.sub(r"^; %bb\.(\d+):", r".LBB%s_\1:" % fn, lines[k])
                mb = re.match(r"^(\.LBB\d+_\d+):", l)
                if mb:
                    depth, label = 0, mb.group(1)
                    for q in range(k, min(k + 6, j)):
                        mm = re.search(r"(?:in Loop|Loop Header|Inner Loop Header).*?Depth=(\d+)", lines[q])
                        if mm and "Parent" not in lines[q]:
                            depth = int(mm.group(1)); break
                    blocks.append((label, depth, {}))
                    continue
                mi = re.match(r"^\s+([a-z][a-z0-9_]+)\b", l)
                if not mi:
                    continue
                cl = classify(mi.group(1))
                if cl is None:
                    continue
                dd = by_depth.setdefault(depth, {})
                dd[cl] = dd.get(cl, 0) + 1
                if blocks:
                    blocks[-1][2][cl] = blocks[-1][2].get(cl, 0) + 1
            print(name[:110])
            tot = {}
            for dpt in sorted(by_depth):
                print("    depth %d: %s" % (dpt, fmt(by_depth[dpt])))
                for kk, vv in by_depth[dpt].items():
                    tot[kk] = tot.get(kk, 0) + vv
            print("    kernel : %s" % fmt(tot))
            if ranges:
                rsum, on = {}, [False] * len(ranges)
                for label, dpt, c in blocks:
                    for q, (first, last) in enumerate(ranges):
                        if label == "." + first.lstrip("."):
                            on[q] = True
                        if label == "." + last.lstrip("."):
                            on[q] = False
                    if any(on):
                        for kk, vv in c.items():
                            rsum[kk] = rsum.get(kk, 0) + vv
                print("    ranges : %s" % fmt(rsum))
            if per_block:
                for label, dpt, c in blocks:
                    if dpt >= 2 and c:
                        print("      %-12s depth %d: %s" % (label, dpt, fmt(c)))
        i = j


if __name__ == "__main__":
    main()
