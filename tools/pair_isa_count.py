"""Instruction count of the pair-pass kernels, from the compiler's gfx950 assembly (no GPU needed): the pair pass is bound by VALU issue
(DESIGN_HISTORY "What bounds what": one wave instruction = one quad-cycle), so the count of its loop body prices a change before it runs.
   python tools/pair_isa_count.py [--src sfm-toy-library_amd/csrc/ba_pairs.hip] [--check] [extra compiler flags ...]
Per kernel whose name contains k_schur_pairs: wave instructions before / inside / after the pair loop (the innermost loop that loads
16-byte point-table words), the loop body by class, registers, scratch, and whether a full vector-memory wait (vmcnt(0)) stands between
the loop's first load and its point-table loads (the look-ahead of the point slot is real only if there is none).
--check: exit status 1 unless the fp32 wave-per-chunk kernels have a loop body <= 210 with no fp64 arithmetic, <= 128 VGPRs and no scratch."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-Wno-unused-function", "-Wno-unused-command-line-argument"]


def classify(op):
    if op.startswith("v_cvt_"):
        return "convert"
    if op.startswith("v_pk_mov"):
        return "v_pk_mov"
    if op.startswith("v_mov_b") or op.startswith("v_accvgpr"):
        return "v_mov"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith("v_pk_"):
        return "packed fp32"
    if op.startswith("v_") and ("_f64" in op):
        return "fp64"
    if op.startswith("v_") and ("_f32" in op):
        return "scalar fp32"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("global_load") or op.startswith("buffer_load") or op.startswith("flat_load") or op.startswith("s_load"):
        return "load"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "SALU / branch"
    return "other"


ORDER = ["fp64", "convert", "select", "packed fp32", "scalar fp32", "other VALU", "v_mov", "v_pk_mov", "load", "LDS", "wait", "SALU / branch", "other"]


def kernels(asm):
    """name -> (instruction lines [(text, label-or-None)], metadata dict)"""
    out = {}
    lines = asm.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):\s*; @", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        body, meta = [], {}
        i += 1
        code = True
        while i < len(lines) and not re.match(r"^(_Z\w+):\s*; @", lines[i]):
            ln = lines[i]
            if ln.startswith(".Lfunc_end"):
                code = False
            mm = re.match(r"^; (NumVgprs|ScratchSize|Occupancy|NumAgprs): (\d+)", ln)
            if mm:
                meta[mm.group(1)] = int(mm.group(2))
            lab = re.match(r"^(\.LBB\d+_\d+):", ln)
            if not code:
                pass
            elif lab:
                body.append((None, lab.group(1)))
            elif ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;"):
                body.append((ln.strip().split(";")[0].strip(), None))
            i += 1
        out[name] = (body, meta)
    return out


def pair_loop(body):
    """(start, end) indices into body of the longest innermost loop that holds 16-byte loads (the epilogue of the sixteen-lane form has a
    short one of its own); None if there is none"""
    pos = {lab: k for k, (_, lab) in enumerate(body) if lab}
    best = None
    for k, (ins, _) in enumerate(body):
        if not ins or not ins.startswith("s_cbranch"):
            continue
        tgt = ins.split()[-1]
        if tgt in pos and pos[tgt] < k:
            seg = [x for x, _ in body[pos[tgt]:k + 1] if x]
            inner = not any(x and x.startswith("s_cbranch") and pos[tgt] <= pos.get(x.split()[-1], len(body)) < q
                            for q, (x, _) in enumerate(body[:k]) if q > pos[tgt])
            if inner and any(x.startswith("global_load_dwordx4") for x in seg) and (best is None or k - pos[tgt] > best[1] - best[0]):
                best = (pos[tgt], k + 1)
    return best


def main():
    args = sys.argv[1:]
    check = "--check" in args
    args = [a for a in args if a != "--check"]
    src = os.path.join(ROOT, "sfm-toy-library_amd", "csrc", "ba_pairs.hip")
    if "--src" in args:
        k = args.index("--src")
        src = args[k + 1]
        del args[k:k + 2]
    asm = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *args, "--cuda-device-only", "-S", "-o", "-", src], check=True, capture_output=True, text=True).stdout
    bad = []
    for name, (body, meta) in sorted(kernels(asm).items()):
        if "k_schur_pairs" not in name:
            continue
        pretty = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
        loop = pair_loop(body)
        if loop is None:
            continue
        ins = [x for x, _ in body if x]
        seg = [x for x, _ in body[loop[0]:loop[1]] if x]
        before = len([x for x, _ in body[:loop[0]] if x])
        counts = {}
        for x in seg:
            c = classify(x.split()[0])
            counts[c] = counts.get(c, 0) + 1
        # a full wait between the first load of the round and the point-table loads of the same round?
        first_load = next(k for k, x in enumerate(seg) if classify(x.split()[0]) == "load")
        first_x4 = next(k for k, x in enumerate(seg) if x.startswith("global_load_dwordx4"))
        stall = any(x.startswith("s_waitcnt") and "vmcnt(0)" in x for x in seg[first_load + 1:first_x4]) if first_load < first_x4 else False
        print("%s" % pretty)
        print("    vgprs %d  agprs %d  scratch %d  occupancy %d | instructions: before loop %d, LOOP BODY %d, after loop %d" %
              (meta.get("NumVgprs", -1), meta.get("NumAgprs", 0), meta.get("ScratchSize", -1), meta.get("Occupancy", -1), before, len(seg), len(ins) - before - len(seg)))
        print("    loop body: " + ", ".join("%s %d" % (c, counts[c]) for c in ORDER if counts.get(c)))
        print("    vmcnt(0) between the round's first load and its point-table loads: %s" % ("YES" if stall else "no"))
        if "k_schur_pairs<float" in pretty:
            if len(seg) > 210 or counts.get("fp64", 0) or meta.get("NumVgprs", 999) > 128 or meta.get("ScratchSize", 1) != 0:
                bad.append(pretty)
    if check and bad:
        print("FAILED conditions (loop body <= 210, no fp64, <= 128 VGPRs, no scratch): " + ", ".join(bad))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
