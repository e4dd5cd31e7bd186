"""Fingerprint of the gfx950 instructions of every kernel of some .hip units (no GPU needed): shows that a change which only MOVES kernels between
files, or touches the host code around them, left the device code alone.
   python tools/kernel_isa_listing.py UNIT.hip|UNIT.s [...] [--check LISTING] [extra compiler flags ...]
Each .hip is compiled with the Makefile's flags plus --cuda-device-only -S (a .s is taken as that output).  Per kernel symbol the text between its label and
.Lfunc_end is normalised -- `;` comments dropped, the function index taken out of local labels (.LBB<n>_ -> .LBB_, .Ltmp<n> -> .Ltmp), which is all that
moving a function inside or between units changes -- and printed as one line: sha256 prefix, instruction count, demangled name; sorted by name, the unit
not shown, so that two listings compare with diff.  A kernel defined by two of the units is an error.
--check LISTING: exit status 1 unless the kernels and fingerprints equal the stored listing's (lines starting with # are ignored).
   profiles/cg_split_kernel_isa_before.txt / _after.txt: dense_solver.hip + dist_cg.hip before the split into one unit per CG family, and the units after it.
   profiles/ba_split_kernel_isa_before.txt / _after.txt: ba_kernels.hip + implicit_schur.hip before the split into one unit per pass, and the units after it."""
import hashlib
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]


def kernels(asm):
    """mangled name -> (fingerprint, instruction count) of every .amdhsa_kernel of the assembly"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    out = {}
    lines = asm.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):", lines[i])
        i += 1
        if not m or m.group(1) not in names:
            continue
        body = []
        while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
            ln = lines[i].split(";")[0].rstrip()
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"\.Ltmp\d+", ".Ltmp", ln)
            if ln.strip():
                body.append(ln)
            i += 1
        n = len([ln for ln in body if ln.startswith("\t") and not ln.startswith("\t.")])
        out[m.group(1)] = (hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], n)
    return out


def main():
    args = sys.argv[1:]
    stored = None
    if "--check" in args:
        k = args.index("--check")
        stored = args[k + 1]
        del args[k:k + 2]
    units = [a for a in args if a.endswith((".hip", ".s"))]
    extra = [a for a in args if a not in units]
    rows = {}
    for u in units:
        if u.endswith(".s"):
            asm = open(u).read()
        else:
            asm = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "--cuda-device-only", "-S", "-o", "-", os.path.basename(u)],
                                 cwd=os.path.dirname(os.path.abspath(u)), check=True, capture_output=True, text=True).stdout
        for name, v in kernels(asm).items():
            if name in rows:
                print("kernel defined twice: %s (again in %s)" % (name, u))
                return 1
            rows[name] = v
    pretty = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.splitlines()
    # (the name without its parameter list: cut at the parenthesis that closes last, `(anonymous namespace)` stays)
    def short(p):
        depth = 0
        for k in range(len(p) - 1, -1, -1):
            depth += (p[k] == ")") - (p[k] == "(")
            if depth == 0 and p[k] == "(":
                return p[:k]
        return p
    listing = sorted(("%s %6d  %s" % (rows[n][0], rows[n][1], short(p)) for n, p in zip(rows, pretty)), key=lambda ln: ln.split(None, 2)[2])
    print("\n".join(listing))
    if stored is not None:
        want = [ln.rstrip("\n") for ln in open(stored) if ln.strip() and not ln.startswith("#")]
        if sorted(want) != sorted(listing):
            for ln in sorted(set(want) ^ set(listing)):
                print(("only stored:  " if ln in want else "only built:   ") + ln)
            return 1
        print("# %d kernels, equal to %s" % (len(listing), stored))
    return 0


if __name__ == "__main__":
    sys.exit(main())
