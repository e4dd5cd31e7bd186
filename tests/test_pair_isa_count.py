"""The pair pass is bound by VALU issue, so its cost is its instruction count -- checked where it is produced, from the compiler's gfx950
assembly (tools/pair_isa_count.py --check, no GPU): the fp32 wave-per-chunk kernels keep a loop body of at most 210 instructions (279 before
both observations of a pair became packed halves; 139 at the time of writing) with no fp64 arithmetic in it, at most 128 VGPRs and no scratch,
and no full vector-memory wait stands between the point-slot load and the point-table loads of a round."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_pair_pass_keeps_its_instruction_budget():
    assert os.path.exists("/opt/rocm/bin/hipcc"), "the count needs the compiler that builds the library"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pair_isa_count.py"), "--check"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    blocks = r.stdout.split("void sfmba::")
    wave = [b for b in blocks if b.startswith("k_schur_pairs<float")]
    assert len(wave) == 2
    for b in wave:
        assert "point-table loads: no" in b, b
