"""The host half of sfmba_png_decode (csrc/png_inflate.cpp: chunk walk, CRC-32, zlib wrapper and inflate) under AddressSanitizer +
UBSan, as one instrumented stand-alone executable on the CPU: `make -C sfm-toy-library_amd/host png_asan`.  It decodes every fixture,
every prefix of two of them, 2100 single-byte mutations of a third, and feeds 2100 single-byte mutations of two bare deflate streams
to the inflate directly (past the CRC and the Adler-32, which would otherwise refuse nearly all of them before the decoder saw them);
every outcome must be OK, UNSUPPORTED or CORRUPT and the sanitizers must stay silent (-fno-sanitize-recover: any report fails the
target)."""
import os
import re
import shutil
import subprocess

import pytest

import png_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sfm-toy-library_amd", "host")


def _san_works(flag):
    """the sanitizer runtimes are part of gcc here; probe instead of assuming"""
    if shutil.which("g++") is None:
        return False
    r = subprocess.run("echo 'int main(){return 0;}' | g++ -x c++ - %s -o /tmp/_sfmba_png_san_probe && /tmp/_sfmba_png_san_probe" % flag, shell=True,
                       capture_output=True)
    return r.returncode == 0


def test_png_chunk_walk_and_inflate_under_address_and_ub_sanitizer():
    if not _san_works("-fsanitize=address,undefined"):
        pytest.skip("no AddressSanitizer runtime")
    r = subprocess.run(["make", "-C", HOST, "png_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    m = re.search(r"png_sanitize: (\d+) files \((\d+) decodable\), (\d+) truncations, (\d+) mutations: (\d+) ok, (\d+) unsupported, (\d+) corrupt; "
                  r"(\d+) raw mutations \((\d+) inflate\)", r.stdout)
    assert m, r.stdout[-2000:]
    files, decodable, truncations, mutations, ok, unsupported, corrupt, raw, raw_ok = (int(v) for v in m.groups())
    assert files == len(pc.small_names()) and decodable == len(pc.decodable_names())
    assert truncations == len(pc.small_file("t3_d4_37x20")) + len(pc.small_file("dynamic_t2_d8_40x30")) and mutations == 2100 and raw == 2100
    assert ok + unsupported + corrupt == files + truncations + mutations and corrupt > 2000
    assert 0 < raw_ok < raw                                             # the inflate saw streams it accepts and streams it refuses
