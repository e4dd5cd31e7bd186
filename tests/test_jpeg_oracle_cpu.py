"""CPU-side checks of the image reader's contract (include/sfmba.h: sfmba_jpeg_decode, sfmba_resize_images): no GPU needed.

  restatement     tests/jpeg_oracle.py (header parse, Huffman decode, integer inverse DCT, triangle upsampling, fixed-point colour)
                  equals libjpeg's stored decode on every file of tests/golden/jpeg_small, and the stored SHA-256 of libjpeg's decode on
                  the seven 512 x 384 photographs of tests/golden/crazyhorse_half
  host program    tools/micro/jpeg_math_host.hip (csrc/jpeg_entropy.cpp and csrc/jpeg_math.h, the arithmetic the kernels run, compiled
                  for the host) equals the restatement in coefficients, component planes, pixels and resized pixels at the factors
                  0.5, 0.25, 0.37, 1.0 and 1.5
  resize          the restatement is never more than 1 level from the rounded float64 bilinear value (each 11-bit weight is off by at
                  most 2^-12, so the value is off by less than 255 * 2 * 2^-12 + 0.5 < 1); at 0.5 on even sizes it equals
                  (a + b + c + d + 2) >> 2
  C ABI           sfmba_jpeg_info and sfmba_resized_size through ctypes: geometry of every fixture, UNSUPPORTED for the progressive and
                  the CMYK file and for headers patched to 12-bit samples / a 16-bit quantisation table, CORRUPT for truncations
  program         sfmtoy -h exits 0, no input directory exits 2
  symbols         the libraries export the new entry points and drivers"""
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_oracle as jo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-toy-library_amd", "csrc")


@pytest.fixture(scope="module")
def decoded_small():
    """name -> (header, coefficients, planes, pixels) of the restatement, computed once."""
    out = {}
    for name in jc.decodable_names():
        data = jc.small_file(name)
        hdr = jo.parse(data)
        co = jo.coefficients(data, hdr)
        pl = jo.planes(hdr, co)
        out[name] = (hdr, co, pl, jo.pixels(hdr, pl))
    return out


@pytest.mark.parametrize("name", jc.decodable_names())
def test_restatement_equals_libjpeg_on_the_small_files(decoded_small, name):
    px = decoded_small[name][3]
    want = jc.small_pixels(name)
    assert px.shape == want.shape and px.dtype == np.uint8
    assert np.array_equal(px, want), (name, int(np.abs(px.astype(int) - want.astype(int)).max()))


def test_the_checker_file_makes_the_clamps_act(decoded_small):
    px = jc.small_pixels("c420_checker_q10")
    assert (px == 0).any() and (px == 255).any()


def test_restatement_equals_libjpeg_on_the_photographs():
    hashes = jc.photo_hashes()
    assert len(hashes) == 7 and sorted(hashes) == jc.photo_names()
    for name in jc.photo_names():
        status, px = jo.decode(jc.photo_file(name))
        assert status == jo.OK and px.shape == (384, 512, 3)
        assert jc.sha256(px) == hashes[name], name


def test_restatement_reports_the_status():
    for name in jc.UNSUPPORTED:
        assert jo.decode(jc.small_file(name)) == (jo.UNSUPPORTED, None)
    data = jc.small_file("c420_17x9")
    assert jo.decode(data[:len(data) // 2])[0] == jo.CORRUPT and jo.decode(data[:40])[0] == jo.CORRUPT


# ---- the device arithmetic on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    exe = str(tmp_path_factory.mktemp("jpeg") / "jpeg_math_host")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tools", "micro", "jpeg_math_host.hip"), os.path.join(CSRC, "jpeg_entropy.cpp")])
    return exe


def host_decode(exe, tmp_path, data):
    """(status, coefficient arrays, planes, pixels) as the host program writes them."""
    src, dst = tmp_path / "in.jpg", tmp_path / "out.bin"
    src.write_bytes(data)
    subprocess.check_call([exe, "decode", str(src), str(dst)])
    raw = dst.read_bytes()
    head = np.frombuffer(raw[:16], np.int32) if len(raw) >= 16 else np.frombuffer(raw[:4], np.int32)
    if head[0] != 0:
        return int(head[0]), None, None, None
    w, h, nc = (int(v) for v in head[1:4])
    dims = np.frombuffer(raw[16:16 + 8 * nc], np.int32).reshape(nc, 2)
    at = 16 + 8 * nc
    coefs, planes = [], []
    for bw, bh in dims:
        n = int(bw) * int(bh) * 64
        coefs.append(np.frombuffer(raw[at:at + 2 * n], np.int16).reshape(bh, bw, 64))
        at += 2 * n
    for bw, bh in dims:
        n = int(bw) * int(bh) * 64
        planes.append(np.frombuffer(raw[at:at + n], np.uint8).reshape(8 * bh, 8 * bw))
        at += n
    px = np.frombuffer(raw[at:], np.uint8).reshape((h, w) if nc == 1 else (h, w, 3))
    return 0, coefs, planes, px


@pytest.mark.parametrize("name", jc.decodable_names())
def test_device_arithmetic_on_the_host_against_the_restatement(host_exe, tmp_path, decoded_small, name):
    """csrc/jpeg_entropy.cpp and csrc/jpeg_math.h compiled for the host: coefficients, planes and pixels."""
    hdr, co, pl, px = decoded_small[name]
    status, hco, hpl, hpx = host_decode(host_exe, tmp_path, jc.small_file(name))
    assert status == 0 and len(hco) == hdr["ncomp"]
    for c in range(hdr["ncomp"]):
        assert np.array_equal(hco[c], co[c]), (name, "coefficients", c)
        assert np.array_equal(hpl[c], pl[c]), (name, "plane", c)
    assert np.array_equal(hpx, px), name


def test_host_program_on_a_photograph_and_on_files_it_must_refuse(host_exe, tmp_path):
    name = jc.photo_names()[0]
    status, _, _, px = host_decode(host_exe, tmp_path, jc.photo_file(name))
    assert status == 0 and jc.sha256(px) == jc.photo_hashes()[name]
    for bad in jc.UNSUPPORTED:
        assert host_decode(host_exe, tmp_path, jc.small_file(bad))[0] == jo.UNSUPPORTED
    data = jc.small_file("c422_33x17_rst3")
    assert host_decode(host_exe, tmp_path, data[:len(data) - 200])[0] == jo.CORRUPT
    broken = bytearray(data)
    at = data.index(b"\xff\xd0", jo.parse(data)["scan"])                  # the first restart marker becomes RST5
    broken[at + 1] = 0xD5
    assert host_decode(host_exe, tmp_path, bytes(broken))[0] == jo.CORRUPT


@pytest.mark.parametrize("name", list(jc.resize_sources()))
def test_host_resize_against_the_restatement(host_exe, tmp_path, name):
    img = jc.resize_sources()[name]
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(img.tobytes())
    for f in jc.FACTORS:
        ow, oh = jo.resized_size(w, h, f)
        rc = subprocess.call([host_exe, "resize", str(w), str(h), str(ch), repr(float(np.float32(f))), str(src), str(dst)])
        if ow < 1 or oh < 1:
            assert rc == 3, (name, f)                                    # a zero side is refused
            continue
        assert rc == 0
        raw = dst.read_bytes()
        assert np.frombuffer(raw[:8], np.int32).tolist() == [ow, oh]
        got = np.frombuffer(raw[8:], np.uint8).reshape((oh, ow) if ch == 1 else (oh, ow, 3))
        assert np.array_equal(got, jo.resize(img, f)), (name, f)


# ---- the resize rule ----------------------------------------------------------------------------------------------------------------
def test_resize_is_within_one_level_of_the_float_bilinear_value():
    worst = 0.0
    for name, img in jc.resize_sources().items():
        for f in jc.FACTORS:
            ow, oh = jo.resized_size(img.shape[1], img.shape[0], f)
            if ow < 1 or oh < 1:
                continue
            got = jo.resize(img, f).astype(np.float64)
            exact = jo.resize_float(img, f)
            worst = max(worst, float(np.abs(got - exact).max()))
            assert np.all(np.abs(got - np.rint(exact)) <= 1), (name, f)
            assert np.all(np.abs(got - exact) < 1.0), (name, f)
    print("resize: largest distance from the exact bilinear value %.4f levels" % worst)


def test_resize_at_one_half_on_even_sizes_is_the_rounded_box_mean():
    for name in ("512x384x1", "512x384x3"):
        img = jc.resize_sources()[name].astype(np.int64)
        box = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
        assert np.array_equal(jo.resize(jc.resize_sources()[name], 0.5), box.astype(np.uint8))


def test_resize_at_factor_one_is_the_identity_and_sizes_round_half_to_even():
    img = jc.resize_sources()["67x43x3"]
    assert np.array_equal(jo.resize(img, 1.0), img)
    assert jo.resized_size(5, 3, 0.5) == (2, 2) and jo.resized_size(7, 1, 0.5) == (4, 0)      # 2.5 -> 2, 1.5 -> 2, 3.5 -> 4, 0.5 -> 0
    assert jo.resized_size(1024, 768, 0.37) == (379, 284)


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    return capi


def test_jpeg_info_reports_the_geometry_of_every_fixture(capi):
    names = jc.small_names()
    infos = capi.jpeg_info([jc.small_file(n) for n in names] + [jc.photo_file(n) for n in jc.photo_names()])
    for n, d in zip(names, infos):
        want = jo.info(jc.small_file(n))
        if n in jc.UNSUPPORTED:
            assert want == (jo.UNSUPPORTED,)
            assert d == dict(status=1, width=0, height=0, channels=0, h_samp=0, v_samp=0, restart_interval=0), n
        else:
            assert (d["status"], d["width"], d["height"], d["channels"], d["h_samp"], d["v_samp"], d["restart_interval"]) == want, n
            assert (d["height"], d["width"]) == jc.small_pixels(n).shape[:2]
    for d in infos[len(names):]:
        assert d == dict(status=0, width=512, height=384, channels=3, h_samp=2, v_samp=1, restart_interval=0)
    by_name = dict(zip(names, infos))
    assert by_name["c422_33x17_rst3"]["restart_interval"] == 3 and by_name["gray_70x45"]["channels"] == 1
    assert capi.jpeg_info([]) == []


def test_jpeg_info_refuses_what_is_out_of_scope_and_what_is_broken(capi):
    data = jc.small_file("c420_70x45_q60")
    sof = data.index(b"\xff\xc0")
    scan = jo.parse(data)["scan"]
    files = [jc.patch_sof_precision(data, 12), jc.patch_dqt_16bit(data), data[:sof + 6], data[:scan - 3], data[:2], b"", data[1:],
             data[:sof + 5] + b"\x00\x00" + data[sof + 7:], data]
    status = [d["status"] for d in capi.jpeg_info(files)]
    assert status == [1, 1, 2, 2, 2, 2, 2, 2, 0]              # 12-bit, 16-bit table; truncations, no SOI, zero height; the file itself


def test_resized_size_through_the_abi(capi):
    for w, h in ((1024, 768), (67, 43), (2, 3), (1, 1), (16384, 16384), (5, 3)):
        for f in jc.FACTORS:
            ow, oh = jo.resized_size(w, h, f)
            if 1 <= ow <= 16384 and 1 <= oh <= 16384:
                assert capi.resized_size(w, h, f) == (ow, oh), (w, h, f)
            else:
                with pytest.raises(capi.SfmbaError):
                    capi.resized_size(w, h, f)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.SfmbaError):
            capi.resized_size(10, 10, bad)


# ---- the program and the symbols ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_dir():
    import __graft_entry__ as ge
    ge.build_hip()
    ge.build_host()
    return os.path.join(ROOT, "sfm-toy-library_amd", "host")


def test_sfmtoy_usage(host_dir):
    exe = os.path.join(host_dir, "sfmtoy")
    ok = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert ok.returncode == 0 and "--downscale" in ok.stdout and "--input-directory" in ok.stdout
    none = subprocess.run([exe], capture_output=True, text=True)
    assert none.returncode == 2 and "no input directory" in none.stderr
    for bad in (["-s"], ["--downscale=zero", "x"], ["--frobnicate", "x"], ["a", "b"], ["-d", "7", "x"]):
        assert subprocess.run([exe] + bad, capture_output=True).returncode == 2, bad


def test_libraries_export_the_symbols(host_dir):
    lib = os.path.join(CSRC, "libsfmba_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    for sym in ("sfmba_jpeg_info", "sfmba_resized_size", "sfmba_jpeg_decode", "sfmba_resize_images"):
        assert " T %s\n" % sym in exported, sym
    syms = subprocess.check_output(["nm", "-C", os.path.join(host_dir, "libsfmba_shim.so")]).decode()
    for sym in ("sfmba_shim_read_images", "sfmba_shim_resize_images", "sfmba_shim_read_images_directory_scaled", "sfmba_shim_run_sfm_directory"):
        assert " T %s\n" % sym in syms, sym
    assert " T sfmtoylib::SfMImageUtilities::readImages(" in syms and " T sfmtoylib::SfMImageUtilities::resizeImages(" in syms
    hdr = open(os.path.join(host_dir, "SfM.h")).read()
    assert "no resize kernel" not in hdr and "there is no imread here" not in hdr


def test_a_frame_its_file_cannot_hold_is_corrupt_before_anything_is_sized(capi):
    """632 bytes that declare 16384 x 16384 x 3 (1.6 GB of coefficients): a block takes at least 2 bits, so the header is refused."""
    data = jc.small_file("c420_1x1")
    sof = data.index(b"\xff\xc0")
    huge = data[:sof + 5] + b"\x40\x00\x40\x00" + data[sof + 9:]
    assert len(huge) == len(data) < 700 and capi.jpeg_info([huge, data]) [0]["status"] == 2 and capi.jpeg_info([data])[0]["status"] == 0
    wide = data[:sof + 5] + b"\x00\x08\x00\x10" + data[sof + 9:]          # 16 x 8: one MCU, as the file has -- the size alone is no reason
    assert capi.jpeg_info([wide])[0] == dict(status=0, width=16, height=8, channels=3, h_samp=2, v_samp=2, restart_interval=0)
