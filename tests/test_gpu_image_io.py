"""sfmba_jpeg_decode and sfmba_resize_images on the MI355X (-m gpu) against libjpeg's stored decode (tests/golden) and against the
Python restatement of the contract (tests/jpeg_oracle.py), byte for byte; the host drivers (SfMImageUtilities, SfM::setImagesDirectory)
against the C ABI.

  decode      every decodable file of tests/golden/jpeg_small equals libjpeg; a mixed call (4:2:0, gray, 4:2:2 with restarts, CMYK) equals
              the single calls and reports UNSUPPORTED for the CMYK file alone; the seven photographs in one call match their hashes; a
              file whose scan is cut or whose restart marker is wrong is CORRUPT without disturbing its neighbours; cap too small is
              SFMBA_ERR_CAPACITY with the needed total and out untouched
  resize      1 and 3 channels at 1 x 1, 2 x 3, 67 x 43 and 512 x 384, the factors 0.5 0.25 0.37 1.0 1.5, a mixed batch; a fused
              decode at 0.5 equals decode followed by resize; a factor that gives a zero side is SFMBA_ERR_INVALID_ARG"""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_oracle as jo
import sfm_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi
    return capi


@pytest.fixture(scope="module")
def small_decoded(capi):
    """One call over every file of jpeg_small: name -> (info, image)."""
    names = jc.small_names()
    infos, images = capi.jpeg_decode([jc.small_file(n) for n in names])
    return {n: (i, im) for n, i, im in zip(names, infos, images)}


@pytest.mark.parametrize("name", jc.decodable_names())
def test_decode_equals_libjpeg(small_decoded, name):
    info, img = small_decoded[name]
    want = jc.small_pixels(name)
    assert info["status"] == 0 and (info["height"], info["width"]) == want.shape[:2]
    assert img.shape == want.shape and np.array_equal(img, want), (name, int(np.abs(img.astype(int) - want.astype(int)).max()))


def test_unsupported_files_have_no_pixels(small_decoded):
    for name in jc.UNSUPPORTED:
        info, img = small_decoded[name]
        assert info["status"] == 1 and img is None


def test_mixed_batch_equals_the_single_calls(capi):
    names = ["c420_67x43_q95", "gray_70x45", "c422_33x17_rst3", "cmyk_24x16"]
    infos, images = capi.jpeg_decode([jc.small_file(n) for n in names])
    assert [i["status"] for i in infos] == [0, 0, 0, 1] and images[3] is None
    assert [i["channels"] for i in infos] == [3, 1, 3, 0]
    for n, i, im in zip(names[:3], infos, images):
        one_info, one = capi.jpeg_decode([jc.small_file(n)])
        assert one_info[0] == i and one[0].tobytes() == im.tobytes() and np.array_equal(im, jc.small_pixels(n)), n
    assert capi.jpeg_decode([jc.small_file("cmyk_24x16")]) == ([infos[3]], [None])
    assert capi.jpeg_decode([]) == ([], [])


def test_the_seven_photographs_in_one_call(capi):
    names = jc.photo_names()
    infos, images = capi.jpeg_decode([jc.photo_file(n) for n in names])
    hashes = jc.photo_hashes()
    for n, i, im in zip(names, infos, images):
        assert i["status"] == 0 and im.shape == (384, 512, 3)
        assert jc.sha256(im) == hashes[n], n


def test_corrupt_scan_data_is_reported_per_image(capi):
    data = jc.small_file("c422_33x17_rst3")
    wrong = bytearray(data)
    wrong[data.index(b"\xff\xd0", jo.parse(data)["scan"]) + 1] = 0xD5          # the first restart marker becomes RST5
    good = jc.small_file("c420_17x9")
    infos, images = capi.jpeg_decode([good, data[:len(data) - 200], bytes(wrong), good, data[:30]])
    assert [i["status"] for i in infos] == [0, 2, 2, 0, 2]
    assert images[1] is None and images[2] is None and images[4] is None
    assert np.array_equal(images[0], jc.small_pixels("c420_17x9")) and np.array_equal(images[3], images[0])


def test_capacity_too_small_reports_the_total_and_writes_nothing(capi):
    files = [jc.small_file("c420_17x9"), jc.small_file("gray_70x45")]
    ptr, flat = capi._flat_files(files)
    need = 17 * 9 * 3 + 70 * 45
    info = (capi._ImageInfo * 2)()
    out_ptr, total = np.zeros(3, np.int64), C.c_int64(0)
    out = np.full(need, 0xAB, np.uint8)
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    rc = capi.lib().sfmba_jpeg_decode(C.c_int(0), C.c_int(2), ptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), C.c_float(1.0), info,
                                      out_ptr.ctypes.data_as(lp), out.ctypes.data_as(bp), C.c_int64(need - 1), C.byref(total))
    assert rc == capi.SFMBA_ERR_CAPACITY and total.value == need and out_ptr.tolist() == [0, 17 * 9 * 3, need]
    assert np.all(out == 0xAB)
    rc = capi.lib().sfmba_jpeg_decode(C.c_int(0), C.c_int(2), ptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), C.c_float(1.0), info,
                                      out_ptr.ctypes.data_as(lp), out.ctypes.data_as(bp), C.c_int64(need), C.byref(total))
    assert rc == 0 and np.array_equal(out[:17 * 9 * 3].reshape(9, 17, 3), jc.small_pixels("c420_17x9"))
    assert np.array_equal(out[17 * 9 * 3:].reshape(45, 70), jc.small_pixels("gray_70x45"))


# ---- resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resize_reference():
    """(name, factor) -> the restatement's result, computed once."""
    return {(n, f): jo.resize(img, f) for n, img in jc.resize_sources().items() for f in jc.FACTORS
            if min(jo.resized_size(img.shape[1], img.shape[0], f)) >= 1}


@pytest.mark.parametrize("factor", jc.FACTORS)
@pytest.mark.parametrize("channels", (1, 3))
def test_resize_equals_the_restatement(capi, resize_reference, channels, factor):
    """All sizes of one kind that the factor admits as ONE mixed batch, and the largest once more alone."""
    names = [n for n in jc.resize_sources() if n.endswith("x%d" % channels) and (n, factor) in resize_reference]
    assert "512x384x%d" % channels in names and "67x43x%d" % channels in names
    got = capi.resize_images([jc.resize_sources()[n] for n in names], factor)
    for n, g in zip(names, got):
        want = resize_reference[(n, factor)]
        assert g.shape == want.shape and np.array_equal(g, want), (n, factor)
    alone = capi.resize_images([jc.resize_sources()[names[-1]]], factor)[0]
    assert alone.tobytes() == got[-1].tobytes()


def test_a_factor_that_gives_a_zero_side_is_refused(capi):
    src = jc.resize_sources()
    assert jo.resized_size(1, 1, 0.25) == (0, 0) and jo.resized_size(2, 3, 0.25)[0] == 0
    for names, f in ((["1x1x1"], 0.25), (["67x43x3", "2x3x3"], 0.25), (["67x43x1"], 0.001), (["67x43x1"], 1000.0)):
        with pytest.raises(capi.SfmbaError) as e:
            capi.resize_images([src[n] for n in names], f)
        assert "rc=1:" in str(e.value)                              # SFMBA_ERR_INVALID_ARG
    with pytest.raises(capi.SfmbaError) as e:
        capi.jpeg_decode([jc.small_file("c422_70x45"), jc.small_file("c420_1x1")], factor=0.25)
    assert "rc=1:" in str(e.value)                              # SFMBA_ERR_INVALID_ARG


def test_fused_decode_and_resize_equals_decode_then_resize(capi):
    names = ["c420_67x43_q95", "c422_71x45", "c444_70x45", "c420_64x48_q30"] + jc.photo_names()[:2]
    files = [jc.small_file(n) if not n.endswith(".JPG") else jc.photo_file(n) for n in names]
    for f in (0.5, 0.37):
        infos, fused = capi.jpeg_decode(files, factor=f)
        _, full = capi.jpeg_decode(files)
        twice = capi.resize_images(full[:4], f) + capi.resize_images(full[4:], f)
        for n, i, a, b, src in zip(names, infos, fused, twice, full):
            assert i["status"] == 0 and (i["height"], i["width"]) == src.shape[:2]        # info keeps the size of the file's own image
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (n, f)
            assert np.array_equal(a, jo.resize(src, f)), (n, f)
    gray_info, gray = capi.jpeg_decode([jc.small_file("gray_70x45")], factor=0.5)
    assert gray[0].shape == (22, 35) and np.array_equal(gray[0], jo.resize(jc.small_pixels("gray_70x45"), 0.5))


# ---- the host side --------------------------------------------------------------------------------------------------------------------
def read_directory(path, factor, cap_images=16, cap=16 << 20):
    lib = C.CDLL(sfm_loop.SHIM)
    w, h, ch = np.zeros(cap_images, np.int32), np.zeros(cap_images, np.int32), C.c_int(0)
    px = np.zeros(cap, np.uint8)
    n = lib.sfmba_shim_read_images_directory_scaled(str(path).encode(), C.c_float(factor), C.c_int(cap_images), C.c_int64(cap),
                                                    w.ctypes.data_as(sfm_loop.ip), h.ctypes.data_as(sfm_loop.ip), C.byref(ch), px.ctypes.data_as(sfm_loop.bp))
    if n < 0:
        return n
    out, at = [], 0
    for i in range(n):
        size = int(w[i]) * int(h[i]) * ch.value
        out.append(px[at:at + size].reshape((h[i], w[i]) if ch.value == 1 else (h[i], w[i], 3)).copy())
        at += size
    return out


def write_ppm(path, bgr):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]) + bgr[:, :, ::-1].tobytes())


def test_set_images_directory_reads_jpeg_and_pnm_in_name_order_and_applies_the_factor(capi, tmp_path):
    a, b = jc.small_pixels("c420_70x45_q60"), jc.small_pixels("c422_70x45")
    (tmp_path / "b_second.JPG").write_bytes(jc.small_file("c422_70x45"))
    (tmp_path / "a_first.jpeg").write_bytes(jc.small_file("c420_70x45_q60"))
    write_ppm(tmp_path / "c_third.ppm", a[::-1].copy())
    (tmp_path / "notes.txt").write_bytes(b"not an image")
    full = read_directory(tmp_path, 1.0)
    assert len(full) == 3 and np.array_equal(full[0], a) and np.array_equal(full[1], b) and np.array_equal(full[2], a[::-1])
    half = read_directory(tmp_path, 0.5)
    assert [im.shape for im in half] == [(22, 35, 3)] * 3
    for got, src in zip(half, full):
        assert np.array_equal(got, jo.resize(src, 0.5))
    (tmp_path / "d_gray.jpg").write_bytes(jc.small_file("gray_70x45"))                 # not of the kind of the files before it
    assert read_directory(tmp_path, 1.0) == -1
    os.remove(tmp_path / "d_gray.jpg")
    (tmp_path / "d_progressive.jpg").write_bytes(jc.small_file("progressive_24x16"))
    assert read_directory(tmp_path, 1.0) == -1


def test_shim_drivers_of_read_and_resize(capi, tmp_path):
    lib = C.CDLL(sfm_loop.SHIM)
    names = ["c420_67x43_q95", "c422_71x45"]
    paths = []
    for n in names:
        (tmp_path / (n + ".jpg")).write_bytes(jc.small_file(n))
        paths.append(str(tmp_path / (n + ".jpg")).encode())
    arr = (C.c_char_p * len(paths))(*paths)
    w, h, ch = np.zeros(4, np.int32), np.zeros(4, np.int32), C.c_int(0)
    px = np.zeros(1 << 20, np.uint8)
    tail = (C.c_int(4), C.c_int64(len(px)), w.ctypes.data_as(sfm_loop.ip), h.ctypes.data_as(sfm_loop.ip), C.byref(ch), px.ctypes.data_as(sfm_loop.bp))
    assert lib.sfmba_shim_read_images(C.c_int(2), arr, C.c_float(0.37), *tail) == 2
    at = 0
    for i, n in enumerate(names):
        want = jo.resize(jc.small_pixels(n), 0.37)
        assert (h[i], w[i], ch.value) == want.shape
        assert np.array_equal(px[at:at + want.size].reshape(want.shape), want), n
        at += want.size
    src = [jc.resize_sources()["67x43x1"], jc.resize_sources()["2x3x1"]]
    flat = np.concatenate([s.reshape(-1) for s in src])
    ptr = np.array([0, src[0].size, flat.size], np.int64)
    sw, sh = np.array([67, 2], np.int32), np.array([43, 3], np.int32)
    assert lib.sfmba_shim_resize_images(C.c_int(2), ptr.ctypes.data_as(sfm_loop.lp), flat.ctypes.data_as(sfm_loop.bp), sw.ctypes.data_as(sfm_loop.ip),
                                        sh.ctypes.data_as(sfm_loop.ip), C.c_int(1), C.c_float(1.5), *tail) == 2
    at = 0
    for i, s in enumerate(src):
        want = jo.resize(s, 1.5)
        assert (h[i], w[i]) == want.shape and ch.value == 1
        assert np.array_equal(px[at:at + want.size].reshape(want.shape), want)
        at += want.size
    missing = (C.c_char_p * 1)(str(tmp_path / "missing.jpg").encode())
    assert lib.sfmba_shim_read_images(C.c_int(1), missing, C.c_float(1.0), *tail) == -1
