"""sfmba_png_decode on the MI355X (-m gpu) against the stored pixels of tests/golden/png_small and against the Python restatement of
the contract (tests/png_oracle.py), byte for byte; the host drivers (SfMImageUtilities::readImages, SfM::setImagesDirectory, runSfM,
sfmtoy) on directories of PNG files against the same pixels given as JPEG, PPM or arrays.

  decode      every decodable fixture equals its stored pixels; all fixtures in one call equal the single calls; a refused file has no
              pixels and does not disturb its neighbours; cap too small is SFMBA_ERR_CAPACITY with the needed total and out untouched;
              a factor that gives a zero side is SFMBA_ERR_INVALID_ARG
  sweep       60 images built here with a fixed seed -- width and height 1..200, every type / depth, random filter types per row,
              stored / fixed / dynamic blocks -- in one call, each held to the restatement
  resize      the fused decode at 0.5 and 0.37 equals decode followed by sfmba_resize_images and the restated resize
  large       640 x 480 x 3 with random filters: 8 bands of 64 rows, 11 tiles of 64 pixels per band
  photographs the seven Crazy Horse photographs, decoded by sfmba_jpeg_decode, written as PNG by the test's writer and read back: one
              call, the directory driver at 1.0 and 0.5 against the JPEG directory, a directory mixing .png, .jpg and .ppm, a gray
              PNG among colour files
  pipeline    runSfM from a directory of PNG files (fresh deterministic processes) equals setImages with those pixels; sfmtoy on the
              PNG directory at 0.5 writes the PLY files it writes for the same pixels as PPM"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_oracle as jo
import png_cases as pc
import png_oracle as po
import sfm_loop

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SFMTOY = os.path.join(ROOT, "sfm-toy-library_amd", "host", "sfmtoy")


@pytest.fixture(scope="module")
def capi():
    from sfm_toy_library_amd import capi
    return capi


@pytest.fixture(scope="module")
def small_decoded(capi):
    """One call over every file of png_small: name -> (info, image)."""
    names = pc.small_names()
    infos, images = capi.png_decode([pc.small_file(n) for n in names])
    return {n: (i, im) for n, i, im in zip(names, infos, images)}


def samples_of(img):
    """uint8 pixels [h, w] or [h, w, 3] B, G, R -> the sample array of an 8-bit gray or RGB file."""
    return img[:, :, None] if img.ndim == 2 else img[:, :, ::-1]


def png_of(img, rng, **kw):
    return po.write_png(samples_of(img), 0 if img.ndim == 2 else 2, 8, rng=rng, **kw)


# ---- decode -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.decodable_names())
def test_decode_equals_the_stored_pixels(small_decoded, name):
    info, img = small_decoded[name]
    want = pc.small_pixels(name)
    assert tuple(info[k] for k in ("status", "width", "height", "channels", "bit_depth", "colour_type", "interlace")) == po.info(pc.small_file(name))
    assert img.shape == want.shape and np.array_equal(img, want), (name, int(np.abs(img.astype(int) - want.astype(int)).max()))


def test_the_batch_equals_the_single_calls(capi, small_decoded):
    for name in pc.small_names():
        one_info, one = capi.png_decode([pc.small_file(name)])
        info, img = small_decoded[name]
        assert one_info[0] == info, name
        assert (one[0] is None) == (img is None) and (img is None or one[0].tobytes() == img.tobytes()), name
    assert capi.png_decode([]) == ([], [])


def test_refusals_have_no_pixels_and_their_neighbours_decode(capi, small_decoded):
    for name, (status, _) in pc.REFUSALS.items():
        info, img = small_decoded[name]
        assert info == dict(status=status, width=0, height=0, channels=0, bit_depth=0, colour_type=0, interlace=0) and img is None, name
    good = "t6_d8_37x70"
    files = [pc.small_file(good)]
    for name in pc.REFUSALS:
        files += [pc.small_file(name), pc.small_file(good)]
    infos, images = capi.png_decode(files)
    assert [i["status"] for i in infos] == [0] + [s for st, _ in pc.REFUSALS.values() for s in (st, 0)]
    for i, im in zip(infos, images):
        assert (im is None) if i["status"] else np.array_equal(im, pc.small_pixels(good))


def test_capacity_too_small_reports_the_total_and_writes_nothing(capi):
    names = ["t2_d8_37x70_two_idat", "t0_d1_13x65"]
    ptr, flat = capi._flat_files([pc.small_file(n) for n in names])
    need = 37 * 70 * 3 + 13 * 65
    info = (capi._PngInfo * 2)()
    out_ptr, total = np.zeros(3, np.int64), C.c_int64(0)
    out = np.full(need, 0xAB, np.uint8)
    lp, bp = C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)
    args = (C.c_int(0), C.c_int(2), ptr.ctypes.data_as(lp), flat.ctypes.data_as(bp), C.c_float(1.0), info, out_ptr.ctypes.data_as(lp), out.ctypes.data_as(bp))
    rc = capi.lib().sfmba_png_decode(*args, C.c_int64(need - 1), C.byref(total))
    assert rc == capi.SFMBA_ERR_CAPACITY and total.value == need and out_ptr.tolist() == [0, 37 * 70 * 3, need]
    assert [info[0].status, info[0].width, info[1].channels] == [0, 37, 1] and np.all(out == 0xAB)
    rc = capi.lib().sfmba_png_decode(*args, C.c_int64(need), C.byref(total))
    assert rc == 0 and np.array_equal(out[:37 * 70 * 3].reshape(70, 37, 3), pc.small_pixels(names[0]))
    assert np.array_equal(out[37 * 70 * 3:].reshape(65, 13), pc.small_pixels(names[1]))


def test_a_factor_that_gives_a_zero_side_is_refused(capi):
    for names, f in ((["t2_d8_37x70_two_idat", "w1_t2_d8_1x70"], 0.25), (["t0_d8_37x129"], 0.001), (["t0_d8_37x129"], 1000.0)):
        with pytest.raises(capi.SfmbaError) as e:
            capi.png_decode([pc.small_file(n) for n in names], factor=f)
        assert "rc=1:" in str(e.value)                              # SFMBA_ERR_INVALID_ARG
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.SfmbaError):
            capi.png_decode([pc.small_file("t0_d8_37x129")], factor=bad)


# ---- the random sweep -------------------------------------------------------------------------------------------------------------------
def test_random_sweep_equals_the_restatement(capi):
    rng = np.random.default_rng(60)
    files, wants = [], []
    for k in range(60):
        ct, depth = po.ALL_PAIRS[k % 15] if k < 30 else po.ALL_PAIRS[int(rng.integers(0, 15))]
        w, h = int(rng.integers(1, 201)), int(rng.integers(1, 201))
        palette = po.random_palette(rng, int(rng.integers(1, (1 << depth) + 1))) if ct == 3 else None
        samples = po.random_samples(rng, w, h, ct, depth)
        if k % 3 == 0:                                                 # a smooth image: the filters then leave something to compress
            samples = (samples // 8 + (np.add.outer(np.arange(h), np.arange(w))[:, :, None] * 3)) % (1 << depth)
        data = po.write_png(samples, ct, depth, rng=rng, mode=("stored", "fixed", "dynamic")[int(rng.integers(0, 3))], palette=palette,
                            splits=sorted(int(v) for v in rng.integers(1, 400, int(rng.integers(0, 4)))))
        status, want = po.decode(data)
        assert status == po.OK, k
        files.append(data)
        wants.append(want)
    infos, images = capi.png_decode(files)
    wrong = [k for k, (i, im, want) in enumerate(zip(infos, images, wants)) if i["status"] != 0 or im.shape != want.shape or not np.array_equal(im, want)]
    assert not wrong, (wrong, [po.info(files[k]) for k in wrong])


# ---- resize and the large image ------------------------------------------------------------------------------------------------------
def test_fused_decode_and_resize_equals_decode_then_resize(capi):
    colour = ["t2_d8_37x70_two_idat", "t3_d8_37x70", "t6_d16_21x33", "fixed_t2_d8_40x30"]
    gray = ["t0_d8_37x129", "t4_d8_37x70", "t0_d2_13x63"]
    for names in (colour, gray):
        files = [pc.small_file(n) for n in names]
        _, full = capi.png_decode(files)
        for f in (0.5, 0.37):
            infos, fused = capi.png_decode(files, factor=f)
            twice = capi.resize_images(full, f)
            for n, i, a, b, src in zip(names, infos, fused, twice, full):
                assert i["status"] == 0 and (i["height"], i["width"]) == src.shape[:2]        # info keeps the size of the file's own image
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (n, f)
                assert np.array_equal(a, jo.resize(src, f)), (n, f)


def test_one_larger_image_with_random_filters(capi):
    rng = np.random.default_rng(640)
    ramp = np.add.outer(np.arange(480) * 2, np.arange(640))[:, :, None] + np.arange(3) * 40
    img = ((ramp + rng.integers(0, 32, (480, 640, 3))) % 256).astype(np.uint8)
    data = png_of(img, rng)
    assert len(set(po.stream(data, po.walk(data))[1][0::640 * 3 + 1])) == 5
    infos, images = capi.png_decode([data])
    assert infos[0] == dict(status=0, width=640, height=480, channels=3, bit_depth=8, colour_type=2, interlace=0)
    assert np.array_equal(images[0], img)
    _, half = capi.png_decode([data], factor=0.5)
    assert np.array_equal(half[0], jo.resize(img, 0.5))


# ---- the photographs and the host side ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def photographs(capi, tmp_path_factory):
    """(names, decoded pixels, PNG files, directory of the PNG files, directory of the JPEG files)."""
    names = jc.photo_names()
    infos, pixels = capi.jpeg_decode([jc.photo_file(n) for n in names])
    assert all(i["status"] == 0 for i in infos)
    rng = np.random.default_rng(7)
    pngs = [png_of(px, rng, splits=(8192, 70000)) for px in pixels]
    png_dir, jpeg_dir = tmp_path_factory.mktemp("photos_png"), tmp_path_factory.mktemp("photos_jpeg")
    for n, data in zip(names, pngs):
        (png_dir / (os.path.splitext(n)[0] + ".png")).write_bytes(data)
        shutil.copy(os.path.join(jc.PHOTOS, n), jpeg_dir)
    return names, pixels, pngs, str(png_dir), str(jpeg_dir)


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


def test_the_seven_photographs_come_back_in_one_call(capi, photographs):
    names, pixels, pngs, _, _ = photographs
    infos, images = capi.png_decode(pngs)
    hashes = jc.photo_hashes()
    for n, i, im, want in zip(names, infos, images, pixels):
        assert i == dict(status=0, width=512, height=384, channels=3, bit_depth=8, colour_type=2, interlace=0)
        assert im.tobytes() == want.tobytes() and jc.sha256(im) == hashes[n], n


def test_the_png_directory_equals_the_jpeg_directory(photographs):
    _, pixels, _, png_dir, jpeg_dir = photographs
    for f in (1.0, 0.5):
        a, b = read_directory(png_dir, f), read_directory(jpeg_dir, f)
        assert len(a) == len(b) == 7
        for x, y, src in zip(a, b, pixels):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), f
            assert np.array_equal(x, src if f == 1.0 else jo.resize(src, f))


def test_a_directory_mixing_png_jpeg_and_ppm_is_read_in_name_order(capi, tmp_path):
    rng = np.random.default_rng(3)
    a, b = jc.small_pixels("c420_70x45_q60"), jc.small_pixels("c422_70x45")
    (tmp_path / "a_first.PNG").write_bytes(png_of(b, rng))
    (tmp_path / "b_second.jpg").write_bytes(jc.small_file("c420_70x45_q60"))
    write_ppm(tmp_path / "c_third.ppm", a[::-1].copy())
    (tmp_path / "d_fourth.png").write_bytes(po.write_png(a[:, :, ::-1].astype(np.int64) * 257, 2, 16, rng=rng))      # 16 bits: the high byte is a
    (tmp_path / "notes.txt").write_bytes(b"not an image")
    full = read_directory(tmp_path, 1.0)
    assert len(full) == 4
    assert np.array_equal(full[0], b) and np.array_equal(full[1], a) and np.array_equal(full[2], a[::-1]) and np.array_equal(full[3], a)
    half = read_directory(tmp_path, 0.5)
    assert [im.shape for im in half] == [(22, 35, 3)] * 4
    for got, src in zip(half, full):
        assert np.array_equal(got, jo.resize(src, 0.5))
    (tmp_path / "e_gray.png").write_bytes(png_of(a[:, :, 1].copy(), rng))              # not of the kind of the files before it
    assert read_directory(tmp_path, 1.0) == -1
    os.remove(tmp_path / "e_gray.png")
    (tmp_path / "e_interlaced.png").write_bytes(pc.small_file("bad_interlaced"))
    assert read_directory(tmp_path, 1.0) == -1
    os.remove(tmp_path / "e_interlaced.png")
    (tmp_path / "e_named_wrongly.png").write_bytes(jc.small_file("c422_70x45"))         # the signature decides: this is a JPEG file
    assert np.array_equal(read_directory(tmp_path, 1.0)[4], b)


# ---- one pipeline run -------------------------------------------------------------------------------------------------------------------
CHILD_TIMEOUT = 180
FAILED = []
KEYS = ("code", "added_view", "added_posed", "added_cloud", "done", "good", "view_ptr", "view_idx", "feat_idx", "poses", "xyz", "K")


def child(cmd, what):
    """One fresh deterministic process; nothing more is started on the device after one went wrong."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
    env.update(SFMBA_DETERMINISTIC="1", SFMBA_SHIM_CACHE="0")
    if FAILED:
        pytest.fail("not started: an earlier child process failed (%s)" % FAILED[0])
    try:
        done = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except subprocess.TimeoutExpired:
        FAILED.append("%s overran %d s" % (what, CHILD_TIMEOUT))
        pytest.fail("%s overran its %d s" % (what, CHILD_TIMEOUT))
    if done.returncode < 0 or done.returncode > 2:
        FAILED.append("%s ended with %d" % (what, done.returncode))
        pytest.fail("%s ended with %d:\n%s" % (what, done.returncode, done.stderr.decode()[-2000:]))
    return done


def run_program(script, args, out):
    done = child([sys.executable, os.path.join(HERE, script)] + args + [out], script + " " + args[0])
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def corner_dirs(tmp_path_factory):
    """The four rendered 640 x 480 corner views as PNG files (random filters) and as PPM files, and their pixels."""
    import sfm_scene
    gray = np.stack(sfm_scene.make_corner(seed=0)["images"])
    bgr = np.stack([255 - gray, gray, gray], axis=3)                    # the blue channel inverted: a B / R swap would show
    png_dir, ppm_dir = tmp_path_factory.mktemp("corner_png"), tmp_path_factory.mktemp("corner_ppm")
    rng = np.random.default_rng(11)
    for i, im in enumerate(bgr):
        (png_dir / ("view%02d.png" % i)).write_bytes(png_of(im, rng))
        write_ppm(ppm_dir / ("view%02d.ppm" % i), im)
    return str(png_dir), str(ppm_dir), bgr


def test_run_sfm_from_a_png_directory_equals_set_images(corner_dirs, tmp_path):
    png_dir, _, bgr = corner_dirs
    from_dir = run_program("image_io_loop.py", ["class", png_dir, "1.0"], str(tmp_path / "dir.npz"))
    src = str(tmp_path / "in.npz")
    np.savez(src, images=bgr)
    from_images = run_program("sfm_loop.py", ["class", src], str(tmp_path / "images.npz"))
    assert int(from_dir["code"]) == 0 and int(from_images["code"]) == 0 and from_dir["good"].sum() >= 3
    for k in KEYS:
        assert from_dir[k].shape == from_images[k].shape and from_dir[k].tobytes() == from_images[k].tobytes(), k


def test_sfmtoy_on_png_files_writes_the_ply_files_of_the_same_pixels_as_ppm(corner_dirs, tmp_path):
    png_dir, ppm_dir, _ = corner_dirs
    out = {}
    for kind, directory in (("png", png_dir), ("ppm", ppm_dir)):
        prefix = str(tmp_path / kind)
        done = child([SFMTOY, "-p", directory, "-s", "0.5", "-o", prefix], "sfmtoy " + kind)
        assert done.returncode == 0, done.stderr.decode()[-2000:]
        out[kind] = [open(prefix + suffix, "rb").read() for suffix in ("_points.ply", "_cameras.ply")]
    assert len(out["png"][0]) > 300 and out["png"] == out["ppm"]
