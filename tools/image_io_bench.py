"""Image-reader measurement (sfmba_jpeg_decode, sfmba_resize_images): a text report, one block per shape.

  (a) decode of the seven 512 x 384 4:2:2 photographs of tests/golden/crazyhorse_half in ONE call: the host time of the header parse +
      entropy decode (wall clock, at most 16 threads) and the HIP-event times of upload, dequantise + inverse DCT kernel, upsample +
      colour kernel and download (SFMBA_JPEG_TIMING), plus the end-to-end call time
  (b) one resize of a 1024 x 768 x 3 image at 0.5      (c) seven of them in one call
  (d) with --pipeline: sfmtoylib::SfM from the directory of the seven photographs at factor 1 in a fresh deterministic process:
      runSfM's code, the views registered, the cloud size and the RMS reprojection error of the cloud in the final cameras

  (e) with --png: the same seven photographs (their decoded pixels) written as PNG files with a random filter type per row, decoded by
      sfmba_png_decode in ONE call, and one 1024 x 768 x 3 image likewise: host chunk walk + inflate (wall clock, at most 16 threads)
      and the HIP-event times of upload, unfilter kernel, pixel kernel and download (SFMBA_PNG_TIMING); whether the unfilter kernel is
      shorter than the host inflate of the same call; Pillow's decode of the same files on the host where Pillow is importable, for
      scale only

Medians over --reps calls after --warmup.  Every repetition is compared byte for byte with the first.  The 1024 x 768 images are the
decoded photographs enlarged by the resize itself (factor 2), so the tool needs nothing but the repository.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PHASES = ("entropy_ms", "upload_ms", "idct_ms", "colour_ms", "resize_ms", "download_ms")
PNG_PHASES = ("inflate_ms", "upload_ms", "unfilter_ms", "pixels_ms", "resize_ms", "download_ms")


def timed(what, fn, phases=PHASES):
    """fn() with the library's stderr timing line of `what` captured: (result, phases, wall ms)."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = fn()
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    m = re.findall(r"\[sfmba " + what + r"\] " + " ".join(k + r" (\S+)" for k in phases), text)
    if not m:
        raise RuntimeError("no timing line from the library: %r" % text)
    return res, dict(zip(phases, map(float, m[-1]))), wall


def measure(what, fn, same, warmup, reps, phases=PHASES):
    first = None
    rows = []
    for r in range(warmup + reps):
        res, ph, wall = timed(what, fn, phases)
        if first is None:
            first = res
        elif not same(first, res):
            raise RuntimeError("%s: a repetition differs from the first" % what)
        if r >= warmup:
            rows.append(dict(ph, call_ms=wall))
    return first, {k: float(np.median([row[k] for row in rows])) for k in rows[0]}


def same_images(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--png", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ["SFMBA_JPEG_TIMING"] = "1"
    os.environ["SFMBA_PNG_TIMING"] = "1"
    import jpeg_cases as jc
    from sfm_toy_library_amd import capi
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    files = [jc.photo_file(n) for n in jc.photo_names()]
    total = 7 * 512 * 384 * 3
    (_, photos), med = measure("jpeg_decode", lambda: capi.jpeg_decode(files, cap=total), lambda a, b: same_images(a[1], b[1]), args.warmup, args.reps)
    hashes = jc.photo_hashes()
    assert all(jc.sha256(im) == hashes[n] for n, im in zip(jc.photo_names(), photos))
    device = med["upload_ms"] + med["idct_ms"] + med["colour_ms"] + med["download_ms"]
    say("(a) decode, 7 photographs of 512 x 384 (4:2:2, %d file bytes), one call; medians of %d after %d warm-up calls" % (sum(map(len, files)), args.reps, args.warmup))
    say("    host entropy decode %.3f ms | upload %.3f ms | idct kernel %.3f ms | colour kernel %.3f ms | download %.3f ms | call %.3f ms"
        % (med["entropy_ms"], med["upload_ms"], med["idct_ms"], med["colour_ms"], med["download_ms"], med["call_ms"]))
    say("    host entropy decode = %.1f x the two kernels, %.2f x everything on the device side (copies included)"
        % (med["entropy_ms"] / (med["idct_ms"] + med["colour_ms"]), med["entropy_ms"] / device))

    big = capi.resize_images(photos, 2.0)
    assert big[0].shape == (768, 1024, 3)
    for label, imgs in (("(b) resize, 1 image", big[:1]), ("(c) resize, 7 images", big)):
        _, med = measure("resize_images", lambda: capi.resize_images(imgs, 0.5, cap=len(imgs) * 512 * 384 * 3), same_images, args.warmup, args.reps)
        moved = len(imgs) * (1024 * 768 * 3 + 512 * 384 * 3)
        say("%s of 1024 x 768 x 3 at 0.5, one call" % label)
        say("    upload %.3f ms | resize kernel %.3f ms (%.1f GB/s over the %d bytes read and written once) | download %.3f ms | call %.3f ms"
            % (med["upload_ms"], med["resize_ms"], moved / med["resize_ms"] / 1e6, moved, med["download_ms"], med["call_ms"]))

    if args.png:
        import png_oracle as po
        rng = np.random.default_rng(7)
        for label, imgs in (("(e) PNG decode, the 7 photographs of 512 x 384 x 3", photos), ("    PNG decode, 1 image of 1024 x 768 x 3", big[:1])):
            pngs = [po.write_png(im[:, :, ::-1], 2, 8, rng=rng) for im in imgs]
            cap = sum(im.size for im in imgs)
            (_, got), med = measure("png_decode", lambda: capi.png_decode(pngs, cap=cap), lambda a, b: same_images(a[1], b[1]), args.warmup, args.reps, PNG_PHASES)
            assert same_images(got, imgs)
            say("%s (%d file bytes, random filter types per row), one call" % (label, sum(map(len, pngs))))
            say("    host inflate %.3f ms | upload %.3f ms | unfilter kernel %.3f ms | pixel kernel %.3f ms | download %.3f ms | call %.3f ms"
                % (med["inflate_ms"], med["upload_ms"], med["unfilter_ms"], med["pixels_ms"], med["download_ms"], med["call_ms"]))
            say("    the unfilter kernel is %s than the host inflate of the same call (%.2f x)"
                % ("SHORTER" if med["unfilter_ms"] < med["inflate_ms"] else "NOT shorter", med["unfilter_ms"] / med["inflate_ms"]))
            try:
                import io
                from PIL import Image
                t = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    for data in pngs:
                        Image.open(io.BytesIO(data)).load()
                    t.append(1e3 * (time.perf_counter() - t0))
                say("    Pillow on the host, one file after another, for scale: %.3f ms" % float(np.median(t)))
            except ImportError:
                say("    (Pillow is not importable here)")

    if args.pipeline:
        import shutil
        import sfm_loop
        import image_io_loop
        tmp = tempfile.mkdtemp()
        directory = os.path.join(tmp, "photos")
        os.makedirs(directory)
        for n in jc.photo_names():
            shutil.copy(os.path.join(jc.PHOTOS, n), directory)
        env = {k: v for k, v in os.environ.items() if not k.startswith("SFMBA_")}
        env.update(SFMBA_DETERMINISTIC="1", SFMBA_SHIM_CACHE="0")
        out = os.path.join(tmp, "class.npz")
        t0 = time.perf_counter()
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "image_io_loop.py"), "class", directory, "1.0", out], env=env, check=True, timeout=300)
        wall = time.perf_counter() - t0
        res = dict(np.load(out))
        say("(d) sfmtoylib::SfM on the directory of the 7 photographs (512 x 384, f = 2500), factor 1, a fresh process of %.1f s" % wall)
        if int(res["code"]) == 0:
            views, cloud, rms = image_io_loop.figures(res, sfm_loop.extract_features(np.stack(photos)))
            say("    runSfM OKAY: %d of 7 views registered (good %s), cloud %d points, rms reprojection %.4f px"
                % (views, "".join(str(int(g)) for g in res["good"]), cloud, rms))
        else:
            say("    runSfM ERROR (the baseline did not start)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
