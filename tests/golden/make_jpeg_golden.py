"""Writes the JPEG fixtures: tests/golden/jpeg_small/ (small files + libjpeg's decode of each in decoded.npz) and
tests/golden/crazyhorse_half/ (the seven Crazy Horse photographs at 512 x 384 + decoded_sha256.json).

    python tests/golden/make_jpeg_golden.py --photos DIR        DIR holds the seven 1024 x 768 photographs (P1000965.JPG ...)

Needs Pillow (built on libjpeg-turbo); the tests do not: they read what this wrote.  The stored pixels are Pillow's default
decode (integer "islow" inverse DCT, fancy upsampling) with the channels turned into B, G, R, the layout sfmba_jpeg_decode returns.
Everything is derived from a fixed seed, so a rerun with the same Pillow reproduces the files."""
import argparse
import hashlib
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def decoded(data):
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return a if a.ndim == 2 else np.ascontiguousarray(a[:, :, ::-1])


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photos", required=True)
    args = ap.parse_args()
    names = sorted(n for n in os.listdir(args.photos) if n.lower().endswith((".jpg", ".jpeg")))
    assert len(names) == 7, names
    rng = np.random.default_rng(20260101)
    photo = np.asarray(Image.open(os.path.join(args.photos, names[0])).convert("RGB"))

    def cut(w, h):                                            # a detailed patch of the photograph with noise on top
        patch = photo[300:300 + h, 420:420 + w].astype(np.int32) + rng.integers(-12, 13, (h, w, 3))
        return np.clip(patch, 0, 255).astype(np.uint8)

    def gray(a):
        return np.asarray(Image.fromarray(a).convert("L"))

    checker = np.zeros((32, 40, 3), np.uint8)
    checker[(np.add.outer(np.arange(32), np.arange(40)) % 2) == 1] = 255
    cmyk = np.concatenate([cut(24, 16), cut(24, 16)[:, :, :1]], axis=2)
    cases = {
        "c444_70x45": encode(cut(70, 45), quality=85, subsampling=0),
        "c422_70x45": encode(cut(70, 45), quality=85, subsampling=1),
        "c422_71x45": encode(cut(71, 45), quality=85, subsampling=1),
        "c420_70x45_q60": encode(cut(70, 45), quality=60, subsampling=2),
        "c420_67x43_q95": encode(cut(67, 43), quality=95, subsampling=2),
        "c420_64x48_q30": encode(cut(64, 48), quality=30, subsampling=2),
        "gray_70x45": encode(gray(cut(70, 45)), quality=85),
        "c422_33x17_rst3": encode(cut(33, 17), quality=85, subsampling=1, restart_marker_blocks=3),
        "c420_40x40_rst2": encode(cut(40, 40), quality=85, subsampling=2, restart_marker_blocks=2),
        "c420_48x32_optimised": encode(cut(48, 32), quality=75, subsampling=2, optimize=True),
        "c422_40x24_app1_com": encode(cut(40, 24), quality=85, subsampling=1, exif=b"Exif\x00\x00" + bytes(rng.integers(0, 256, 6000, dtype=np.uint8)),
                                      comment=b"a comment segment " * 20),
        "c420_1x1": encode(cut(1, 1), quality=85, subsampling=2),
        "c422_8x8": encode(cut(8, 8), quality=85, subsampling=1),
        "c444_16x16": encode(cut(16, 16), quality=85, subsampling=0),
        "c420_17x9": encode(cut(17, 9), quality=85, subsampling=2),
        "c420_checker_q10": encode(checker, quality=10, subsampling=2),
        "progressive_24x16": encode(cut(24, 16), quality=85, subsampling=2, progressive=True),
        "cmyk_24x16": encode_cmyk(cmyk),
    }
    small = os.path.join(HERE, "jpeg_small")
    os.makedirs(small, exist_ok=True)
    px = {}
    for name, data in cases.items():
        with open(os.path.join(small, name + ".jpg"), "wb") as f:
            f.write(data)
        if not name.startswith(("progressive", "cmyk")):
            px[name] = decoded(data)
    np.savez_compressed(os.path.join(small, "decoded.npz"), **px)

    half = os.path.join(HERE, "crazyhorse_half")
    os.makedirs(half, exist_ok=True)
    sums = {}
    for n in names:
        im = Image.open(os.path.join(args.photos, n)).convert("RGB").resize((512, 384), Image.LANCZOS)
        data = encode(np.asarray(im), quality=80, subsampling=1)
        with open(os.path.join(half, n), "wb") as f:
            f.write(data)
        sums[n] = hashlib.sha256(decoded(data).tobytes()).hexdigest()
    with open(os.path.join(half, "decoded_sha256.json"), "w") as f:
        json.dump({"layout": "384 x 512 x 3 bytes, B, G, R interleaved, rows tight", "sha256": sums}, f, indent=1, sort_keys=True)
        f.write("\n")


def encode_cmyk(arr):
    buf = io.BytesIO()
    Image.fromarray(arr, "CMYK").save(buf, "JPEG", quality=85)
    return buf.getvalue()


if __name__ == "__main__":
    main()
