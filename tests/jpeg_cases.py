"""The JPEG fixtures of tests/golden (written by tests/golden/make_jpeg_golden.py) and the resize cases shared by the CPU and the GPU
tests of sfmba_jpeg_decode / sfmba_resize_images -- TEST INFRASTRUCTURE ONLY.  Nothing here needs Pillow."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(HERE, "golden", "jpeg_small")
PHOTOS = os.path.join(HERE, "golden", "crazyhorse_half")
UNSUPPORTED = ("progressive_24x16", "cmyk_24x16")
FACTORS = (0.5, 0.25, 0.37, 1.0, 1.5)
_cache = {}


def small_names():
    return sorted(n[:-4] for n in os.listdir(SMALL) if n.endswith(".jpg"))


def decodable_names():
    return [n for n in small_names() if n not in UNSUPPORTED]


def small_file(name):
    with open(os.path.join(SMALL, name + ".jpg"), "rb") as f:
        return f.read()


def small_pixels(name):
    """libjpeg's decode: [h, w] gray or [h, w, 3] B, G, R."""
    if "npz" not in _cache:
        _cache["npz"] = dict(np.load(os.path.join(SMALL, "decoded.npz")))
    return _cache["npz"][name]


def photo_names():
    return sorted(n for n in os.listdir(PHOTOS) if n.lower().endswith(".jpg"))


def photo_file(name):
    with open(os.path.join(PHOTOS, name), "rb") as f:
        return f.read()


def photo_hashes():
    with open(os.path.join(PHOTOS, "decoded_sha256.json")) as f:
        return json.load(f)["sha256"]


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def resize_sources():
    """name -> uint8 image: 1 and 3 channels at 1 x 1, 2 x 3, 67 x 43 and 512 x 384 (w x h), noise over a gradient."""
    if "src" not in _cache:
        rng = np.random.default_rng(5)
        out = {}
        for w, h in ((1, 1), (2, 3), (67, 43), (512, 384)):
            for ch in (1, 3):
                ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256)[:, :, None]
                img = np.clip(ramp + rng.integers(-40, 41, (h, w, ch)), 0, 255).astype(np.uint8)
                out["%dx%dx%d" % (w, h, ch)] = img[:, :, 0] if ch == 1 else img
        _cache["src"] = out
    return _cache["src"]


def patch_sof_precision(data, precision):
    """The file with the sample precision of its SOF0 segment overwritten."""
    at = data.index(b"\xff\xc0")
    return data[:at + 4] + bytes([precision]) + data[at + 5:]


def patch_dqt_16bit(data):
    """The file with the precision nibble of its first quantisation table set to 1 (16-bit entries)."""
    at = data.index(b"\xff\xdb")
    return data[:at + 4] + bytes([data[at + 4] | 0x10]) + data[at + 5:]
