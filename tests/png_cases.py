"""The PNG fixtures of tests/golden/png_small (written by tests/golden/make_png_golden.py) shared by the CPU and the GPU tests of
sfmba_png_info / sfmba_png_decode -- TEST INFRASTRUCTURE ONLY.  Nothing here needs Pillow."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(HERE, "golden", "png_small")
# name -> (status of the decode, status of the chunk walk alone): what sfmba_png_decode and sfmba_png_info must report
REFUSALS = {
    "bad_interlaced": (1, 1),
    "bad_crc": (2, 2),
    "bad_cut_file": (2, 2),            # the file ends inside its IDAT chunk: a chunk length past the end
    "bad_no_plte": (2, 2),
    "bad_depth3": (2, 2),
    "bad_adler": (2, 0),               # these four are in order as far as the chunks go; the zlib stream is not
    "bad_truncated_idat": (2, 0),
    "bad_filter5": (2, 0),
    "bad_surplus": (2, 0),
}
_cache = {}


def small_names():
    return sorted(n[:-4] for n in os.listdir(SMALL) if n.endswith(".png"))


def decodable_names():
    return [n for n in small_names() if n not in REFUSALS]


def small_file(name):
    with open(os.path.join(SMALL, name + ".png"), "rb") as f:
        return f.read()


def small_pixels(name):
    """The stored decode: [h, w] gray or [h, w, 3] B, G, R."""
    if "npz" not in _cache:
        _cache["npz"] = dict(np.load(os.path.join(SMALL, "decoded.npz")))
    return _cache["npz"][name]
