"""The images of the float-descriptor extraction tests -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_surf_extract.py holds the device
to the oracle on every one of them; tests/test_surf_oracle_cpu.py holds the host build of csrc/surf_math.h to the oracle on the same
set.  The oracle's answer is computed once per case and shared (oracle(name)); nobody may change what it returns."""
import numpy as np

import surf_oracle as so


def smooth3(a):
    """3 x 3 box mean of an array, edges replicated."""
    p = np.pad(a.astype(np.float64), 1, mode="edge")
    return sum(p[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(3) for dx in range(3)) / 9.0


def noise(seed, w, h, channels=1):
    """Uniform noise smoothed 3 x 3 (per channel), stretched to 0..255."""
    rng = np.random.default_rng(seed)
    planes = []
    for _ in range(channels):
        a = smooth3(rng.random((h, w)))
        planes.append(np.floor((a - a.min()) / max(a.max() - a.min(), 1e-12) * 255.0 + 0.5).astype(np.uint8))
    return planes[0] if channels == 1 else np.ascontiguousarray(np.stack(planes, axis=2))


def tiled_block(seed=5, w=150, h=120, block=32):
    blk = noise(seed, block, block)
    return np.ascontiguousarray(np.tile(blk, (h // block + 1, w // block + 1))[:h, :w])


def blob(w, h, cx, cy, sigma):
    """A bright Gaussian blob on a dark ground."""
    y, x = np.mgrid[0:h, 0:w]
    return np.floor(20.0 + 200.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma)) + 0.5).astype(np.uint8)


_texture = None


def texture():
    """The 300 x 300 texture of the descriptor sanity test, as float64 in 0..255 (not yet rounded)."""
    global _texture
    if _texture is None:
        from scipy.ndimage import gaussian_filter
        rng = np.random.default_rng(5)
        t = gaussian_filter(rng.random((300, 300)), 2) + 0.5 * gaussian_filter(rng.random((300, 300)), 5)
        _texture = (t - t.min()) / (t.max() - t.min()) * 255.0
        _texture.setflags(write=False)
    return _texture


def to_u8(a):
    return np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)


P = dict(n_features=300, n_octaves=3, hessian_threshold=2.0, upright=0)      # what the noise cases share (so they can form a batch)


def _build():
    c = {}
    c["noise_1x1"] = (lambda: noise(1, 1, 1), P)
    c["none_23x40"] = (lambda: noise(2, 23, 40), P)
    c["none_40x23"] = (lambda: noise(3, 40, 23), P)
    c["noise_24x24"] = (lambda: noise(14, 24, 24), dict(P, hessian_threshold=0.0))      # four admissible positions; seed chosen by the oracle: one is a key point
    c["noise_25x31"] = (lambda: noise(5, 25, 31), dict(P, hessian_threshold=0.0))
    c["noise_40x40"] = (lambda: noise(6, 40, 40), P)                                    # octave 1 has no admissible position
    for k, wd in enumerate((63, 64, 65)):
        c["width_%d" % wd] = (lambda wd=wd, k=k: noise(10 + k, wd, 50), P)
    c["noise_130x257"] = (lambda: noise(7, 130, 257), P)
    for n in (1, 2, 3, 4):
        c["octaves_%d_100x90" % n] = (lambda: noise(8, 100, 90), dict(P, n_octaves=n))
    c["upright_100x90"] = (lambda: noise(8, 100, 90), dict(P, upright=1))
    c["ties_150x120"] = (tiled_block, dict(P, n_features=10, n_octaves=1))              # 10: inside a group of equal H (asserted)
    c["bgr_100x90"] = (lambda: noise(9, 100, 90, 3), P)
    c["uniform_60x60"] = (lambda: np.full((60, 60), 77, np.uint8), dict(P, hessian_threshold=0.0))
    c["texture_300x300"] = (lambda: to_u8(texture()), dict(P, hessian_threshold=20.0))
    c["four_octaves_260x250"] = (lambda: to_u8(texture()[20:270, 10:270]), dict(P, n_octaves=4, hessian_threshold=20.0))
    c["blob_300x300"] = (lambda: blob(300, 300, 152, 152, 16.0), dict(P, n_octaves=4))  # found in octave 3 (step 8; 152 = 19 * 8)
    return c


CASES = _build()
BATCH = ["noise_130x257", "noise_40x40", "none_23x40", "width_64", "noise_1x1", "octaves_3_100x90"]   # six sizes, two without key points
_images, _oracle = {}, {}


def image(name):
    if name not in _images:
        img = CASES[name][0]()
        img.setflags(write=False)
        _images[name] = img
    return _images[name]


def params(name):
    return dict(CASES[name][1])


def oracle(name):
    if name not in _oracle:
        _oracle[name] = so.extract(image(name), **CASES[name][1])
    return _oracle[name]
