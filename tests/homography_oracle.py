"""CPU restatement of the baseline-ranking contract (include/sfmba.h, sfmba_homography_ransac) -- TEST INFRASTRUCTURE ONLY.

The contract is this project's own (the seeded splitmix64 sample stream of sfmba_pnp_ransac, a four-point homography with a
collinearity and an orientation test, an all-hypotheses consensus on the forward transfer error, no refit); it is NOT the sample
stream of cv::findHomography.  Everything here is fp64 numpy and takes a different route from the device where there is a choice:

  sample        pnp_oracle.sample (Python ints, masked to 64 bits)
  determinants  numpy.linalg.det of the 3 x 3 matrices of normalised homogeneous points (LU; the device expands twice the signed
                triangle area)
  homography    the null vector of the 8 x 9 DLT matrix of the normalised points, by SVD (the device: a closed form from the Cramer
                ratios of those determinants), then de-normalised and scaled

Allowed importers: tests/ and tools/.
"""
import numpy as np

import pnp_oracle

MIN_DET = 1e-3                # |triple determinant| at or below this: three of the four sample points nearly collinear
TRIPLES = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))       # triple k omits point k and keeps ascending order


def sample(seed, p, h, n):
    return pnp_oracle.sample(seed, p, h, n)


def normalise(pts4):
    """(normalised points [4,2], c [2], s): c = the mean, s = the mean of |coordinate - c| over the eight numbers (None if s == 0)."""
    pts4 = np.asarray(pts4, np.float64).reshape(4, 2)
    c = pts4.mean(axis=0)
    s = np.abs(pts4 - c).mean()
    if not s > 0:
        return None, c, s
    return (pts4 - c) / s, c, s


def triple_determinants(n4):
    a = np.concatenate([np.asarray(n4, np.float64), np.ones((4, 1))], axis=1)
    return np.array([np.linalg.det(a[list(t)].T) for t in TRIPLES])


def hypothesis(l4, r4):
    """The contract's hypothesis from four correspondences l4 -> r4: (H [3,3] or None, info).  info: dl, dr (the triple
    determinants of the two sides, None when a side has no scale)."""
    nl, cl, sl = normalise(l4)
    nr, cr, sr = normalise(r4)
    info = dict(dl=None, dr=None)
    if nl is None or nr is None:
        return None, info
    dl, dr = triple_determinants(nl), triple_determinants(nr)
    info.update(dl=dl, dr=dr)
    if not (np.all(np.abs(dl) > MIN_DET) and np.all(np.abs(dr) > MIN_DET)):
        return None, info
    prod = dl * dr
    if not (np.all(prod > 0) or np.all(prod < 0)):
        return None, info
    A = np.zeros((8, 9))
    for i in range(4):
        x, y = nl[i]
        u, v = nr[i]
        A[2 * i] = [x, y, 1, 0, 0, 0, -u * x, -u * y, -u]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y, -v]
    Hn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    Tl = np.array([[1 / sl, 0, -cl[0] / sl], [0, 1 / sl, -cl[1] / sl], [0, 0, 1]])
    Tri = np.array([[sr, 0, cr[0]], [0, sr, cr[1]], [0, 0, 1]])
    H = Tri @ Hn @ Tl
    w = H[2] @ np.array([cl[0], cl[1], 1.0])
    if not (np.isfinite(w) and w != 0):
        return None, info
    return H / w, info


def ill_conditioned(info):
    """The rule of tests/test_gpu_homography_ransac.py: some |d| lies within 1e-9 of the 1e-3 validity threshold or of 0 (the
    verdict, or the sign of a product, then hangs on the last bits of a determinant)."""
    if info["dl"] is None or info["dr"] is None:
        return False
    d = np.abs(np.concatenate([info["dl"], info["dr"]]))
    return bool(np.any(np.abs(d - MIN_DET) <= 1e-9) or np.any(d <= 1e-9))


def hypotheses(left, right, n_hyp, seed=0, p=0):
    """[(sample or None, H or None, info)] for h = 0 .. n_hyp - 1 over the aligned correspondences left -> right."""
    left = np.asarray(left, np.float64).reshape(-1, 2)
    right = np.asarray(right, np.float64).reshape(-1, 2)
    out = []
    for h in range(n_hyp):
        s = sample(seed, p, h, len(left))
        if s is None:
            out.append((None, None, dict(dl=None, dr=None)))
            continue
        H, info = hypothesis(left[s], right[s])
        out.append((s, H, info))
    return out


def transfer(H, left):
    """(H x de-homogenised [n,2], w [n]) in fp64."""
    left = np.asarray(left, np.float64).reshape(-1, 2)
    q = np.concatenate([left, np.ones((len(left), 1))], axis=1) @ np.asarray(H, np.float64).reshape(3, 3).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[:, :2] / q[:, 2:3], q[:, 2]


def transfer_errors(H, left, right):
    """(forward transfer error in px [n], w [n]) in fp64."""
    proj, w = transfer(H, left)
    with np.errstate(invalid="ignore"):
        return np.sqrt(((proj - np.asarray(right, np.float64).reshape(-1, 2)) ** 2).sum(axis=1)), w


def inlier_mask(H, left, right, threshold_px):
    err, w = transfer_errors(H, left, right)
    with np.errstate(invalid="ignore"):
        return (w > 0) & (err * err <= float(threshold_px) ** 2)


def border_points(H, left, right, threshold_px, margin=5e-3):
    """Number of correspondences whose fp64 transfer error lies within `margin` px of the threshold, or whose |w| <= 1e-6 (a float
    decision may differ there)."""
    err, w = transfer_errors(H, left, right)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero((np.abs(err - threshold_px) <= margin) | (np.abs(w) <= 1e-6)))


def scene_arrays(scene, seed, extra=7):
    """A scene of make_homography_scene as the C ABI takes a pair: (pts_left, pts_right, query_idx, train_idx).  The key points of
    each image are the scene's points in a shuffled order, with `extra` unmatched key points mixed in, so that
    pts_left[query_idx[i]] == scene["left"][i] and pts_right[train_idx[i]] == scene["right"][i] only through the index arrays."""
    rng = np.random.default_rng([int(seed), 77])
    out = []
    for side in ("left", "right"):
        pts = scene[side]
        n = len(pts)
        slot = rng.permutation(n + extra)[:n]                 # where correspondence i sits in the image's key point list
        img = rng.uniform(0, 700, (n + extra, 2)).astype(np.float32)
        img[slot] = pts
        out += [img, slot.astype(np.int32)]
    return out[0], out[2], out[1], out[3]


def homography_ransac(left, right, n_hyp=2000, threshold_px=10.0, seed=0, p=0):
    """The whole contract for one pair of aligned correspondences: dict(status, best_hypothesis, n_inliers, n_matches, H, inlier,
    hyp (the list of hypotheses()), hyp_count)."""
    left = np.asarray(left, np.float64).reshape(-1, 2)
    right = np.asarray(right, np.float64).reshape(-1, 2)
    n = len(left)
    out = dict(status=1, best_hypothesis=-1, n_inliers=0, n_matches=n, H=np.eye(3), inlier=np.zeros(n, bool), hyp=[],
               hyp_count=np.full(n_hyp, -1, np.int64))
    if n < 4:
        return out
    hyp = hypotheses(left, right, n_hyp, seed, p)
    counts = np.array([-1 if H is None else int(inlier_mask(H, left, right, threshold_px).sum()) for _, H, _ in hyp], np.int64)
    out.update(hyp=hyp, hyp_count=counts)
    if counts.max() < 0:
        out["status"] = 2
        return out
    best = int(np.argmax(counts))                           # the first maximum: ties go to the lowest h
    mask = inlier_mask(hyp[best][1], left, right, threshold_px)
    out.update(status=0, best_hypothesis=best, n_inliers=int(mask.sum()), H=hyp[best][1], inlier=mask)
    return out
