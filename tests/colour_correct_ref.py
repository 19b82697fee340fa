"""Restatement of the colour correction in numpy, written from its formula:

    row(p)  = [r r, r g, r b, g g, g b, b b, r, g, b, 1] of the current image's pixel p = (r, g, b)
    mask_c  = unclipped(img[c]) & unclipped(cur[c]) & unclipped(ref[c]),   unclipped(z) = eps <= z <= 1 - eps
    warp_c  = lstsq over the rows of mask_c (masked rows as zero rows, which changes nothing) of ref[c] on row
    cur    <- clip(row . warp, 0, 1),   num_iters times

in the dtype asked for: float64 is the truth both the reference's float32 result and the device's are measured against, float32 is the
formulation's own rounding at a size no fixture records.  Shared by tests/test_colour_correct_cpu.py and tests/test_colour_correct_gpu.py,
which read only tests/golden/colour_correct.npz."""
import os

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
EPS_DEFAULT = 0.5 / 255
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_correct.npz")
SHAPES = ((4, 5), (24, 20), (67, 129))
REGIMES = ("a", "b", "c")
CASES = tuple(f"{r}_{h}x{w}" for r in REGIMES for (h, w) in SHAPES)
MARGIN = 1e-5          # no value of a fixture within this of a threshold, unless it is exactly 0 or 1


def design(cur):
    r, g, b = cur[:, 0:1], cur[:, 1:2], cur[:, 2:3]
    return np.concatenate([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, np.ones_like(r)], axis=1)


def unclipped(z, eps):
    return (z >= eps) & (z <= 1 - eps)


def restate(img, ref, num_iters=5, eps=EPS_DEFAULT, dtype=np.float64):
    """-> dict(out [.., 3], iterates [num_iters + 1, n, 3] (the input first), warps [num_iters, 10, 3], masks [num_iters, n, 3])."""
    shape = np.shape(img)
    img0 = np.asarray(img, dtype=dtype).reshape(-1, 3)
    b = np.asarray(ref, dtype=dtype).reshape(-1, 3)
    eps = dtype(eps)
    mask0, maskb = unclipped(img0, eps), unclipped(b, eps)
    cur, iterates, warps, masks = img0, [img0], [], []
    for _ in range(num_iters):
        a = design(cur)
        mask = mask0 & unclipped(cur, eps) & maskb
        warp = np.stack([np.linalg.lstsq(np.where(mask[:, c:c + 1], a, 0), np.where(mask[:, c], b[:, c], 0), rcond=None)[0]
                         for c in range(3)], axis=-1).astype(dtype)
        cur = np.clip(a @ warp, 0, 1)
        iterates.append(cur)
        warps.append(warp)
        masks.append(mask)
    return dict(out=cur.reshape(shape), iterates=np.stack(iterates), warps=np.stack(warps) if warps else np.zeros((0, 10, 3), dtype),
                masks=np.stack(masks) if masks else np.zeros((0,) + img0.shape, bool))


def threshold_gap(values, eps=EPS_DEFAULT, thresholds=None):
    """The least distance of any value to a mask or clip threshold (eps, 1 - eps, 0, 1), values exactly 0 or 1 set aside."""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[(v != 0.0) & (v != 1.0)]
    if v.size == 0:
        return np.inf
    return float(min(np.abs(v - t).min() for t in (thresholds or (eps, 1 - eps, 0.0, 1.0))))


def condition_gap(regime, img, ref, res, eps=EPS_DEFAULT):
    """The fixtures' condition is condition_gap >= MARGIN: then a float32 rounding cannot flip a mask or a clip between implementations.
    The inputs and every iterate keep their distance from eps, 1 - eps, 0 and 1 -- except regime c's iterates from 0 and 1: a value that
    one estimate clips to 0 or 1 comes back from the next, nearly identical, warp as 0 or 1 give or take 1e-3 .. 1e-12, closer with every
    iteration, so no seed avoids it.  The clip is continuous, so a rounding that flips it moves the value by no more than itself; the
    masks, which are not, are guarded in every regime."""
    iter_thresholds = (eps, 1 - eps) if regime == "c" else None
    return min(threshold_gap(img, eps), threshold_gap(ref, eps), threshold_gap(res["iterates"][1:], eps, iter_thresholds))


def saturating_rows(res, eps=EPS_DEFAULT):
    """The share of rows whose current-estimate mask term is true at iteration 0 and false at iteration 4 in some channel."""
    it = res["iterates"]
    return float((unclipped(it[0], eps) & ~unclipped(it[4], eps)).any(axis=1).mean())


def condition_number(img, ref, res, eps=EPS_DEFAULT):
    """The largest 2-norm condition number of a masked design matrix over iterations and channels."""
    worst = 0.0
    for it, mask in enumerate(res["masks"]):
        a = design(res["iterates"][it])
        for c in range(3):
            s = np.linalg.svd(a[mask[:, c]], compute_uv=False)
            worst = max(worst, float(s[0] / s[-1]))
    return worst


def max_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


def allowed(ref_err, want):
    """The bracket of DESIGN.md 7h: four times the float32 formulation's own error against the float64 restatement, and never below four
    float32 roundings of the largest value."""
    return max(4 * ref_err, 4 * EPS32 * float(np.abs(want).max()))


def fixture():
    return dict(np.load(GOLDEN))


# ---------------------------------------------------------------- inputs (the generator's, and the larger seeded case of the GPU tests)
# mild: a contraction -- every pixel of [0, 1]^3 lands in [0.1, 0.9], so no iterate of regimes a and b comes near a threshold
WARP_MILD = np.array([[0.04, -0.02, 0.01], [0.02, 0.03, -0.01], [-0.01, 0.02, 0.02], [-0.02, 0.04, 0.01], [0.01, -0.02, 0.03],
                      [0.02, 0.01, -0.03], [0.55, 0.03, -0.02], [0.02, 0.52, 0.03], [-0.02, 0.03, 0.56], [0.20, 0.21, 0.19]])
# strong: per channel the bump 0.15 + 3.9 x (1 - x) plus the same small cross terms.  Regime c's img lives in U(0.03, 0.22) and
# U(0.78, 0.97), which land in about [0.25, 0.85], and so do the values pushed to 0 or 1 (0.15); 0.7 % of its values are drawn from
# U(0.42, 0.58), land above 1.09 and saturate in every corrected estimate.  A larger saturated share cannot meet the fixtures' condition:
# a value clipped to 1 comes back from the next, nearly identical, warp within about 0.01 of 1, where 1 - eps lies
WARP_STRONG = np.array([[-3.90, -0.02, 0.01], [0.02, 0.03, -0.01], [-0.01, 0.02, 0.02], [-0.02, -3.90, 0.01], [0.01, -0.02, 0.03],
                        [0.02, 0.01, -3.90], [3.90, 0.03, -0.02], [0.02, 3.90, 0.03], [-0.02, 0.03, 3.90], [0.15, 0.14, 0.16]])


def make_inputs(regime, h, w, seed):
    """float32 (img, ref) of one regime (module docstring of tests/golden/make_colour_correct_golden.py)."""
    rng = np.random.default_rng(seed)
    n = h * w
    img = rng.uniform(0.05, 0.95, size=(n, 3))
    if regime == "c":
        img = rng.uniform(0.03, 0.22, size=(n, 3)) + 0.75 * rng.integers(0, 2, size=(n, 3))
        mid = rng.choice(img.size, size=max(1, round(0.007 * img.size)), replace=False)
        img.reshape(-1)[mid] = rng.uniform(0.42, 0.58, size=mid.size)
    ref = design(img) @ (WARP_STRONG if regime == "c" else WARP_MILD) + rng.normal(0.0, 0.01, size=(n, 3))
    ref = np.clip(ref, 0.0, 1.0)
    if regime != "a":
        for arr in (img, ref):
            hit = rng.uniform(size=arr.shape) < 0.15
            arr[hit] = rng.integers(0, 2, size=arr.shape)[hit].astype(np.float64)
    # a reference value closer than 1e-4 to a threshold goes to the clipped value beside it
    ref[ref < EPS_DEFAULT + 1e-4] = 0.0
    ref[ref > 1 - EPS_DEFAULT - 1e-4] = 1.0
    return img.reshape(h, w, 3).astype(np.float32), ref.reshape(h, w, 3).astype(np.float32)
