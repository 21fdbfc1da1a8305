"""numpy restatement of the visibility classes (include/fsmi.h, fsmi_disp_visibility).

Every value is np.float32 and every operation one numpy ufunc call, so each is rounded once, in the
header's order: the classes, counts and error map are the kernel's bit for bit and the tests need no
tolerance.  The algorithm is not the kernel's: whole-array masks, and the z-buffer as one
``np.maximum.at`` scatter over (row, rounded column) pairs instead of a per-row LDS atomic.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

VISIBLE, INVALID, OUT_OF_VIEW, OCCLUDED, MISMATCH = range(5)
F = np.float32


def _rows(d, dr, occlusion, occlusion_tol, lr_thresh):
    """d, dr: (R,W) float32 rows (dr may be None) -> classes (R,W) uint8, err (R,W) float32 or None."""
    R, W = d.shape
    u = np.arange(W, dtype=F)[None, :]
    row = np.broadcast_to(np.arange(R)[:, None], (R, W))
    with np.errstate(all="ignore"):
        invalid = ~(np.isfinite(d) & (d > 0))
        xr = u - d                                              # float32 - float32
        assert xr.dtype == F
        out = ~invalid & (xr < 0)
        inview = ~invalid & ~out
        cls = np.zeros((R, W), np.uint8)
        cls[invalid] = INVALID
        cls[out] = OUT_OF_VIEW
        occluded = np.zeros((R, W), bool)
        if occlusion:
            c = np.where(inview, np.floor(xr + F(0.5)), F(0)).astype(np.int64)
            assert c.min() >= 0 and c.max() <= W - 1            # the header's claim: no clamp needed
            z = np.zeros((R, W), F)
            np.maximum.at(z, (row[inview], c[inview]), d[inview])
            occluded = inview & (z[row, c] - d > F(occlusion_tol))
        mismatch = np.zeros((R, W), bool)
        err = None
        if dr is not None:
            x0 = np.where(inview, np.floor(xr), F(0)).astype(np.int64)
            assert x0.min() >= 0 and x0.max() <= W - 1
            t = xr - x0.astype(F)
            x1 = np.minimum(x0 + 1, W - 1)
            a, b = dr[row, x0], dr[row, x1]
            r = np.where(t == 0, a, a + t * (b - a))
            e = np.abs(d - r)
            assert r.dtype == F and e.dtype == F
            mismatch = inview & ~(e <= F(lr_thresh))
            err = np.where(inview, e, F(np.nan)).astype(F)
        cls[occluded] = OCCLUDED
        cls[mismatch & ~occluded] = MISMATCH
    return cls, err


def classify_oracle(disp, disp_right=None, occlusion=True, occlusion_tol=1.0, lr_thresh=1.0, workers=1):
    """disp, disp_right: (B,H,W) -> (classes (B,H,W) uint8, counts (B,5) int64, err (B,H,W) float32 or
    None without disp_right).  ``workers`` > 1 splits the rows over that many threads (rows are
    independent); the result does not depend on it."""
    d = np.ascontiguousarray(disp, dtype=F)
    B, H, W = d.shape
    d2 = d.reshape(B * H, W)
    r2 = None if disp_right is None else np.ascontiguousarray(disp_right, dtype=F).reshape(B * H, W)
    bounds = np.linspace(0, B * H, min(max(int(workers), 1), B * H) + 1).astype(int)
    parts = [(lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]

    def run(part):
        lo, hi = part
        return _rows(d2[lo:hi], None if r2 is None else r2[lo:hi], occlusion, occlusion_tol, lr_thresh)

    if len(parts) == 1:
        done = [run(parts[0])]
    else:
        with ThreadPoolExecutor(max_workers=len(parts)) as ex:
            done = list(ex.map(run, parts))
    cls = np.concatenate([c for c, _ in done]).reshape(B, H, W)
    err = None if r2 is None else np.concatenate([e for _, e in done]).reshape(B, H, W)
    counts = np.stack([np.bincount(cls[b].reshape(-1), minlength=5) for b in range(B)]).astype(np.int64)
    return cls, counts, err


def analytic_scene(H=2):
    """A fronto-parallel foreground (d = 20 on columns [30,50)) before a background (d = 4), W = 64:
    (left disparity (1,H,W), the matching right-view disparity, the closed-form classes of the
    occlusion test alone, the closed-form classes of the left-right test alone)."""
    W = 64
    left = np.full((1, H, W), 4.0, F)
    left[..., 30:50] = 20.0
    right = np.full((1, H, W), 4.0, F)
    right[..., 10:30] = 20.0                 # the foreground, 20 columns to the left
    occ = np.zeros((1, H, W), np.uint8)
    occ[..., 0:4] = OUT_OF_VIEW              # u - 4 < 0
    occ[..., 14:30] = OCCLUDED               # background that lands on columns [10,26), under the foreground
    lr = occ.copy()
    lr[..., 14:30] = MISMATCH
    return left, right, occ, lr


def fuzz_maps(shape, seed, with_right):
    """The fuzz inputs of the GPU test: disparities uniform in [0.25, W/2] in steps of 1/4 (ties on a
    z-buffer column and t == 0 both occur), 5 % of the entries drawn from {0, -1, NaN, +inf}."""
    B, H, W = shape
    rng = np.random.default_rng(seed)

    def one():
        steps = max(int(W / 2 * 4), 1)
        d = (rng.integers(1, steps + 1, shape) * 0.25).astype(F)
        bad = rng.uniform(0, 1, shape) < 0.05
        d[bad] = rng.choice(np.array([0.0, -1.0, np.nan, np.inf], F), int(bad.sum()))
        return d

    left = one()
    return left, (one() if with_right else None)
