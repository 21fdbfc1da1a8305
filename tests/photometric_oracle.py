"""numpy restatement of the photometric consistency stage (include/fsmi.h, fsmi_photo_consistency).

``oracle32``: every value np.float32 and every operation one numpy ufunc call, so each is rounded once,
in the header's order.  ``oracle64``: the same formulas with the image arithmetic in np.float64.  The
geometry (``xr = (float)u - d``, the classes, ``x0``, ``t``, ``yr``, ``y0``, ``ty``) is fp32 in both: it is
part of the definition of which pixel is which, and ``t`` and ``ty`` are exact differences.  The
algorithm is not the kernel's: whole-array gathers and nine shifted views instead of tiles and LDS.

The 3x3 windows need all nine neighbours SAMPLED, and column 0 never is (``0 - d < 0`` for every valid
``d``): SSIM is defined on columns 2 .. W-2 and rows 1 .. H-2 only, so a 3x3 map has no SSIM pixel at all
and every width below 5 likewise.

DSSIM_O32_O64_MAX is max |oracle32 - oracle64| of the dssim map over every fuzz input of the GPU tests
(``GPU_CASES``), measured on the CPU (tests/test_photometric_host.py re-measures it and fails if it is
exceeded); DSSIM_TOL = 4 x that is what a device may differ from oracle64 by: its correctly rounded
division and numpy's can differ in the last bit through the two quotients.  (On MI355X they do not: the
device's dssim map is oracle32's bit for bit, and tests/test_gpu_photometric.py asserts that as well.)
"""
import numpy as np

F = np.float32
C1, C2 = F(6.5025), F(58.5225)
NFIXED = 8
N_SCORED, N_SSIM, N_INVALID, N_OUT_OF_VIEW, L1_MEAN, L1_RMS, DSSIM_MEAN, PHOTOMETRIC = range(8)

# (B,H,W) of the GPU tests; every case runs with C in (1, 3) and both formats
GPU_SHAPES = ((1, 3, 3), (2, 5, 7), (1, 9, 17), (2, 33, 65), (1, 70, 131))
FORMATS = ("f32", "u8")
SEEDS = {(1, 3, 3): 1, (2, 5, 7): 1, (1, 9, 17): 0, (2, 33, 65): 0, (1, 70, 131): 0}
GPU_CASES = tuple((s, C, fmt) for s in GPU_SHAPES for C in (1, 3) for fmt in FORMATS)

DSSIM_O32_O64_MAX = 1.27e-7          # measured 1.2639e-07: (2,33,65), C = 1, uint8, no mask
DSSIM_TOL = 4 * DSSIM_O32_O64_MAX


def planar(img, T):
    """fp32 (B,C,H,W) or uint8 (B,H,W,C) -> (B,C,H,W) of dtype T."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        img = np.moveaxis(img, 3, 1)
    return np.ascontiguousarray(img).astype(T)


def _oracle(T, disp, left, right, mask=None, row_offsets=(), alpha=0.85):
    d = np.ascontiguousarray(disp, dtype=F)
    B, H, W = d.shape
    L, R = planar(left, T), planar(right, T)
    C = L.shape[1]
    assert C in (1, 3) and L.shape == R.shape == (B, C, H, W)
    bi = np.arange(B)[:, None, None]
    vi = np.broadcast_to(np.arange(H)[None, :, None], (B, H, W))
    with np.errstate(all="ignore"):
        u = np.arange(W, dtype=F)[None, None, :]
        invalid = ~(np.isfinite(d) & (d > 0))
        xr = u - d
        assert xr.dtype == F
        oov = ~invalid & (xr < 0)
        sampled = ~invalid & ~oov
        scored = sampled if mask is None else sampled & (np.asarray(mask).reshape(B, H, W) != 0)
        xs = np.where(sampled, xr, F(0))
        x0f = np.floor(xs)
        x0 = x0f.astype(np.int64)
        assert x0.min() >= 0 and x0.max() <= W - 1                      # the header's claim: no clamp needed
        t = (xs - x0f).astype(T)
        x1 = np.minimum(x0 + 1, W - 1)

        def h(y):
            """(B,C,H,W): every channel's row tap at rows y (B,H,W)."""
            out = []
            for c in range(C):
                a, b = R[:, c][bi, y, x0], R[:, c][bi, y, x1]
                out.append(np.where(t == 0, a, a + t * (b - a)))
            return np.stack(out, axis=1)

        def l1_of(w):
            e = np.abs(L[:, 0] - w[:, 0])
            if C == 3:
                e = ((e + np.abs(L[:, 1] - w[:, 1])) + np.abs(L[:, 2] - w[:, 2])) / T(3)
            return e

        w = h(vi)
        assert w.dtype == T
        warped = np.where(sampled[:, None], w, T(0))
        e0 = l1_of(w)
        l1 = np.where(scored, e0, T(np.inf))

        rows = []
        for dy in row_offsets:
            yr = vi.astype(F) + F(dy)
            inr = (yr >= 0) & (yr <= F(H - 1))
            ys = np.where(inr, yr, F(0))
            y0f = np.floor(ys)
            y0 = y0f.astype(np.int64)
            ty = (ys - y0f).astype(T)
            y1 = np.minimum(y0 + 1, H - 1)
            h0 = h(y0)
            wr = np.where((ty == 0)[:, None], h0, h0 + ty[:, None] * (h(y1) - h0))
            er = l1_of(wr)
            sel = scored & inr
            rows.append((sel, er))

        dssim = np.full((B, H, W), np.inf, T)
        has = np.zeros((B, H, W), bool)
        if H >= 3 and W >= 3:
            taps = [(a, q) for a in range(3) for q in range(3)]
            all_s = np.ones((B, H - 2, W - 2), bool)
            for a, q in taps:
                all_s &= sampled[:, a:H - 2 + a, q:W - 2 + q]
            has[:, 1:H - 1, 1:W - 1] = scored[:, 1:H - 1, 1:W - 1] & all_s
            ds = None
            for c in range(C):
                xk = [L[:, c, a:H - 2 + a, q:W - 2 + q] for a, q in taps]
                yk = [warped[:, c, a:H - 2 + a, q:W - 2 + q] for a, q in taps]
                sx, sy = xk[0], yk[0]
                for k in range(1, 9):
                    sx, sy = sx + xk[k], sy + yk[k]
                mx, my = sx / T(9), sy / T(9)
                vx = vy = cxy = None
                for k in range(9):
                    ex, ey = xk[k] - mx, yk[k] - my
                    pxx, pyy, pxy = ex * ex, ey * ey, ex * ey
                    vx = pxx if k == 0 else vx + pxx
                    vy = pyy if k == 0 else vy + pyy
                    cxy = pxy if k == 0 else cxy + pxy
                vx, vy, cxy = vx / T(9), vy / T(9), cxy / T(9)
                num = ((T(2) * mx) * my + T(C1)) * (T(2) * cxy + T(C2))
                den = ((mx * mx + my * my) + T(C1)) * ((vx + vy) + T(C2))
                dc = (T(1) - num / den) * T(0.5)
                dc = np.where(dc >= 0, dc, T(0))
                dc = np.where(dc > 1, T(1), dc)
                assert dc.dtype == T
                ds = dc if c == 0 else ds + dc
            if C == 3:
                ds = ds / T(3)
            dssim[:, 1:H - 1, 1:W - 1] = ds
            dssim = np.where(has, dssim, T(np.inf))

    Rn = len(row_offsets)
    sums = np.zeros((B, NFIXED + 2 * Rn), np.float64)
    table = np.zeros_like(sums)
    a64 = float(alpha)
    for b in range(B):
        lv, sv = l1[b][scored[b]].astype(np.float64), has[b]
        s = sums[b]
        s[0], s[1], s[2], s[3] = scored[b].sum(), sv.sum(), invalid[b].sum(), oov[b].sum()
        s[4], s[5] = lv.sum(), (lv * lv).sum()
        s[6], s[7] = dssim[b][sv].astype(np.float64).sum(), l1[b][sv].astype(np.float64).sum()
        for r, (sel, er) in enumerate(rows):
            s[NFIXED + 2 * r], s[NFIXED + 2 * r + 1] = sel[b].sum(), er[b][sel[b]].astype(np.float64).sum()
        o = table[b]
        o[:4] = s[:4]
        if s[0] > 0:
            o[4], o[5] = s[4] / s[0], np.sqrt(s[5] / s[0])
        if s[1] > 0:
            o[6], o[7] = s[6] / s[1], (a64 * s[6] + ((1.0 - a64) * s[7]) / 255.0) / s[1]
        for r in range(Rn):
            n = s[NFIXED + 2 * r]
            o[NFIXED + 2 * r] = n
            o[NFIXED + 2 * r + 1] = s[NFIXED + 2 * r + 1] / n if n > 0 else 0.0
    return {"table": table, "sums": sums, "warped": warped, "l1": l1, "dssim": dssim, "invalid": invalid,
            "out_of_view": oov, "sampled": sampled, "scored": scored, "has_ssim": has}


def oracle32(disp, left, right, mask=None, row_offsets=(), alpha=0.85):
    """dict: table, sums (B, 8 + 2R) float64; warped (B,C,H,W), l1, dssim (B,H,W) float32; and the boolean
    maps invalid, out_of_view, sampled, scored, has_ssim."""
    return _oracle(np.float32, disp, left, right, mask, row_offsets, alpha)


def oracle64(disp, left, right, mask=None, row_offsets=(), alpha=0.85):
    """The same with the image arithmetic in float64 (the maps are float64)."""
    return _oracle(np.float64, disp, left, right, mask, row_offsets, alpha)


def _texture(rng, B, C, H, W, shift):
    v, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64) + shift, indexing="ij")
    out = np.empty((B, C, H, W), np.float64)
    for b in range(B):
        for c in range(C):
            out[b, c] = (128 + 50 * np.sin(0.37 * x + 0.11 * v + c + 0.5 * b) + 40 * np.cos(0.23 * v - 0.05 * x + 2 * c)
                         + rng.normal(0, 12, (H, W)))
    return np.clip(out, 0, 255)


def fuzz(shape, seed, C, fmt):
    """(disp (B,H,W) float32, left, right, mask (B,H,W) uint8) of the GPU tests.  Images: a smooth texture
    plus noise, the right one two columns further along it; ``fmt`` "f32" gives float32 (B,C,H,W) with
    non-integer grey levels, "u8" uint8 (B,H,W,C).  Disparities per pixel, column u >= 1: 6 % one of
    {NaN, +inf, 0, -1.5} (INVALID), 3 % the float after u and 3 % u + 0.5 .. u + 3 (OUT OF VIEW), the rest
    SAMPLED: 35 % an integer in [1, u] (t == 0), 10 % u itself (xr == 0), 55 % any float in (0, u).  Column 0
    cannot be sampled: 70 % positive (OUT OF VIEW), 30 % INVALID.  The mask drops 10 % of the pixels."""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    u = np.broadcast_to(np.arange(W, dtype=F)[None, None, :], shape)
    kind = rng.uniform(0, 1, shape)
    sub = rng.uniform(0, 1, shape)
    integer = np.floor(1 + rng.uniform(0, 1, shape) * np.maximum(u, 1)).clip(1, np.maximum(u, 1)).astype(F)
    frac = (rng.uniform(0.02, 0.98, shape) * u).astype(F)
    d = np.where(sub < 0.35, integer, np.where(sub < 0.45, u, frac)).astype(F)
    d = np.where(kind < 0.12, np.where(kind < 0.09, np.nextafter(u, F(np.inf)), u + rng.uniform(0.5, 3, shape).astype(F)), d)
    bad = rng.choice(np.array([np.nan, np.inf, 0.0, -1.5], F), shape)
    d = np.where(kind < 0.06, bad, d).astype(F)
    col0 = np.where(rng.uniform(0, 1, shape) < 0.7, rng.uniform(0.25, 3, shape).astype(F), bad)
    d = np.where(u == 0, col0, d).astype(F)
    mask = (rng.uniform(0, 1, shape) >= 0.1).astype(np.uint8)
    left, right = _texture(rng, B, C, H, W, 0.0), _texture(rng, B, C, H, W, 2.0)
    if fmt == "u8":
        left, right = (np.ascontiguousarray(np.moveaxis(np.rint(a), 1, 3)).astype(np.uint8) for a in (left, right))
    else:
        left, right = left.astype(F), right.astype(F)
    return d, left, right, mask


def gpu_fuzz(shape, C, fmt):
    """The fuzz input of one GPU case."""
    return fuzz(shape, SEEDS[tuple(shape)], C, fmt)


def shift_scene(H, W, d, dy, C=3):
    """(disp (1,H,W), left, right) uint8 (1,H,W,C): right = left moved by the integers ``d`` columns to the
    left and ``dy`` rows down, so that left[v][u] == right[v + dy][u - d]; the rest of right is 0."""
    rng = np.random.default_rng(11)
    left = rng.integers(1, 256, (1, H, W, C)).astype(np.uint8)
    right = np.zeros_like(left)
    v0, v1 = max(0, -dy), min(H, H - dy)                 # left rows whose right row exists
    right[:, v0 + dy:v1 + dy, :W - d] = left[:, v0:v1, d:]
    return np.full((1, H, W), d, F), left, right
