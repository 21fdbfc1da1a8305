"""numpy restatement of the sequence metrics (include/fsmi.h, "scoring a sequence of disparity maps"),
the reference the GPU tests compare against.  Everything per pixel is np.float32 in the header's order
of operations (numpy rounds every fp32 operation, so nothing is contracted); sums, means, rates and the
loss are float64."""
import numpy as np

NACC, MAXT, MAX_ROWS = 14, 8, 64
N_VALID, EPE, RMSE, SMOOTH_L1, D1_ALL, N_NONFINITE, BAD0 = range(7)
COUNTS = [0, 4, 5] + list(range(6, 14))          # columns of ``sums`` that are exact counts
RATES = [4] + list(range(6, 14))                 # columns of ``table`` that are count / n_valid
f32 = np.float32


def default_valid(gt):
    with np.errstate(invalid="ignore"):
        return (gt > 0) & (gt < np.inf)


def taps(n_in, n_out):
    """F.interpolate(align_corners=False)'s taps along one axis: (i0, i1, l0, l1), fp32 weights"""
    s = f32(n_in) / f32(n_out)
    dst = np.arange(n_out, dtype=f32)
    src = s * (dst + f32(0.5)) - f32(0.5)
    src = np.where(src < 0, f32(0), src).astype(f32)
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def upsample(p, H, W):
    """(..., h, w) float32 -> (..., H, W) float32:
    l0y * (l0x * p00 + l1x * p01) + l1y * (l0x * p10 + l1x * p11), every operation rounded to fp32"""
    p = np.asarray(p, f32)
    y0, y1, ly0, ly1 = taps(p.shape[-2], H)
    x0, x1, lx0, lx1 = taps(p.shape[-1], W)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        top = lx0 * p[..., y0[:, None], x0[None, :]] + lx1 * p[..., y0[:, None], x1[None, :]]
        bot = lx0 * p[..., y1[:, None], x0[None, :]] + lx1 * p[..., y1[:, None], x1[None, :]]
        out = ly0 * top + ly1 * bot
    assert out.dtype == f32
    return out


# fp32 roundings that separate two evaluations of the same four-tap sample (tests/test_seq_host.py derives it)
RESIZE_ROUNDINGS = 12


def resize_gap_bound(max_tap):
    """The largest difference between ``upsample`` and any other fp32 evaluation order of the same taps"""
    return RESIZE_ROUNDINGS * 2.0 ** -24 * float(max_tap)


def row_values(p, H, W, mul=1.0, max_disp=np.inf):
    """Steps 1-3: the row on the ground truth's grid, times its factor, clamped (a NaN stays NaN;
    max_disp = +inf: no clamp at either end)."""
    p = np.asarray(p, f32)
    v = p if p.shape[-2:] == (H, W) else upsample(p, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (v * f32(mul)).astype(f32)
        if max_disp < np.inf:
            v = np.where(v < 0, f32(0), v)
            v = np.where(v > f32(max_disp), f32(max_disp), v).astype(f32)
    return v


def smooth_l1(e, beta):
    beta = f32(beta)
    if beta == 0:
        return e
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(e < beta, (f32(0.5) * (e * e)) / beta, e - f32(0.5) * beta).astype(f32)


def pair_row_sums(v, gt, valid, thresholds, beta):
    """One pair, one row: values on the grid (H,W) -> sums (14) float64"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(v - gt).astype(f32)
        ev, sv = e[valid], smooth_l1(e, beta)[valid]
        ed = ev.astype(np.float64)
        s = np.zeros(NACC, np.float64)
        s[0] = ev.size
        s[1] = ed.sum()
        s[2] = (ed * ed).sum()
        s[3] = sv.astype(np.float64).sum()
        s[4] = np.count_nonzero((ev > f32(3.0)) & (ev > f32(0.05) * np.abs(gt[valid])))
        s[5] = np.count_nonzero(~np.isfinite(ev))
        for k, t in enumerate(thresholds):
            s[BAD0 + k] = np.count_nonzero(ev > f32(t))
    return s


def table_row(s):
    t = np.zeros(NACC, np.float64)
    n = s[0]
    t[0], t[5] = n, s[5]
    if n > 0:
        with np.errstate(invalid="ignore"):
            t[1], t[2], t[3], t[4] = s[1] / n, np.sqrt(s[2] / n), s[3] / n, s[4] / n
            t[6:] = s[6:] / n
    return t


def _per_row(v, R, default):
    if v is None:
        return [default] * R
    if np.isscalar(v):
        return [v] * R
    assert len(v) == R
    return list(v)


def seq_metrics(preds, gt, mask=None, thresholds=(1.0, 3.0, 5.0), max_disparity=np.inf, beta=1.0, weights=None,
                smooth_rows=(), muls=None):
    """preds: R arrays (B,h_r,w_r); gt (B,H,W) -> table (B,R,14), sums (B,R,14), loss (B), float64"""
    gt = np.asarray(gt, f32)
    B, H, W = gt.shape
    R = len(preds)
    maxd, w, mul = _per_row(max_disparity, R, np.inf), _per_row(weights, R, 1.0), _per_row(muls, R, 1.0)
    valid = default_valid(gt) if mask is None else np.asarray(mask).astype(bool)
    sums = np.zeros((B, R, NACC), np.float64)
    for r in range(R):
        v = row_values(preds[r], H, W, mul[r], maxd[r])
        for b in range(B):
            sums[b, r] = pair_row_sums(v[b], gt[b], valid[b], thresholds, beta)
    table = np.stack([[table_row(sums[b, r]) for r in range(R)] for b in range(B)])
    loss = np.zeros(B, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for r in range(R):                               # in row order, two roundings per row
                loss[b] = loss[b] + np.float64(w[r]) * table[b, r, SMOOTH_L1 if r in smooth_rows else EPE]
    return table, sums, loss


def sequence_weights(K, gamma, with_init=True):
    """foundation_stereo_loss's weights: 1 for the initial row, gamma^(K-k) for iteration k = 1..K"""
    return ([1.0] if with_init else []) + [gamma ** (K - (k + 1)) for k in range(K)]


def reference_dict(table_rows, weights):
    """foundation_stereo_loss's (loss, misc) from the table rows (1 + K, 14) of ONE pair, row 0 the
    initial disparity, scored with the thresholds (1, 3, ...).  The reference's quirks: d1_error is the
    rate above 3 px and d3_error the rate above 1 px; the *_iterative figures are weighted SUMS."""
    t = np.asarray(table_rows, np.float64)
    w = np.asarray(weights[1:], np.float64)
    it = t[1:]
    misc = {"epe_initial": t[0, EPE], "d1_error_initial": t[0, BAD0 + 1], "d3_error_initial": t[0, BAD0],
            "epe_iterative": (w * it[:, EPE]).sum(), "d1_error_iterative": (w * it[:, BAD0 + 1]).sum(),
            "d3_error_iterative": (w * it[:, BAD0]).sum(), "loss_initial": t[0, SMOOTH_L1],
            "loss_iterative": (w * it[:, EPE]).sum()}
    misc = {k: float(v) for k, v in misc.items()}
    return misc["loss_initial"] + misc["loss_iterative"], misc


GOLDEN_PARAMS = [(0.9, 192.0), (0.8, 48.0)]                  # (gamma, max_disparity)
GOLDEN_K = 5
GOLDEN_INIT_SMALL = (10, 16)
GOLDEN_TAG = "seq_small_"


def golden_case():
    """The inputs of tests/golden/seq_small.npz, which stores only what the reference returned for them
    (tools/make_goldens.py seq): 3 pairs of 37 x 61 with a tenth of the ground truth zero and pair 1's mask
    empty; K = 5 predictions = ground truth + noise that shrinks with k, a few values above 192 and a few
    below 0 in each; one initial disparity at 10 x 16 (a non-integer ratio, taps clamped at every border)
    and one at full size.  Regenerated from the package's hash PRNG, so the file stays a few KB."""
    from foundationstereo_amd import synth
    shape = (3, 37, 61)

    def u(tag, shp=shape):
        return synth.uniform(synth.name_seed(GOLDEN_TAG + tag), shp).astype(np.float64)

    def n(tag, shp=shape):
        return synth.normal(synth.name_seed(GOLDEN_TAG + tag), shp).astype(np.float64)

    gt = (1.0 + u("gt") * 59.0).astype(f32)                  # 1 .. 60 px: some above max_disparity 48
    gt[u("holes") < 0.1] = 0
    mask = gt > 0
    mask[1] = False
    preds = []
    for k in range(GOLDEN_K):
        p = gt + n(f"noise{k}") * (4.0 * 0.55 ** k) * np.where(u(f"wide{k}") < 0.15, 3.0, 1.0)
        sel = u(f"out{k}")
        p = np.where(sel < 0.004, 200.0 + 50.0 * sel, p)      # above max_disparity 192
        p = np.where(sel > 0.996, -3.0 * sel, p)              # below 0
        preds.append(p.astype(f32))
    init_small = (5.0 + u("init_small", (3,) + GOLDEN_INIT_SMALL) * 45.0).astype(f32)
    init_full = (gt + n("init_full") * 5.0).astype(f32)
    return {"gt": gt, "mask": mask, "preds": preds, "init_small": init_small, "init_full": init_full}


def checksums(case):
    return [float(case["gt"].astype(np.float64).sum()), float(case["mask"].sum()),
            float(sum(p.astype(np.float64).sum() for p in case["preds"])),
            float(case["init_small"].astype(np.float64).sum()), float(case["init_full"].astype(np.float64).sum())]


def load_golden(path):
    """seq_small.npz merged with its regenerated inputs, the inputs held to the file's checksums"""
    g = np.load(path)
    out = {k: g[k] for k in g.files}
    case = golden_case()
    assert checksums(case) == out["checksums"].tolist(), (checksums(case), out["checksums"])
    out.update(case)
    return out
