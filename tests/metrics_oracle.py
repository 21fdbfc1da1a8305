"""numpy restatement of the disparity metrics (include/fsmi.h, "scoring a disparity map"), the
reference the GPU tests compare against.  The per-pixel error and every comparison are np.float32, as
torch evaluates them on fp32 tensors; sums, means and rates are float64."""
import numpy as np

NACC, MAXT = 17, 8
f32 = np.float32


def decode(u8, scale=1000.0):
    """depth_uint8_decoding (Utils.py:137-140) rounded to float32: (...,3) uint8 -> (...) float32"""
    u = u8.astype(np.float64)
    return ((u[..., 0] * 255 * 255 + u[..., 1] * 255 + u[..., 2]) / scale).astype(f32)


def default_valid(gt):
    with np.errstate(invalid="ignore"):
        return (gt > 0) & (gt < np.inf)


def pair_sums(pred, gt, mask=None, thresholds=(1.0, 3.0, 5.0)):
    """One pair (H,W) -> (sums (17) float64, error (H,W) float32, valid (H,W) bool)"""
    pred, gt = np.asarray(pred, f32), np.asarray(gt, f32)
    valid = default_valid(gt) if mask is None else np.asarray(mask).astype(bool)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(pred - gt).astype(f32)
        ev = e[valid]
        ed = ev.astype(np.float64)
        s = np.zeros(NACC, np.float64)
        s[0] = ev.size
        s[1] = ed.sum()
        s[2] = (ed * ed).sum()
        s[3] = np.count_nonzero((ev > f32(3.0)) & (ev > f32(0.05) * np.abs(gt[valid])))
        s[4] = np.count_nonzero(~np.isfinite(ev))
        x = pred.astype(np.float64).ravel()
        d = x - x[0]
        s[5] = d.sum()
        s[6] = (d * d).sum()
        s[7] = np.nan if np.isnan(x).any() else x.min()
        s[8] = np.nan if np.isnan(x).any() else x.max()
        for k, t in enumerate(thresholds):
            s[9 + k] = np.count_nonzero(ev > f32(t))
    return s, np.where(valid, e, f32(np.inf)).astype(f32), valid


def table_row(s, pred00, P):
    """The metrics of one pair from its sums, its first prediction and its pixel count"""
    t = np.zeros(NACC, np.float64)
    n = s[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        t[0], t[4] = n, s[4]
        if n > 0:
            t[1], t[2], t[3] = s[1] / n, np.sqrt(s[2] / n), s[3] / n
            t[9:] = s[9:] / n
        t[5] = np.float64(pred00) + s[5] / P
        dev2 = s[6] - s[5] * s[5] / P
        t[6] = np.sqrt((0.0 if dev2 < 0 else dev2) / np.float64(P - 1))     # NaN stays NaN; P = 1 is 0 / 0
        t[7], t[8] = s[7], s[8]
    return t


def metrics(pred, gt, mask=None, thresholds=(1.0, 3.0, 5.0)):
    """(B,H,W) -> table (B,17), sums (B,17), error (B,H,W) float32.  ``sums`` also carries what the
    tests' bounds need: see ``abs_dev``."""
    B = pred.shape[0]
    out = [pair_sums(pred[b], gt[b], None if mask is None else mask[b], thresholds) for b in range(B)]
    sums = np.stack([o[0] for o in out])
    P = pred[0].size
    table = np.stack([table_row(sums[b], pred[b].ravel()[0], P) for b in range(B)])
    return table, sums, np.stack([o[1] for o in out])


def abs_dev(pred):
    """sum |x - x0| of one pair in float64: the scale of pred_mean's summation-error bound"""
    x = np.asarray(pred, f32).astype(np.float64).ravel()
    return np.abs(x - x[0]).sum()


def reference_dict(table_rows, thresholds):
    """compute_stereo_metrics's dict from table rows: the mean over pairs (train/utils.py:120)"""
    row = np.asarray(table_rows, np.float64).reshape(-1, NACC).mean(axis=0)
    out = {"epe": row[1], "rmse": row[2], "mae": row[1]}
    for k, t in enumerate(thresholds):
        out[f"d{int(t)}_error"] = row[9 + k]
    return out


GOLDEN_THRESHOLDS = [0.5, 1.0, 3.0, 5.0]


def golden_case():
    """The inputs of tests/golden/metrics_small.npz, which stores only what the reference returned for
    them (tools/make_goldens.py metrics, which also holds ``decode`` below to the reference's decode on
    every pixel): uint8 ground truth (3,37,61,3) with a tenth of the pixels zero, its decode, a prediction
    = ground truth + noise (a fifth of it 6 px wide), and gt > 0 as the mask with pair 1's emptied.
    Regenerated from the package's hash PRNG, so the file stays a few KB."""
    from foundationstereo_amd import synth
    shape = (3, 37, 61)

    def u(tag):
        return synth.uniform(synth.name_seed("metrics_small_" + tag), shape).astype(np.float64)

    gt_u8 = np.zeros(shape + (3,), np.uint8)                 # r = 0: below 65.025 px at scale 1000
    gt_u8[..., 1] = np.minimum(u("g") * 200, 199).astype(np.uint8)
    gt_u8[..., 2] = np.minimum(u("b") * 256, 255).astype(np.uint8)
    gt_u8[u("holes") < 0.1] = 0
    gt = decode(gt_u8, 1000.0)
    noise = synth.normal(synth.name_seed("metrics_small_noise"), shape).astype(np.float64)
    pred = (gt + noise * np.where(u("wide") < 0.2, 6.0, 0.7)).astype(f32)
    mask = gt > 0
    mask[1] = False
    return {"gt_u8": gt_u8, "gt": gt, "pred": pred, "mask": mask, "thresholds": list(GOLDEN_THRESHOLDS)}


def load_golden(path):
    """metrics_small.npz merged with its regenerated inputs, the inputs held to the file's checksums"""
    g = np.load(path)
    out = {k: g[k] for k in g.files}
    case = golden_case()
    sums = [float(case["gt_u8"].sum()), float(case["pred"].astype(np.float64).sum()), float(case["mask"].sum())]
    assert sums == out["checksums"].tolist(), (sums, out["checksums"])
    assert case["thresholds"] == out["thresholds"].tolist()
    out.update({k: case[k] for k in ("gt_u8", "gt", "pred", "mask")})
    return out
