"""numpy restatements of the confidence maps and the risk-coverage histogram (include/fsmi.h,
fsmi_disp_confidence and fsmi_risk_coverage), and the tolerances the device is held to.

``confidence_ref`` is the mathematical definition in fp64.  ``confidence_f32`` is the same thing in
float32 in the kernel's operation order (every sum starts at 0 and adds d = 0 .. D-1 in order, mu and
var divide the e-weighted sums by s once, mass divides its sum by s once); it differs from the device
only in expf / logf (numpy's against the device library's), so it shows how much of a tolerance plain
fp32 evaluation uses, on the CPU.  ``risk_oracle`` is exact: integers.

Tolerances, absolute against the fp64 reference, u = 2^-24, D bins:

  peak     (D + 8) u                  1 / s with s = sum of D terms in (0, 1], the largest 1: each addition
                                      rounds by at most u relative to a partial sum <= s, so |ds| / s <= D u;
                                      8 u for expf (a few ulp on the terms) and the division.  peak <= 1, so
                                      the relative bound is the absolute one.
  mass     (2 D + 16) u + 1e-6        a ratio of two such sums, (D + 8) u each; the ramp has slope 1, so the
                                      fp32 rounding of d - q (at most D u for q in [-2, D + 1], whose
                                      magnitudes stay below D + 2 <= 2^k u-steps) carries over one to one
                                      into a weight and, the weights being averaged with sum p = 1, into
                                      the mass: covered by the 1e-6 for D <= 16 and by the second D u above.
  entropy  2 (D + 8) u + 1e-6         Hn / ln D with Hn = ln s - set / s: two terms of the peak's kind, and
                                      the division by ln D >= ln 2 does not enlarge them by more than 1.45;
                                      logf's few ulp on ln s <= ln D scale to u after the division: the 1e-6.
  spread   (D + 12) u ref + softargmin_tol(D)
                                      var + (mu - q)^2 is a sum of non-negative terms, so its relative
                                      error (D + 12) u / 2 .. (D + 12) u survives the square root (halved);
                                      the device forms it as var + (mu - q)^2 with its own fp32 mu, and
                                      |sqrt(a + (x + eps)^2) - sqrt(a + x^2)| <= |eps| with eps the error of
                                      mu, which is soft-argmin's: softargmin_tol(D) of
                                      tests/backbone_reference.py.
  self     mass gains softargmin_tol(D): the query is the device's own mu, and mass moves by at most the
           query's error (slope 1, sum p = 1).

On this CPU, over D in {1, 2, 7, 48, 104, 200, 512}, logits of std 2, std 12 and the +-88 alternation,
radius in {0, 1, 2.5} and q uniform in [-2, D + 1], ``confidence_f32`` stays within half of each
(tests/test_confidence_host.py asserts that).
"""
import numpy as np

from tests.backbone_reference import softargmin_tol

U = 2.0 ** -24
CHANNELS = ("mass", "spread", "peak", "entropy")


def peak_tol(D):
    return (D + 8) * U


def mass_tol(D, self_mode=False):
    return (2 * D + 16) * U + 1e-6 + (softargmin_tol(D) if self_mode else 0.0)


def entropy_tol(D):
    return 2 * (D + 8) * U + 1e-6


def spread_tol(D, ref):
    """Elementwise: ``ref`` is the fp64 reference map (NaN stays NaN)."""
    return (D + 12) * U * np.asarray(ref, dtype=np.float64) + softargmin_tol(D)


def tolerances(D, ref, self_mode=False):
    """channel -> tolerance (a float, or for spread an array of ref's shape)."""
    return {"mass": mass_tol(D, self_mode), "spread": spread_tol(D, ref["spread"]), "peak": peak_tol(D),
            "entropy": entropy_tol(D)}


def make_logits(kind, B, D, h, w, seed=0):
    """The three logit families of the tests: "std2", "std12" (peaked) and "alt88" (+88 on even bins, -88
    on odd ones, sign flipped on every other column: half the bins underflow to probability 0)."""
    rng = np.random.default_rng(seed)
    if kind == "std2":
        return (2.0 * rng.standard_normal((B, D, h, w))).astype(np.float32)
    if kind == "std12":
        return (12.0 * rng.standard_normal((B, D, h, w))).astype(np.float32)
    if kind == "alt88":
        x = np.where(np.arange(D)[None, :, None, None] % 2 == 0, 88.0, -88.0)
        flip = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0, 1.0, -1.0)
        return np.broadcast_to(x * flip[None, None], (B, D, h, w)).astype(np.float32).copy()
    raise ValueError(kind)


def _expand(a, up):
    """(B,h,w) -> (B,h*up,w*up): pixel (y,x) takes column (y // up, x // up)."""
    return np.repeat(np.repeat(a, up, axis=1), up, axis=2)


def _bad_columns(x):
    with np.errstate(invalid="ignore"):
        return np.isnan(x).any(1) | (x == np.inf).any(1) | (x == -np.inf).all(1)


def confidence_ref(logits, disp=None, up=4, disp_scale=None, radius=1.0):
    """fp64.  logits (B,D,h,w), disp None or (B,h*up,w*up) -> {channel: (B,h*up,w*up) float64}."""
    x = np.asarray(logits, dtype=np.float64)
    B, D, h, w = x.shape
    bad = _bad_columns(x)
    x = np.where(bad[:, None], 0.0, x)
    dd = np.arange(D, dtype=np.float64)[None, :, None, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = x - x.max(1, keepdims=True)
        e = np.exp(t)
        s = e.sum(1)
        p = e / s[:, None]
        mu = (p * dd).sum(1)
        var = (p * (dd - mu[:, None]) ** 2).sum(1)
        Hn = np.log(s) - np.where(e != 0, e * np.where(e != 0, t, 0.0), 0.0).sum(1) / s
        entropy = np.ones_like(s) if D == 1 else 1.0 - Hn / np.log(float(D))
        peak = 1.0 / s
        P = np.repeat(np.repeat(p, up, axis=2), up, axis=3)                 # (B,D,H,W)
        mu_p, var_p = _expand(mu, up), _expand(var, up)
        if disp is None:
            q = mu_p
        else:
            scale = np.float32(1.0 / up if disp_scale is None else disp_scale)
            q = (np.asarray(disp, dtype=np.float32) * scale).astype(np.float64)    # the one fp32 multiply
        qf = np.where(np.isfinite(q), q, 0.0)
        wgt = np.clip(radius + 1.0 - np.abs(dd - qf[:, None]), 0.0, 1.0)
        mass = (P * wgt).sum(1)
        spread = np.sqrt((P * (dd - qf[:, None]) ** 2).sum(1))
    nan_col = _expand(bad, up)
    nan_q = nan_col | ~np.isfinite(q)
    out = {"mass": np.where(nan_q, np.nan, mass), "spread": np.where(nan_q, np.nan, spread),
           "peak": np.where(nan_col, np.nan, _expand(peak, up)), "entropy": np.where(nan_col, np.nan, _expand(entropy, up))}
    return out


def confidence_f32(logits, disp=None, up=4, disp_scale=None, radius=1.0):
    """float32, in the kernel's operation order (numpy's exp / log for the device's)."""
    f = np.float32
    x = np.asarray(logits, dtype=f)
    B, D, h, w = x.shape
    bad = _bad_columns(x)
    x = np.where(bad[:, None], f(0), x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(1)
        t = x - m[:, None]
        e = np.exp(t)                                                       # float32 in, float32 out
        s, st, sd = (np.zeros((B, h, w), f) for _ in range(3))
        for d in range(D):
            s = s + e[:, d]
            st = st + np.where(e[:, d] != 0, e[:, d] * np.where(e[:, d] != 0, t[:, d], f(0)), f(0))
            sd = sd + e[:, d] * f(d)
        mu = sd / s
        sv = np.zeros((B, h, w), f)
        for d in range(D):
            dm = f(d) - mu
            sv = sv + e[:, d] * (dm * dm)
        var = sv / s
        peak = f(1) / s
        hn = np.log(s) - st / s
        entropy = np.ones_like(s) if D == 1 else np.minimum(np.maximum(f(1) - hn / np.log(f(D)), f(0)), f(1))
        mu_p, var_p, s_p = _expand(mu, up), _expand(var, up), _expand(s, up)
        if disp is None:
            q = mu_p
        else:
            q = np.asarray(disp, dtype=f) * f(1.0 / up if disp_scale is None else disp_scale)
        qf = np.where(np.isfinite(q), q, f(0))
        r1 = f(radius) + f(1)
        acc = np.zeros_like(qf)
        for d in range(D):                                                  # bins outside the trapezoid add an exact 0
            wd = np.minimum(np.maximum(r1 - np.abs(f(d) - qf), f(0)), f(1))
            acc = acc + _expand(e[:, d], up) * wd
        mass = np.minimum(acc / s_p, f(1))
        dq = mu_p - qf
        spread = np.sqrt(var_p + dq * dq)
    assert all(a.dtype == f for a in (mass, spread, peak, entropy))
    nan_col = _expand(bad, up)
    nan_q = nan_col | ~np.isfinite(q)
    return {"mass": np.where(nan_q, f(np.nan), mass), "spread": np.where(nan_q, f(np.nan), spread),
            "peak": np.where(nan_col, f(np.nan), _expand(peak, up)),
            "entropy": np.where(nan_col, f(np.nan), _expand(entropy, up))}


def fraction_used(got, ref, tol):
    """max |got - ref| / tol over the finite reference values; NaNs must sit at the same places."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    return float((np.abs(got - ref)[ok] / tol[ok]).max())


# ---------------------------------------------------------------- risk-coverage

def risk_oracle(conf, pred, gt, mask=None, nbins=256, err_bin_scale=16.0):
    """Exact.  conf None or (B,H,W), pred, gt (B,H,W) float32, mask None or (B,H,W) ->
    (count (B,nbins), err_q20 (B,nbins), dropped (B)) int64."""
    f = np.float32
    pred, gt = np.asarray(pred, dtype=f), np.asarray(gt, dtype=f)
    B = pred.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.asarray(mask) != 0) if mask is not None else ((gt > 0) & np.isfinite(gt))
        e = np.abs(pred - gt)
        ok = np.isfinite(pred)
        if conf is not None:
            c = np.asarray(conf, dtype=f)
            ok = ok & (c >= 0) & (c <= 1)
            v = np.where(ok, c, f(0)) * f(nbins)
            bins = np.minimum(nbins - 1, v.astype(np.int64))
        else:
            v = e * f(err_bin_scale)
            small = v < f(nbins - 1)                                        # NaN compares false
            bins = nbins - 1 - np.where(small, np.where(small, v, f(0)).astype(np.int64), nbins - 1)
        q20 = (np.fmin(e, f(4096)) * f(1048576)).astype(np.float64)         # fmin: a NaN e gives 4096
        q20 = np.where(np.isnan(q20), 0, q20).astype(np.int64)
    count = np.zeros((B, nbins), np.int64)
    err = np.zeros((B, nbins), np.int64)
    dropped = np.zeros((B,), np.int64)
    for b in range(B):
        sc = (valid[b] & ok[b]).reshape(-1)
        dropped[b] = int((valid[b] & ~ok[b]).sum())
        np.add.at(count[b], bins[b].reshape(-1)[sc], 1)
        np.add.at(err[b], bins[b].reshape(-1)[sc], q20[b].reshape(-1)[sc])
    return count, err, dropped


def curve_ref(count, err_q20):
    """One pair's rows -> (f, m) float64: metrics.Sparsification.curve restated."""
    n = np.asarray(count, dtype=np.int64)
    e = np.asarray(err_q20, dtype=np.int64)
    R = np.cumsum(n[::-1])[::-1]
    E = np.cumsum(e[::-1])[::-1]
    keep = R > 0
    R, E = R[keep].astype(np.float64), E[keep].astype(np.float64)
    if len(R) == 0:
        return R, R
    return 1.0 - R / R[0], E / 2.0 ** 20 / R


def area_ref(count, err_q20):
    f, m = curve_ref(count, err_q20)
    if len(f) < 2:
        return 0.0
    return float(np.sum((f[1:] - f[:-1]) * (m[1:] + m[:-1]) * 0.5))
