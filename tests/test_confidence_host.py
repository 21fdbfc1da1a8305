"""CPU-only checks of the confidence and risk-coverage stages: the numpy oracle against closed forms,
how much of each tolerance plain fp32 evaluation uses, the entry points' refusals (made before any HIP
call), the front ends' refusals, and the sparsification curve arithmetic (plain torch, so it runs on
CPU tensors)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import confidence_oracle as co

DS = (1, 2, 7, 48, 104, 200, 512)
KINDS = ("std2", "std12", "alt88")
RADII = (0.0, 1.0, 2.5)


def _lib():
    from foundationstereo_amd import _lib
    return _lib, _lib.load()


def test_entry_points_are_exported_and_declared():
    _l, lib = _lib()
    assert len(_l.SIGNATURES["fsmi_disp_confidence"]) == 14 and len(_l.SIGNATURES["fsmi_risk_coverage"]) == 13
    assert hasattr(lib, "fsmi_disp_confidence") and hasattr(lib, "fsmi_risk_coverage")
    from foundationstereo_amd import confidence, ops, torch_ops
    assert "disp_confidence" in torch_ops.OPS and "risk_coverage" in torch_ops.OPS
    assert confidence.CHANNELS == ops.CONF_CHANNELS == co.CHANNELS


# ---------------------------------------------------------------- the oracle against closed forms

@pytest.mark.parametrize("fn", [co.confidence_ref, co.confidence_f32])
@pytest.mark.parametrize("D,k", [(1, 0), (2, 1), (7, 3), (48, 0), (48, 47)])
def test_one_hot_column_at_its_bin_is_exact(fn, D, k):
    logits = np.full((1, D, 2, 3), -np.inf, np.float32)
    logits[:, k] = 5.0
    logits[0, :, 1, 2] = -200.0                       # expf(-200 - 5) underflows to 0 in fp32 ...
    logits[0, k, 1, 2] = 5.0
    disp = np.full((1, 4, 6), 2.0 * k, np.float32)    # up = 2: q = disp / 2 = k
    for radius in RADII:
        got = fn(logits, disp, up=2, radius=radius)
        exact = fn is co.confidence_f32
        for name, want in (("mass", 1.0), ("peak", 1.0), ("entropy", 1.0), ("spread", 0.0)):
            if exact:
                assert np.all(got[name] == want), (name, radius)
            else:                                     # ... and to 1e-89 in fp64 (spread: its square root)
                np.testing.assert_allclose(got[name], want, atol=1e-40, rtol=0)
        self_mode = fn(logits, None, up=2, radius=radius)
        assert np.all(self_mode["mass"] == 1.0)
        assert np.all(self_mode["spread"] == 0.0) if exact else np.all(self_mode["spread"] < 1e-40)


@pytest.mark.parametrize("D,r", [(D, r) for D in (2, 7, 48, 104) for r in (0, 1, 2) if 2 * r + 1 <= D])
def test_uniform_column(D, r):
    logits = np.full((1, D, 1, 2), 3.25, np.float32)
    qs = np.array([[[float(r), float(D - 1 - r)]]], np.float32)         # integer queries whose window is inside
    got = co.confidence_ref(logits, qs, up=1, radius=float(r))
    np.testing.assert_allclose(got["peak"], 1.0 / D, rtol=1e-15)
    np.testing.assert_allclose(got["entropy"], 0.0, atol=1e-15)
    np.testing.assert_allclose(got["mass"], (2 * r + 1) / D, rtol=1e-14)
    mu = (D - 1) / 2.0
    np.testing.assert_allclose(got["spread"], np.sqrt((D * D - 1) / 12.0 + (mu - qs.astype(np.float64)) ** 2), rtol=1e-13)
    f32 = co.confidence_f32(logits, qs, up=1, radius=float(r))
    assert np.all(f32["peak"] == np.float32(1) / np.float32(D))


def test_non_finite_inputs_give_the_stated_nans():
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((1, 5, 2, 4)).astype(np.float32)
    logits[0, 2, 0, 0] = np.nan
    logits[0, 0, 0, 1] = np.inf
    logits[0, :, 0, 2] = -np.inf
    logits[0, 1, 1, 0] = -np.inf                       # probability 0, everything stays finite
    disp = rng.uniform(0, 4, (1, 2, 4)).astype(np.float32)
    disp[0, 1, 1] = np.nan
    disp[0, 1, 2] = np.inf
    for fn in (co.confidence_ref, co.confidence_f32):
        got = fn(logits, disp, up=1)
        for name in co.CHANNELS:
            assert np.isnan(got[name][0, 0, :3]).all() and np.isfinite(got[name][0, 0, 3]) and np.isfinite(got[name][0, 1, 0])
        for name in ("mass", "spread"):
            assert np.isnan(got[name][0, 1, 1:3]).all() and np.isfinite(got[name][0, 1, 3])
        for name in ("peak", "entropy"):
            assert np.isfinite(got[name][0, 1]).all()


# ---------------------------------------------------------------- fp32 against the tolerances

@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_evaluation_uses_at_most_half_of_each_tolerance(D, kind):
    h, w, up = 3, 8, 2
    logits = co.make_logits(kind, 1, D, h, w, seed=D)
    rng = np.random.default_rng(1000 + D)
    disp = (rng.uniform(-2.0, D + 1.0, (1, h * up, w * up)) * up).astype(np.float32)
    worst = {}
    for radius in RADII:
        for d, self_mode in ((disp, False), (None, True)):
            ref = co.confidence_ref(logits, d, up=up, radius=radius)
            got = co.confidence_f32(logits, d, up=up, radius=radius)
            tol = co.tolerances(D, ref, self_mode)
            for name in co.CHANNELS:
                worst[name] = max(worst.get(name, 0.0), co.fraction_used(got[name], ref[name], tol[name]))
    print(f"D={D} {kind}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.5, worst


# ---------------------------------------------------------------- refusals

def _conf_call(lib, B=1, D=8, h=2, w=4, up=4, radius=1.0, logits=1, outs=(1, 1, 1, 1), offset=0):
    # pointer values are never dereferenced: every refusal below happens before a HIP call
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    return lib.fsmi_disp_confidence(p + offset if logits else None, B, D, h, w, None, up, 0.25, radius,
                                    *[p if o else None for o in outs], None)


def test_disp_confidence_refusals():
    _, lib = _lib()
    for kw, word in ((dict(D=0), b"D = 0"), (dict(D=1025), b"D = 1025"), (dict(up=0), b"up = 0"), (dict(up=9), b"up = 9"),
                     (dict(radius=-0.5), b"radius"), (dict(radius=float("inf")), b"radius"),
                     (dict(radius=float("nan")), b"radius"), (dict(outs=(0, 0, 0, 0)), b"null"),
                     (dict(logits=0), b"null"), (dict(B=0), b"shape"), (dict(h=-1), b"shape"),
                     (dict(h=16384, w=16384, up=4), b"2^31"), (dict(offset=2), b"aligned")):
        assert _conf_call(lib, **kw) == 1001, kw
        msg = lib.fsmi_last_error()
        assert b"fsmi_disp_confidence" in msg and word in msg, (kw, msg)


def test_risk_coverage_refusals():
    _, lib = _lib()
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(B=1, H=2, W=4, nbins=16, scale=1.0, pred=p, count=p):
        return lib.fsmi_risk_coverage(None, pred, p, None, B, H, W, nbins, scale, count, p, p, None)
    for kw, word in ((dict(nbins=1), b"nbins = 1"), (dict(nbins=1025), b"nbins = 1025"), (dict(scale=0.0), b"err_bin_scale"),
                     (dict(scale=float("nan")), b"err_bin_scale"), (dict(pred=None), b"null"), (dict(count=None), b"null"),
                     (dict(B=0), b"shape"), (dict(H=65536, W=65536), b"2^31"), (dict(count=p + 4), b"aligned")):
        assert call(**kw) == 1001, kw
        msg = lib.fsmi_last_error()
        assert b"fsmi_risk_coverage" in msg and word in msg, (kw, msg)


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    from foundationstereo_amd import confidence, metrics, ops
    logits, d = torch.zeros(1, 8, 2, 4), torch.ones(1, 8, 16)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_confidence(logits, d)
    with pytest.raises(RuntimeError, match="ROCm"):
        confidence.from_logits(logits)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.risk_coverage(d, d, d)
    with pytest.raises(RuntimeError, match="ROCm"):
        metrics.sparsification(None, d, d)
    with pytest.raises(RuntimeError, match="want"):
        ops.disp_confidence(logits, d, want=())
    with pytest.raises(RuntimeError, match="want"):
        ops.disp_confidence(logits, d, want=("mass", "variance"))
    with pytest.raises(RuntimeError, match="up = 0"):
        ops.disp_confidence(logits, d, up=0)
    with pytest.raises(RuntimeError, match="radius"):
        ops.disp_confidence(logits, d, radius=-1.0)
    with pytest.raises(RuntimeError, match="radius"):
        ops.disp_confidence(logits, d, radius=float("nan"))
    with pytest.raises(RuntimeError, match="nbins"):
        ops.risk_coverage(d, d, d, nbins=1)
    with pytest.raises(RuntimeError, match="err_bin_scale"):
        ops.risk_coverage(d, d, d, err_bin_scale=0.0)
    with pytest.raises(ValueError, match="err_cap"):
        metrics.sparsification(None, d, d, err_cap=0.0)
    with pytest.raises(ValueError, match=r"\(H,W\)"):
        confidence.from_logits(logits, torch.ones(8))

    class NoLogits:
        last_logits = None
    with pytest.raises(RuntimeError, match="keep_logits"):
        confidence.from_model(NoLogits(), d)


def test_keep_logits_is_a_plain_attribute():
    from foundationstereo_amd import synth
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    m = FoundationStereo(synth.make_args(max_disp=32, corr_levels=2, vit_size="vits"))
    assert m.keep_logits is False and m.last_logits is None
    keys = set(m.state_dict())
    m.keep_logits = True
    assert set(m.state_dict()) == keys and not any("logits" in k for k in keys)
    assert not any("logits" in n for n, _ in m.named_buffers())


# ---------------------------------------------------------------- the sparsification curve

def _scene(seed=5, B=2, H=23, W=31):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(1.0, 60.0, (B, H, W)).astype(np.float32)
    gt[:, ::7, ::5] = 0.0                                                   # invalid
    err = (rng.exponential(1.5, (B, H, W)) * rng.choice([-1.0, 1.0], (B, H, W))).astype(np.float32)
    pred = (gt + err).astype(np.float32)
    conf = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    return conf, pred, gt


def _spars(count, err, dropped):
    from foundationstereo_amd import metrics
    return metrics.Sparsification(torch.from_numpy(count), torch.from_numpy(err), torch.from_numpy(dropped))


def test_curve_area_and_ause_match_numpy():
    conf, pred, gt = _scene()
    nbins, scale = 64, 4.0
    s = _spars(*co.risk_oracle(conf, pred, gt, None, nbins, scale))
    o = _spars(*co.risk_oracle(None, pred, gt, None, nbins, scale))
    for b in range(2):
        f, m = s.curve(b)
        fr, mr = co.curve_ref(s.count[b].numpy(), s.err_q20[b].numpy())
        assert f.dtype == torch.float64 and f[0] == 0.0
        np.testing.assert_allclose(f.numpy(), fr, rtol=1e-12, atol=0)
        np.testing.assert_allclose(m.numpy(), mr, rtol=1e-12, atol=0)
        a, ao = co.area_ref(s.count[b].numpy(), s.err_q20[b].numpy()), co.area_ref(o.count[b].numpy(), o.err_q20[b].numpy())
        np.testing.assert_allclose(float(s.area(b)), a, rtol=1e-12)
        np.testing.assert_allclose(float(s.ause(o, b)), a - ao, rtol=1e-12)
        assert float(o.ause(o, b)) == 0.0                                   # the oracle ranking against itself
        assert float(s.ause(o, b)) > 0.0                                    # a random confidence is worse than the oracle
        # the first point is the plain mean error over the scored pixels
        valid = gt[b] > 0
        np.testing.assert_allclose(float(m[0]), np.abs(pred[b] - gt[b])[valid].astype(np.float64).mean(), rtol=1e-5)


def test_empty_and_single_bin_curves():
    z = np.zeros((1, 8), np.int64)
    s = _spars(z, z, np.zeros(1, np.int64))
    f, m = s.curve()
    assert len(f) == 0 and len(m) == 0 and float(s.area()) == 0.0
    one = z.copy()
    one[0, 7] = 5
    s = _spars(one, one * 2 ** 20, np.zeros(1, np.int64))
    f, m = s.curve()
    assert f.tolist() == [0.0] * 8 and m.tolist() == [1.0] * 8 and float(s.area()) == 0.0


def test_confidence_decreasing_in_the_error_has_ause_within_one_bin():
    """conf = 1 - e / cap is the oracle's own binning up to the rounding of the two products, so a
    pixel moves by at most one bin between the two histograms.  A shift of pixels by one bin moves the
    curve's point j only through the pixels of bin j - 1 / j, whose error differs from the bin edge by at
    most one bin width cap / nbins: the two areas differ by at most that width."""
    _, pred, gt = _scene(seed=6)
    nbins, cap = 64, 16.0
    e = np.abs(pred - gt)
    conf = np.clip(1.0 - e / np.float32(cap), 0.0, 1.0).astype(np.float32)
    s = _spars(*co.risk_oracle(conf, pred, gt, None, nbins, nbins / cap))
    o = _spars(*co.risk_oracle(None, pred, gt, None, nbins, nbins / cap))
    for b in range(2):
        assert abs(float(s.ause(o, b))) <= cap / nbins
