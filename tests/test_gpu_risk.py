"""ops.risk_coverage (csrc/risk.hip) on the GPU against the numpy oracle of tests/confidence_oracle.py:
equality everywhere, no tolerance (every sum is an integer)."""
import functools

import numpy as np
import pytest
import torch

from tests import confidence_oracle as co

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 255, 256, 257, 65539)          # H * W: below, at and past a workgroup, past a workgroup's 8192 pixels
F = np.float32
ONE_DOWN, ONE_UP = np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _hw(P):
    return (1, P) if P < 255 else (P // 5, 5) if P % 5 == 0 else (1, P) if P % 257 else (257, P // 257)


@functools.lru_cache(maxsize=None)
def _scene(B, P, seed=0):
    H, W = _hw(P)
    rng = np.random.default_rng(seed + P + 7 * B)
    gt = rng.uniform(0.5, 80.0, (B, H, W)).astype(F)
    gt[rng.uniform(size=gt.shape) < 0.1] = 0.0                              # invalid without a mask
    gt.reshape(-1)[::97] = np.inf
    gt.reshape(-1)[5::193] = np.nan
    gt.reshape(-1)[3::211] = -4.0
    err = (rng.exponential(2.0, gt.shape) * rng.choice([-1.0, 1.0], gt.shape)).astype(F)
    pred = np.where(np.isfinite(gt), gt, F(7)) + err
    pred = pred.astype(F)
    flat = pred.reshape(-1)
    flat[1::101] = np.nan                                                   # dropped where valid
    flat[2::103] = np.inf
    flat[4::107] += F(4096.0)                                               # errors at and above the cap
    flat[6::109] = np.where(np.isfinite(gt.reshape(-1)[6::109]), gt.reshape(-1)[6::109], F(1)) + F(4096.0)
    conf = rng.uniform(0, 1, gt.shape).astype(F)
    special = np.array([0.0, -0.0, 1.0, ONE_DOWN, ONE_UP, np.nan, -1e-9, 2.0, np.inf, -np.inf, 0.5, 0.999999], F)
    c = conf.reshape(-1)
    c[:: 11] = special[np.arange(len(c[::11])) % len(special)]
    mask = rng.uniform(size=gt.shape) < 0.7
    return conf, pred, gt, mask


def _run(dev, conf, pred, gt, mask, nbins, scale):
    from foundationstereo_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return tuple(o.cpu().numpy() for o in ops.risk_coverage(t(conf), t(pred), t(gt), t(mask), nbins, scale))


def _same(got, want, what):
    for g, w, name in zip(got, want, ("count", "err_q20", "dropped")):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(-1))[:8])


@pytest.mark.parametrize("nbins", [2, 256, 1024])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", SIZES)
def test_equals_the_oracle(P, B, nbins):
    dev = _gpu()
    conf, pred, gt, mask = _scene(B, P)
    scale = nbins / 16.0
    for c, m, what in ((conf, None, "conf"), (conf, mask, "conf+mask"), (None, None, "oracle"), (None, mask, "oracle+mask")):
        want = co.risk_oracle(c, pred, gt, m, nbins, scale)
        _same(_run(dev, c, pred, gt, m, nbins, scale), want, (P, B, nbins, what))
    if P >= 255:
        want = co.risk_oracle(conf, pred, gt, None, nbins, scale)
        assert want[0].sum() > 0 and want[2].sum() > 0                      # the scene scores and drops pixels


@pytest.mark.parametrize("value,bin_of", [(1.0, lambda n: n - 1), (float(ONE_DOWN), lambda n: n - 1), (0.0, lambda n: 0),
                                          (-0.0, lambda n: 0), (0.5, lambda n: n // 2)])
def test_everything_in_one_bin(value, bin_of):
    dev = _gpu()
    _, pred, gt, _ = _scene(3, 65539)
    conf = np.full(gt.shape, value, F)
    for nbins in (2, 256, 1024):
        got = _run(dev, conf, pred, gt, None, nbins, 1.0)
        _same(got, co.risk_oracle(conf, pred, gt, None, nbins, 1.0), (value, nbins))
        k = bin_of(nbins)
        assert np.array_equal(got[0].sum(1), got[0][:, k]) and got[0][:, k].min() > 40000


@pytest.mark.parametrize("value", [float(ONE_UP), float("nan"), -1e-30, float("inf")])
def test_confidence_outside_the_unit_interval_is_dropped(value):
    dev = _gpu()
    _, pred, gt, mask = _scene(1, 257)
    conf = np.full(gt.shape, value, F)
    got = _run(dev, conf, pred, gt, mask, 16, 1.0)
    assert got[0].sum() == 0 and got[1].sum() == 0 and got[2][0] == mask.sum()
    _same(got, co.risk_oracle(conf, pred, gt, mask, 16, 1.0), value)


def test_error_cap_and_oracle_bins():
    """e = 4096 and above adds exactly 2^32 per pixel; the oracle ranking puts e * scale >= nbins - 1
    (and a NaN error under a mask) into bin 0."""
    dev = _gpu()
    gt = np.full((1, 1, 8), 10.0, F)
    pred = gt + np.array([0.0, 0.24, 0.25, 1.0, 4095.0, 4096.0, 5000.0, 1e30], F)
    got = _run(dev, None, pred, gt, None, 8, 4.0)                           # bin = 7 - min(7, int(4 e))
    assert got[0][0].tolist() == [4, 0, 0, 1, 0, 0, 1, 2]
    assert got[1][0, 0] == int(4095.0 * 2 ** 20) + 3 * 2 ** 32 and got[2][0] == 0
    _same(got, co.risk_oracle(None, pred, gt, None, 8, 4.0), "cap")
    gt2 = gt.copy()
    gt2[0, 0, 1] = np.nan
    gt2[0, 0, 2] = np.inf
    mask = np.ones(gt.shape, bool)
    got = _run(dev, None, pred, gt2, mask, 8, 4.0)
    _same(got, co.risk_oracle(None, pred, gt2, mask, 8, 4.0), "non-finite gt under a mask")
    assert got[0][0, 0] == 6 and got[1][0, 0] == int(4095.0 * 2 ** 20) + 5 * 2 ** 32


def test_two_calls_give_equal_bits_and_torch_op_agrees():
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    conf, pred, gt, mask = (torch.from_numpy(a).to(dev) for a in _scene(3, 65539))
    a, b = ops.risk_coverage(conf, pred, gt, mask), ops.risk_coverage(conf, pred, gt, mask)
    c = torch.ops.fsmi.risk_coverage(conf, pred, gt, mask)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    a, c = ops.risk_coverage(None, pred, gt, None, 64, 2.0), torch.ops.fsmi.risk_coverage(None, pred, gt, None, 64, 2.0)
    for x, z in zip(a, c):
        assert torch.equal(x, z)
    # a uint8 mask and a non-contiguous view go in too
    wide = torch.cat([pred, pred], dim=2)[:, :, :pred.shape[2]]
    d = ops.risk_coverage(conf, wide, gt, mask.to(torch.uint8))
    for x, y in zip(ops.risk_coverage(conf, pred, gt, mask), d):
        assert torch.equal(x, y)


def test_sparsification_on_the_device():
    dev = _gpu()
    from foundationstereo_amd import metrics
    conf, pred, gt, mask = _scene(3, 65539)
    t = lambda a: torch.from_numpy(a).to(dev)
    s = metrics.sparsification(t(conf), t(pred), t(gt), t(mask), nbins=64, err_cap=8.0)
    o = metrics.sparsification(None, t(pred), t(gt), t(mask), nbins=64, err_cap=8.0)
    want = co.risk_oracle(conf, pred, gt, mask, 64, 8.0)
    wo = co.risk_oracle(None, pred, gt, mask, 64, 8.0)
    assert np.array_equal(s.count.cpu().numpy(), want[0]) and np.array_equal(o.err_q20.cpu().numpy(), wo[1])
    for b in range(3):
        f, m = s.curve(b)
        assert f.is_cuda and f.dtype == torch.float64
        fr, mr = co.curve_ref(want[0][b], want[1][b])
        np.testing.assert_allclose(f.cpu().numpy(), fr, rtol=1e-12)
        np.testing.assert_allclose(m.cpu().numpy(), mr, rtol=1e-12)
        np.testing.assert_allclose(float(s.ause(o, b)), co.area_ref(want[0][b], want[1][b]) - co.area_ref(wo[0][b], wo[1][b]),
                                   rtol=1e-12)
        assert float(o.ause(o, b)) == 0.0 and float(s.ause(o, b)) > 0.0
    # (H,W) and (B,1,H,W) go in as visibility.classify takes them
    one = metrics.sparsification(t(conf)[0], t(pred)[0], t(gt)[0], t(mask)[0], nbins=64, err_cap=8.0)
    four = metrics.sparsification(t(conf)[:, None], t(pred)[:, None], t(gt)[:, None], t(mask)[:, None], nbins=64, err_cap=8.0)
    assert torch.equal(one.count[0], s.count[0]) and torch.equal(four.err_q20, s.err_q20)
