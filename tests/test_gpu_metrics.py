"""The metrics stage on the GPU (csrc/metrics.hip through ops, metrics and torch.ops.fsmi) against
tests/metrics_oracle.py.  Counts, rates, min / max and the error map are exact; the fp64 sums differ
from the oracle's only in the order of the additions, which bounds them:
  sum e, sum e^2, epe, rmse   (N + 4) * 2^-52 relative, N = valid pixels (non-negative terms, N - 1 adds,
                              the division and the square root)
  pred_mean                   (P + 4) * 2^-52 * sum |x - x0| / P, P = pixels of the pair
  variance                    (P + 4) * 2^-52 * sum (x - x0)^2 / (P - 1); pred_std through the square root:
                              |d std| <= |d var| / std, plus one rounding
"""
import os

import numpy as np
import pytest
import torch

from tests import metrics_oracle as mo

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
COUNTS = [0, 3, 4] + list(range(9, 17))
RATES = [3] + list(range(9, 17))
# fewer pixels than a block; H*W odd with B > 1 (pair bases off the 16-byte grid); aligned; >= 3 blocks
# per pair with a ragged last one
SHAPES = [(1, 3, 5), (3, 37, 61), (2, 32, 64), (2, 97, 101)]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _data(shape, seed, holes=0.1):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 60.0, shape).astype(np.float32)
    gt[rng.random(shape) < holes] = 0.0
    noise = rng.standard_normal(shape) * np.where(rng.random(shape) < 0.25, 6.0, 0.6)
    return (gt + noise).astype(np.float32), gt


def _close(got, want, rel):
    """|got - want| <= rel * |want| elementwise; NaN and inf must coincide"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (got, want)
    assert np.all(np.abs(got[fin] - want[fin]) <= rel[fin] * np.abs(want[fin])), (got, want, rel)


def _check(pred, gt, mask, thr, table, sums, error=None):
    """Every figure of (table, sums, error) (device tensors) against the oracle on numpy inputs."""
    wt, ws, we = mo.metrics(pred, gt, mask, thr)
    table, sums = table.cpu().numpy(), sums.cpu().numpy()
    B, P = pred.shape[0], pred[0].size
    assert table.shape == sums.shape == (B, 17) and table.dtype == np.float64
    assert np.array_equal(sums[:, COUNTS], ws[:, COUNTS])
    assert np.array_equal(table[:, [0, 4]], wt[:, [0, 4]])
    assert np.array_equal(table[:, RATES], wt[:, RATES])                    # the same fp64 division
    assert np.array_equal(table[:, 7:9], wt[:, 7:9], equal_nan=True) and np.array_equal(sums[:, 7:9], ws[:, 7:9],
                                                                                       equal_nan=True)
    N = ws[:, 0]
    relN = (N + 4) * EPS
    for col in (1, 2):
        _close(sums[:, col], ws[:, col], relN)
        _close(table[:, col], wt[:, col], relN)
    for b in range(B):
        dev1, dev2 = mo.abs_dev(pred[b]), ws[b, 6]
        if not np.isfinite(dev1):                                           # NaN or inf in the prediction
            assert np.array_equal(table[b, 5:7], wt[b, 5:7], equal_nan=True), (table[b, 5:7], wt[b, 5:7])
            assert np.array_equal(sums[b, 5:7], ws[b, 5:7], equal_nan=True)
            continue
        assert abs(sums[b, 5] - ws[b, 5]) <= (P + 4) * EPS * dev1
        assert abs(sums[b, 6] - ws[b, 6]) <= (P + 4) * EPS * dev2
        assert abs(table[b, 5] - wt[b, 5]) <= (P + 4) * EPS * dev1 / P
        if P == 1:
            assert np.isnan(table[b, 6])
            continue
        bvar = (P + 4) * EPS * dev2 / (P - 1)
        var_got = (sums[b, 6] - sums[b, 5] * sums[b, 5] / P) / (P - 1)
        assert abs(var_got - wt[b, 6] ** 2) <= bvar + 2 * EPS * wt[b, 6] ** 2
        if wt[b, 6] > 0:
            assert abs(table[b, 6] - wt[b, 6]) <= bvar / wt[b, 6] + EPS * wt[b, 6]
        else:
            assert table[b, 6] == 0
    if error is not None:
        assert np.array_equal(error.cpu().numpy(), we, equal_nan=True)
    return wt, ws


def _run(pred, gt, mask=None, thr=(1.0, 3.0, 5.0), want_error=True):
    dev = _gpu()
    from foundationstereo_amd import ops
    table, sums, error = ops.disp_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev),
                                          None if mask is None else torch.from_numpy(mask).to(dev), thr,
                                          want_error=want_error)
    assert (error is not None) == want_error
    return table, sums, error


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_oracle(shape, with_mask):
    _gpu()
    from foundationstereo_amd import ops
    B, H, W = shape
    nb = ops.disp_metrics_blocks(H, W)
    if shape == (1, 3, 5):
        assert nb == 1 and H * W < 256
    if shape == (2, 97, 101):
        assert nb >= 3 and ((H * W) // 4) % (nb * 256) != 0 and (H * W) % 4 != 0
    pred, gt = _data(shape, 7 + H)
    mask = (np.random.default_rng(3).random(shape) < 0.7) if with_mask else None   # valid where gt == 0 too
    wt, ws = _check(pred, gt, mask, (1.0, 3.0, 5.0), *_run(pred, gt, mask))
    assert (ws[:, 0] > 0).all()
    if H * W > 1000:                                                        # the data exercises every counter
        assert (ws[:, 3] > 0).all() and (ws[:, 9] > ws[:, 11]).all() and (ws[:, 11] > 0).all()


def test_default_validity_without_mask():
    """gt of 0, a negative value, +inf and NaN are invalid pixels; the prediction under them still
    enters the prediction's own statistics."""
    shape = (2, 9, 13)
    pred, gt = _data(shape, 11, holes=0.0)
    gt[0, 0, :4] = [0.0, -2.0, np.inf, np.nan]
    gt[1, 8, 12] = np.nan
    table, sums, error = _run(pred, gt)
    wt, ws = _check(pred, gt, None, (1.0, 3.0, 5.0), table, sums, error)
    assert ws[:, 0].tolist() == [9 * 13 - 4, 9 * 13 - 1] and ws[:, 4].tolist() == [0, 0]
    assert np.isinf(error[0, 0, :4].cpu().numpy()).all() and np.isfinite(wt[:, 1]).all()


def test_empty_pair_and_single_pixel_pair():
    """A pair without a valid pixel between pairs that have some scores zeros and leaves its
    neighbours alone; a pair with exactly one valid pixel."""
    shape = (4, 37, 61)
    pred, gt = _data(shape, 12)
    mask = gt > 0
    mask[1] = False
    mask[2] = False
    mask[2, 36, 60] = True
    gt[2, 36, 60], pred[2, 36, 60] = 10.0, 14.5
    table, sums, error = _run(pred, gt, mask)
    wt, ws = _check(pred, gt, mask, (1.0, 3.0, 5.0), table, sums, error)
    t = table.cpu().numpy()
    assert t[1, [0, 1, 2, 3]].tolist() == [0, 0, 0, 0] and not t[1, 9:].any()
    assert t[2, [0, 1, 2, 3]].tolist() == [1, 4.5, 4.5, 1.0] and t[2, 9:12].tolist() == [1.0, 1.0, 0.0]
    assert t[0, 0] > 1000 and t[3, 0] > 1000
    assert np.isinf(error[1].cpu().numpy()).all()


@pytest.mark.parametrize("K", [0, 3, 8])
def test_threshold_counts(K):
    thr = (0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 8.0)[:K] if K != 3 else (1.0, 3.0, 5.0)
    pred, gt = _data((2, 21, 23), 13)
    table, sums, error = _run(pred, gt, None, thr)
    wt, ws = _check(pred, gt, None, thr, table, sums, error)
    assert not ws[:, 9 + K:].any() and not table[:, 9 + K:].any()             # unused slots are 0
    if K == 8:
        assert (np.diff(ws[:, 9:], axis=1) <= 0).all() and (ws[:, 16] > 0).all()


def test_threshold_is_compared_in_fp32():
    """torch compares an fp32 tensor with the Python float 0.1 in fp32: an error of float32(0.1) is
    not > 0.1, the next float up is."""
    e = np.float32(0.1)
    pred = np.zeros((1, 2, 5), np.float32)
    pred[0, 0, :3] = [e, np.nextafter(e, np.float32(1)), np.nextafter(e, np.float32(0))]
    gt = np.zeros_like(pred)
    mask = np.ones(pred.shape, bool)
    table, sums, error = _run(pred, gt, mask, (0.1,))
    _check(pred, gt, mask, (0.1,), table, sums, error)
    assert sums[0, 9].item() == 1 and table[0, 9].item() == 0.1 and sums[0, 0].item() == 10


def test_hand_made_edge_inputs():
    """The inputs of the oracle's self-check (tests/test_metrics_host.py) through the kernels, a one-pixel
    map (unbiased std: NaN) and a constant map (std exactly 0)."""
    pred = np.array([[[1.0, 2.0, np.nan, 4.0]]], np.float32)
    gt = np.array([[[1.0 + np.float32(0.1), 0.0, 3.0, np.inf]]], np.float32)
    table, sums, error = _run(pred, gt, None, (0.1,))
    _check(pred, gt, None, (0.1,), table, sums, error)
    assert sums[0, [0, 4, 9]].tolist() == [2, 1, 1] and np.isnan(table[0, [1, 7, 8]].cpu().numpy()).all()
    one = np.ones((1, 1, 1), np.float32)
    table, sums, error = _run(one, one)
    _check(one, one, None, (1.0, 3.0, 5.0), table, sums, error)
    assert np.isnan(table[0, 6].item()) and table[0, 5].item() == 1.0
    flat = np.full((2, 7, 9), 12.34, np.float32)
    table, sums, error = _run(flat, flat + np.float32(1.5))
    _check(flat, flat + np.float32(1.5), None, (1.0, 3.0, 5.0), table, sums, error)
    assert table[:, 6].tolist() == [0.0, 0.0] and table[:, 5].tolist() == [float(np.float32(12.34))] * 2


def test_nan_prediction_under_valid_and_invalid_pixels():
    shape = (3, 10, 11)
    pred, gt = _data(shape, 14, holes=0.0)
    gt[0, 4, 4] = 0.0
    pred[0, 4, 4] = np.nan             # under an invalid pixel: only the prediction's statistics see it
    pred[1, 2, 3] = np.nan             # under a valid one
    pred[1, 5, 5] = np.inf
    pred[2, 7, 1] = np.inf             # inf without a NaN: an infinite mean, equal to the oracle's
    table, sums, error = _run(pred, gt)
    wt, ws = _check(pred, gt, None, (1.0, 3.0, 5.0), table, sums, error)
    t = table.cpu().numpy()
    assert np.isfinite(t[0, 1:4]).all() and t[0, 4] == 0 and np.isnan(t[0, 5:9]).all()
    assert np.isnan(t[1, 1]) and np.isnan(t[1, 2]) and t[1, 4] == 2 and np.isnan(t[1, 7]) and np.isnan(t[1, 8])
    assert np.isfinite(t[1, 9:12]).all()
    assert t[2, 1] == np.inf and t[2, 4] == 1 and t[2, 5] == np.inf and np.isnan(t[2, 6]) and t[2, 8] == np.inf
    assert np.isfinite(t[2, 7]) and np.isfinite(t[2, 9:12]).all()
    # the NaN is "not bad", the inf is bad at every threshold
    fin = pred[1].copy()
    fin[2, 3], fin[5, 5] = gt[1, 2, 3], gt[1, 5, 5]
    assert ws[1, 9] == mo.pair_sums(fin, gt[1])[0][9] + 1


def test_u8_ground_truth_equals_decode_then_float_path():
    dev = _gpu()
    from foundationstereo_amd import metrics, ops
    rng = np.random.default_rng(15)
    shape = (3, 37, 61)
    u8 = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    u8[..., 0] = 0
    u8[..., 1] //= 2
    u8[rng.random(shape) < 0.1] = 0
    u8[0, 0, 0] = 255                                                       # the largest code
    dec = mo.decode(u8, 1000.0)
    pred = (dec + rng.standard_normal(shape) * 2).astype(np.float32)
    tu8, tp = torch.from_numpy(u8).to(dev), torch.from_numpy(pred).to(dev)
    got = metrics.decode_gt(tu8, 1000.0)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), dec)
    assert np.array_equal(metrics.decode_gt(tu8[1], 250.0).cpu().numpy(), mo.decode(u8[1], 250.0))
    assert np.array_equal(metrics.decode_gt(u8[2, :5, :7]).cpu().numpy(), dec[2, :5, :7])     # numpy in, 35 pixels
    a = ops.disp_metrics(tp, tu8, None, (1.0, 3.0, 5.0), 1000.0, True)
    b = ops.disp_metrics(tp, got, None, (1.0, 3.0, 5.0), want_error=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _check(pred, dec, None, (1.0, 3.0, 5.0), *a)
    mask = torch.from_numpy(rng.random(shape) < 0.5).to(dev)
    a = ops.disp_metrics(tp, tu8, mask, (2.0,), 1000.0, True)
    b = ops.disp_metrics(tp, got, mask, (2.0,), want_error=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_views_shapes_and_error_switch():
    """A non-contiguous prediction (what padder.unpad hands in), the (H,W) and (B,1,H,W) forms, a uint8
    mask, and want_error off."""
    dev = _gpu()
    from foundationstereo_amd import metrics
    shape = (2, 37, 61)
    pred, gt = _data(shape, 16)
    big = torch.zeros((2, 1, 48, 72), device=dev)
    big[:, :, 5:42, 4:65] = torch.from_numpy(pred).to(dev)[:, None]
    view = big[..., 5:42, 4:65]
    assert not view.is_contiguous()
    tg = torch.from_numpy(gt).to(dev)
    m = metrics.stereo_metrics(view, tg[:, None], want_error=True)
    _check(pred, gt, None, (1.0, 3.0, 5.0), m.table, m.sums, m.error)
    assert m.bad.shape == (2, 3) and torch.equal(m.epe, m.table[:, 1]) and torch.equal(m.mae, m.epe)
    assert torch.equal(m.d1_all, m.table[:, 3]) and torch.equal(m.n_valid, m.sums[:, 0])
    off = metrics.stereo_metrics(view, tg)
    assert off.error is None and torch.equal(off.table, m.table) and torch.equal(off.sums, m.sums)
    one = metrics.stereo_metrics(view[1, 0], tg[1], mask=(tg[1] > 0).to(torch.uint8), want_error=True)
    # pair 1 alone starts on the 16-byte grid, inside the batch it does not: another order of additions
    _check(pred[1:], gt[1:], gt[1:] > 0, (1.0, 3.0, 5.0), one.table, one.sums, one.error)
    assert torch.equal(one.error[0], m.error[1]) and torch.equal(one.table[0, RATES], m.table[1, RATES])


def test_reproducible_and_capturable():
    """The same input gives the same bits twice, and once more from a captured graph replayed on it."""
    dev = _gpu()
    from foundationstereo_amd import ops
    pred, gt = _data((2, 97, 101), 17)
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    first = ops.disp_metrics(tp, tg, want_error=True)
    second = ops.disp_metrics(tp, tg, want_error=True)
    assert all(torch.equal(x, y) for x, y in zip(first[:2], second[:2]))
    assert torch.equal(first[2], second[2])
    torch.cuda.synchronize()
    sp = torch.zeros_like(tp)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            table, sums, _ = ops.disp_metrics(sp, tg)
    torch.cuda.current_stream().wait_stream(side)
    sp.copy_(tp)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(table, first[0]) and torch.equal(sums, first[1])


def test_does_not_synchronise():
    """stereo_metrics, decode_gt and MetricsAccumulator.update under torch's synchronisation check."""
    dev = _gpu()
    from foundationstereo_amd import metrics
    pred, gt = _data((2, 37, 61), 21)
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    u8 = torch.zeros((2, 37, 61, 3), dtype=torch.uint8, device=dev)
    mask = tg > 0
    metrics.stereo_metrics(tp, tg)                                          # library load, first launches
    acc = metrics.MetricsAccumulator()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = metrics.stereo_metrics(tp, tg, mask, want_error=True)
        acc.update(m)
        acc.update(metrics.stereo_metrics(tp, u8, thresholds=(1.0, 3.0, 5.0)))
        metrics.decode_gt(u8)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert acc.result()["n_pairs"] == 4


def test_reference_wrappers_against_golden():
    """compute_stereo_metrics and monitoring_stereo on device tensors against the reference's own
    outputs, within the host test's bounds (the reference sums in fp32)."""
    dev = _gpu()
    from foundationstereo_amd import metrics
    g = mo.load_golden(os.path.join(REPO, "tests", "golden", "metrics_small.npz"))
    thr, keys = g["thresholds"].tolist(), g["keys"].tolist()
    pred, mask = torch.from_numpy(g["pred"]).to(dev), torch.from_numpy(g["mask"]).to(dev)
    gt = metrics.decode_gt(torch.from_numpy(g["gt_u8"]).to(dev))
    eps32 = 2.0 ** -24
    N = g["mask"].reshape(3, -1).sum(1)

    def compare(got, want, n):
        assert sorted(got) == keys and all(isinstance(v, float) for v in got.values())
        for k, w in zip(keys, want):
            bound = eps32 * w if k.startswith("d") else (n + 2) * eps32 * w
            assert abs(got[k] - w) <= bound, (k, got[k], w)

    for b in range(3):
        compare(metrics.compute_stereo_metrics(pred[b], gt[b], mask[b], thr), g[f"pair{b}"], N[b])
        mon = metrics.monitoring_stereo(pred[b])
        want = g[f"monitoring{b}"]
        # within fp32 rounding of the reference's fp32 reductions: a few roundings of the value
        assert abs(mon["disparity_mean"] - want[0]) <= 4 * eps32 * abs(want[0]), (mon, want)
        assert abs(mon["disparity_std"] - want[1]) <= 4 * eps32 * want[1], (mon, want)
        half = metrics.monitoring_stereo(pred[b].half())                    # any floating dtype, as the reference
        assert half == metrics.monitoring_stereo(pred[b].half().float())
        assert mon["disparity_min"] == want[2] and mon["disparity_max"] == want[3]
    got = metrics.compute_stereo_metrics(pred, gt, mask, thr)
    assert sorted(got) == keys
    for k, w in zip(keys, g["batch"]):                                      # rates: a mean of fp32-rounded quotients
        rel = eps32 + 4 * 2.0 ** -52 if k.startswith("d") else (N.max() + 2) * eps32
        assert w > 0 and abs(got[k] - w) <= rel * w, k
    assert sorted(metrics.compute_stereo_metrics(pred, gt, mask, [0.5, 1.0])) == ["d0_error", "d1_error", "epe", "mae",
                                                                                  "rmse"]


def test_accumulator_on_device_equals_one_call():
    dev = _gpu()
    from foundationstereo_amd import metrics
    pred, gt = _data((3, 37, 61), 18)
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    acc = metrics.MetricsAccumulator()
    acc.update(metrics.stereo_metrics(tp[:2], tg[:2]))
    acc.update(metrics.stereo_metrics(tp[2:], tg[2:]))
    r = acc.result()
    wt, ws, _ = mo.metrics(pred, gt)
    n = ws[:, 0].sum()
    assert r["n_pairs"] == 3 and r["n_valid"] == n
    assert r["per_pair"]["epe"] == pytest.approx(wt[:, 1].mean(), rel=1e-12)
    assert r["per_pair"]["bad_3"] == pytest.approx(wt[:, 10].mean(), rel=1e-12)
    assert r["pooled"]["epe"] == pytest.approx(ws[:, 1].sum() / n, rel=1e-12)
    assert r["pooled"]["rmse"] == pytest.approx(np.sqrt(ws[:, 2].sum() / n), rel=1e-12)
    assert r["pooled"]["d1_all"] == ws[:, 3].sum() / n


def test_torch_ops_match_ops():
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    pred, gt = _data((2, 37, 61), 19)
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    mask = tg > 1.0
    a = torch.ops.fsmi.disp_metrics(tp, tg, mask, [1.0, 2.0], 1000.0, True)
    b = ops.disp_metrics(tp, tg, mask, (1.0, 2.0), want_error=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = torch.ops.fsmi.disp_metrics(tp, tg)
    b = ops.disp_metrics(tp, tg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].numel() == 0 and b[2] is None
    u8 = torch.from_numpy(np.random.default_rng(20).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)).to(dev)
    assert torch.equal(torch.ops.fsmi.gt_decode(u8, 500.0), ops.gt_decode(u8, 500.0))
    a = torch.ops.fsmi.disp_metrics(tp[:, :9, :11], u8, None, [1.0], 500.0, False)
    b = ops.disp_metrics(tp[:, :9, :11], u8, None, (1.0,), 500.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bad_inputs_raise():
    dev = _gpu()
    from foundationstereo_amd import metrics, ops
    x = torch.ones(1, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_metrics(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_metrics(x, x.cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.disp_metrics(x.clone().requires_grad_(True), x)
    with torch.no_grad():
        ops.disp_metrics(x.clone().requires_grad_(True), x)                  # allowed without grad mode
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.disp_metrics(x, x, thresholds=range(9))
    with pytest.raises(RuntimeError, match="gt must be"):
        ops.disp_metrics(x, x[:, :3])
    with pytest.raises(RuntimeError, match="mask"):
        ops.disp_metrics(x, x, mask=x)
    with pytest.raises(RuntimeError, match="gt_scale"):
        ops.disp_metrics(x, torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev), gt_scale=0.0)
    with pytest.raises(ValueError, match="pred must be"):
        metrics.stereo_metrics(torch.ones(2, 2, 4, 4, device=dev), x)
