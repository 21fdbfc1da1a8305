"""CPU-only checks of the metrics stage: the numpy oracle against the reference's own outputs
(tests/golden/metrics_small.npz, tools/make_goldens.py metrics), the C ABI's argument checks, the
block-count function, the reference's key naming and MetricsAccumulator on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import metrics_oracle as mo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return mo.load_golden(os.path.join(REPO, "tests", "golden", "metrics_small.npz"))


def test_decode_is_bit_equal_to_the_reference(golden):
    got = mo.decode(golden["gt_u8"], 1000.0)
    assert got.dtype == np.float32 and np.array_equal(got[0, :8], golden["gt0_decoded_f64"].astype(np.float32))
    assert golden["gt0_decoded_f64"].shape == (8, 61) and (golden["gt0_decoded_f64"] == 0).any()
    assert int(got.max() * 1000) <= 16605816 and (got == 0).any()


def test_oracle_matches_reference_metrics(golden):
    """The reference sums fp32 terms in fp32, the oracle in fp64: for non-negative terms any fp32
    summation order stays within (N + 2) * 2^-24 relative of the exact sum, N = valid pixels of the
    pair.  Measured on this case (3,37,61; 2048, 0 and 2029 valid pixels): the largest relative gap of
    epe / rmse is 3.9e-8 against a bound of 1.2e-4.  Rates are fp32 quotients of exact counts: one fp32
    rounding."""
    thr = golden["thresholds"].tolist()
    keys = golden["keys"].tolist()
    gt = mo.decode(golden["gt_u8"], 1000.0)
    table, sums, _ = mo.metrics(golden["pred"], gt, golden["mask"], thr)
    assert sums[1, 0] == 0 and sums[0, 0] > 1000                    # pair 1's mask is empty
    worst = 0.0
    for b in range(3):
        ref = dict(zip(keys, golden[f"pair{b}"]))
        mine = mo.reference_dict(table[b], thr)
        assert sorted(mine) == keys
        N = sums[b, 0]
        for k in ("epe", "rmse", "mae"):
            if N == 0:
                assert ref[k] == 0.0 and mine[k] == 0.0
                continue
            gap = abs(mine[k] - ref[k]) / ref[k]
            worst = max(worst, gap)
            assert gap <= (N + 2) * EPS32, (b, k, gap)
        for k in keys:
            if k.startswith("d"):
                assert abs(mine[k] - ref[k]) <= EPS32 * max(ref[k], 2.0 ** -126), (b, k)
    print(f"largest relative gap of epe / rmse: {worst:.2e}")
    # the batched call: the mean over pairs, the empty pair counting as zeros
    ref = dict(zip(keys, golden["batch"]))
    mine = mo.reference_dict(table, thr)
    Nmax = sums[:, 0].max()
    for k in keys:
        # a mean of fp32-rounded non-negative quotients stays within one fp32 rounding (the fp64 mean's own
        # roundings beside it); the summed figures keep the summation bound
        rel = EPS32 + 4 * 2.0 ** -52 if k.startswith("d") else (Nmax + 2) * EPS32
        assert ref[k] > 0 and abs(mine[k] - ref[k]) <= rel * ref[k], k


def test_oracle_matches_reference_monitoring(golden):
    """mean / std agree within fp32 rounding: 4 * 2^-24 relative, a few roundings of the value (torch
    reduces in fp32 by a tree and rounds the result; measured here, the gaps are 1 to 2 ulp: mean up to
    3.1e-6 of ~22.4, std up to 0.8e-6 of ~16.3).  A population (biased) std is 3.6e-3 away and fails.  min / max
    exact."""
    table, _, _ = mo.metrics(golden["pred"], mo.decode(golden["gt_u8"]), golden["mask"], ())
    P = golden["pred"][0].size
    for b in range(3):
        mean, std, mn, mx = golden[f"monitoring{b}"]
        assert abs(table[b, 5] - mean) <= 4 * EPS32 * abs(mean), (b, table[b, 5], mean)
        assert abs(table[b, 6] - std) <= 4 * EPS32 * std, (b, table[b, 6], std)
        biased = table[b, 6] * np.sqrt((P - 1) / P)
        assert abs(biased - std) > 4 * EPS32 * std                   # the bound tells the two definitions apart
        assert table[b, 7] == mn and table[b, 8] == mx


def test_oracle_edge_rules_and_table_layout():
    """A self-check of tests/metrics_oracle.py on hand-made edge inputs (tests/test_gpu_metrics.py drives the
    same inputs through the kernels), and the package's column names against the oracle's layout."""
    from foundationstereo_amd import metrics
    assert (metrics.NACC, metrics.MAX_THRESHOLDS) == (mo.NACC, mo.MAXT)
    assert [metrics.N_VALID, metrics.EPE, metrics.RMSE, metrics.D1_ALL, metrics.N_NONFINITE, metrics.PRED_MEAN,
            metrics.PRED_STD, metrics.PRED_MIN, metrics.PRED_MAX, metrics.BAD0] == list(range(10))
    pred = np.array([[[1.0, 2.0, np.nan, 4.0]]], np.float32)
    gt = np.array([[[1.0 + np.float32(0.1), 0.0, 3.0, np.inf]]], np.float32)
    table, sums, err = mo.metrics(pred, gt, None, (0.1,))
    assert sums[0, 0] == 2 and sums[0, 4] == 1                       # gt 0 and +inf invalid; the NaN is counted
    assert np.isnan(table[0, 1]) and np.isnan(table[0, 7]) and np.isnan(table[0, 8])
    assert np.isinf(err[0, 0, 1]) and np.isinf(err[0, 0, 3]) and np.isnan(err[0, 0, 2])
    e0 = np.abs(np.float32(1.0) - gt[0, 0, 0])
    assert sums[0, 9] == (1 if e0 > np.float32(0.1) else 0)
    assert not (np.float32(0.1) > np.float32(0.1))                   # fp32 threshold: an error of float32(0.1) is not bad
    one = mo.metrics(np.ones((1, 1, 1), np.float32), np.ones((1, 1, 1), np.float32))[0]
    assert np.isnan(one[0, 6]) and one[0, 5] == 1.0                  # unbiased std of one pixel


def _lib():
    from foundationstereo_amd import _lib
    return _lib.load()


def test_abi_rejects_bad_args_without_gpu():
    lib = _lib()
    thr = (ctypes.c_float * 3)(1.0, 3.0, 5.0)
    P = 16                                                            # a non-null, aligned stand-in pointer

    def call(pred=P, gt=P, gt_u8=None, mask=None, thresholds=thr, K=3, gt_scale=1000.0, partials=P, sums=P, table=P,
             error=None, B=1, H=4, W=4):
        return lib.fsmi_disp_metrics(pred, gt, gt_u8, mask, thresholds, K, gt_scale, partials, sums, table, error,
                                     B, H, W, None)

    for kw in (dict(pred=None), dict(gt=None), dict(partials=None), dict(sums=None), dict(table=None),
               dict(gt=P, gt_u8=P), dict(K=9), dict(K=-1), dict(K=3, thresholds=None), dict(B=0), dict(H=0), dict(W=-2),
               dict(gt=None, gt_u8=P, gt_scale=0.0), dict(gt=None, gt_u8=P, gt_scale=-1.0)):
        assert call(**kw) == 1001, kw
        assert b"fsmi_disp_metrics" in lib.fsmi_last_error()
    assert lib.fsmi_gt_decode(None, P, 1, 4, 4, 1000.0, None) == 1001
    assert lib.fsmi_gt_decode(P, None, 1, 4, 4, 1000.0, None) == 1001
    assert lib.fsmi_gt_decode(P, P, 1, 0, 4, 1000.0, None) == 1001
    assert lib.fsmi_gt_decode(P, P, 1, 4, 4, 0.0, None) == 1001


def test_blocks_depend_on_pixel_count_only():
    lib = _lib()
    for H, W in ((1, 1), (3, 5), (37, 61), (480, 640), (1024, 1536), (1, 480 * 640), (97, 101), (4000, 6000)):
        n = lib.fsmi_disp_metrics_blocks(H, W)
        assert n >= 1 and n == lib.fsmi_disp_metrics_blocks(W, H) == lib.fsmi_disp_metrics_blocks(1, H * W), (H, W)
    assert lib.fsmi_disp_metrics_blocks(3, 5) == 1 and lib.fsmi_disp_metrics_blocks(97, 101) >= 3
    assert lib.fsmi_disp_metrics_blocks(0, 5) >= 1
    sizes = [lib.fsmi_disp_metrics_blocks(1, p) for p in (1, 10_000, 100_000, 1_000_000, 10_000_000)]
    assert sizes == sorted(sizes)


def test_reference_key_naming():
    from foundationstereo_amd import metrics
    assert [metrics.error_key(t) for t in (0.5, 1.0, 3.0, 5.0)] == ["d0_error", "d1_error", "d3_error", "d5_error"]
    assert sorted(mo.reference_dict(np.zeros(17), [0.5, 1.0])) == ["d0_error", "d1_error", "epe", "mae", "rmse"]


def test_ops_refuse_cpu_tensors_and_grad():
    import foundationstereo_amd
    from foundationstereo_amd import metrics, ops
    assert foundationstereo_amd.stereo_metrics is metrics.stereo_metrics
    x = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_metrics(x, x)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.gt_decode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm"):
        metrics.compute_stereo_metrics(x, x, x > 0)


def test_accumulator_on_cpu_tensors():
    """Two updates (2 pairs, then 1) against a hand computation: per-pair means and pixel-pooled values."""
    from foundationstereo_amd import metrics
    thr = (1.0, 3.0)

    def rows(spec):
        # spec: per pair (n, sum e, sum e2, n_d1, n_bad1, n_bad3)
        table = torch.zeros(len(spec), 17, dtype=torch.float64)
        sums = torch.zeros(len(spec), 17, dtype=torch.float64)
        for i, (n, se, se2, d1, b1, b3) in enumerate(spec):
            sums[i, [0, 1, 2, 3, 9, 10]] = torch.tensor([n, se, se2, d1, b1, b3], dtype=torch.float64)
            if n:
                table[i, [0, 1, 2, 3, 9, 10]] = torch.tensor([n, se / n, (se2 / n) ** 0.5, d1 / n, b1 / n, b3 / n],
                                                             dtype=torch.float64)
        return metrics.StereoMetrics(table=table, sums=sums, thresholds=thr)

    acc = metrics.MetricsAccumulator()
    acc.update(rows([(10, 20.0, 90.0, 2, 6, 2), (0, 0.0, 0.0, 0, 0, 0)]))
    acc.update(rows([(30, 15.0, 30.0, 0, 3, 0)]))
    r = acc.result()
    assert r["n_pairs"] == 3 and r["n_valid"] == 40 and r["thresholds"] == [1.0, 3.0]
    assert r["per_pair"]["epe"] == pytest.approx((2.0 + 0.0 + 0.5) / 3, rel=1e-15)
    assert r["per_pair"]["rmse"] == pytest.approx((3.0 + 0.0 + 1.0) / 3, rel=1e-15)
    assert r["per_pair"]["d1_all"] == pytest.approx((0.2 + 0 + 0) / 3, rel=1e-15)
    assert r["per_pair"]["bad_1"] == pytest.approx((0.6 + 0 + 0.1) / 3, rel=1e-15)
    assert r["pooled"]["epe"] == pytest.approx(35.0 / 40, rel=1e-15)
    assert r["pooled"]["rmse"] == pytest.approx((120.0 / 40) ** 0.5, rel=1e-15)
    assert r["pooled"]["bad_1"] == pytest.approx(9 / 40, rel=1e-15) and r["pooled"]["bad_3"] == pytest.approx(2 / 40)
    with pytest.raises(ValueError, match="thresholds"):
        acc.update(metrics.StereoMetrics(table=torch.zeros(1, 17, dtype=torch.float64),
                                         sums=torch.zeros(1, 17, dtype=torch.float64), thresholds=(2.0,)))
