"""CPU-only checks of the sequence metrics: the numpy oracle (tests/seq_oracle.py) against the
reference's own outputs (tests/golden/seq_small.npz, tools/make_goldens.py seq), the drop-ins' keys and
weights, SequenceAccumulator on CPU tensors and the C ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import seq_oracle as so

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
TINY = 2.0 ** -126
KEYS = ["d1_error_initial", "d1_error_iterative", "d3_error_initial", "d3_error_iterative", "epe_initial",
        "epe_iterative", "loss_initial", "loss_iterative"]


@pytest.fixture(scope="module")
def golden():
    return so.load_golden(os.path.join(REPO, "tests", "golden", "seq_small.npz"))


def _oracle(g, init, gamma, maxd):
    w = so.sequence_weights(so.GOLDEN_K, gamma)
    table, sums, loss = so.seq_metrics([g[init]] + g["preds"], g["gt"], g["mask"], (1.0, 3.0), maxd, 1.0, w, (0,))
    return table, sums, loss, w


def test_golden_case_is_what_the_issue_describes(golden):
    assert golden["keys"].tolist() == KEYS and golden["params"].tolist() == [list(p) for p in so.GOLDEN_PARAMS]
    assert golden["gt"].shape == (3, 37, 61) and not golden["mask"][1].any() and golden["mask"][0].sum() > 1900
    assert golden["init_small"].shape == (3, 10, 16) and len(golden["preds"]) == 5
    for p in golden["preds"]:
        assert 0 < (p > 192).sum() < 60 and (p < 0).sum() > 0
    assert (golden["gt"] > 48).any()


def test_oracle_matches_reference_full_size_rows(golden):
    """Full-size rows: the oracle and the reference see the same fp32 errors; the reference sums them in
    fp32, the oracle in fp64.  For non-negative terms any fp32 summation order stays within
    (N + 2) * 2^-24 relative of the exact sum (tests/test_metrics_host.py), N = the pair's valid pixels:
    that bounds epe_*, loss_initial, loss_iterative and loss.  A rate is an fp32 quotient of exact counts:
    one fp32 rounding.  A weighted figure sums w_k times such terms: sum_k w_k times the per-term bound
    (the reference's K products and additions, in fp64 for the Python floats and in fp32 for
    loss_iterative, sit far inside the summation bound's slack at N ~ 2000: K + 1 more roundings)."""
    worst = 0.0
    for pi, (gamma, maxd) in enumerate(so.GOLDEN_PARAMS):
        table, sums, loss, w = _oracle(golden, "init_full", gamma, maxd)
        assert w[1:] == [gamma ** (5 - k) for k in range(1, 6)] and w[0] == 1.0
        for b in range(3):
            ref = golden[f"fsl_p{pi}_init_full_pair{b}"]
            ref_loss, ref_misc = ref[0], dict(zip(KEYS, ref[1:]))
            mine_loss, mine = so.reference_dict(table[b], w)
            assert sorted(mine) == KEYS
            N = sums[b, 0, 0]
            if N == 0:
                assert ref_loss == 0.0 and mine_loss == 0.0 and not any(ref_misc.values()) and not any(mine.values())
                continue
            rel = (N + 2) * EPS32
            for k in ("epe_initial", "loss_initial", "loss_iterative", "epe_iterative"):
                gap = abs(mine[k] - ref_misc[k]) / ref_misc[k]
                worst = max(worst, gap)
                assert gap <= rel, (pi, b, k, gap)
            assert abs(mine_loss - ref_loss) <= rel * ref_loss, (pi, b)
            assert abs(loss[b] - mine_loss) <= 16 * 2.0 ** -52 * mine_loss      # the kernel's order of the same sum
            for k in ("d1_error_initial", "d3_error_initial"):
                assert abs(mine[k] - ref_misc[k]) <= EPS32 * max(ref_misc[k], TINY), (pi, b, k)
            for k, col in (("d1_error_iterative", so.BAD0 + 1), ("d3_error_iterative", so.BAD0)):
                bound = sum(wk * EPS32 * max(r, TINY) for wk, r in zip(w[1:], table[b, 1:, col]))
                assert abs(mine[k] - ref_misc[k]) <= bound + 8 * 2.0 ** -52 * ref_misc[k], (pi, b, k)
            assert ref_misc["d3_error_iterative"] > 1.0                         # a weighted sum, not a mean
    assert golden["fsl_p0_init_full_pair0"][0] != golden["fsl_p1_init_full_pair0"][0]
    print(f"largest relative gap of the summed figures: {worst:.2e}")


def test_oracle_matches_reference_single_map_losses(golden):
    """disparity_l1_loss, disparity_smooth_l1_loss (beta 0.5), disparity_epe_loss on the last full-size
    prediction: the bounds of the test above."""
    for pi, (gamma, maxd) in enumerate(so.GOLDEN_PARAMS):
        last = golden["preds"][-1]
        for beta, rows in ((1.0, (0, 2)), (0.5, (1,))):
            table, sums, _ = so.seq_metrics([last], golden["gt"], golden["mask"], (1.0, 3.0), maxd, beta)
            for b in range(3):
                N = sums[b, 0, 0]
                for i in rows:
                    loss, epe, d1, d3 = golden[f"single_p{pi}_pair{b}"][i]
                    mine = table[b, 0]
                    if N == 0:
                        assert (loss, epe, d1, d3) == (0, 0, 0, 0) and not mine[1:].any()
                        continue
                    assert abs(mine[so.SMOOTH_L1 if i == 1 else so.EPE] - loss) <= (N + 2) * EPS32 * loss
                    assert abs(mine[so.EPE] - epe) <= (N + 2) * EPS32 * epe
                    assert abs(mine[so.BAD0 + 1] - d1) <= EPS32 * d1 and abs(mine[so.BAD0] - d3) <= EPS32 * d3


def test_oracle_matches_reference_resized_initial_row(golden):
    """The 10 x 16 initial disparity resized to 37 x 61.  The oracle evaluates
    l0y * (l0x * p00 + l1x * p01) + l1y * (l0x * p10 + l1x * p11); F.interpolate on the CPU takes another
    order of the same four products.  Both orders use the same taps and the same fp32 weights (each
    l1 = src - i0 and l0 = 1 - l1 is one rounding of one formula), and l0 + l1 = 1 within 2^-24, so every
    intermediate is at most M = max |tap| (1 + 2^-23) in size.  An evaluation is two 2-tap stages in
    some order or one 4-term sum of weight products: at most 4 products (with, for the product form, 4
    weight products folded in: 2 roundings per term on terms that sum to M) and 3 additions, i.e. at most
    6 roundings of 2^-24 * M each when the stages' errors are weighed by the weights that multiply them.
    Two evaluations differ by at most 12 * 2^-24 * M = seq_oracle.resize_gap_bound.  The clamp and the
    absolute value are 1-Lipschitz, and so is smooth-L1: a pixel's error and loss term move by at most
    that gap, hence so do their means; the summation bound comes on top.  A rate moves only through
    pixels whose error lies within the gap of its threshold: M_thr such pixels move it by M_thr / N."""
    import torch.nn.functional as F
    small, gt, mask = golden["init_small"], golden["gt"], golden["mask"]
    H, W = gt.shape[1:]
    ref_up = F.interpolate(torch.from_numpy(small)[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    mine_up = so.upsample(small, H, W)
    measured, bound = float(np.abs(mine_up - ref_up.numpy()).max()), so.resize_gap_bound(np.abs(small).max())
    print(f"resize: measured gap {measured:.3e}, bound {bound:.3e}")
    assert measured <= bound
    # the taps are clamped at every border, and the ratio is not an integer
    y0, y1, _, ly1 = so.taps(10, H)
    assert y0[0] == y1[0] == 0 or ly1[0] == 0
    assert y0[-1] == 9 and y1[-1] == 9 and len(set(np.diff(y0).tolist())) > 1
    for pi, (gamma, maxd) in enumerate(so.GOLDEN_PARAMS):
        table, sums, loss, w = _oracle(golden, "init_small", gamma, maxd)
        e = np.abs(so.row_values(small, H, W, 1.0, maxd) - gt)
        for b in range(3):
            ref = dict(zip(KEYS, golden[f"fsl_p{pi}_init_small_pair{b}"][1:]))
            _, mine = so.reference_dict(table[b], w)
            N = sums[b, 0, 0]
            if N == 0:
                assert not any(ref.values()) and not any(mine.values())
                continue
            for k in ("epe_initial", "loss_initial"):
                assert abs(mine[k] - ref[k]) <= bound + (N + 2) * EPS32 * ref[k], (pi, b, k, mine[k], ref[k])
            ev = e[b][mask[b]]
            for k, t in (("d1_error_initial", 3.0), ("d3_error_initial", 1.0)):
                M = int((np.abs(ev - t) <= bound).sum())
                assert M <= 2                                                   # the golden case's condition
                assert abs(mine[k] - ref[k]) <= M / N + EPS32 * ref[k], (pi, b, k, M)
            for k in ("epe_iterative", "loss_iterative"):                       # the full-size rows, unchanged
                assert abs(mine[k] - ref[k]) <= (N + 2) * EPS32 * ref[k]
        # the resized smooth-L1 loss alone (disparity_smooth_l1_loss resizes too)
        for b in (0, 2):
            loss1, epe1, _, _ = golden[f"single_p{pi}_pair{b}"][3]
            N = sums[b, 0, 0]
            assert abs(table[b, 0, so.SMOOTH_L1] - loss1) <= bound + (N + 2) * EPS32 * loss1
            assert abs(table[b, 0, so.EPE] - epe1) <= bound + (N + 2) * EPS32 * epe1


def test_oracle_edge_rules():
    """A self-check of tests/seq_oracle.py on hand-made inputs: the clamp keeps NaN, +inf means no clamp
    at either end, beta = 0 is plain L1, an exact x4 resize of a constant map is that constant."""
    v = so.row_values(np.array([[[-1.0, 5.0, np.nan, 300.0]]], np.float32), 1, 4, 1.0, 192.0)
    assert v[0, 0, :2].tolist() == [0.0, 5.0] and np.isnan(v[0, 0, 2]) and v[0, 0, 3] == 192.0
    v = so.row_values(np.array([[[-1.0, 300.0]]], np.float32), 1, 2)
    assert v[0, 0].tolist() == [-1.0, 300.0]
    e = np.array([0.25, 0.5, 2.0], np.float32)
    assert so.smooth_l1(e, 0.0) is e
    assert so.smooth_l1(e, 0.5).tolist() == [0.0625, 0.25, 1.75] and so.smooth_l1(e, 1.0).tolist() == [0.03125, 0.125, 1.5]
    assert np.array_equal(so.upsample(np.full((1, 8, 16), 3.5, np.float32), 32, 64), np.full((1, 32, 64), 3.5, np.float32))
    one = so.upsample(np.array([[[7.0]]], np.float32), 3, 5)
    assert one.shape == (1, 3, 5) and (one == 7.0).all()
    table, sums, loss = so.seq_metrics([np.ones((1, 2, 2), np.float32)] * 2, np.full((1, 2, 2), 3.0, np.float32),
                                       weights=[1.0, 0.5], smooth_rows=(0,))
    assert table[0, :, so.EPE].tolist() == [2.0, 2.0] and table[0, 0, so.SMOOTH_L1] == 1.5 and loss[0] == 2.5


def test_package_layout_and_weights():
    from foundationstereo_amd import losses
    assert (losses.NACC, losses.MAX_ROWS) == (so.NACC, so.MAX_ROWS)
    assert [losses.N_VALID, losses.EPE, losses.RMSE, losses.SMOOTH_L1, losses.D1_ALL, losses.N_NONFINITE,
            losses.BAD0] == list(range(7))
    assert losses.sequence_weights(3, 0.5) == [1.0, 0.25, 0.5, 1.0] == so.sequence_weights(3, 0.5)
    assert losses.sequence_weights(2, 0.9, with_init=False) == [0.9, 1.0]
    import foundationstereo_amd
    assert foundationstereo_amd.sequence_metrics is losses.sequence_metrics


def test_drop_ins_refuse_cpu_tensors_and_grad():
    from foundationstereo_amd import losses, ops
    x = torch.zeros(4, 4)
    for fn in (losses.disparity_l1_loss, losses.disparity_smooth_l1_loss, losses.disparity_epe_loss):
        with pytest.raises(RuntimeError, match="ROCm"):
            fn(x, x, x > 0)
    with pytest.raises(RuntimeError, match="ROCm"):
        losses.foundation_stereo_loss(x, [x, x], x, x > 0)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.seq_metrics([x[None]], x[None])
    with pytest.raises(RuntimeError, match="rows"):
        ops.seq_metrics([], x[None])
    with pytest.raises(ValueError, match="does not resize"):
        losses.disparity_epe_loss(torch.zeros(2, 2), x, x > 0)


def test_accumulator_on_cpu_tensors():
    """Two updates (2 pairs, then 1) of 2 rows against a hand computation."""
    from foundationstereo_amd import losses
    thr, w = (1.0, 3.0), (1.0, 1.0)

    def m(spec, loss):
        # spec: per pair, per row (n, sum e, sum e2, sum sl1, n_d1, n_bad1, n_bad3)
        B, R = len(spec), len(spec[0])
        table = torch.zeros(B, R, 14, dtype=torch.float64)
        sums = torch.zeros(B, R, 14, dtype=torch.float64)
        for b in range(B):
            for r, (n, se, se2, sl1, d1, b1, b3) in enumerate(spec[b]):
                sums[b, r, [0, 1, 2, 3, 4, 6, 7]] = torch.tensor([n, se, se2, sl1, d1, b1, b3], dtype=torch.float64)
                if n:
                    table[b, r, [0, 1, 2, 3, 4, 6, 7]] = torch.tensor(
                        [n, se / n, (se2 / n) ** 0.5, sl1 / n, d1 / n, b1 / n, b3 / n], dtype=torch.float64)
        return losses.SequenceMetrics(table=table, sums=sums, loss=torch.tensor(loss, dtype=torch.float64),
                                      thresholds=thr, weights=w)

    acc = losses.SequenceAccumulator()
    acc.update(m([[(10, 20.0, 90.0, 15.0, 2, 6, 2), (10, 10.0, 40.0, 6.0, 1, 3, 1)],
                  [(0, 0.0, 0.0, 0.0, 0, 0, 0), (0, 0.0, 0.0, 0.0, 0, 0, 0)]], [2.5, 0.0]))
    acc.update(m([[(30, 15.0, 30.0, 9.0, 0, 3, 0), (30, 6.0, 7.5, 3.0, 0, 0, 0)]], [0.5]))
    r = acc.result()
    assert r["n_pairs"] == 3 and r["rows"] == 2 and r["n_valid"] == [40, 40] and r["thresholds"] == [1.0, 3.0]
    assert r["loss"] == pytest.approx(1.0, rel=1e-15)
    assert r["per_pair"]["epe"] == pytest.approx([(2.0 + 0 + 0.5) / 3, (1.0 + 0 + 0.2) / 3], rel=1e-15)
    assert r["per_pair"]["rmse"] == pytest.approx([(3.0 + 0 + 1.0) / 3, (2.0 + 0 + 0.5) / 3], rel=1e-15)
    assert r["per_pair"]["smooth_l1"] == pytest.approx([(1.5 + 0 + 0.3) / 3, (0.6 + 0 + 0.1) / 3], rel=1e-15)
    assert r["per_pair"]["bad_1"] == pytest.approx([(0.6 + 0 + 0.1) / 3, (0.3 + 0 + 0) / 3], rel=1e-15)
    assert r["pooled"]["epe"] == pytest.approx([35.0 / 40, 16.0 / 40], rel=1e-15)
    assert r["pooled"]["rmse"] == pytest.approx([(120.0 / 40) ** 0.5, (47.5 / 40) ** 0.5], rel=1e-15)
    assert r["pooled"]["d1_all"] == pytest.approx([2 / 40, 1 / 40], rel=1e-15)
    assert r["pooled"]["bad_3"] == pytest.approx([2 / 40, 1 / 40], rel=1e-15)
    with pytest.raises(ValueError, match="thresholds"):
        acc.update(losses.SequenceMetrics(table=torch.zeros(1, 2, 14, dtype=torch.float64),
                                          sums=torch.zeros(1, 2, 14, dtype=torch.float64),
                                          loss=torch.zeros(1, dtype=torch.float64), thresholds=(2.0,), weights=w))
    with pytest.raises(RuntimeError, match="no update"):
        losses.SequenceAccumulator().result()


def test_abi_rejects_bad_args_without_gpu():
    from foundationstereo_amd import _lib
    lib = _lib.load()
    P = 16                                                            # a non-null, aligned stand-in pointer
    thr = (ctypes.c_float * 3)(1.0, 3.0, 5.0)

    def call(R=2, rows=(P, P), bs=(16, 16), rs=(4, 4), hs=(4, 4), ws=(4, 4), gt=P, gt_u8=None, mask=None, thresholds=thr,
             K=3, gt_scale=1000.0, beta=1.0, partials=P, sums=P, table=P, loss=P, B=1, H=4, W=4, maxd=(192.0, 192.0)):
        n = len(rows)
        parr, _keep = _lib.ptr_array(list(rows))
        return lib.fsmi_seq_metrics(parr, (ctypes.c_longlong * n)(*bs), (ctypes.c_longlong * n)(*rs),
                                    (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws), (ctypes.c_float * n)(*([1.0] * n)),
                                    (ctypes.c_float * n)(*maxd), (ctypes.c_double * n)(*([1.0] * n)), bytes(n), R, gt,
                                    gt_u8, mask, thresholds, K, gt_scale, beta, partials, sums, table, loss, B, H, W, None)

    for kw in (dict(R=0), dict(R=65), dict(K=9), dict(K=-1), dict(K=3, thresholds=None), dict(hs=(4, 0)),
               dict(ws=(0, 4)), dict(rs=(4, 3)), dict(rows=(P, None)), dict(rows=(P, 18)), dict(gt=None),
               dict(gt=P, gt_u8=P), dict(gt=None, gt_u8=P, gt_scale=0.0), dict(partials=None), dict(sums=None),
               dict(table=None), dict(loss=None), dict(B=0), dict(H=0), dict(W=-1), dict(beta=-1.0),
               dict(maxd=(192.0, float("nan"))), dict(bs=(16, -16))):
        assert call(**kw) == 1001, kw
        assert b"fsmi_seq_metrics" in lib.fsmi_last_error()


def test_blocks_are_a_function_of_the_arguments():
    from foundationstereo_amd import _lib, ops
    lib = _lib.load()
    for H, W in ((1, 1), (3, 5), (37, 61), (480, 640), (1024, 1536), (97, 101)):
        for R in (1, 6, 33, 64):
            n = lib.fsmi_seq_metrics_blocks(H, W, R)
            assert n >= 1 and n == lib.fsmi_seq_metrics_blocks(W, H, R) == ops.seq_metrics_blocks(H, W, R)
    assert lib.fsmi_seq_metrics_blocks(3, 5, 1) == 1 and lib.fsmi_seq_metrics_blocks(97, 101, 6) >= 3
    assert lib.fsmi_seq_metrics_blocks(0, 5, 1) >= 1
    assert (ops.SEQ_NACC, ops.SEQ_MAX_ROWS) == (14, 64)
