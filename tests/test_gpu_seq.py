"""The sequence metrics on the GPU (csrc/seq_metrics.hip through ops, losses and torch.ops.fsmi) against
tests/seq_oracle.py.  Counts, rates and the bilinear samples are exact; the fp64 sums differ from the
oracle's only in the order of the additions of non-negative terms, which bounds them:
  sum e, sum e^2, sum sl1, epe, rmse, smooth_l1   (N + 4) * 2^-52 relative, N = valid pixels (N - 1 adds,
                                                  the division and the square root)
  loss                                            (N + 4 + 2 R) * 2^-52 relative: R products and R adds of
                                                  non-negative terms on top (the weights here are >= 0)
"""
import os

import numpy as np
import pytest
import torch

from tests import seq_oracle as so

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
EPS32 = 2.0 ** -24
# metrics' shapes: fewer pixels than a block; pair bases off the 16-byte grid; aligned; >= 3 blocks per
# pair with a ragged last one.  With each, the size of its resized row.
SHAPES = {(1, 3, 5): (1, 1), (3, 37, 61): (10, 16), (2, 32, 64): (8, 16), (2, 97, 101): (25, 26)}
THR = (1.0, 3.0, 5.0)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _gt(shape, seed, holes=0.1):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 60.0, shape).astype(np.float32)
    gt[rng.random(shape) < holes] = 0.0
    return gt


def _rows(gt, R, small, seed):
    """R maps: row 0 at the size ``small`` (to be resized), the others the ground truth + noise that shrinks"""
    rng = np.random.default_rng(seed)
    B = gt.shape[0]
    rows = [rng.uniform(0.2, 15.0, (B,) + small).astype(np.float32)]
    for k in range(1, R):
        noise = rng.standard_normal(gt.shape) * np.where(rng.random(gt.shape) < 0.25, 6.0, 0.6) * (0.5 + 3.0 / k)
        rows.append((gt + noise).astype(np.float32))
    return rows


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(rows, gt, mask=None, **kw):
    dev = _gpu()
    from foundationstereo_amd import ops
    return ops.seq_metrics([_dev(r, dev) for r in rows], _dev(gt, dev), _dev(mask, dev), **kw)


def _close(got, want, rel):
    """|got - want| <= rel * |want| elementwise; NaN and inf must coincide"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = np.broadcast_to(np.asarray(rel, np.float64), want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (got, want)
    assert np.all(np.abs(got[fin] - want[fin]) <= rel[fin] * np.abs(want[fin])), (got, want, rel)


def _check(rows, gt, mask, got, **kw):
    """Every figure of (table, sums, loss) (device tensors) against the oracle on the numpy inputs."""
    wt, ws, wl = so.seq_metrics(rows, gt, mask, **kw)
    table, sums, loss = (x.cpu().numpy() for x in got)
    B, R = gt.shape[0], len(rows)
    assert table.shape == sums.shape == (B, R, 14) and loss.shape == (B,) and table.dtype == loss.dtype == np.float64
    assert np.array_equal(sums[..., so.COUNTS], ws[..., so.COUNTS])
    assert np.array_equal(table[..., [0, 5]], wt[..., [0, 5]])
    assert np.array_equal(table[..., so.RATES], wt[..., so.RATES])         # the same fp64 division
    relN = (ws[..., 0] + 4) * EPS
    for col in (1, 2, 3):
        _close(sums[..., col], ws[..., col], relN)
        _close(table[..., col], wt[..., col], relN)
    _close(loss, wl, (ws[..., 0].max(axis=1) + 4 + 2 * R) * EPS)
    return wt, ws, wl


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("R", [1, 6, 33])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_and_row_counts_against_oracle(shape, R, with_mask):
    """R = 33 crosses the 32-rows-per-launch split and leaves a ragged group of 4; row 0 is resized
    ((8,16) -> (32,64) is an exact x4 with the factor 4), some rows clamp at 50, some not at all."""
    _gpu()
    from foundationstereo_amd import ops
    B, H, W = shape
    nb = ops.seq_metrics_blocks(H, W, R)
    if shape == (1, 3, 5):
        assert nb == 1
    if shape == (2, 97, 101):
        assert nb >= 3 and (H * W) % 1024 != 0
    gt = _gt(shape, 7 + H)
    rows = _rows(gt, R, SHAPES[shape], 3 + R)
    mask = (np.random.default_rng(5).random(shape) < 0.7) if with_mask else None   # valid where gt == 0 too
    kw = dict(thresholds=THR, max_disparity=[192.0 if r == 0 else (50.0 if r % 3 == 1 else np.inf) for r in range(R)],
              beta=1.0, weights=so.sequence_weights(R - 1, 0.9), smooth_rows=(0,),
              muls=[4.0 if shape == (2, 32, 64) else 1.0] + [1.0] * (R - 1))
    wt, ws, wl = _check(rows, gt, mask, _run(rows, gt, mask, **kw), **kw)
    assert (ws[..., 0] > 0).all() and (wl > 0).all()
    if H * W > 1000 and R > 1:                                              # the data exercises every counter
        assert (ws[:, 1, 4] > 0).all() and (ws[:, 1, 6] > ws[:, 1, 8]).all() and (ws[:, 1, 8] > 0).all()
        assert (wt[:, 1, so.EPE] > wt[:, R - 1, so.EPE]).all()              # the noise shrinks along the sequence


@pytest.mark.parametrize("small,full,mul", [((10, 16), (37, 61), 1.0), ((8, 16), (32, 64), 4.0), ((1, 1), (3, 5), 1.0),
                                            ((25, 26), (97, 101), 1.0)])
def test_every_bilinear_sample_is_exact(small, full, mul):
    """One pair per pixel: its mask holds that pixel alone, the ground truth is 0 and beta is 0, so
    sum e of the pair IS the sample (taps > 0).  The small map is one array expanded over the pairs
    (batch stride 0).  (25,26) -> (97,101) probes every fourth pixel."""
    dev = _gpu()
    from foundationstereo_amd import ops
    H, W = full
    small_map = np.random.default_rng(small[0]).uniform(0.5, 50.0, small).astype(np.float32)
    want = so.row_values(small_map[None], H, W, mul)[0].reshape(-1)
    pix = np.arange(H * W)[::4 if H * W > 5000 else 1]
    B = len(pix)
    mask = np.zeros((B, H * W), bool)
    mask[np.arange(B), pix] = True
    row = _dev(small_map, dev)[None].expand(B, *small)
    assert row.stride(0) == 0
    table, sums, loss = ops.seq_metrics([row], torch.zeros((B, H, W), device=dev), _dev(mask.reshape(B, H, W), dev),
                                        THR, beta=0.0, muls=[mul])
    sums = sums.cpu().numpy()
    assert (sums[:, 0, 0] == 1).all()
    assert np.array_equal(sums[:, 0, 1], want[pix].astype(np.float64))
    assert np.array_equal(sums[:, 0, 3], sums[:, 0, 1]) and np.array_equal(loss.cpu().numpy(), sums[:, 0, 1])


def test_views_give_the_bits_of_their_contiguous_clones():
    """Rows taken as padded[:, 0, 3:-2, 5:-1] (what padder.unpad hands out: row stride != w, base 4-byte but
    not 16-byte aligned) against their clones, and a batch-strided [:, 0] of a (B,2,h,w) tensor."""
    dev = _gpu()
    from foundationstereo_amd import ops
    shape = (2, 37, 61)
    gt = _gt(shape, 31)
    rows = _rows(gt, 6, (10, 16), 32)
    tg = _dev(gt, dev)
    views = []
    for k, r in enumerate(rows):
        h, w = r.shape[1:]
        big = torch.full((2, 2, h + 5, w + 6), float("nan"), device=dev)
        big[:, 0, 3:-2, 5:-1] = _dev(r, dev)
        v = big[:, 0, 3:-2, 5:-1]
        assert not v.is_contiguous() and v.stride(1) == w + 6 and v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0
        views.append(v)
    kw = dict(max_disparity=192.0, weights=so.sequence_weights(5, 0.9), smooth_rows=(0,))
    a = ops.seq_metrics(views, tg, None, THR, **kw)
    b = ops.seq_metrics([v.clone() for v in views], tg, None, THR, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _check(rows, gt, None, a, thresholds=THR, **kw)
    # an innermost stride of 2 is the one layout that is copied
    wide = torch.zeros((2, 37, 122), device=dev)
    wide[:, :, ::2] = views[1]
    c = ops.seq_metrics([views[0], wide[:, :, ::2]] + views[2:], tg, None, THR, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_allocates_the_outputs_and_the_workspace_only():
    """No copy of a view, no decoded ground truth, no resized map: the peak grows by the three outputs
    and the partial rows (each rounded up to the allocator's 512 bytes), far less than one map."""
    dev = _gpu()
    from foundationstereo_amd import ops
    shape = (2, 97, 101)
    gt = _gt(shape, 33)
    rows = _rows(gt, 6, (25, 26), 34)
    big = [torch.zeros((2, 1, 104, 110), device=dev) for _ in rows[1:]]
    for t, r in zip(big, rows[1:]):
        t[:, 0, 3:-4, 5:-4] = _dev(r, dev)
    views = [_dev(rows[0], dev)] + [t[:, 0, 3:-4, 5:-4] for t in big]
    tg = _dev(gt, dev)
    u8 = torch.zeros(shape + (3,), dtype=torch.uint8, device=dev)
    mask = tg > 0
    ops.seq_metrics(views, tg, mask)                                         # library load, first launches
    nb = ops.seq_metrics_blocks(97, 101, 6)

    def up(n):
        return (n + 511) // 512 * 512

    budget = up(2 * 6 * nb * 14 * 8) + 2 * up(2 * 6 * 14 * 8) + up(2 * 8)
    assert budget < 97 * 101 * 4
    for g in (tg, u8):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = ops.seq_metrics(views, g, mask, max_disparity=192.0)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - before <= budget
        assert torch.cuda.memory_allocated() - before <= budget - up(2 * 6 * nb * 14 * 8)
        del out


def test_clamp_and_nan_propagation():
    """Values above max_disparity and below 0 are clamped (torch.clamp keeps NaN); a NaN under a valid
    pixel reaches that row's sums and n_nonfinite and no other row; under an invalid pixel, nothing."""
    shape = (2, 10, 11)
    gt = _gt(shape, 35, holes=0.0)
    gt[0, 4, 4] = 0.0
    rows = _rows(gt, 4, (3, 4), 36)
    rows[1][0, 0, :3] = [250.0, -7.0, 1e9]
    rows[2][0, 4, 4] = np.nan            # under an invalid pixel
    rows[3][1, 2, 3] = np.nan            # under a valid one
    rows[3][1, 5, 5] = np.inf            # clamped to max_disparity: finite again
    kw = dict(thresholds=THR, max_disparity=64.0, weights=[1.0] * 4, smooth_rows=(0,))
    got = _run(rows, gt, None, **kw)
    wt, ws, wl = _check(rows, gt, None, got, **kw)
    t = got[0].cpu().numpy()
    assert np.isfinite(t[0]).all() and np.isfinite(t[1, :3]).all() and (t[:, :3, 5] == 0).all()
    assert np.isnan(t[1, 3, 1:4]).all() and t[1, 3, 5] == 1 and np.isfinite(t[1, 3, 6:9]).all()
    loss = got[2].cpu().numpy()
    assert np.isfinite(loss[0]) and np.isnan(loss[1])
    clean = [r.copy() for r in rows]
    clean[1][0, 0, :3] = [64.0, 0.0, 64.0]
    assert np.array_equal(so.seq_metrics(clean, gt, None, **kw)[1][0, 1], ws[0, 1])
    # without a clamp the inf stays: an infinite sum, counted
    kw["max_disparity"] = np.inf
    rows[3][1, 2, 3] = 1.0
    got = _run(rows, gt, None, **kw)
    _check(rows, gt, None, got, **kw)
    assert got[0][1, 3, 1].item() == np.inf and got[0][1, 3, 5].item() == 1 and got[1][0, 1, 1].item() > 1e9


def test_default_validity_and_empty_pair():
    shape = (3, 9, 13)
    gt = _gt(shape, 37, holes=0.0)
    gt[0, 0, :4] = [0.0, -2.0, np.inf, np.nan]
    rows = _rows(gt, 3, (2, 3), 38)
    got = _run(rows, gt, None, thresholds=THR)
    wt, ws, wl = _check(rows, gt, None, got, thresholds=THR)
    assert ws[:, 0, 0].tolist() == [9 * 13 - 4, 9 * 13, 9 * 13]
    mask = np.ones(shape, bool)
    mask[1] = False
    gt = np.nan_to_num(gt, nan=1.0, posinf=1.0)
    rows = _rows(gt, 3, (2, 3), 38)                                         # finite under the mask of ones
    got = _run(rows, gt, mask, thresholds=(1.0,), smooth_rows=(0,))
    _check(rows, gt, mask, got, thresholds=(1.0,), smooth_rows=(0,))
    assert not got[0][1].any() and got[2][1].item() == 0 and got[2][0].item() > 0
    assert not got[0][:, :, 7:].any()                                       # unused threshold slots are 0


def test_u8_ground_truth_equals_decode_then_float_path():
    dev = _gpu()
    from foundationstereo_amd import ops
    rng = np.random.default_rng(39)
    shape = (3, 37, 61)
    u8 = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    u8[..., 0] = 0
    u8[..., 1] //= 2
    u8[rng.random(shape) < 0.1] = 0
    tu8 = _dev(u8, dev)
    for scale in (1000.0, 250.0):
        dec = ops.gt_decode(tu8, scale)
        rows = [_dev(r, dev) for r in _rows(dec.cpu().numpy(), 6, (10, 16), 40)]
        a = ops.seq_metrics(rows, tu8, None, THR, 192.0, gt_scale=scale)
        b = ops.seq_metrics(rows, dec, None, THR, 192.0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    mask = _dev(rng.random(shape) < 0.5, dev)
    a = ops.seq_metrics(rows, tu8[:, :, :, :], mask, (2.0,), gt_scale=250.0)
    b = ops.seq_metrics(rows, dec, mask.to(torch.uint8), (2.0,))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_reproducible_and_capturable():
    """The same input gives the same bits twice, and once more from a captured graph replayed on it."""
    dev = _gpu()
    from foundationstereo_amd import ops
    gt = _gt((2, 97, 101), 41)
    rows = [_dev(r, dev) for r in _rows(gt, 33, (25, 26), 42)]
    tg = _dev(gt, dev)
    kw = dict(max_disparity=192.0, weights=so.sequence_weights(32, 0.9), smooth_rows=(0,))
    first = ops.seq_metrics(rows, tg, None, THR, **kw)
    second = ops.seq_metrics(rows, tg, None, THR, **kw)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    torch.cuda.synchronize()
    stand_in = [torch.zeros_like(r) for r in rows]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = ops.seq_metrics(stand_in, tg, None, THR, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for s, r in zip(stand_in, rows):
        s.copy_(r)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, first))


def test_does_not_synchronise():
    """sequence_metrics and SequenceAccumulator.update under torch's synchronisation check."""
    dev = _gpu()
    from foundationstereo_amd import losses
    gt = _gt((2, 37, 61), 43)
    rows = [_dev(r, dev) for r in _rows(gt, 6, (10, 16), 44)]
    tg = _dev(gt, dev)
    u8 = torch.zeros((2, 37, 61, 3), dtype=torch.uint8, device=dev)
    mask = tg > 0
    losses.sequence_metrics(rows[0], rows[1:], tg)                          # library load, first launches
    acc = losses.SequenceAccumulator()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = losses.sequence_metrics(rows[0][:, None], [r[:, None] for r in rows[1:]], tg[:, None], mask, init_scale=4.0)
        acc.update(m)
        acc.update(losses.sequence_metrics(rows[0], rows[1:], u8))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    r = acc.result()
    assert r["n_pairs"] == 4 and r["rows"] == 6 and len(r["per_pair"]["epe"]) == 6
    assert m.epe.shape == (2, 6) and m.bad.shape == (2, 6, 3) and m.d1_all.shape == m.rmse.shape == (2, 6)
    assert m.weights == tuple(so.sequence_weights(5, 0.9)) and m.loss.shape == (2,)


def test_rows_equal_the_single_map_stage():
    """Row r of seq_metrics against ops.disp_metrics on the same full-size map: counts bit for bit, sums
    within the summation bound (the two kernels add in different orders)."""
    dev = _gpu()
    from foundationstereo_amd import ops
    for shape in ((3, 37, 61), (2, 97, 101)):
        gt = _gt(shape, 45)
        rows = _rows(gt, 5, shape[1:], 46)
        tr, tg = [_dev(r, dev) for r in rows], _dev(gt, dev)
        table, sums, _ = ops.seq_metrics(tr, tg, None, THR)
        for r in range(5):
            t1, s1, _ = ops.disp_metrics(tr[r], tg, None, THR)
            assert torch.equal(sums[:, r][:, [0, 4, 5, 6, 7, 8]], s1[:, [0, 3, 4, 9, 10, 11]])
            assert torch.equal(table[:, r][:, [0, 4, 5, 6, 7, 8]], t1[:, [0, 3, 4, 9, 10, 11]])
            rel = 2 * (s1[:, 0].cpu().numpy() + 4) * EPS                    # each within (N + 4) eps of the exact sum
            _close(sums[:, r, 1:3].cpu().numpy(), s1[:, 1:3].cpu().numpy(), rel[:, None])
            _close(table[:, r, 1:3].cpu().numpy(), t1[:, 1:3].cpu().numpy(), rel[:, None])


def test_drop_ins_against_the_reference_golden():
    """foundation_stereo_loss and the single-map losses on device tensors against the reference's own
    outputs, within tests/test_seq_host.py's bounds (the reference sums in fp32)."""
    dev = _gpu()
    from foundationstereo_amd import losses
    g = so.load_golden(os.path.join(REPO, "tests", "golden", "seq_small.npz"))
    keys = g["keys"].tolist()
    gt, mask = _dev(g["gt"], dev), _dev(g["mask"], dev)
    preds = [_dev(p, dev) for p in g["preds"]]
    N = g["mask"].reshape(3, -1).sum(1)
    gap = so.resize_gap_bound(np.abs(g["init_small"]).max())
    for pi, (gamma, maxd) in enumerate(so.GOLDEN_PARAMS):
        wsum = sum(so.sequence_weights(5, gamma)[1:])
        for name in ("init_full", "init_small"):
            init = _dev(g[name], dev)
            e0 = np.abs(so.row_values(g[name], 37, 61, 1.0, maxd) - g["gt"])
            for b in range(3):
                loss, misc = losses.foundation_stereo_loss(init[b], [p[b] for p in preds], gt[b], mask[b], gamma=gamma,
                                                           max_disparity=maxd)
                ref = g[f"fsl_p{pi}_{name}_pair{b}"]
                assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
                assert sorted(misc) == keys and all(isinstance(v, float) for v in misc.values())
                if N[b] == 0:
                    assert float(loss) == 0.0 and not any(misc.values()) and not ref.any()
                    continue
                rel = (N[b] + 2) * EPS32
                slack = gap if name == "init_small" else 0.0
                assert abs(float(loss) - ref[0]) <= slack + rel * ref[0] + EPS32 * ref[0]
                for k, w in zip(keys, ref[1:]):
                    if k in ("d1_error_initial", "d3_error_initial"):
                        t = 3.0 if k.startswith("d1") else 1.0
                        M = int((np.abs(e0[b][g["mask"][b]] - t) <= slack).sum()) if slack else 0
                        bound = M / N[b] + EPS32 * w
                    elif k.startswith("d"):
                        bound = wsum * EPS32 + 8 * EPS * w                  # sum_k w_k * 2^-24 * rate_k, rate_k <= 1
                    else:
                        bound = (slack if k.endswith("initial") else 0.0) + rel * w
                    assert abs(misc[k] - w) <= bound, (pi, name, b, k, misc[k], w)
        last = preds[-1]
        for b in (0, 2):
            outs = [losses.disparity_l1_loss(last[b], gt[b], mask[b], max_disparity=maxd),
                    losses.disparity_smooth_l1_loss(last[b], gt[b], mask[b], beta=0.5, max_disparity=maxd),
                    losses.disparity_epe_loss(last[b], gt[b], mask[b], max_disparity=maxd),
                    losses.disparity_smooth_l1_loss(_dev(g["init_small"], dev)[b], gt[b], mask[b], max_disparity=maxd)]
            for i, (loss, misc) in enumerate(outs):
                want = g[f"single_p{pi}_pair{b}"][i]
                slack = gap if i == 3 else 0.0
                assert sorted(misc) == ["d1_error", "d3_error", "epe"] and loss.dtype == torch.float32 and loss.dim() == 0
                assert abs(float(loss) - want[0]) <= slack + ((N[b] + 2) * EPS32 + EPS32) * want[0]
                assert abs(misc["epe"] - want[1]) <= slack + (N[b] + 2) * EPS32 * want[1]
                if i < 3:
                    assert abs(misc["d1_error"] - want[2]) <= EPS32 * want[2]
                    assert abs(misc["d3_error"] - want[3]) <= EPS32 * want[3]
    # the batched call: the mean over pairs, the empty pair counting as zeros; init_scale is the opt-in
    loss, misc = losses.foundation_stereo_loss(_dev(g["init_full"], dev), preds, gt, mask)
    per = [g[f"fsl_p0_init_full_pair{b}"] for b in range(3)]
    assert abs(float(loss) - np.mean([p[0] for p in per])) <= (N.max() + 3) * EPS32 * float(loss)
    a = losses.sequence_metrics(_dev(g["init_small"], dev), preds, gt, mask, init_scale=4.0)
    _check([g["init_small"]] + g["preds"], g["gt"], g["mask"], (a.table, a.sums, a.loss), thresholds=THR,
           max_disparity=192.0, beta=1.0, weights=list(a.weights), smooth_rows=(0,), muls=[4.0] + [1.0] * 5)
    none = losses.sequence_metrics(None, preds, gt, mask)
    assert none.table.shape == (3, 5, 14) and torch.equal(none.table, a.table[:, 1:]) and not none.has_init


def test_torch_ops_match_ops():
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    gt = _gt((2, 37, 61), 47)
    rows = [_dev(r, dev) for r in _rows(gt, 6, (10, 16), 48)]
    tg = _dev(gt, dev)
    mask = tg > 1.0
    w = so.sequence_weights(5, 0.8)
    a = torch.ops.fsmi.seq_metrics(rows, tg, mask, [1.0, 2.0], 64.0, 0.5, w, [0], 1000.0)
    b = ops.seq_metrics(rows, tg, mask, (1.0, 2.0), 64.0, 0.5, w, (0,))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = torch.ops.fsmi.seq_metrics(rows, tg)
    b = ops.seq_metrics(rows, tg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    u8 = _dev(np.random.default_rng(49).integers(0, 256, (2, 37, 61, 3), dtype=np.uint8), dev)
    view = [r[:, 1:, 1:] if r.shape[1] == 37 else r for r in rows]
    a = torch.ops.fsmi.seq_metrics(view, u8[:, 1:, 1:].contiguous(), None, [1.0], None, 1.0, None, [], 500.0)
    b = ops.seq_metrics(view, u8[:, 1:, 1:].contiguous(), None, (1.0,), gt_scale=500.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_bad_inputs_raise():
    dev = _gpu()
    from foundationstereo_amd import losses, ops
    x = torch.ones(1, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.seq_metrics([x.cpu()], x)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.seq_metrics([x], x.cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.seq_metrics([x.clone().requires_grad_(True)], x)
    with pytest.raises(RuntimeError, match="inference-only"):
        losses.foundation_stereo_loss(x[0], [x[0].clone().requires_grad_(True)], x[0], x[0] > 0)
    with torch.no_grad():
        ops.seq_metrics([x.clone().requires_grad_(True)], x)                  # allowed without grad mode
    with pytest.raises(RuntimeError, match="rows"):
        ops.seq_metrics([x] * 65, x)
    with pytest.raises(RuntimeError, match="thresholds"):
        ops.seq_metrics([x], x, thresholds=range(9))
    with pytest.raises(RuntimeError, match="row 1 must be"):
        ops.seq_metrics([x, torch.ones(2, 4, 4, device=dev)], x)
    with pytest.raises(RuntimeError, match="mask"):
        ops.seq_metrics([x], x, mask=x)
    with pytest.raises(RuntimeError, match="weights"):
        ops.seq_metrics([x, x], x, weights=[1.0])
    with pytest.raises(RuntimeError, match="smooth row"):
        ops.seq_metrics([x], x, smooth_rows=(1,))
    with pytest.raises(RuntimeError, match="beta"):
        ops.seq_metrics([x], x, beta=-1.0)
    with pytest.raises(RuntimeError, match="gt_scale"):
        ops.seq_metrics([x], torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev), gt_scale=0.0)
    with pytest.raises(ValueError, match="must be"):
        losses.sequence_metrics(None, [torch.ones(2, 2, 4, 4, device=dev)], x)
