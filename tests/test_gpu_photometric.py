"""The photometric consistency stage on the device against tests/photometric_oracle.py.

warped, the l1 map, the counts and every n_r are the oracle's (float32, the header's order) bit for bit.
So is the dssim map: on MI355X the device's IEEE divisions round as numpy's do, so the test asserts the
bits of oracle32 and, as the weaker statement that does not lean on that, the distance to oracle64
within DSSIM_TOL = 4 x the measured max |oracle32 - oracle64| on these same inputs
(tests/photometric_oracle.py records both; measured on the device: at most 1.27e-07).  The means are held to fp64 sums of oracle32's
per-pixel values at 1e-10 relative: a fixed-order fp64 sum of at most 10^4 non-negative terms is good to
about n * 2^-53 ~ 1e-12.  A (1,3,3) map has no SSIM pixel (column 0 is never sampled): that case checks
the zero means.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import photometric_oracle as po

pytestmark = pytest.mark.gpu

OFFSETS = (-2.0, -1.0, 0.0, 1.0, 2.0)
FRACTIONAL = (-0.5, 0.5)
REL = 1e-10


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_CASES = {}


def _case(shape, C, fmt, masked=False, offsets=OFFSETS):
    """Inputs and both oracles' answers, computed once per case and left unchanged."""
    key = (shape, C, fmt, masked, offsets)
    if key not in _CASES:
        d, left, right, mask = po.gpu_fuzz(shape, C, fmt)
        m = mask if masked else None
        _CASES[key] = (d, left, right, m, po.oracle32(d, left, right, m, offsets), po.oracle64(d, left, right, m, offsets))
    return _CASES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    print(f"{what}: max rel err {float((err / np.maximum(np.abs(want), 1e-300)).max()) if err.size else 0.0:.3e}")
    assert (err <= REL * np.abs(want)).all(), (what, got, want)


def _assert_matches(got, o32, o64, R, maps=True, what=""):
    table, sums, warped, l1, dssim = got
    table, sums = table.cpu().numpy(), sums.cpu().numpy()
    nf = po.NFIXED
    assert np.array_equal(table[:, :4], o32["table"][:, :4]) and np.array_equal(sums[:, :4], o32["sums"][:, :4])
    assert np.array_equal(table[:, nf::2], o32["table"][:, nf::2]) and table.shape == (len(table), nf + 2 * R)
    assert not np.isnan(table).any() and not np.isnan(sums).any()
    _close(table[:, 4:nf], o32["table"][:, 4:nf], what + " means")
    _close(table[:, nf + 1::2], o32["table"][:, nf + 1::2], what + " row means")
    _close(sums[:, 4:], o32["sums"][:, 4:], what + " sums")
    if not maps:
        return
    assert np.array_equal(_bits(warped.cpu().numpy()), _bits(o32["warped"]))
    assert np.array_equal(_bits(l1.cpu().numpy()), _bits(o32["l1"]))
    ds, has = dssim.cpu().numpy(), o32["has_ssim"]
    assert np.array_equal(np.isposinf(ds), ~has)
    if has.any():
        e64 = float(np.abs(ds[has].astype(np.float64) - o64["dssim"][has]).max())
        print(f"{what} dssim: max |device - oracle64| {e64:.3e} (allowed {po.DSSIM_TOL:.3e}); bit-equal to oracle32: "
              f"{np.array_equal(_bits(ds), _bits(o32['dssim']))}")
        assert e64 <= po.DSSIM_TOL
    assert np.array_equal(_bits(ds), _bits(o32["dssim"]))


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@pytest.mark.parametrize("shape,C,fmt", po.GPU_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fuzz_matches_the_oracle(shape, C, fmt):
    dev = _gpu()
    from foundationstereo_amd import ops
    for masked in (False, True):
        d, left, right, mask, o32, o64 = _case(shape, C, fmt, masked)
        td, tl, tr, tm = _dev(dev, d, left, right, mask)
        got = ops.photo_consistency(td, tl, tr, tm, OFFSETS, want_warped=True)
        _assert_matches(got, o32, o64, len(OFFSETS), what=f"{shape} C={C} {fmt} mask={masked}")
    if shape[1] < 3 or shape[2] < 5:
        assert int(got[0][:, po.N_SSIM].sum()) == 0 and float(got[0][:, po.DSSIM_MEAN].abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_strided_views_of_a_padded_batch(shape):
    """The unpadded crop of a (B,2,3,Hp,Wp) batch with a left pad of 1: row bases are not 16-byte aligned."""
    dev = _gpu()
    from foundationstereo_amd import ops
    B, H, W = shape
    d, left, right, mask, o32, o64 = _case(shape, 3, "f32", True)
    pt, pb, pl, pr = 2, 1, 1, 2
    batch = torch.full((B, 2, 3, H + pt + pb, W + pl + pr), -7.0, device=dev)
    batch[:, 0, :, pt:pt + H, pl:pl + W], batch[:, 1, :, pt:pt + H, pl:pl + W] = _dev(dev, left, right)
    dpad = torch.full((B, 1, H + pt + pb, W + pl + pr), float("nan"), device=dev)
    dpad[:, 0, pt:pt + H, pl:pl + W] = _dev(dev, d)[0]
    lv, rv, dv = batch[:, 0, :, pt:pt + H, pl:pl + W], batch[:, 1, :, pt:pt + H, pl:pl + W], dpad[:, :, pt:pt + H, pl:pl + W]
    assert not lv.is_contiguous() and lv.data_ptr() % 16 != 0 and lv.untyped_storage().data_ptr() == batch.untyped_storage().data_ptr()
    got = ops.photo_consistency(dv, lv, rv, _dev(dev, mask)[0], OFFSETS, want_warped=True)
    _assert_matches(got, o32, o64, len(OFFSETS), what=f"view {shape}")
    assert float(batch[:, :, :, 0].min()) == -7.0 and float(batch[:, :, :, :, 0].min()) == -7.0       # inputs untouched


@pytest.mark.parametrize("shape,C,fmt", [((2, 33, 65), 3, "u8"), ((1, 70, 131), 1, "f32")], ids=["2x33x65-u8", "1x70x131-f32"])
def test_mask_changes_the_scores_only(shape, C, fmt):
    dev = _gpu()
    from foundationstereo_amd import ops
    d, left, right, mask, o32, _ = _case(shape, C, fmt, True)
    plain32 = _case(shape, C, fmt, False)[4]
    td, tl, tr, tm = _dev(dev, d, left, right, mask)
    plain = ops.photo_consistency(td, tl, tr, None, OFFSETS, want_warped=True)
    masked = ops.photo_consistency(td, tl, tr, tm.bool(), OFFSETS, want_warped=True)
    assert torch.equal(plain[2].view(torch.int32), masked[2].view(torch.int32))                # warped untouched
    assert np.array_equal(masked[0][:, 0].cpu().numpy(), o32["table"][:, 0])
    assert (o32["table"][:, 0] < plain32["table"][:, 0]).all() and np.array_equal(plain[0][:, 0].cpu().numpy(), plain32["table"][:, 0])
    _close(masked[0][:, 4:8].cpu().numpy(), o32["table"][:, 4:8], "masked means")
    # nothing scored: zero means, no NaN; invalid and out-of-view counts do not depend on the mask
    none = ops.photo_consistency(td, tl, tr, torch.zeros_like(tm), OFFSETS, want_warped=True)
    t = none[0].cpu().numpy()
    assert not np.isnan(t).any() and not t[:, [0, 1, 4, 5, 6, 7]].any() and not t[:, 8:].any()
    assert np.array_equal(t[:, 2:4], o32["table"][:, 2:4])
    assert torch.isposinf(none[3]).all() and torch.isposinf(none[4]).all()
    assert torch.equal(none[2].view(torch.int32), plain[2].view(torch.int32))


@pytest.mark.parametrize("shape,C,fmt", [((2, 33, 65), 3, "f32"), ((1, 9, 17), 1, "u8")], ids=["2x33x65-f32", "1x9x17-u8"])
def test_fractional_row_offsets(shape, C, fmt):
    dev = _gpu()
    from foundationstereo_amd import ops
    d, left, right, mask, o32, o64 = _case(shape, C, fmt, True, FRACTIONAL)
    got = ops.photo_consistency(*_dev(dev, d, left, right, mask), FRACTIONAL, want_warped=True)
    _assert_matches(got, o32, o64, len(FRACTIONAL), what=f"fractional {shape}")
    assert (o32["table"][:, po.NFIXED::2] < o32["table"][:, :1]).all()            # the offsets drop the edge rows


def test_row_probe_on_the_shift_scene():
    dev = _gpu()
    from foundationstereo_amd import photometric
    disp, left, right = po.shift_scene(20, 40, 3, 1)
    td, tl, tr = _dev(dev, disp, left, right)
    p = photometric.row_probe(td, tl, tr)
    assert p.offsets.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0] and p.l1.shape == (1, 5)
    assert float(p.l1[0, 3]) == 0.0 and (p.l1[0, [0, 1, 2, 4]] > 0).all()
    assert 0.5 < float(p.offset[0]) < 1.5
    want = po.oracle32(disp, left, right, None, OFFSETS)["table"]
    assert np.array_equal(p.n.cpu().numpy(), want[:, po.NFIXED::2])
    _close(p.l1.cpu().numpy(), want[:, po.NFIXED + 1::2], "probe means")
    # the minimum at an end: the shift is outside the probed range
    end = photometric.row_probe(td, tl, tr, max_offset=1.0)
    assert end.offsets.tolist() == [-1.0, 0.0, 1.0] and float(end.l1[0, 2]) == 0.0 and torch.isnan(end.offset).all()
    # half-row steps bracket it again; planar fp32 views give what uint8 gives
    fl, fr_ = tl.permute(0, 3, 1, 2).float(), tr.permute(0, 3, 1, 2).float()
    half = photometric.row_probe(td[0], fl[0], fr_[0], max_offset=1.5, step=0.5)
    assert half.offsets.tolist() == [-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5] and float(half.l1[0, 5]) == 0.0
    assert 0.75 < float(half.offset[0]) < 1.25
    assert torch.equal(photometric.row_probe(td, fl, fr_).l1, p.l1)


def test_consistency_and_warp_right_front_ends():
    dev = _gpu()
    from foundationstereo_amd import photometric
    shape = (2, 33, 65)
    d, left, right, mask, o32, o64 = _case(shape, 3, "u8", True)
    td, tl, tr, tm = _dev(dev, d, left, right, mask)
    p = photometric.consistency(td[:, None], tl, tr, tm[:, None], row_offsets=OFFSETS, want_warped=True)
    _assert_matches((p.table, p.sums, p.warped, p.l1, p.dssim), o32, o64, len(OFFSETS), what="consistency")
    assert torch.equal(p.l1_mean, p.table[:, 4]) and torch.equal(p.photometric, p.table[:, 7])
    assert torch.equal(p.row_l1, p.table[:, 9::2]) and p.row_l1.shape == (2, 5) and p.offsets == OFFSETS
    assert torch.equal(p.n_scored, p.table[:, 0]) and torch.equal(p.n_ssim, p.table[:, 1])
    w = photometric.warp_right(td, tr)
    assert w.shape == (2, 3, 33, 65) and np.array_equal(_bits(w.cpu().numpy()), _bits(o32["warped"]))
    one = photometric.consistency(td[1], tl[1], tr[1], tm[1], want_maps=False)
    assert one.l1 is None and one.dssim is None and one.warped is None
    assert torch.equal(one.table[0], p.table[1, :8])
    with pytest.raises(RuntimeError, match="channels"):
        photometric.consistency(td, tl, tr[..., :1])
    with pytest.raises(RuntimeError, match="uint8"):
        photometric.consistency(td, tl.float().permute(0, 3, 1, 2), tr)


def test_equal_inputs_give_equal_bits_eager_graph_and_side_stream():
    dev = _gpu()
    from foundationstereo_amd import ops
    d, left, right, mask, *_ = _case((2, 33, 65), 3, "f32", True)
    td, tl, tr, tm = _dev(dev, d, left, right, mask)

    def run(dd):
        return ops.photo_consistency(dd, tl, tr, tm, OFFSETS, want_warped=True)

    def same(a, b):
        return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
    first, second = run(td), run(td)
    assert same(first, second)
    torch.cuda.synchronize()
    sd = torch.zeros_like(td)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = run(sd)
    torch.cuda.current_stream().wait_stream(side)
    sd.copy_(td)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, first)
    other = torch.cuda.Stream()
    other.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(other):
        third = run(td)
    other.synchronize()
    assert same(third, first)


def test_photo_consistency_does_not_synchronise():
    dev = _gpu()
    from foundationstereo_amd import ops
    d, left, right, mask, o32, o64 = _case((1, 9, 17), 3, "u8", True)
    args = _dev(dev, d, left, right, mask)
    ops.photo_consistency(*args, OFFSETS)                                  # library load, first launch
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.photo_consistency(*args, OFFSETS, want_warped=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _assert_matches(got, o32, o64, len(OFFSETS), what="no sync")


def test_maps_not_asked_for_cost_nothing_and_change_nothing():
    dev = _gpu()
    from foundationstereo_amd import ops
    d, left, right, mask, *_ = _case((1, 70, 131), 3, "u8", True)
    args = _dev(dev, d, left, right, mask)
    full = ops.photo_consistency(*args, OFFSETS, want_warped=True)
    bare = ops.photo_consistency(*args, OFFSETS, want_warped=False, want_l1=False, want_dssim=False)
    assert bare[2] is None and bare[3] is None and bare[4] is None
    assert torch.equal(bare[0].view(torch.int64), full[0].view(torch.int64))
    assert torch.equal(bare[1].view(torch.int64), full[1].view(torch.int64))
    # without the SSIM columns the rest of the table keeps its bits
    nossim = ops.photo_consistency(*args, OFFSETS, want_dssim=False, ssim=False)
    keep = [0, 2, 3, 4, 5] + list(range(8, 18))
    assert torch.equal(nossim[0][:, keep].view(torch.int64), full[0][:, keep].view(torch.int64))
    assert not nossim[0][:, [1, 6, 7]].any() and torch.equal(nossim[3].view(torch.int32), full[3].view(torch.int32))


def test_torch_operator_equals_ctypes():
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    for C, fmt in ((3, "f32"), (1, "u8")):
        d, left, right, mask, *_ = _case((2, 33, 65), C, fmt, True)
        td, tl, tr, tm = _dev(dev, d, left, right, mask)
        a = torch.ops.fsmi.photo_consistency(td, tl, tr, tm, list(OFFSETS), 0.7, True, True, True)
        b = ops.photo_consistency(td, tl, tr, tm, OFFSETS, 0.7, True, True, True)
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        a = torch.ops.fsmi.photo_consistency(td, tl, tr)
        b = ops.photo_consistency(td, tl, tr)
        assert a[2].numel() == 0 and b[2] is None and a[0].shape == (2, 8)
        for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3], b[3]), (a[4], b[4])):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        a = torch.ops.fsmi.photo_consistency(td, tl, tr, None, [], 0.85, False, False, False)
        assert a[2].numel() == a[3].numel() == a[4].numel() == 0 and torch.equal(a[0], b[0])
    with pytest.raises(RuntimeError, match="row offsets"):
        torch.ops.fsmi.photo_consistency(td, tl, tr, None, [0.0] * 9)


# ------------------------------------------------------------------ where it plugs in

H, W, MAX_DISP, ITERS = 64, 96, 32, 4


def _pair_files(tmp_path):
    rng = np.random.default_rng(50)
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = np.roll(left, -4, axis=1)                                     # left[v][u] == right[v][u - 4]
    np.save(tmp_path / "L.npy", left)
    np.save(tmp_path / "R.npy", right)
    (tmp_path / "K.txt").write_text("80.0 0.0 47.5 0.0 80.0 31.5 0.0 0.0 1.0\n0.1\n")
    return ["--synthetic", "--max_disp", str(MAX_DISP), "--left_file", str(tmp_path / "L.npy"), "--right_file",
            str(tmp_path / "R.npy"), "--valid_iters", str(ITERS)]


def test_demo_main_with_photo_check(tmp_path, capsys):
    _gpu()
    from foundationstereo_amd import demo
    common = _pair_files(tmp_path) + ["--intrinsic_file", str(tmp_path / "K.txt"), "--z_far", "20.0", "--denoise_radius",
                                      "0.4", "--denoise_nb_points", "10"]
    plain = demo.main(common + ["--out_dir", str(tmp_path / "plain")])
    new_keys = {"photometric", "row_offset", "warped_png", "photometric_png"}
    assert not new_keys & set(plain)
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(["K.txt", "left.npy", "right.npy", "vis.png", "cloud.ply", "depth_meter.npy",
                                                            "cloud_denoise.ply"])
    res = demo.main(common + ["--out_dir", str(tmp_path / "photo"), "--photo_check", "1"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and set(res) == set(plain) | new_keys
    assert {k: v for k, v in res.items() if k not in new_keys and k != "out_dir" and not str(v).startswith(str(tmp_path))} == \
           {k: v for k, v in plain.items() if k != "out_dir" and not str(v).startswith(str(tmp_path))}
    ph = res["photometric"]
    assert set(ph) == {"l1_mean", "l1_rms", "dssim_mean", "photometric", "n_scored", "n_ssim"}
    assert 0 <= ph["n_ssim"] <= ph["n_scored"] <= H * W and ph["l1_mean"] >= 0 and 0 <= ph["dssim_mean"] <= 1
    assert ph["l1_rms"] >= ph["l1_mean"] and 0 <= ph["photometric"] <= 1
    assert res["row_offset"] is None or -2.0 <= res["row_offset"] <= 2.0
    import struct
    for name in ("warped.png", "photometric.png"):
        raw = open(tmp_path / "photo" / name, "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (W, H)
    assert sorted(os.listdir(tmp_path / "photo")) == sorted(os.listdir(tmp_path / "plain") + ["warped.png", "photometric.png"])


def test_evaluate_without_a_ground_truth(tmp_path, capsys):
    dev = _gpu()
    from foundationstereo_amd import evaluate
    common = _pair_files(tmp_path)
    res = evaluate.main(common + ["--photometric", "--row_probe", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and res["mode"] == "model" and res["image_size"] == [H, W] and "epe" not in res
    assert set(res["photometric"]) == {"l1_mean", "l1_rms", "dssim_mean", "photometric", "n_scored", "n_ssim"}
    assert res["row_probe"]["offsets"] == [-2, -1, 0, 1, 2] and len(res["row_probe"]["l1"]) == 5
    assert res["row_probe"]["offset"] is None or -2.0 <= res["row_probe"]["offset"] <= 2.0
    # a stored disparity that is the scene's own: right is left moved 4 columns, so the residual vanishes
    np.save(tmp_path / "pred.npy", np.full((H, W), 4.0, np.float32))
    files = common[3:7]
    st = evaluate.main(["--pred_file", str(tmp_path / "pred.npy"), "--photometric", "--row_probe", "1"] + files)
    assert st["mode"] == "pred_file" and st["photometric"]["n_scored"] == H * (W - 4)
    assert st["photometric"]["l1_mean"] == 0.0 and st["photometric"]["dssim_mean"] == 0.0 and st["photometric"]["photometric"] == 0.0
    assert st["photometric"]["n_ssim"] == (H - 2) * (W - 6)
    assert st["row_probe"]["l1"][1] == 0.0 and st["row_probe"]["offset"] is not None and abs(st["row_probe"]["offset"]) < 0.5
    # with a ground truth the line keeps its fields and gains the two objects; --noc masks both
    np.save(tmp_path / "gt.npy", np.full((H, W), 4.0, np.float32))
    flags = ["--pred_file", str(tmp_path / "pred.npy"), "--gt_file", str(tmp_path / "gt.npy")] + files
    plain = evaluate.main(flags + ["--noc"])
    both = evaluate.main(flags + ["--photometric", "--row_probe", "1", "--noc"])
    assert "photometric" not in plain and "row_probe" not in plain
    assert {k: v for k, v in both.items() if k not in ("photometric", "row_probe")} == plain
    assert both["photometric"]["n_scored"] == H * (W - 4) and both["mask"] == "noc"
