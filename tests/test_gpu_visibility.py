"""The visibility stage on the GPU (csrc/visibility.hip) against tests/visibility_oracle.py.

Every class is an exact function of the inputs (include/fsmi.h fixes the order of the fp32 operations
and the oracle repeats it), so every comparison here is equality: classes, counts and the bits of the
error map, NaN positions included.  No tolerance appears anywhere.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import visibility_oracle as vo

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1),        # smallest possible
          (1, 3, 5),        # fewer columns than a wave
          (3, 37, 61),      # odd W, B > 1: unaligned row bases; 8 rows per block, a last block of 5
          (2, 8, 257),      # one column past a 256-thread pass
          (2, 5, 160),      # several rows per block, fewer rows than a block takes
          (1, 2, 8192),     # the LDS cap
          (1100, 17, 5),    # more pairs than the grid takes blocks: a block loops over 3 row groups (8, 8, 1 rows)
          (500, 40, 5)]     # 4 blocks for a pair's 5 row groups: the first takes groups 0 and 4
MODES = [(True, False), (True, True), (False, True), (False, False)]      # (occlusion, disp_right given)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


_CASES = {}


def _case(shape, occlusion, with_right):
    """Inputs and the oracle's answer, computed once per (shape, mode) and left unchanged."""
    key = (shape, occlusion, with_right)
    if key not in _CASES:
        left, right = vo.fuzz_maps(shape, seed=1000 + SHAPES.index(shape), with_right=True)
        right = right if with_right else None
        tol, thr = 1.0, 1.0
        _CASES[key] = (left, right, tol, thr, vo.classify_oracle(left, right, occlusion, tol, thr))
    return _CASES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_equal(got, want, want_error):
    classes, counts, error = got
    ocls, ocounts, oerr = want
    assert classes.dtype == torch.uint8 and counts.dtype == torch.int64
    assert np.array_equal(classes.cpu().numpy(), ocls)
    assert np.array_equal(counts.cpu().numpy(), ocounts)
    if want_error:
        assert error.dtype == torch.float32 and error.shape == classes.shape
        e = error.cpu().numpy()
        assert np.array_equal(np.isnan(e), np.isnan(oerr))
        unseen = (ocls == vo.INVALID) | (ocls == vo.OUT_OF_VIEW)
        assert np.isnan(e[unseen]).all()
        # elsewhere e is NaN only where the right view's value is: never a VISIBLE pixel
        assert np.isin(ocls[np.isnan(e) & ~unseen], (vo.OCCLUDED, vo.MISMATCH)).all()
        assert np.array_equal(_bits(e)[~np.isnan(e)], _bits(oerr)[~np.isnan(oerr)])
    else:
        assert error is None


# ------------------------------------------------------------------ the analytic scene

def test_analytic_scene_occlusion_and_left_right_agree():
    dev = _gpu()
    from foundationstereo_amd import visibility
    left, right, occ, lr = vo.analytic_scene(H=2)
    d, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    v = visibility.classify(d)
    assert np.array_equal(v.classes.cpu().numpy(), occ) and v.error is None
    assert v.counts.tolist() == [[88, 0, 8, 32, 0]]                       # [44, 0, 4, 16, 0] per row
    assert v.fractions.dtype == torch.float64 and v.fractions.tolist() == [[88 / 128, 0, 8 / 128, 32 / 128, 0]]
    assert v.visible.dtype == torch.bool and np.array_equal(v.visible.cpu().numpy(), occ == 0)
    w = visibility.classify(d, r, occlusion=False, want_error=True)
    assert np.array_equal(w.classes.cpu().numpy(), lr) and w.counts.tolist() == [[88, 0, 8, 0, 32]]
    assert torch.equal(v.classes == visibility.OCCLUDED, w.classes == visibility.MISMATCH)
    assert (w.error[..., 14:30] == 16).all() and torch.isnan(w.error[..., :4]).all()
    both = visibility.classify(d, r)
    assert torch.equal(both.classes, v.classes)                           # occlusion takes precedence


# ------------------------------------------------------------------ fuzz against the oracle

@pytest.mark.parametrize("occlusion,with_right", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fuzz_matches_oracle_exactly(shape, occlusion, with_right):
    dev = _gpu()
    from foundationstereo_amd import visibility
    left, right, tol, thr, want = _case(shape, occlusion, with_right)
    if min(shape) > 1 and shape[2] >= 61:
        for k in ((1, 2) + ((3,) if occlusion else ()) + ((4,) if with_right else ())):
            assert want[1][:, k].all(), f"the fuzz input holds no pixel of class {k}"
        x = np.arange(shape[2], dtype=np.float32) - left
        inview = np.isfinite(left) & (left > 0) & (x >= 0)
        assert (x[inview] == np.floor(x[inview])).any() and (x[inview] != np.floor(x[inview])).any()     # t == 0 and t != 0
    d = torch.from_numpy(left).to(dev)
    r = torch.from_numpy(right).to(dev) if with_right else None
    for want_error in (False, True):
        if want_error and not with_right:
            with pytest.raises(ValueError, match="want_error"):           # there is no right view to differ from
                visibility.classify(d, None, occlusion=occlusion, want_error=True)
            continue
        v = visibility.classify(d, r, occlusion=occlusion, occlusion_tol=tol, lr_thresh=thr, want_error=want_error)
        _assert_equal((v.classes, v.counts, v.error), want, want_error)


def test_unaligned_input_bases():
    """Maps that start 4 and 12 bytes off the 16-byte grid: the front end makes them aligned."""
    dev = _gpu()
    from foundationstereo_amd import visibility
    left, right, tol, thr, want = _case((3, 37, 61), True, True)
    n = left.size
    for off in (1, 3):
        d = torch.zeros(n + 4, device=dev)[off:off + n].copy_(torch.from_numpy(left).reshape(-1).to(dev)).view(left.shape)
        r = torch.zeros(n + 4, device=dev)[off:off + n].copy_(torch.from_numpy(right).reshape(-1).to(dev)).view(left.shape)
        assert d.data_ptr() % 16 == 4 * off
        v = visibility.classify(d, r, want_error=True)
        _assert_equal((v.classes, v.counts, v.error), want, True)


# ------------------------------------------------------------------ ties on a z-buffer column

def test_ties_on_one_column():
    """At one disparity a row's pixels land on distinct columns (c grows by one per column), so "equal d
    on one column" is only ever the pixel itself.  The two halves that can occur: equal disparities
    along the row occlude nobody, and a row whose pixels ALL land on one column (d = u) is hidden by its
    largest disparity alone, up to the tolerance; 1023 lanes hit one LDS word."""
    dev = _gpu()
    from foundationstereo_amd import visibility
    W = 1024
    flat = torch.full((1, 1, W), 7.0, device=dev)
    v = visibility.classify(flat, occlusion_tol=0.0)
    assert v.counts.tolist() == [[W - 7, 0, 7, 0, 0]]
    flat[0, 0, 500] = 9.0                                                 # lands on 491, on top of column 498
    v = visibility.classify(flat, occlusion_tol=0.0)
    assert v.counts.tolist() == [[W - 8, 0, 7, 1, 0]] and int(v.classes[0, 0, 498]) == visibility.OCCLUDED
    ramp = torch.arange(W, dtype=torch.float32, device=dev).view(1, 1, W)     # xr = 0 for every column
    v = visibility.classify(ramp, occlusion_tol=float(W))
    assert v.counts.tolist() == [[W - 1, 1, 0, 0, 0]]                     # d = 0 at column 0 is INVALID
    v = visibility.classify(ramp, occlusion_tol=0.0)
    assert v.counts.tolist() == [[1, 1, 0, W - 2, 0]] and int(v.classes[0, 0, W - 1]) == visibility.VISIBLE
    v = visibility.classify(ramp, occlusion_tol=1.0)                      # 1023 - d > 1
    assert v.classes[0, 0].tolist() == [1] + [3] * (W - 3) + [0, 0]
    for tol in (0.0, 1.0):
        want = vo.classify_oracle(ramp.cpu().numpy(), occlusion_tol=tol)
        got = visibility.classify(ramp, occlusion_tol=tol)
        _assert_equal((got.classes, got.counts, None), want, False)


# ------------------------------------------------------------------ determinism, shapes, streams

def test_two_calls_give_equal_bits():
    dev = _gpu()
    from foundationstereo_amd import ops
    left, right, *_ = _case((3, 37, 61), True, True)
    d, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    a = ops.disp_visibility(d, r, want_error=True)
    b = ops.disp_visibility(d, r, want_error=True)
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_shapes_and_views_give_the_same_classes():
    dev = _gpu()
    from foundationstereo_amd import visibility
    left, right, _, _, want = _case((3, 37, 61), True, True)
    d, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    base = visibility.classify(d, r)
    assert np.array_equal(base.classes.cpu().numpy(), want[0])
    assert torch.equal(visibility.classify(d[:, None], r[:, None]).classes, base.classes)
    one = visibility.classify(d[1], r[1])
    assert one.classes.shape == (1, 37, 61) and torch.equal(one.classes[0], base.classes[1])
    assert torch.equal(one.counts[0], base.counts[1])
    wide_d, wide_r = torch.zeros(3, 37, 122, device=dev), torch.zeros(3, 37, 122, device=dev)
    wide_d[:, :, ::2], wide_r[:, :, ::2] = d, r
    view_d, view_r = wide_d[:, :, ::2], wide_r[:, :, ::2]
    assert not view_d.is_contiguous()
    assert torch.equal(visibility.classify(view_d, view_r).classes, base.classes)
    with pytest.raises(RuntimeError, match="float32"):
        visibility.classify(d.double())
    with pytest.raises(RuntimeError, match="disp_right"):
        visibility.classify(d, r[:, :, :60])
    from foundationstereo_amd import _lib
    with pytest.raises(_lib.FsmiError, match="W = 8193"):
        visibility.classify(torch.ones(1, 1, 8193, device=dev))


def test_disp_visibility_does_not_synchronise():
    dev = _gpu()
    from foundationstereo_amd import ops
    left, right, _, _, want = _case((2, 8, 257), True, True)
    d, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    ops.disp_visibility(d, r, want_error=True)                            # library load, first launch
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.disp_visibility(d, r, want_error=True)
        plain = ops.disp_visibility(d)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _assert_equal(got, want, True)
    assert int(plain[1].sum()) == left.size


def test_runs_on_the_current_stream():
    dev = _gpu()
    from foundationstereo_amd import ops
    left, right, _, _, want = _case((2, 8, 257), True, True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        got = ops.disp_visibility(d, r, want_error=True)
    side.synchronize()
    _assert_equal(got, want, True)


def test_torch_operator_equals_ctypes():
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    left, right, *_ = _case((3, 37, 61), True, True)
    d, r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    for rr, occ, err in ((r, True, True), (r, False, False), (None, True, False), (None, False, False)):
        a = torch.ops.fsmi.disp_visibility(d, rr, 0.5, 1.5, occ, err)
        b = ops.disp_visibility(d, rr, 0.5, 1.5, occ, err)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if err:
            assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
        else:
            assert a[2].numel() == 0 and b[2] is None
    with pytest.raises(RuntimeError, match="want_error"):
        torch.ops.fsmi.disp_visibility(d, None, 1.0, 1.0, True, True)


# ------------------------------------------------------------------ the model's right view

H, W, MAX_DISP, ITERS = 64, 96, 32, 4


@pytest.fixture(scope="module")
def model():
    dev = _gpu()
    from foundationstereo_amd import synth
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    args = synth.make_args(max_disp=MAX_DISP, corr_levels=2, vit_size="vits")
    m = FoundationStereo(args).eval()
    synth.init_module_(m, seed=1234)
    return m.to(dev)


def test_right_disparity_is_the_flipped_forward(model):
    dev = _gpu()
    from foundationstereo_amd import visibility
    rng = np.random.default_rng(64)
    left = torch.from_numpy(rng.uniform(0, 255, (1, 3, H, W)).astype(np.float32)).to(dev)
    right = torch.from_numpy(rng.uniform(0, 255, (1, 3, H, W)).astype(np.float32)).to(dev)
    got = visibility.right_disparity(model, left, right, iters=ITERS)
    with torch.no_grad():
        want = torch.flip(model.forward(torch.flip(right, dims=[-1]), torch.flip(left, dims=[-1]), iters=ITERS,
                                        test_mode=True), dims=[-1])
    assert got.shape == (1, 1, H, W) and torch.equal(got, want)
    # two identical textureless frames, end to end; no claim about an untrained model's class shares
    grey = torch.full((1, 3, H, W), 128.0, device=dev)
    with torch.no_grad():
        disp = model.forward(grey, grey, iters=ITERS, test_mode=True).float()
    v = visibility.classify(disp, visibility.right_disparity(model, grey, grey, iters=ITERS).float(), want_error=True)
    assert v.classes.shape == (1, H, W) and int(v.counts.sum()) == H * W and v.error.shape == (1, H, W)


# ------------------------------------------------------------------ where it plugs in

KMAT = np.array([[80.0, 0, 31.5], [0, 80.0, 2.5], [0, 0, 1]], dtype=np.float32)


def test_cloud_keep_mask():
    dev = _gpu()
    from foundationstereo_amd import cloud, visibility
    left, _, occ, _ = vo.analytic_scene(H=6)
    d = torch.from_numpy(left).to(dev)
    vis = visibility.classify(d).visible
    plain = cloud.disparity_to_cloud(d, KMAT, 0.1, denoise=False, z_far=100.0)[0]
    none = cloud.disparity_to_cloud(d, KMAT, 0.1, denoise=False, z_far=100.0, keep=None)[0]
    kept = cloud.disparity_to_cloud(d, KMAT, 0.1, denoise=False, z_far=100.0, keep=vis)[0]
    for name in ("points", "xyz_map", "depth", "valid", "inliers"):
        assert torch.equal(getattr(plain, name), getattr(none, name)), name
    assert int(plain.valid.sum()) == 6 * 60                               # the reference drops u - d < 0 only
    assert torch.equal(kept.valid, plain.valid & vis[0]) and int(kept.valid.sum()) == 6 * 44
    assert np.array_equal(kept.valid.cpu().numpy(), occ[0] == 0)
    assert torch.equal(kept.points, plain.xyz_map[plain.valid & vis[0]])
    assert torch.equal(kept.xyz_map, plain.xyz_map) and torch.equal(kept.depth, plain.depth)
    a = cloud.disparity_to_xyz(d, KMAT, 0.1)
    b = cloud.disparity_to_xyz(d, KMAT, 0.1, keep=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="keep"):
        cloud.disparity_to_xyz(d, KMAT, 0.1, keep=vis[:, :3])
    with pytest.raises(ValueError, match="keep"):
        cloud.disparity_to_xyz(d, KMAT, 0.1, keep=vis.to(torch.uint8))


def test_run_pair_with_checks(model):
    _gpu()
    from foundationstereo_amd import demo, visibility
    rng = np.random.default_rng(50)
    left, right = rng.integers(0, 256, (50, 90, 3), dtype=np.uint8), rng.integers(0, 256, (50, 90, 3), dtype=np.uint8)
    kw = dict(valid_iters=ITERS, z_far=20.0, denoise_radius=0.4, denoise_nb_points=10)
    Kd = np.array([[80.0, 0, 44.5], [0, 80.0, 24.5], [0, 0, 1]], dtype=np.float32)
    base = demo.run_pair(model, left, right, Kd, 0.1, **kw)
    assert "visibility" not in base
    for flags in (dict(occlusion_check=1), dict(lr_check=1, lr_thresh=0.5), dict(occlusion_check=1, lr_check=1)):
        out = demo.run_pair(model, left, right, Kd, 0.1, **kw, **flags)
        v = out["visibility"]
        assert torch.equal(out["disp"], base["disp"])                     # the forward's map is not touched
        assert v.classes.shape == (1, 50, 90) and int(v.counts.sum()) == 50 * 90
        if "lr_check" not in flags:
            assert int(v.counts[0, visibility.MISMATCH]) == 0
            assert torch.equal(v.classes, visibility.classify(out["disp"]).classes)
        if "occlusion_check" not in flags:
            assert int(v.counts[0, visibility.OCCLUDED]) == 0
        assert len(out["cloud"][0]) <= len(base["cloud"][0])
        assert len(out["cloud"][0]) <= int(v.counts[0, visibility.VISIBLE])
    with pytest.raises(ValueError, match="pinhole"):
        demo.run_pair(model, left, right, Kd, 0.1, camera_type="panorama", occlusion_check=1, **kw)


def test_demo_main_with_occlusion_check(tmp_path, capsys):
    _gpu()
    from foundationstereo_amd import demo
    Hd, Wd = 50, 90
    rng = np.random.default_rng(50)
    np.save(tmp_path / "L.npy", rng.integers(0, 256, (Hd, Wd, 3), dtype=np.uint8))
    np.save(tmp_path / "R.npy", rng.integers(0, 256, (Hd, Wd, 3), dtype=np.uint8))
    (tmp_path / "K.txt").write_text("80.0 0.0 44.5 0.0 80.0 24.5 0.0 0.0 1.0\n0.1\n")
    common = ["--synthetic", "--max_disp", str(MAX_DISP), "--left_file", str(tmp_path / "L.npy"), "--right_file",
              str(tmp_path / "R.npy"), "--intrinsic_file", str(tmp_path / "K.txt"), "--valid_iters", str(ITERS),
              "--z_far", "20.0", "--denoise_radius", "0.4", "--denoise_nb_points", "10"]
    plain = demo.main(common + ["--out_dir", str(tmp_path / "plain")])
    assert "visibility" not in plain and not os.path.exists(tmp_path / "plain" / "visibility.png")
    res = demo.main(common + ["--out_dir", str(tmp_path / "occ"), "--occlusion_check", "1"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    assert len(res["visibility"]) == 5 and sum(res["visibility"]) == Hd * Wd and res["visibility"][4] == 0
    assert res["cloud_points"] <= plain["cloud_points"] and res["cloud_points"] <= res["visibility"][0]
    raw = open(tmp_path / "occ" / "visibility.png", "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    import struct
    assert struct.unpack(">II", raw[16:24]) == (Wd, Hd)
    assert sorted(os.listdir(tmp_path / "occ")) == sorted(os.listdir(tmp_path / "plain") + ["visibility.png"])


def test_evaluate_noc(tmp_path, capsys):
    """Ground truth: the analytic scene with its four out-of-view columns set to 0, which the default
    mask (gt > 0) leaves out as well; what --noc takes away on top is then exactly the 16 occluded
    pixels of every row."""
    _gpu()
    from foundationstereo_amd import evaluate
    Hs = 6
    left, _, occ, _ = vo.analytic_scene(H=Hs)
    gt = left[0].copy()
    gt[:, :4] = 0.0
    pred = left[0] + np.float32(0.5)
    pred[:, 14:30] += np.float32(8.0)                                     # a wrong guess behind the foreground
    np.save(tmp_path / "gt.npy", gt)
    np.save(tmp_path / "pred.npy", pred)
    np.save(tmp_path / "seq.npy", np.stack([pred + np.float32(1.0), pred]))
    flags = ["--pred_file", str(tmp_path / "pred.npy"), "--gt_file", str(tmp_path / "gt.npy")]
    default = evaluate.main(flags)
    noc = evaluate.main(flags + ["--noc"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == noc and noc["mask"] == "noc" and "mask" not in default
    assert default["n_valid"] == Hs * 60 and noc["n_valid"] == default["n_valid"] - 16 * Hs == Hs * 44
    assert noc["epe"] == 0.5 and default["epe"] > noc["epe"]
    seq = evaluate.main(["--pred_file", str(tmp_path / "seq.npy"), "--gt_file", str(tmp_path / "gt.npy"), "--per_iter",
                         "--noc"])
    assert seq["mask"] == "noc" and seq["n_valid"] == Hs * 44 and seq["per_iter"]["epe"] == [1.5, 0.5]
