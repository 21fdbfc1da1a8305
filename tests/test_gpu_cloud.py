"""The point-cloud stage on the GPU (csrc/cloud.hip) against tests/cloud_oracle.py.

Tolerances are derived, not measured.  Pinhole: a value is at most ~6 fp32 roundings (6e-8 each)
away from the fp64 oracle fed the same fp32 disparity and camera -> 1e-6 of the point's largest
component.  Panorama: ~10 roundings times the conditioning of cos at 80 degrees (<= 6) -> 1e-5 |tr|.
Radius mask: the decision is exact except where the oracle itself flips between r (1 - 1e-6) and
r (1 + 1e-6) (fp32 d^2 carries ~2.4e-7); those points are skipped and capped at 0.1 %.
"""
import os

import numpy as np
import pytest
import torch

from tests import cloud_oracle

pytestmark = pytest.mark.gpu

K0 = np.array([[60.0, 0.0, 31.3], [0.0, 60.0, 23.6], [0.0, 0.0, 1.0]], dtype=np.float32)
BASELINE = 0.1


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ unprojection

def _pinhole_disp(B, H, W, fxb, zmin, z_far, seed):
    """Seeded disparity with every class of pixel; pixels closer than 1e-4 (relative) to a threshold
    are replaced by NaN (a class of its own), so the decision of every finite pixel is unambiguous."""
    rng = np.random.default_rng(seed)
    u = np.broadcast_to(np.arange(W, dtype=np.float64), (B, H, W))
    z = rng.uniform(0.3, 8.0, (B, H, W))
    cls = rng.integers(0, 16, (B, H, W))
    z = np.where(cls == 5, rng.uniform(0.01, 0.09, z.shape), z)           # below zmin
    z = np.where(cls == 6, rng.uniform(11.0, 50.0, z.shape), z)           # beyond z_far
    d = fxb / z
    d = np.where(cls == 0, 0.0, d)
    d = np.where(cls == 1, -rng.uniform(0.1, 9.0, z.shape), d)
    d = np.where(cls == 2, np.nan, d)
    d = np.where(cls == 3, np.inf, d)
    d = np.where(cls == 4, u + 0.5 + rng.uniform(0.0, 5.0, z.shape), d)   # falls outside the right image
    d = d.astype(np.float32)
    d64 = d.astype(np.float64)
    with np.errstate(all="ignore"):
        zz = fxb / d64
        near = (np.abs(u - d64) < 1e-4 * np.maximum(np.maximum(u, np.abs(d64)), 1.0)) \
            | (np.abs(zz - zmin) < 1e-4 * zmin) | (np.abs(zz - z_far) < 1e-4 * z_far)
    d[near & np.isfinite(d)] = np.nan
    return d


def _assert_clear_of_thresholds(d, fxb, zmin, z_far):
    fin = np.isfinite(d) & (d != 0)
    d64 = d.astype(np.float64)[fin]
    u = np.broadcast_to(np.arange(d.shape[-1], dtype=np.float64), d.shape)[fin]
    z = fxb / d64
    assert (np.abs(u - d64) >= 1e-4 * np.maximum(np.maximum(u, np.abs(d64)), 1.0)).all()
    assert (np.abs(z - zmin) >= 1e-4 * zmin).all() and (np.abs(z - z_far) >= 1e-4 * z_far).all()


def _compare_xyz(got, want, rel):
    xyz, depth, valid = (t.cpu().numpy() for t in got)
    oxyz, odepth, ovalid = want
    assert valid.dtype == np.bool_ and np.array_equal(valid, ovalid)
    assert np.isfinite(xyz).all()
    zero = ~oxyz.any(-1)
    assert not xyz[zero].any()
    bound = rel * np.abs(oxyz).max(-1, keepdims=True)
    err = np.abs(xyz - oxyz)
    print(f"xyz: max err / bound = {np.max(err[~zero] / bound[~zero]) if (~zero).any() else 0:.3f}")
    assert (err <= bound).all()
    fin = np.isfinite(odepth)
    assert np.array_equal(np.isnan(depth), np.isnan(odepth))
    assert np.array_equal(depth[~fin & ~np.isnan(odepth)], odepth[~fin & ~np.isnan(odepth)])   # signed inf
    assert (np.abs(depth[fin] - odepth[fin]) <= rel * np.abs(odepth[fin])).all()


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 33, 70), (1, 48, 64)])
@pytest.mark.parametrize("remove_invisible,scale", [(True, 1.0), (False, 1.0), (True, 0.5)])
def test_pinhole_matches_oracle(shape, remove_invisible, scale):
    dev = _gpu()
    from foundationstereo_amd import cloud
    zmin, z_far = 0.1, 10.0
    fxb = float(np.float32(K0[0, 0] * np.float32(scale))) * float(np.float32(BASELINE))
    d = _pinhole_disp(*shape, fxb, zmin, z_far, seed=11)
    _assert_clear_of_thresholds(d, fxb, zmin, z_far)
    u = np.arange(shape[2])
    with np.errstate(all="ignore"):
        classes = (d == 0, d < 0, np.isnan(d), np.isposinf(d), np.isfinite(d) & (u - d < 0),
                   np.isfinite(d) & (d > 0) & (fxb / np.where(d > 0, d, 1) < zmin),
                   np.isfinite(d) & (d > 0) & (fxb / np.where(d > 0, d, 1) > z_far))
    for present in classes:
        assert present.any() or shape == (1, 5, 7)                # 35 pixels cannot hold every class
    want = cloud_oracle.xyz_oracle(d, K0, BASELINE, "pinhole", remove_invisible, zmin, z_far, scale)
    assert want[2].any() and not want[2].all()
    got = cloud.disparity_to_xyz(torch.from_numpy(d).to(dev)[:, None], K0, BASELINE, scale=scale,
                                 remove_invisible=remove_invisible, zmin=zmin, z_far=z_far)
    assert got[0].shape == shape + (3,) and got[1].shape == shape and got[2].shape == shape
    _compare_xyz(got, want, 1e-6)


def test_pinhole_accepts_hw_and_bhw():
    dev = _gpu()
    from foundationstereo_amd import cloud
    d = torch.from_numpy(_pinhole_disp(1, 9, 13, 6.0, 0.1, 10.0, seed=2)).to(dev)
    a = cloud.disparity_to_xyz(d[0], K0, BASELINE)
    b = cloud.disparity_to_xyz(d, K0, BASELINE)
    c = cloud.disparity_to_xyz(d[:, None], K0, BASELINE)
    for x, y, z in zip(a, b, c):                                  # bitwise: depth holds NaN for NaN disparity
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(y.view(torch.uint8), z.view(torch.uint8))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_depth_maps_match_reference(golden_dir, tag):
    """The HIP path on the reference's own depth2xyzmap cases: disp = fx b / depth, depth 0 -> inf."""
    dev = _gpu()
    from foundationstereo_amd import cloud
    g = np.load(os.path.join(golden_dir, "cloud_small.npz"))
    depth, ref, K = g[f"depth_{tag}"], g[f"xyz_{tag}"], g["K"]
    zmin = 0.1
    assert (np.abs(depth[depth > 0] - zmin) >= 1e-4 * zmin).all()
    with np.errstate(divide="ignore"):
        disp = (np.float64(K[0, 0]) * np.float64(np.float32(BASELINE)) / depth.astype(np.float64)).astype(np.float32)
    xyz, dep, valid = cloud.disparity_to_xyz(torch.from_numpy(disp).to(dev), K, BASELINE, remove_invisible=False,
                                             zmin=zmin, z_far=1e3)
    xyz, valid = xyz[0].cpu().numpy(), valid[0].cpu().numpy()
    zeroed = depth < np.float32(zmin)
    assert zeroed.any() and np.array_equal(valid, ~zeroed) and not xyz[zeroed].any()
    assert (np.abs(xyz - ref) <= 1e-6 * np.abs(ref).max(-1, keepdims=True)).all()


def test_panorama_matches_oracle():
    dev = _gpu()
    from foundationstereo_amd import cloud
    B, H, W = 1, 32, 64
    rng = np.random.default_rng(5)
    u = np.broadcast_to(np.arange(W, dtype=np.float64), (B, H, W))
    lo = np.maximum(0.11, u - 60.4)
    hi = np.minimum(15.0, u - 3.6)
    d = np.where(u < 4, u + 1.0 + rng.uniform(0, 3, u.shape), lo + (hi - lo) * rng.uniform(0, 1, u.shape))
    d = d.astype(np.float32)
    kept = u - d >= 0
    assert np.array_equal(kept, u >= 4)
    ang = d.astype(np.float64) * 2 * np.pi / W
    lat_down = ((u - d) * 2 / W - 1) * np.pi / 2
    assert (ang[kept] >= 0.01).all() and (ang[kept] <= np.pi / 2).all()
    assert (np.abs(lat_down[kept]) <= np.deg2rad(80.0)).all()
    oxyz, otr, ovalid = cloud_oracle.xyz_oracle(d, np.eye(3), BASELINE, "panorama")
    assert np.array_equal(ovalid, kept)
    xyz, tr, valid = (t.cpu().numpy() for t in cloud.disparity_to_xyz(torch.from_numpy(d).to(dev), np.eye(3),
                                                                       BASELINE, camera_type="panorama"))
    assert np.array_equal(valid, ovalid)
    assert not xyz[~kept].any() and not tr[~kept].any()
    bound = 1e-5 * np.abs(otr[kept])
    print(f"panorama: max |dtr| / bound = {np.max(np.abs(tr[kept] - otr[kept]) / bound):.3f}")
    assert (np.abs(tr[kept] - otr[kept]) <= bound).all()
    assert (np.abs(xyz[kept] - oxyz[kept]) <= bound[:, None]).all()


def test_disp_to_xyz_does_not_synchronise():
    dev = _gpu()
    from foundationstereo_amd import ops
    d = torch.full((1, 33, 70), 3.0, device=dev)
    ops.disp_to_xyz(d, 60.0, 60.0, 31.3, 23.6, 0.1)               # library load, first launch
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        xyz, depth, valid = ops.disp_to_xyz(d, 60.0, 60.0, 31.3, 23.6, 0.1)
        xyz2, _, _ = ops.disp_to_xyz(d, 60.0, 60.0, 31.3, 23.6, 0.1, camera_type="panorama")
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert bool(valid[0, 0, 10]) and float(depth[0, 0, 10]) == pytest.approx(2.0)


# ------------------------------------------------------------------ radius outlier mask

def _check_mask(points, valid, radius, nb_points, dev, expect_both=False):
    """ops.radius_outlier_mask against the oracle; returns the inlier share."""
    from foundationstereo_amd import ops
    pts = np.ascontiguousarray(points, dtype=np.float32)
    keep = ops.radius_outlier_mask(torch.from_numpy(pts).to(dev),
                                   None if valid is None else torch.from_numpy(np.asarray(valid)).to(dev),
                                   nb_points=nb_points, radius=radius)
    assert keep.dtype == torch.bool and keep.shape == (len(pts),)
    keep = keep.cpu().numpy()
    want, amb = cloud_oracle.radius_mask_oracle(pts, radius, nb_points, valid)
    assert amb.mean() <= 1e-3, f"{amb.sum()} ambiguous points"
    wrong = (keep != want) & ~amb
    print(f"N {len(pts)} r {radius} nb {nb_points}: inliers {want.mean():.4f}, ambiguous {amb.sum()}, wrong {wrong.sum()}")
    assert not wrong.any(), np.flatnonzero(wrong)[:10]
    if valid is not None:
        assert not keep[~np.asarray(valid).astype(bool)].any()
    if expect_both:
        assert 0 < want.mean() < 1
    return want.mean()


@pytest.fixture(scope="module")
def cloud_a():
    rng = np.random.default_rng(7)
    pts = rng.uniform(-0.2, 0.2, (4000, 3)).astype(np.float32)
    pts[:, 2] += np.float32(0.1)
    return np.concatenate([pts, pts[:50]])                        # 50 exact duplicates


@pytest.mark.parametrize("nb_points", [0, 8, 14, 30])
def test_radius_mask_uniform_cloud(cloud_a, nb_points):
    dev = _gpu()
    assert (cloud_a < 0).any() and len(cloud_a) == 4050
    share = _check_mask(cloud_a, None, 0.03, nb_points, dev, expect_both=nb_points in (8, 14))
    if nb_points == 0:
        assert share == 1.0                                       # every point counts itself
    if nb_points == 30:
        assert share == 0.0


@pytest.fixture(scope="module")
def cloud_b():
    """The unprojection of a slanted plane with 5 % spiked pixels, by the kernel under test above."""
    dev = _gpu()
    from foundationstereo_amd import ops
    H, W = 48, 64
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 4.0 + 0.03 * u + 0.02 * v
    rng = np.random.default_rng(21)
    spike = rng.uniform(0, 1, d.shape) < 0.05
    d = np.where(spike, d * rng.uniform(0.4, 2.5, d.shape), d).astype(np.float32)
    xyz, _, valid = ops.disp_to_xyz(torch.from_numpy(d).to(dev)[None], 60.0, 60.0, 31.3, 23.6, 0.1)
    return xyz[0].reshape(-1, 3).cpu().numpy(), valid[0].reshape(-1).cpu().numpy(), spike.reshape(-1)


@pytest.mark.parametrize("nb_points", [30, 12])
def test_radius_mask_slanted_plane(cloud_b, nb_points):
    dev = _gpu()
    pts, valid, spike = cloud_b
    assert valid.any() and not valid.all()
    _check_mask(pts, valid, 0.05, nb_points, dev, expect_both=True)
    if nb_points == 12:
        from foundationstereo_amd import ops
        keep = ops.radius_outlier_mask(torch.from_numpy(pts).to(dev), torch.from_numpy(valid).to(dev),
                                       nb_points=12, radius=0.05).cpu().numpy()
        assert keep[valid & spike].mean() < 0.5 < keep[valid & ~spike].mean()


def test_radius_mask_edge_sizes():
    dev = _gpu()
    from foundationstereo_amd import ops
    one = torch.tensor([[0.1, -0.2, 0.3]], device=dev)
    assert ops.radius_outlier_mask(one, nb_points=0).tolist() == [True]
    assert ops.radius_outlier_mask(one, nb_points=1).tolist() == [False]
    empty = ops.radius_outlier_mask(torch.zeros((0, 3), device=dev))
    assert empty.dtype == torch.bool and empty.shape == (0,)
    pts = torch.rand((300, 3), device=dev) * 0.01
    none = ops.radius_outlier_mask(pts, torch.zeros(300, dtype=torch.bool, device=dev), nb_points=0)
    assert none.shape == (300,) and not none.any()


def test_radius_mask_respects_valid(cloud_a):
    dev = _gpu()
    valid = np.arange(len(cloud_a)) % 2 == 0
    _check_mask(cloud_a, valid, 0.03, 3, dev, expect_both=True)
    _check_mask(cloud_a, valid.astype(np.uint8), 0.03, 3, dev)


def test_radius_mask_one_cell():
    dev = _gpu()
    rng = np.random.default_rng(9)
    pts = rng.uniform(0.005, 0.02, (500, 3)).astype(np.float32)   # diagonal 0.026 < radius
    assert _check_mask(pts, None, 0.03, 30, dev) == 1.0
    assert _check_mask(pts, None, 0.03, 499, dev) == 1.0          # 500 in range, the point itself included
    assert _check_mask(pts, None, 0.03, 500, dev) == 0.0          # strict: 500 is not more than 500


def test_radius_mask_far_coordinates():
    """Coordinates at +-1e5 m: cell indices beyond the clamp (1e5 / 0.03 > 2^20), fp32 spacing 2^-7 m."""
    dev = _gpu()
    rng = np.random.default_rng(13)
    step = 2.0 ** -7
    parts = []
    for corner in ([1e5, 1e5, 1e5], [-1e5, 1e5, -1e5], [-1e5, -1e5, -1e5]):
        parts.append(np.array(corner) + step * rng.integers(0, 9, (200, 3)))
    parts.append(rng.uniform(-0.1, 0.1, (400, 3)))
    pts = np.concatenate(parts).astype(np.float32)
    assert np.array_equal(pts[:600].astype(np.float64), np.concatenate(parts)[:600])      # exactly representable
    _check_mask(pts, None, 0.03, 6, dev, expect_both=True)


def test_radius_mask_nonfinite_rows(cloud_a):
    dev = _gpu()
    pts = cloud_a[:1500].copy()
    pts[::7, 0] = np.nan
    pts[3::11, 2] = np.inf
    pts[5::13] = -np.inf
    from foundationstereo_amd import ops
    keep = ops.radius_outlier_mask(torch.from_numpy(pts).to(dev), nb_points=2).cpu().numpy()
    assert not keep[~np.isfinite(pts).all(1)].any()
    _check_mask(pts, None, 0.03, 2, dev, expect_both=True)


# ------------------------------------------------------------------ operators, end to end

def test_torch_operators_equal_ctypes(cloud_a):
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    d = torch.from_numpy(_pinhole_disp(2, 33, 70, 6.0, 0.1, 10.0, seed=4)).to(dev)
    for cam in (0, 1):
        a = torch.ops.fsmi.disp_to_xyz(d, 60.0, 61.0, 31.3, 23.6, 0.1, 0.1, 10.0, True, cam)
        b = ops.disp_to_xyz(d, 60.0, 61.0, 31.3, 23.6, 0.1, camera_type=("pinhole", "panorama")[cam])
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))      # bit for bit, NaN depth included
    pts = torch.from_numpy(cloud_a).to(dev)
    valid = torch.arange(len(cloud_a), device=dev) % 3 != 0
    for v in (None, valid):
        a = torch.ops.fsmi.radius_outlier_mask(pts, v, 8, 0.03)
        b = ops.radius_outlier_mask(pts, v, nb_points=8, radius=0.03)
        assert a.dtype == torch.bool and torch.equal(a, b) and a.any() and not a.all()


def test_disparity_to_cloud_end_to_end():
    """cloud.disparity_to_cloud on the smoke configuration's forward (64x96) with a made-up camera."""
    dev = _gpu()
    from foundationstereo_amd import cloud, synth
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    H, W, md, iters, L, shift = 64, 96, 32, 4, 2, 2
    args = synth.make_args(max_disp=md, corr_levels=L, vit_size="vits")
    model = FoundationStereo(args).eval()
    synth.init_module_(model, seed=1234)
    fl, fr, vf = synth.backbone_features(1, H, W, "vits", shift_px=shift)
    left, right = synth.stereo_images(1, H, W)
    model = model.to(dev)
    model.feature.set_features([torch.from_numpy(a).to(dev) for a in fl],
                               [torch.from_numpy(a).to(dev) for a in fr], torch.from_numpy(vf).to(dev))
    left = torch.from_numpy(left).to(dev)
    with torch.no_grad():
        disp = model(left, torch.from_numpy(right).to(dev), iters=iters, test_mode=True).float()
    K = np.array([[80.0, 0, 47.5], [0, 80.0, 31.5], [0, 0, 1]])
    z_far, radius, nb = 20.0, 0.4, 10
    out = cloud.disparity_to_cloud(disp, K, 0.1, image=left, nb_points=nb, radius=radius, z_far=z_far)
    assert len(out) == 1
    c = out[0]
    assert c.xyz_map.shape == (H, W, 3) and c.depth.shape == (H, W) and c.valid.shape == (H, W)
    assert c.inliers.dtype == torch.bool and c.inliers.shape == (H, W)
    M = int(c.inliers.sum())
    assert 0 < M == c.points.shape[0] and c.points.shape[1] == 3
    assert not (c.inliers & ~c.valid).any()
    assert torch.isfinite(c.points).all() and (c.points[:, 2] > 0).all() and (c.points[:, 2] <= z_far).all()
    assert torch.equal(c.points, c.xyz_map[c.inliers])
    assert c.colors.shape == (M, 3) and torch.equal(c.colors, left[0].permute(1, 2, 0)[c.inliers])
    want, amb = cloud_oracle.radius_mask_oracle(c.xyz_map.reshape(-1, 3).cpu().numpy(), radius, nb,
                                                c.valid.reshape(-1).cpu().numpy())
    assert amb.mean() <= 1e-3
    assert np.array_equal(c.inliers.reshape(-1).cpu().numpy()[~amb], want[~amb])
    raw = cloud.disparity_to_cloud(disp, K, 0.1, denoise=False, z_far=z_far)[0]
    assert raw.colors is None and torch.equal(raw.inliers, raw.valid) and raw.points.shape[0] == int(raw.valid.sum())
