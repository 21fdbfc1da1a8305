"""CPU-only checks of the point-cloud stage: the oracle against the reference's golden, the argument
checks of the three new entry points, loud failure on CPU tensors, and the host-side file helpers."""
import os

import numpy as np
import pytest
import torch

from tests import cloud_oracle


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cloud_small.npz"))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_reproduces_reference_depth2xyzmap(golden, tag):
    """tests/golden/cloud_small.npz holds the reference's own depth2xyzmap output (tools/make_goldens.py
    cloud): exact on the zeroed pixels, within 1e-6 of the largest |z| elsewhere."""
    depth, ref, K = golden[f"depth_{tag}"], golden[f"xyz_{tag}"], golden["K"]
    zeroed = depth < np.float32(golden["zmin"])
    assert zeroed.any() and (depth == 0).any() and ((depth > 0) & zeroed).any() and not zeroed.all()
    got = cloud_oracle.depth_to_xyz_oracle(depth, K, zmin=0.1)
    assert got.shape == ref.shape
    assert np.array_equal(got[zeroed], np.zeros_like(got[zeroed])) and not ref[zeroed].any()
    bound = 1e-6 * np.abs(ref[..., 2]).max()
    assert np.abs(got - ref)[~zeroed].max() <= bound
    # the same through the disparity entry: disp = fx b / depth, depth 0 -> inf -> removed
    b = 0.12
    with np.errstate(divide="ignore"):
        disp = (np.float64(K[0, 0]) * np.float64(np.float32(b)) / depth.astype(np.float64)).astype(np.float32)
    xyz, dep, valid = cloud_oracle.xyz_oracle(disp, K, b, zmin=0.1, z_far=100.0, remove_invisible=False)
    assert np.array_equal(xyz[zeroed], np.zeros_like(xyz[zeroed]))
    assert np.array_equal(valid, ~zeroed)
    assert np.abs(xyz - ref)[~zeroed].max() <= 2 * bound          # one more fp32 rounding: disp itself


def test_oracle_nonfinite_and_removed_pixels():
    K = np.array([[60, 0, 3.0], [0, 60, 2.0], [0, 0, 1]], np.float32)
    disp = np.array([[np.nan, np.inf, 0.0, -2.0, 1.0, 6.0, 1e3, 0.5]], np.float32)
    xyz, depth, valid = cloud_oracle.xyz_oracle(disp, K, 0.1, z_far=10.0)
    #            nan    inf    0      neg    u-d>=0  u-d<0  u-d<0  z>z_far
    assert valid.tolist() == [[False, False, False, False, True, False, False, False]]
    assert np.isfinite(xyz).all() and not xyz[0, [0, 1, 2, 3, 5, 6]].any()
    assert depth[0, 1] == 0 and depth[0, 5] == 0 and np.isinf(depth[0, 2]) and np.isnan(depth[0, 0])
    assert xyz[0, 7, 2] == pytest.approx(12.0)                    # beyond z_far: kept in the map, not valid
    xyz, depth, valid = cloud_oracle.xyz_oracle(disp, K, 0.1, z_far=10.0, remove_invisible=False)
    #            nan    inf    0      neg    z=6   z=1   z<zmin z>z_far
    assert valid.tolist() == [[False, False, False, False, True, True, False, False]]
    assert depth[0, 1] == 0 and depth[0, 6] == pytest.approx(0.006) and not xyz[0, 6].any()


def test_radius_count_oracle_small():
    pts = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.02, 0], [1, 1, 1], [np.nan, 0, 0]], np.float32)
    assert cloud_oracle.radius_count_oracle(pts, 0.03).tolist() == [3, 3, 3, 1, 0]
    assert cloud_oracle.radius_count_oracle(pts, 0.03, valid=[1, 0, 1, 1, 1]).tolist() == [2, 0, 2, 1, 0]
    keep, amb = cloud_oracle.radius_mask_oracle(pts, 0.03, 2)
    assert keep.tolist() == [True, True, True, False, False] and not amb.any()


def test_cloud_entry_points_reject_bad_args_without_gpu():
    """Argument validation happens before any HIP call, so it is testable on the CPU."""
    from foundationstereo_amd import _lib
    lib = _lib.load()
    cam = (60.0, 60.0, 3.0, 2.0, 0.1, 0.1, 10.0, 1, 0)
    assert lib.fsmi_disp_to_xyz(None, 16, 16, 16, 1, 4, 4, *cam, None) == 1001
    assert b"null" in lib.fsmi_last_error()
    assert lib.fsmi_disp_to_xyz(16, 16, 16, 16, 1, 0, 4, *cam, None) == 1001
    assert lib.fsmi_disp_to_xyz(16, 16, 16, 16, 1, 1 << 16, 1 << 16, *cam, None) == 1001      # H*W overflows
    assert b"2^31" in lib.fsmi_last_error()
    assert lib.fsmi_disp_to_xyz(16, 16, 16, 16, 4, 1 << 15, 1 << 15, *cam, None) == 1001      # B*H*W overflows
    assert lib.fsmi_disp_to_xyz(16, 16, 16, 16, 1, 4, 4, *cam[:8], 7, None) == 1001           # camera_type
    assert lib.fsmi_disp_to_xyz(20, 16, 16, 16, 1, 4, 4, *cam, None) == 1001                  # unaligned disp
    assert lib.fsmi_disp_to_xyz(16, 16, 16, 16, 1, 4, 4, 0.0, *cam[1:], None) == 1001         # fx = 0

    assert lib.fsmi_cloud_cell_keys(None, None, 16, 8, 0.03, None) == 1001
    assert lib.fsmi_cloud_cell_keys(16, None, None, 8, 0.03, None) == 1001
    assert lib.fsmi_cloud_cell_keys(16, None, 16, -1, 0.03, None) == 1001
    assert lib.fsmi_cloud_cell_keys(16, None, 16, 8, 0.0, None) == 1001
    assert b"radius" in lib.fsmi_last_error()
    assert lib.fsmi_cloud_cell_keys(16, None, 16, 8, -1.0, None) == 1001
    assert lib.fsmi_cloud_cell_keys(None, None, None, 0, 0.03, None) == 0                     # N = 0: nothing to do

    assert lib.fsmi_radius_count(None, 16, 16, 16, 8, 0.03, 30, None) == 1001
    assert lib.fsmi_radius_count(16, None, 16, 16, 8, 0.03, 30, None) == 1001
    assert lib.fsmi_radius_count(16, 16, None, 16, 8, 0.03, 30, None) == 1001
    assert lib.fsmi_radius_count(16, 16, 16, None, 8, 0.03, 30, None) == 1001
    assert lib.fsmi_radius_count(16, 16, 16, 16, -2, 0.03, 30, None) == 1001
    assert lib.fsmi_radius_count(16, 16, 16, 16, 2 ** 31 - 1, 0.03, 30, None) == 1001       # slot + lane would overflow
    assert lib.fsmi_radius_count(16, 16, 16, 16, 8, 0.0, 30, None) == 1001
    assert lib.fsmi_radius_count(16, 16, 16, 16, 8, 0.03, -1, None) == 1001
    assert b"nb_points" in lib.fsmi_last_error()
    assert lib.fsmi_radius_count(None, None, None, None, 0, 0.03, 30, None) == 0


def test_cloud_ops_refuse_cpu_tensors():
    from foundationstereo_amd import cloud, ops
    K = np.eye(3)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_to_xyz(torch.ones(1, 4, 8), 60.0, 60.0, 4.0, 2.0, 0.1)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.radius_outlier_mask(torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="ROCm"):
        cloud.disparity_to_xyz(torch.ones(1, 1, 4, 8), K, 0.1)
    with pytest.raises(RuntimeError, match="ROCm"):
        cloud.disparity_to_cloud(torch.ones(4, 8), K, 0.1)
    with pytest.raises(ValueError, match="camera_type"):
        ops.disp_to_xyz(torch.ones(1, 4, 8), 60.0, 60.0, 4.0, 2.0, 0.1, camera_type="fisheye")


def test_cloud_torch_operators_registered_without_cpu_kernel():
    from foundationstereo_amd import torch_ops
    torch_ops.load()
    assert "disp_to_xyz" in torch_ops.OPS and "radius_outlier_mask" in torch_ops.OPS
    with pytest.raises(NotImplementedError):
        torch.ops.fsmi.disp_to_xyz(torch.ones(1, 4, 8), 60.0, 60.0, 4.0, 2.0, 0.1)
    with pytest.raises(NotImplementedError):
        torch.ops.fsmi.radius_outlier_mask(torch.zeros(10, 3))


def _parse_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = next(int(ln.split()[2]) for ln in lines if ln.startswith("element vertex"))
    types = {"float": "<f4", "uchar": "u1"}
    dt = np.dtype([(ln.split()[2], types[ln.split()[1]]) for ln in lines if ln.startswith("property")])
    assert len(raw) - end == n * dt.itemsize
    return np.frombuffer(raw[end:], dtype=dt, count=n)


def test_write_ply_round_trip(tmp_path):
    from foundationstereo_amd import cloud
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((100, 3)).astype(np.float32)
    col = rng.integers(0, 256, (100, 3), dtype=np.uint8)
    cloud.write_ply(tmp_path / "c.ply", torch.from_numpy(pts), torch.from_numpy(col))
    rec = _parse_ply(tmp_path / "c.ply")
    assert rec.dtype.names == ("x", "y", "z", "red", "green", "blue")
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), col)
    cloud.write_ply(tmp_path / "p.ply", pts)                      # no colours: 12-byte vertices
    rec = _parse_ply(tmp_path / "p.ply")
    assert rec.dtype.names == ("x", "y", "z") and np.array_equal(rec["z"], pts[:, 2])
    cloud.write_ply(tmp_path / "f.ply", pts, col.astype(np.float32) / 255.0)   # Open3D-style [0,1] colours
    assert np.array_equal(_parse_ply(tmp_path / "f.ply")["green"], col[:, 1])
    with pytest.raises(ValueError):
        cloud.write_ply(tmp_path / "bad.ply", pts, col[:50])


def test_read_intrinsics(tmp_path):
    from foundationstereo_amd import cloud
    p = tmp_path / "K.txt"
    p.write_text("754.668 0.0 489.379 0.0 754.668 265.162 0.0 0.0 1.0\n0.063\n")
    K, b = cloud.read_intrinsics(p)
    assert K.dtype == np.float32 and K.shape == (3, 3)
    assert np.array_equal(K, np.array([[754.668, 0, 489.379], [0, 754.668, 265.162], [0, 0, 1]], np.float32))
    assert b == 0.063
    p.write_text("1 2 3\n0.1\n")
    with pytest.raises(ValueError):
        cloud.read_intrinsics(p)
