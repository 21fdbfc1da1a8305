"""CPU restatement (numpy fp64) of what the reference does after the forward, for the cloud tests.

``xyz_oracle`` restates scripts/run_demo.py:173-251 and depth2xyzmap (Utils.py:56-75);
``radius_count_oracle`` is the neighbour count behind Open3D's ``remove_radius_outlier``
(scripts/run_demo.py:272) on a KD-tree.  Scalars the kernel receives as fp32 (the camera, the
baseline, the radius) are rounded to fp32 first, so the only difference left is the arithmetic.
"""
import numpy as np


def _f32(x):
    return float(np.float32(x))


def depth_to_xyz_oracle(depth, K, zmin=0.1):
    """Utils.py:56-75 with uvs=None: (H,W) depth -> (H,W,3) fp64, zero where depth < zmin."""
    depth = np.asarray(depth, dtype=np.float64)
    K = np.asarray(K, dtype=np.float32).astype(np.float64)
    H, W = depth.shape
    vs, us = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")          # :60
    with np.errstate(invalid="ignore", over="ignore"):
        xyz = np.stack([(us - K[0, 2]) * depth / K[0, 0], (vs - K[1, 2]) * depth / K[1, 1], depth], -1)  # :67-70
    xyz[depth < _f32(zmin)] = 0                                              # :57,73-74
    return xyz


def xyz_oracle(disp, K, baseline, camera_type="pinhole", remove_invisible=True, zmin=0.1, z_far=10.0, scale=1.0):
    """disp (H,W) or (B,H,W) fp32 -> (xyz fp64 (...,3), depth fp64, valid bool), include/fsmi.h's contract."""
    disp = np.asarray(disp)
    if disp.ndim == 3:
        parts = [xyz_oracle(d, K, baseline, camera_type, remove_invisible, zmin, z_far, scale) for d in disp]
        return tuple(np.stack(p) for p in zip(*parts))
    d = disp.astype(np.float64)
    H, W = d.shape
    K = np.array(K, dtype=np.float32).reshape(3, 3)
    K[:2] *= np.float32(scale)                                               # run_demo.py:232
    b = _f32(baseline)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")          # :175
    with np.errstate(all="ignore"):
        us_right = xx - d                                                    # :176
        removed = (us_right < 0) if remove_invisible else np.zeros((H, W), bool)   # :174,177
        if camera_type == "pinhole":
            depth = float(K[0, 0]) * b / d                                   # :235
            depth[removed] = 0                                               # :178, fx*b/inf
            xyz = depth_to_xyz_oracle(depth, K, zmin)                        # :238
            xyz[~np.isfinite(depth)] = 0                                     # the kernel never emits NaN / inf
            z = xyz[..., 2]
            valid = ~removed & np.isfinite(d) & (z > 0) & (z <= _f32(z_far))  # :240,249
        elif camera_type == "panorama":
            half_lat, half_lon = np.pi / 2, np.pi                            # :186-187
            lon_up = (yy * 2 / H - 1) * half_lon                             # :190,194
            lat_up = (xx * 2 / W - 1) * half_lat                             # :191,195
            lat_down = (us_right * 2 / W - 1) * half_lat                     # :198-200
            ang_disp = d * 2 * half_lon / W                                  # :203
            tr = b * np.cos(lat_down) / np.sin(ang_disp)                     # :211
            tr[removed] = 0
            depth = tr
            fin = np.isfinite(tr)
            trf = np.where(fin, tr, 0.0)
            xyz = np.stack([np.sin(lat_up) * trf, -np.cos(lat_up) * np.cos(lon_up) * trf,
                            np.cos(lat_up) * np.sin(lon_up) * trf], -1)      # :214-219
            valid = ~removed & fin & (tr > 0)
        else:
            raise ValueError(camera_type)
    return xyz, depth, valid


def radius_count_oracle(points, r, valid=None, workers=1):
    """Per point, the number of valid finite points (itself included) with distance < r, fp64 on the
    given coordinates; 0 for a point that is masked out or not finite."""
    from scipy.spatial import cKDTree
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(pts).all(1)
    if valid is not None:
        ok &= np.asarray(valid).reshape(-1).astype(bool)
    counts = np.zeros(len(pts), dtype=np.int64)
    if ok.any():
        sel = pts[ok]
        tree = cKDTree(sel)
        # query_ball_point is closed (<= r); the contract is strict.  The tests skip the points whose
        # decision changes anywhere in r (1 +- 1e-6), so an exact tie cannot decide a compared point.
        counts[ok] = tree.query_ball_point(sel, r, return_length=True, workers=workers)
    return counts


def radius_mask_oracle(points, r, nb_points, valid=None, rel=1e-6, workers=1):
    """(keep, ambiguous): keep = count > nb_points; ambiguous where that differs between r(1-rel) and r(1+rel)."""
    r = _f32(r)
    lo = radius_count_oracle(points, r * (1 - rel), valid, workers) > nb_points
    hi = radius_count_oracle(points, r * (1 + rel), valid, workers) > nb_points
    return hi, lo != hi
