"""After the forward: metric depth, an XYZ map and a denoised point cloud, on the device.

The reference does this on the host after every forward (scripts/run_demo.py:173-275): drop the
pixels that fall outside the right image, disparity -> depth -> XYZ (Utils.py:56-75), clip by depth,
Open3D's ``remove_radius_outlier`` and a ``.ply`` file.  Here the unprojection and the neighbour count
are HIP kernels (csrc/cloud.hip) behind ``ops.disp_to_xyz`` / ``ops.radius_outlier_mask``; only the
final compaction ``xyz_map[mask]`` has to know a size on the host and therefore synchronises.

    K, baseline = cloud.read_intrinsics("K.txt")
    disp = model(left, right, iters=32, test_mode=True)
    out = cloud.disparity_to_cloud(disp, K, baseline, image=left)[0]
    cloud.write_ply("cloud_denoise.ply", out.points, out.colors)
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor


@dataclass
class Cloud:
    """One batch element of ``disparity_to_cloud``."""
    points: Tensor              # (M,3) fp32, the pixels of ``inliers`` in row-major order
    colors: Optional[Tensor]    # (M,3) the image values at those pixels (dtype of ``image``), or None
    xyz_map: Tensor             # (H,W,3) fp32
    depth: Tensor               # (H,W) fp32
    valid: Tensor               # (H,W) bool: in view, finite, 0 < z <= z_far
    inliers: Tensor             # (H,W) bool: ``valid`` after the radius outlier removal


def _camera(K, scale: float):
    K = np.array(K, dtype=np.float32).reshape(3, 3)     # a copy: the caller's K stays as it is
    K[:2] *= scale                                      # scripts/run_demo.py:232
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def disparity_to_xyz(disp: Tensor, K, baseline: float, *, scale: float = 1.0, camera_type: str = "pinhole",
                     remove_invisible: bool = True, zmin: float = 0.1, z_far: float = 10.0,
                     keep: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``(xyz_map (B,H,W,3), depth (B,H,W), valid (B,H,W) bool)`` of a disparity map on a HIP device.

    ``K`` is any 3x3 array-like on the host (ignored by ``camera_type="panorama"``) and ``scale`` the
    factor the images were resized by before the forward.  ``keep``, a bool (B,H,W) mask on the device
    of ``disp`` such as ``visibility.classify(disp).visible``, is ANDed into ``valid`` after the kernel;
    ``xyz_map`` and ``depth`` stay as they are.  No host synchronisation."""
    fx, fy, cx, cy = _camera(K, scale)
    xyz, depth, valid = ops.disp_to_xyz(ops._as_bhw(disp, "disparity_to_xyz", "disp"), fx, fy, cx, cy, baseline,
                                        zmin=zmin, z_far=z_far, remove_invisible=remove_invisible, camera_type=camera_type)
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.shape != valid.shape \
                or keep.device != valid.device:
            raise ValueError(f"keep must be a bool mask {tuple(valid.shape)} on {valid.device}")
        valid = valid & keep
    return xyz, depth, valid


def disparity_to_cloud(disp: Tensor, K, baseline: float, image: Optional[Tensor] = None, *, denoise: bool = True,
                       nb_points: int = 30, radius: float = 0.03, scale: float = 1.0,
                       camera_type: str = "pinhole", remove_invisible: bool = True, zmin: float = 0.1,
                       z_far: float = 10.0, keep: Optional[Tensor] = None) -> List[Cloud]:
    """The demo's cloud (scripts/run_demo.py:173-275) per batch element.

    ``image``: (B,3,H,W), (B,H,W,3), (3,H,W) or (H,W,3) on the device of ``disp``; its values at the
    kept pixels become ``colors``.  ``denoise`` applies the radius outlier removal to the valid
    points; ``keep`` (``disparity_to_xyz``) takes pixels out of ``valid`` before it.  Everything queues on the current stream; the compaction ``xyz_map[inliers]`` is the one
    step that synchronises."""
    xyz, depth, valid = disparity_to_xyz(disp, K, baseline, scale=scale, camera_type=camera_type,
                                         remove_invisible=remove_invisible, zmin=zmin, z_far=z_far, keep=keep)
    B, H, W = depth.shape
    if image is not None:
        if image.dim() == 3:
            image = image[None]
        if image.dim() != 4 or image.shape[0] != B:
            raise ValueError(f"image {tuple(image.shape)} does not match disparity {(B, H, W)}")
        if image.shape[1] == 3 and image.shape[2:] == (H, W):
            image = image.permute(0, 2, 3, 1)
        if image.shape[1:] != (H, W, 3) or image.device != xyz.device:
            raise ValueError(f"image {tuple(image.shape)} on {image.device} does not match disparity {(B, H, W)}")
    out = []
    for b in range(B):
        inl = valid[b]
        if denoise:
            inl = ops.radius_outlier_mask(xyz[b].reshape(-1, 3), valid[b].reshape(-1), nb_points=nb_points,
                                          radius=radius).reshape(H, W)
        out.append(Cloud(points=xyz[b][inl], colors=image[b][inl] if image is not None else None,
                         xyz_map=xyz[b], depth=depth[b], valid=valid[b], inliers=inl))
    return out


def read_intrinsics(path) -> Tuple[np.ndarray, float]:
    """The reference's ``K.txt`` (scripts/run_demo.py:226-229): nine floats of the row-major 3x3
    intrinsic matrix on the first line, the baseline in metres on the second -> (K fp32 (3,3), baseline)."""
    with open(path) as f:
        lines = f.readlines()
    vals = [float(v) for v in lines[0].split()]
    if len(vals) != 9 or len(lines) < 2:
        raise ValueError(f"{path}: expected 9 intrinsics on line 1 and the baseline on line 2")
    return np.array(vals, dtype=np.float32).reshape(3, 3), float(lines[1])


def write_ply(path, points, colors=None) -> None:
    """Binary little-endian PLY: float x, y, z and, with ``colors``, uchar red, green, blue.

    ``points`` (M,3) and ``colors`` (M,3) are tensors or arrays; float colours are taken as [0, 1]
    (as Open3D stores them) and integer colours as [0, 255]."""
    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    pts = host(points).astype("<f4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}",
              "property float x", "property float y", "property float z"]
    if colors is not None:
        col = host(colors).reshape(-1, 3)
        if len(col) != len(pts):
            raise ValueError(f"write_ply: {len(pts)} points but {len(col)} colours")
        if col.dtype.kind == "f":
            col = np.rint(np.clip(col, 0.0, 1.0) * 255.0)
        col = np.clip(col, 0, 255).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header.append("end_header")
    rec = np.empty(len(pts), dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if colors is not None:
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())
