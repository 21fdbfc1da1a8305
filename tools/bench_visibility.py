#!/usr/bin/env python3
"""The visibility stage (ops.disp_visibility: occlusion z-buffer and left-right check, one launch)
against the same classes from tests/visibility_oracle.py on host threads, with fsmi_disp_to_xyz at the
same shape as the yardstick: both are single-pass streams over a disparity map.

    python tools/bench_visibility.py [--out profiles/visibility_cfg2.json] [--reps 50] [--rounds 7] [--workers 16]

Shapes: 640x480 with B = 1 and B = 4, and 1536x1024 with B = 8.  Modes: occlusion only (4 B read and
1 B written per pixel) and occlusion plus left-right (8 B read, 1 B written); the kernel reads the left
map twice (splat, classify), the second time from cache, and the algorithmic bytes count it once.
``call`` is timed as tools/bench_frames.py times its ops: the median over ``rounds`` of (device-event
span of ``reps`` back-to-back calls) / reps after a warm-up, allocations included.  ``kernel`` is the
entry point alone into fixed outputs (the memset of the counts and the launch), ``reps`` of them
captured in one graph; ``disp_to_xyz_kernel`` likewise (21 B per pixel).  The maps of the two small
shapes stay in the Infinity Cache between calls, so their GB/s is a rate for cache-resident data.
The scene is a slanted background with a foreground box and 2 % invalid pixels; the right view is
its z-buffered forward warp with the holes filled from the background.  Needs a HIP device.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foundationstereo_amd import _lib, ops  # noqa: E402
from tests import visibility_oracle  # noqa: E402
from tools.bench_frames import HBM_PEAK, gpu_time, kernel_time  # noqa: E402


def scene(B, H, W, seed=3):
    """(left, right) disparities (B,H,W) fp32."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    bg = 0.02 * W + 0.01 * u + 0.005 * v
    left = np.repeat(bg[None], B, axis=0).astype(np.float32)
    rng = np.random.default_rng(seed)
    for b in range(B):
        y0, x0 = H // 4 + 3 * b, W // 3 + 5 * b
        left[b, y0:y0 + H // 2, x0:x0 + W // 4] = np.float32(0.08 * W)
    right = np.repeat((bg + 0.01 * 0.02 * W)[None], B, axis=0).astype(np.float32)       # the background, shifted
    c = np.clip(np.rint(u[None] - left), 0, W - 1).astype(np.int64)
    z = np.zeros((B * H, W), np.float32)
    rows = np.broadcast_to(np.arange(B * H)[:, None], (B * H, W))
    np.maximum.at(z, (rows, c.reshape(B * H, W)), left.reshape(B * H, W))
    z = z.reshape(B, H, W)
    right = np.where(z > 0, z, right).astype(np.float32)
    left[rng.uniform(0, 1, left.shape) < 0.02] = np.inf
    return left, right


def case(B, H, W, a, dev, lib):
    left_np, right_np = scene(B, H, W)
    left, right = torch.from_numpy(left_np).to(dev), torch.from_numpy(right_np).to(dev)
    P = B * H * W
    res = {"shape": [B, H, W]}
    classes = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    counts = torch.empty((B, ops.VIS_NCLASS), device=dev, dtype=torch.int64)
    for mode, r, r_np, per_px in (("occlusion", None, None, 5), ("occlusion_lr", right, right_np, 9)):
        got = ops.disp_visibility(left, r)
        cpu = []
        for _ in range(2):
            t0 = time.perf_counter()
            want = visibility_oracle.classify_oracle(left_np, r_np, workers=a.workers)
            cpu.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
        m = {"counts": want[1].sum(axis=0).tolist(),
             "call": gpu_time(lambda: ops.disp_visibility(left, r), a.reps, a.rounds),
             "kernel": kernel_time(
                 lambda s: _lib.check(lib.fsmi_disp_visibility(left.data_ptr(), r.data_ptr() if r is not None else None,
                                                               classes.data_ptr(), None, counts.data_ptr(), B, H, W,
                                                               1.0, 1.0, 1, s), "disp_visibility"),
                 a.reps, a.rounds, per_px * P + 8 * ops.VIS_NCLASS * B),
             "oracle_host_ms": {"min_ms": min(cpu), "max_ms": max(cpu), "workers": a.workers}}
        m["kernel"]["bytes_per_pixel"] = per_px
        m["speedup_vs_oracle_host"] = min(cpu) / m["call"]["median_ms"]
        res[mode] = m
    xyz = torch.empty((B, H, W, 3), device=dev)
    depth = torch.empty((B, H, W), device=dev)
    res["disp_to_xyz_kernel"] = kernel_time(
        lambda s: _lib.check(lib.fsmi_disp_to_xyz(left.data_ptr(), xyz.data_ptr(), depth.data_ptr(), classes.data_ptr(),
                                                  B, H, W, 600.0, 600.0, W / 2, H / 2, 0.1, 0.1, 10.0, 1, 0, s),
                             "disp_to_xyz"), a.reps, a.rounds, 21 * P)
    res["disp_to_xyz_kernel"]["bytes_per_pixel"] = 21
    for mode in ("occlusion", "occlusion_lr"):
        res[mode]["kernel_time_over_disp_to_xyz"] = res[mode]["kernel"]["median_ms"] / res["disp_to_xyz_kernel"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "visibility_cfg2.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visibility: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "b1_480x640": case(1, 480, 640, a, dev, lib), "b4_480x640": case(4, 480, 640, a, dev, lib),
           "b8_1024x1536": case(8, 1024, 1536, a, dev, lib)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
