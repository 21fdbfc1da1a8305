#!/usr/bin/env python3
"""The photometric consistency stage (ops.photo_consistency: warp, l1, 3x3 SSIM, row probe; two launches)
against a torch restatement on the same device tensors.

    python tools/bench_photometric.py [--out profiles/photometric_cfg2.json] [--reps 50] [--rounds 7]

Shapes: 640x480 with B = 1 and 1536x1024 with B = 8, C = 3, fp32 planar frames, the l1 and dssim maps
written, without and with a 5-offset row probe (-2 .. 2).  Per case and for both implementations:
``enqueue`` is the host time per call with no synchronise inside the window (what the calling thread
pays), ``call`` the device-event span of ``reps`` back-to-back calls / reps after a warm-up, allocations
included (tools/bench_frames.py's ``gpu_time``), both as the median over ``rounds``.  ``kernel`` is the
entry point alone into fixed outputs, ``reps`` of them captured in one graph, with its algorithmic
bytes: disp 4 + left 12 + right 12 read and l1 4 + dssim 4 written per pixel, 36 B; the probe adds none
(its rows are the neighbours' rows, already counted once), so its GB/s counts the same bytes over more
time.  The small shape stays in the Infinity Cache between calls: its GB/s is a rate for cache-resident
data.  The baseline: gather + lerp for the warp, ``avg_pool2d`` chains for the window moments
(E[xy] - E[x]E[y], the usual torch SSIM), boolean-mask means, one more gather pass per offset.  It is
checked against the kernel's table (1e-3 relative on the means; the one-pass variance is not the
kernel's centred one) before anything is timed.  Needs a HIP device.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from foundationstereo_amd import _lib, ops  # noqa: E402
from tools.bench_frames import HBM_PEAK, gpu_time, kernel_time  # noqa: E402

OFFSETS = (-2.0, -1.0, 0.0, 1.0, 2.0)
BYTES_PER_PIXEL = 36


def scene(B, H, W, seed=7):
    """(disp (B,H,W), left, right (B,3,H,W)) fp32: a textured frame, a slanted disparity with a foreground
    box, the right frame the left one resampled by the disparity's mean plus noise; 2 % invalid."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    tex = lambda x, y, c: 128 + 60 * np.sin(0.21 * x + 0.07 * y + c) + 40 * np.cos(0.13 * y - 0.03 * x + 2 * c)  # noqa: E731
    disp = np.repeat((0.02 * W + 0.01 * u + 0.005 * v)[None], B, axis=0).astype(np.float32)
    for b in range(B):
        y0, x0 = H // 4 + 3 * b, W // 3 + 5 * b
        disp[b, y0:y0 + H // 2, x0:x0 + W // 4] = np.float32(0.08 * W)
    left = np.stack([np.stack([tex(u, v, c) for c in range(3)]) for _ in range(B)])
    right = np.stack([np.stack([tex(u + 0.04 * W, v, c) for c in range(3)]) for _ in range(B)])
    left = np.clip(left + rng.normal(0, 4, left.shape), 0, 255).astype(np.float32)
    right = np.clip(right + rng.normal(0, 4, right.shape), 0, 255).astype(np.float32)
    disp[rng.uniform(0, 1, disp.shape) < 0.02] = np.inf
    return disp, left, right


def torch_baseline(disp, left, right, offsets=()):
    """(l1 mean, dssim mean, [row means]) per pair, (B) / (B,R) fp32 tensors: the torch sequence."""
    B, C, H, W = left.shape
    u = torch.arange(W, device=disp.device, dtype=torch.float32)
    xr = u - disp
    sampled = torch.isfinite(disp) & (disp > 0) & (xr >= 0)
    xs = torch.where(sampled, xr, torch.zeros_like(xr))
    x0 = xs.floor()
    t = (xs - x0)[:, None]
    i0 = x0.long()[:, None].expand(B, C, H, W)
    i1 = (i0 + 1).clamp(max=W - 1)

    def warp(img):
        a, b = img.gather(3, i0), img.gather(3, i1)
        return a + t * (b - a)

    def masked_mean(x, m):
        n = m.sum(dim=(1, 2))
        return torch.where(m, x, torch.zeros_like(x)).sum(dim=(1, 2)) / n.clamp(min=1)

    w = warp(right) * sampled[:, None]
    l1 = (left - w).abs().mean(dim=1)
    mx, my = F.avg_pool2d(left, 3, 1), F.avg_pool2d(w, 3, 1)
    vx = F.avg_pool2d(left * left, 3, 1) - mx * mx
    vy = F.avg_pool2d(w * w, 3, 1) - my * my
    cxy = F.avg_pool2d(left * w, 3, 1) - mx * my
    ssim = ((2 * mx * my + 6.5025) * (2 * cxy + 58.5225)) / ((mx * mx + my * my + 6.5025) * (vx + vy + 58.5225))
    ds = ((1 - ssim) * 0.5).clamp(0, 1).mean(dim=1)
    all_s = F.avg_pool2d(sampled[:, None].float(), 3, 1)[:, 0] == 1
    rows = []
    for dy in offsets:
        k = int(dy)
        v0, v1 = max(0, -k), min(H, H - k)
        src = right[:, :, v0 + k:v1 + k]        # rows v0 .. v1 of the left view against rows v0 + k .. v1 + k of the right frame
        a, b = src.gather(3, i0[:, :, v0:v1]), src.gather(3, i1[:, :, v0:v1])
        wk = a + t[:, :, v0:v1] * (b - a)
        rows.append(masked_mean((left[:, :, v0:v1] - wk).abs().mean(dim=1), sampled[:, v0:v1]))
    return masked_mean(l1, sampled), masked_mean(ds, all_s & sampled[:, 1:-1, 1:-1]), rows


def enqueue_time(fn, reps, rounds):
    """ms of host time per call, no synchronise inside the window."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
        torch.cuda.synchronize()
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def case(B, H, W, a, dev, lib):
    disp, left, right = (torch.from_numpy(x).to(dev) for x in scene(B, H, W))
    P = B * H * W
    res = {"shape": [B, 3, H, W], "bytes_per_pixel": BYTES_PER_PIXEL}
    for mode, offs in (("plain", ()), ("probe5", OFFSETS)):
        R = len(offs)
        table = ops.photo_consistency(disp, left, right, None, offs)[0]
        bl1, bds, brows = torch_baseline(disp, left, right, offs)
        got = table.cpu().numpy()
        want = np.stack([bl1.cpu().numpy(), bds.cpu().numpy()] + [r.cpu().numpy() for r in brows], axis=1)
        have = got[:, [4, 6] + [9 + 2 * k for k in range(R)]]
        assert np.allclose(have, want, rtol=1e-3, atol=1e-4), (mode, have, want)
        ws = torch.empty(int(lib.fsmi_photo_consistency_ws_bytes(B, H, W, R)) // 8, device=dev, dtype=torch.float64)
        tb, sm = torch.empty_like(table), torch.empty_like(table)
        l1, ds = torch.empty((B, H, W), device=dev), torch.empty((B, H, W), device=dev)
        coffs = (ctypes.c_float * max(R, 1))(*offs)

        def launch(s):
            _lib.check(lib.fsmi_photo_consistency(disp.data_ptr(), left.data_ptr(), right.data_ptr(), None, None,
                                                  l1.data_ptr(), ds.data_ptr(), tb.data_ptr(), sm.data_ptr(), ws.data_ptr(),
                                                  B, 3, H, W, 0, H * W, W, 3 * H * W, H * W, W, 3 * H * W, H * W, W, coffs, R,
                                                  0.85, 1, s), "photo_consistency")
        m = {"hip": {"enqueue": enqueue_time(lambda: ops.photo_consistency(disp, left, right, None, offs), a.reps, a.rounds),
                     "call": gpu_time(lambda: ops.photo_consistency(disp, left, right, None, offs), a.reps, a.rounds),
                     "kernel": kernel_time(launch, a.reps, a.rounds, BYTES_PER_PIXEL * P)},
             "torch": {"enqueue": enqueue_time(lambda: torch_baseline(disp, left, right, offs), a.reps, a.rounds),
                       "call": gpu_time(lambda: torch_baseline(disp, left, right, offs), a.reps, a.rounds)},
             "l1_mean": got[:, 4].tolist(), "dssim_mean": got[:, 6].tolist()}
        m["call_speedup_vs_torch"] = m["torch"]["call"]["median_ms"] / m["hip"]["call"]["median_ms"]
        m["enqueue_speedup_vs_torch"] = m["torch"]["enqueue"]["median_ms"] / m["hip"]["enqueue"]["median_ms"]
        res[mode] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "photometric_cfg2.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "b1_480x640": case(1, 480, 640, a, dev, lib), "b8_1024x1536": case(8, 1024, 1536, a, dev, lib)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
