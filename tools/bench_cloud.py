#!/usr/bin/env python3
"""The point-cloud stage at the cfg2 size (640x480, B=1): ops.disp_to_xyz and ops.radius_outlier_mask
on the GPU against the same work in tests/cloud_oracle.py on the CPU (numpy fp64, cKDTree).

    python tools/bench_cloud.py [--out profiles/cloud_cfg2.json] [--reps 50] [--rounds 7] [--workers 16]

Synthetic scene: a slanted plane 0.8-2 m away with 5 % spiked pixels, fx = fy = 600, baseline 0.1 m,
the demo's defaults nb_points = 30, radius = 0.03.  Each GPU figure is the median over ``rounds`` of
(device-event span of ``reps`` back-to-back calls) / reps, after a warm-up; min and max are kept.
The whole working set (6.5 MB) stays in the Infinity Cache between calls, so the GB/s of the
unprojection is a rate for cache-resident data, not an HBM rate.  Needs a HIP device.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foundationstereo_amd import _lib, ops  # noqa: E402
from tests import cloud_oracle  # noqa: E402

H, W = 480, 640
FX = FY = 600.0
CX, CY = 319.5, 239.5
BASELINE = 0.1
PAIR_MS = 46.0          # README, round 6: one 640x480 pair through the model


def scene(seed=3):
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 30.0 + 0.05 * u + 0.03 * v
    rng = np.random.default_rng(seed)
    spike = rng.uniform(0, 1, d.shape) < 0.05
    return np.where(spike, d * rng.uniform(0.4, 2.5, d.shape), d).astype(np.float32)


def gpu_time(fn, reps, rounds):
    """ms per call: median / min / max over rounds of an event-timed batch of reps calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_cfg2.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--nb-points", type=int, default=30)
    ap.add_argument("--radius", type=float, default=0.03)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    disp_np = scene()
    disp = torch.from_numpy(disp_np).to(dev)[None]
    P = H * W
    res = {"shape": [1, H, W], "nb_points": a.nb_points, "radius": a.radius, "reps": a.reps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "pair_ms": PAIR_MS}

    # ---- unprojection
    def unproject():
        return ops.disp_to_xyz(disp, FX, FY, CX, CY, BASELINE)
    t = gpu_time(unproject, a.reps, a.rounds)
    t["algorithmic_bytes"] = 21 * P
    t["gb_per_s"] = 21 * P / (t["median_ms"] * 1e-3) / 1e9
    res["disp_to_xyz"] = t
    xyz, depth, valid = unproject()
    # the kernel alone: the same launch into fixed outputs, reps of it captured in one graph, so the
    # host's enqueue rate (three allocations and a ctypes call per op) is out of the figure
    v8 = valid.view(torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(a.reps):
                _lib.check(lib.fsmi_disp_to_xyz(disp.data_ptr(), xyz.data_ptr(), depth.data_ptr(), v8.data_ptr(), 1, H,
                                                W, FX, FY, CX, CY, BASELINE, 0.1, 10.0, 1, 0, side.cuda_stream), "xyz")
    torch.cuda.current_stream().wait_stream(side)
    g = gpu_time(graph.replay, 1, a.rounds)
    res["disp_to_xyz_kernel"] = {k: v / a.reps for k, v in g.items()}
    res["disp_to_xyz_kernel"]["gb_per_s"] = 21 * P / (res["disp_to_xyz_kernel"]["median_ms"] * 1e-3) / 1e9
    pts, vmask = xyz[0].reshape(-1, 3), valid[0].reshape(-1)

    # ---- radius mask: the whole path, then its stages on their own
    def mask():
        return ops.radius_outlier_mask(pts, vmask, nb_points=a.nb_points, radius=a.radius)
    res["radius_outlier_mask"] = gpu_time(mask, max(a.reps // 5, 2), a.rounds)
    s = torch.cuda.current_stream().cuda_stream
    keys = torch.empty(P, device=dev, dtype=torch.int64)
    vm8 = vmask.view(torch.uint8)

    def stage_keys():
        _lib.check(lib.fsmi_cloud_cell_keys(pts.data_ptr(), vm8.data_ptr(), keys.data_ptr(), P, a.radius, s), "keys")
    stage_keys()
    skeys, perm = torch.sort(keys)
    pts4 = torch.zeros((P, 4), device=dev)

    def stage_gather():
        pts4[:, :3] = pts.index_select(0, perm)
    stage_gather()
    keep = torch.empty(P, device=dev, dtype=torch.uint8)

    def stage_count():
        _lib.check(lib.fsmi_radius_count(skeys.data_ptr(), perm.data_ptr(), pts4.data_ptr(), keep.data_ptr(), P,
                                         a.radius, a.nb_points, s), "count")
    n = max(a.reps // 5, 2)
    res["stages"] = {"cell_keys": gpu_time(stage_keys, n, a.rounds),
                     "torch_sort": gpu_time(lambda: torch.sort(keys), n, a.rounds),
                     "gather": gpu_time(stage_gather, n, a.rounds),
                     "radius_count": gpu_time(stage_count, n, a.rounds)}
    # the count with the early exit out of reach: every candidate of the 27 cells is tested
    lim = 1 << 30

    def stage_count_full():
        _lib.check(lib.fsmi_radius_count(skeys.data_ptr(), perm.data_ptr(), pts4.data_ptr(), keep.data_ptr(), P,
                                         a.radius, lim, s), "count")
    res["stages"]["radius_count_no_early_exit"] = gpu_time(stage_count_full, 2, 3)

    # ---- does the mask path synchronise the host?  (torch warns once per synchronising call)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            gpu_keep = mask()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    res["mask_path_sync_warnings"] = [str(w.message)[:120] for w in caught
                                      if "prototype feature" not in str(w.message)]   # the mode's own notice
    gpu_keep = gpu_keep.cpu().numpy()

    # ---- the same work on the CPU
    t0 = time.perf_counter()
    oxyz, odepth, ovalid = cloud_oracle.xyz_oracle(disp_np, [[FX, 0, CX], [0, FY, CY], [0, 0, 1]], BASELINE)
    res["cpu_xyz_oracle_ms"] = (time.perf_counter() - t0) * 1e3
    pts_np, v_np = pts.cpu().numpy(), vmask.cpu().numpy()
    assert np.array_equal(v_np, ovalid.reshape(-1))
    cpu = []
    for _ in range(2):
        t0 = time.perf_counter()
        counts = cloud_oracle.radius_count_oracle(pts_np, float(np.float32(a.radius)), v_np, workers=a.workers)
        cpu.append((time.perf_counter() - t0) * 1e3)
    res["cpu_radius_ckdtree_ms"] = {"min_ms": min(cpu), "max_ms": max(cpu), "workers": a.workers}
    want, amb = cloud_oracle.radius_mask_oracle(pts_np, a.radius, a.nb_points, v_np, workers=a.workers)
    res["agreement"] = {"points": int(v_np.sum()), "inlier_share": float(want[v_np].mean()),
                        "mean_neighbours": float(counts[v_np].mean()), "ambiguous": int(amb.sum()),
                        "mismatches": int(((gpu_keep != want) & ~amb).sum())}
    stage_ms = res["disp_to_xyz"]["median_ms"] + res["radius_outlier_mask"]["median_ms"]
    res["stage_ms"] = stage_ms
    res["stage_over_pair"] = stage_ms / PAIR_MS
    res["speedup_radius_vs_ckdtree"] = min(cpu) / res["radius_outlier_mask"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
