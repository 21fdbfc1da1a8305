#!/usr/bin/env python3
"""The frame / picture stage at the cfg2 size (640x480, B=1): ops.frames_ingest against the torch
sequence of scripts/run_demo.py:156-159 on already-uploaded uint8 frames, and the device
vis_disparity against its numpy restatement (tests/frames_oracle.py) on the host, the D2H copy of the
disparity that the host path needs included.

    python tools/bench_frames.py [--out profiles/frames_cfg2.json] [--reps 50] [--rounds 7] [--workers 16]

Each GPU figure is the median over ``rounds`` of (device-event span of ``reps`` back-to-back calls) /
reps, after a warm-up; min and max are kept.  ``*_kernel`` figures are the launch alone into fixed
outputs, ``reps`` of it captured in one graph, so the host's enqueue rate is out of them; their
share of peak divides the kernel's algorithmic bytes by that time and by the 8 TB/s HBM peak.  The
working set (under 10 MB) stays in the Infinity Cache between calls, so these are rates for
cache-resident data, not HBM rates, and at this size a launch is as long as its floor of a few
microseconds: ``large_2160x3840`` repeats the kernel figures on a 4K frame (ingest: 275 MB per call).
640x480 needs no padding; the 630x470 case (pads 5/5, 5/5) is measured beside it.  Needs a HIP device.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foundationstereo_amd import _lib, frames, ops  # noqa: E402
from foundationstereo_amd.utils import InputPadder  # noqa: E402
from tests import frames_oracle  # noqa: E402

HBM_PEAK = 8.0e12       # B/s, spec
PAIR_MS = 46.0          # README, round 6: one 640x480 pair through the model


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


def kernel_time(launch, reps, rounds, nbytes):
    """``launch(stream)`` captured reps times in one graph -> ms per launch and its share of HBM peak."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(reps):
                launch(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    t = {k: v / reps for k, v in gpu_time(graph.replay, 1, rounds).items()}
    t["algorithmic_bytes"] = nbytes
    t["gb_per_s"] = nbytes / (t["median_ms"] * 1e-3) / 1e9
    t["share_of_hbm_peak"] = nbytes / (t["median_ms"] * 1e-3) / HBM_PEAK
    return t


def host_vis(disp, lut, workers):
    """vis_oracle with the rows of the colour step split over ``workers`` threads (numpy releases the GIL)."""
    valid = disp[~(np.isnan(disp) | np.isinf(disp))]
    mn, mx = valid.min(), valid.max()
    parts = np.array_split(np.arange(disp.shape[0]), workers)
    with ThreadPoolExecutor(workers) as ex:
        out = list(ex.map(lambda r: frames_oracle.vis_oracle(disp[r[0]:r[-1] + 1], lut, min_val=mn, max_val=mx), parts))
    return np.concatenate(out)


def ingest_case(H, W, a, dev, lib, resize=True):
    rng = np.random.default_rng(5)
    left = torch.from_numpy(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev)
    right = torch.from_numpy(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev)

    def ours():
        return ops.frames_ingest(left, right)

    def torch_seq():                                         # scripts/run_demo.py:156-159
        img0 = left.float().permute(0, 3, 1, 2)
        img1 = right.float().permute(0, 3, 1, 2)
        return InputPadder(img0.shape, divis_by=32).pad(img0, img1)
    batch, u8 = ours()
    p0, p1 = torch_seq()
    assert torch.equal(batch[:, 0], p0) and torch.equal(batch[:, 1], p1) and torch.equal(u8, left)
    Hp, Wp = batch.shape[-2:]
    pl, pr, pt, pb = InputPadder((H, W), divis_by=32)._pad
    nbytes = 2 * H * W * 3 + 2 * 3 * 4 * Hp * Wp + 3 * H * W
    res = {"shape": [1, H, W, 3], "padded": [Hp, Wp],
           "frames_ingest": gpu_time(ours, a.reps, a.rounds), "torch_sequence": gpu_time(torch_seq, a.reps, a.rounds)}
    res["frames_ingest_kernel"] = kernel_time(
        lambda s: _lib.check(lib.fsmi_frames_ingest(left.data_ptr(), right.data_ptr(), batch.data_ptr(), u8.data_ptr(),
                                                    1, H, W, 3, 1.0, H, W, pl, pr, pt, pb, 32, s), "ingest"),
        a.reps, a.rounds, nbytes)
    res["speedup_vs_torch_sequence"] = res["torch_sequence"]["median_ms"] / res["frames_ingest"]["median_ms"]
    if resize:
        # the resize path (--scale 0.5): no torch sequence to compare with (the reference resizes on the host)
        half = ops.frames_ingest(left, right, scale=0.5)
        res["frames_ingest_scale_0p5"] = gpu_time(lambda: ops.frames_ingest(left, right, scale=0.5), a.reps, a.rounds)
        res["frames_ingest_scale_0p5"]["padded"] = list(half[0].shape[-2:])
    return res


def picture_kernels(disp, img, lut, a, lib):
    """The three picture launches alone, at the size of ``disp`` (1,H,W)."""
    _, H, W = disp.shape
    P = H * W
    mm = ops.disp_minmax(disp)
    pic, pic2 = ops.disp_colorize(disp, mm, lut), ops.disp_colorize(disp, mm, lut, image=img)
    inf = float("inf")
    res = {"disp_minmax_kernel": kernel_time(
        lambda s: _lib.check(lib.fsmi_disp_minmax(disp.data_ptr(), mm.data_ptr(), 1, H, W, inf, s), "minmax"),
        a.reps, a.rounds, 4 * P + 8)}
    res["disp_minmax_kernel"]["note"] = "two launches: the (+inf, -inf) initialisation and the reduction"
    res["disp_colorize_kernel"] = kernel_time(
        lambda s: _lib.check(lib.fsmi_disp_colorize(disp.data_ptr(), mm.data_ptr(), lut.data_ptr(), None, pic.data_ptr(),
                                                    1, H, W, inf, s), "colorize"), a.reps, a.rounds, 7 * P + 768 + 8)
    res["disp_colorize_side_by_side_kernel"] = kernel_time(
        lambda s: _lib.check(lib.fsmi_disp_colorize(disp.data_ptr(), mm.data_ptr(), lut.data_ptr(), img.data_ptr(),
                                                    pic2.data_ptr(), 1, H, W, inf, s), "colorize"),
        a.reps, a.rounds, 13 * P + 768 + 8)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frames_cfg2.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, W = 480, 640
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "pair_ms": PAIR_MS,
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "ingest_640x480": ingest_case(H, W, a, dev, lib), "ingest_630x470": ingest_case(470, 630, a, dev, lib)}

    # ---- the picture
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(3)
    disp_np = (30.0 + 0.05 * u + 0.03 * v + rng.uniform(0, 1, (H, W))).astype(np.float32)
    disp_np[rng.uniform(0, 1, (H, W)) < 0.02] = np.inf
    disp = torch.from_numpy(disp_np).to(dev)[None]
    img = torch.from_numpy(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)).to(dev)
    lut = torch.from_numpy(frames.TURBO.copy()).to(dev)
    frames.vis_disparity(disp)                               # uploads the default table
    res["vis_disparity"] = gpu_time(lambda: frames.vis_disparity(disp), a.reps, a.rounds)
    res["vis_disparity_side_by_side"] = gpu_time(lambda: frames.vis_disparity(disp, image=img), a.reps, a.rounds)
    pic = ops.disp_colorize(disp, ops.disp_minmax(disp), lut)
    res.update(picture_kernels(disp, img, lut, a, lib))
    # the same kernels on a 4K frame: 8.3 Mpixel, a working set the launch latency no longer hides
    big = disp.repeat(1, 5, 6)[:, :2160].contiguous()
    big_img = img.repeat(1, 5, 6, 1)[:, :2160].contiguous()
    res["large_2160x3840"] = picture_kernels(big, big_img, lut, a, lib)
    res["large_2160x3840"]["ingest"] = ingest_case(2160, 3840, a, dev, lib, resize=False)

    # ---- the same picture on the host: D2H copy of the disparity, then numpy on `workers` threads
    want = host_vis(disp_np, frames.TURBO, a.workers)
    assert np.array_equal(pic[0].cpu().numpy(), want)
    cpu, copy = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = disp[0].cpu().numpy()
        t1 = time.perf_counter()
        host_vis(d, frames.TURBO, a.workers)
        cpu.append((time.perf_counter() - t0) * 1e3)
        copy.append((t1 - t0) * 1e3)
    res["host_vis_numpy"] = {"median_ms": statistics.median(cpu), "min_ms": min(cpu), "max_ms": max(cpu),
                             "d2h_copy_median_ms": statistics.median(copy), "workers": a.workers}
    res["speedup_vis_vs_host"] = res["host_vis_numpy"]["median_ms"] / res["vis_disparity"]["median_ms"]
    stage_ms = res["ingest_640x480"]["frames_ingest"]["median_ms"] + res["vis_disparity_side_by_side"]["median_ms"]
    res["stage_ms"] = stage_ms
    res["stage_over_pair"] = stage_ms / PAIR_MS
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
