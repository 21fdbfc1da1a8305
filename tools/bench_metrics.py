#!/usr/bin/env python3
"""The scoring stage (ops.disp_metrics: EPE, RMSE, D1, K = 3 bad-pixel rates and the prediction's
statistics per pair) against the torch sequence of train/utils.py:106-141 on the same device tensors.

    python tools/bench_metrics.py [--out profiles/metrics_cfg2.json] [--reps 50] [--rounds 7]

Shapes: 640x480 with B = 1 and B = 4, and 1536x1024 with B = 8.  ``disp_metrics`` is timed as
tools/bench_frames.py times its ops: the median over ``rounds`` of (device-event span of ``reps``
back-to-back calls) / reps after a warm-up, allocations included; ``disp_metrics_kernels`` is the two
launches alone into fixed outputs, ``reps`` of them captured in one graph.  The torch sequence reads
``4 + K`` scalars back per pair, so its cost is wall time: ``torch_sequence`` is
(perf_counter span of ``reps`` calls, synchronised at both ends) / reps, and ``disp_metrics_wall`` is the
HIP path measured the same way with ONE read-back of the table per call, which is what a caller who
wants Python floats pays.  At 640x480 the pass moves under 3 MB and a launch is as long as its floor
of a few microseconds: microseconds are the figure there; GB/s is reported for the large shape only
(8 B read per pixel: prediction and ground truth).  Needs a HIP device.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foundationstereo_amd import _lib, ops  # noqa: E402
from tools.bench_frames import HBM_PEAK, gpu_time, kernel_time  # noqa: E402

THRESHOLDS = (1.0, 3.0, 5.0)


def torch_sequence(pred, gt, mask, thresholds=THRESHOLDS):
    """train/utils.py:106-141: a Python loop over the pairs; per pair a mask count, a boolean-mask gather
    and one ``.item()`` per figure.  Returns the per-pair (epe, rmse, rates) rows."""
    rows = []
    for b in range(pred.shape[0]):
        if mask[b].sum() == 0:
            rows.append([0.0] * (2 + len(thresholds)))
            continue
        err = torch.abs(pred[b] - gt[b])[mask[b]]
        row = [err.mean().item(), torch.sqrt((err ** 2).mean()).item()]
        for t in thresholds:
            row.append((err > t).float().mean().item())
        rows.append(row)
    return rows


def wall_time(fn, reps, rounds):
    for _ in range(3):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def case(B, H, W, a, dev, lib, bandwidth):
    rng = np.random.default_rng(B * 1000 + H)
    gt_np = rng.uniform(0.5, 190.0, (B, H, W)).astype(np.float32)
    gt_np[rng.uniform(0, 1, (B, H, W)) < 0.1] = 0.0
    noise = rng.standard_normal((B, H, W)) * np.where(rng.uniform(0, 1, (B, H, W)) < 0.2, 6.0, 0.6)
    pred, gt = torch.from_numpy((gt_np + noise).astype(np.float32)).to(dev), torch.from_numpy(gt_np).to(dev)
    mask = gt > 0

    table, sums, _ = ops.disp_metrics(pred, gt)
    ref = np.array(torch_sequence(pred, gt, mask))
    got = table[:, [1, 2, 9, 10, 11]].cpu().numpy()
    assert np.allclose(got, ref, rtol=1e-4, atol=0), (got, ref)          # the torch sequence sums in fp32

    nb = ops.disp_metrics_blocks(H, W)
    partials = torch.empty((B, nb, ops.METRICS_NACC), device=dev, dtype=torch.float64)
    import ctypes
    thr = (ctypes.c_float * 3)(*THRESHOLDS)
    nbytes = 8 * B * H * W + 2 * 8 * ops.METRICS_NACC * B * nb + 2 * 8 * ops.METRICS_NACC * B
    res = {"shape": [B, H, W], "thresholds": list(THRESHOLDS), "blocks_per_pair": nb,
           "disp_metrics": gpu_time(lambda: ops.disp_metrics(pred, gt), a.reps, a.rounds),
           "disp_metrics_wall": wall_time(lambda: ops.disp_metrics(pred, gt)[0].cpu(), a.reps, a.rounds),
           "torch_sequence": wall_time(lambda: torch_sequence(pred, gt, mask), a.reps, a.rounds)}
    k = kernel_time(
        lambda s: _lib.check(lib.fsmi_disp_metrics(pred.data_ptr(), gt.data_ptr(), None, None, thr, 3, 1000.0,
                                                   partials.data_ptr(), sums.data_ptr(), table.data_ptr(), None,
                                                   B, H, W, s), "disp_metrics"), a.reps, a.rounds, nbytes)
    if not bandwidth:                                                    # launch-bound: a rate would mislead
        k.pop("gb_per_s")
        k.pop("share_of_hbm_peak")
    k["note"] = "two launches: the streaming pass and the per-pair finalize"
    res["disp_metrics_kernels"] = k
    for key in ("disp_metrics", "disp_metrics_wall", "torch_sequence", "disp_metrics_kernels"):
        res[key]["median_us"] = res[key]["median_ms"] * 1e3
    res["torch_sequence_host_syncs_per_call"] = B * (1 + 2 + len(THRESHOLDS))
    res["wall_speedup_vs_torch_sequence"] = res["torch_sequence"]["median_ms"] / res["disp_metrics_wall"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics_cfg2.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "b1_480x640": case(1, 480, 640, a, dev, lib, False), "b4_480x640": case(4, 480, 640, a, dev, lib, False),
           "b8_1024x1536": case(8, 1024, 1536, a, dev, lib, True)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
