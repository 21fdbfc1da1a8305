#!/usr/bin/env python3
"""The sequence-scoring stage (ops.seq_metrics: K refinement iterations and the initial disparity in one
call) against the two ways of getting the same figures without it.

    python tools/bench_seq.py [--out profiles/seq_cfg2.json] [--reps 20] [--rounds 7]

Shapes: 640x480 with K = 32 and the initial disparity at 160x120, B = 1 and B = 4; 1536x1024 with
K = 32, B = 8.  Three timings of one call, each enqueued (device-event span of ``reps`` back-to-back calls
/ reps, allocations included, as tools/bench_metrics.py) and wall (perf_counter span, synchronised at
both ends, with ONE read-back per call where the method allows it):
  seq_metrics         (a) the new call
  disp_metrics_loop   (b) K + 1 calls of ops.disp_metrics on contiguous maps, the initial one after
                          F.interpolate and a multiplication
  torch_sequence      (c) a torch restatement of train/losses.py:379-498 with its ``.item()`` calls (wall only)
``seq_metrics_kernels`` is the launches alone into fixed outputs, ``reps`` of them captured in one graph;
its algorithmic bytes are (R + 1) * P * 4 (every row and the ground truth once) plus the mask.  Needs a
HIP device.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from foundationstereo_amd import _lib, ops  # noqa: E402
from tools.bench_frames import HBM_PEAK, gpu_time, kernel_time  # noqa: E402
from tools.bench_metrics import wall_time  # noqa: E402

THRESHOLDS = (1.0, 3.0)
GAMMA, MAX_DISP = 0.9, 192.0


def torch_sequence(init, preds, gt, mask):
    """train/losses.py:379-498 per pair, with the reference's read-backs; returns the per-pair totals."""
    out = []
    K = len(preds)
    for b in range(gt.shape[0]):
        g, m = gt[b], mask[b]
        p0 = init[b]
        if p0.shape != g.shape:
            p0 = F.interpolate(p0[None, None], size=g.shape, mode="bilinear", align_corners=False)[0, 0]
        p0 = torch.clamp(p0, 0, MAX_DISP)
        d0 = torch.abs(p0 - g)
        sl1 = torch.where(d0 < 1.0, 0.5 * d0.square(), d0 - 0.5)
        loss0 = sl1[m].mean() if m.sum() > 0 else torch.tensor(0.0, device=g.device)
        it = torch.tensor(0.0, device=g.device)
        figures = []
        for k, p in enumerate(preds):
            d = torch.abs(torch.clamp(p[b], 0, MAX_DISP) - g)
            w = GAMMA ** (K - (k + 1))
            it = it + w * (d[m].mean() if m.sum() > 0 else torch.tensor(0.0, device=g.device))
            if m.sum() > 0:
                figures.append((d[m].mean().item(), (d[m] > 3.0).float().mean().item(), (d[m] > 1.0).float().mean().item()))
        if m.sum() > 0:
            figures.append((d0[m].mean().item(), (d0[m] > 3.0).float().mean().item(), (d0[m] > 1.0).float().mean().item()))
        out.append((loss0 + it).item())
    return out


def case(B, H, W, K, init_hw, a, dev, lib, bandwidth):
    rng = np.random.default_rng(B * 1000 + H)
    gt_np = rng.uniform(0.5, 190.0, (B, H, W)).astype(np.float32)
    gt_np[rng.uniform(0, 1, (B, H, W)) < 0.1] = 0.0
    gt = torch.from_numpy(gt_np).to(dev)
    preds = [(gt + torch.randn(gt.shape, device=dev) * (4.0 * 0.9 ** k)).contiguous() for k in range(K)]
    init = torch.from_numpy(rng.uniform(0.5, 190.0, (B,) + init_hw).astype(np.float32)).to(dev)
    mask = gt > 0
    w = [1.0] + [GAMMA ** (K - (k + 1)) for k in range(K)]
    rows = [init] + preds
    R = len(rows)

    def ours():
        return ops.seq_metrics(rows, gt, None, THRESHOLDS, MAX_DISP, 1.0, w, (0,))

    def loop():
        up = init if init_hw == (H, W) else F.interpolate(init[:, None], size=(H, W), mode="bilinear",
                                                           align_corners=False)[:, 0]
        return [ops.disp_metrics(torch.clamp(p, 0, MAX_DISP), gt, None, THRESHOLDS)[0] for p in [up] + preds]

    table, sums, loss = ours()
    ref = torch_sequence(init, preds, gt, mask)
    assert np.allclose(loss.cpu().numpy(), ref, rtol=1e-4), (loss, ref)          # the torch sequence sums in fp32
    one = torch.stack(loop()).cpu().numpy()                                      # (R,B,17)
    assert np.allclose(table[:, :, 1].cpu().numpy().T, one[:, :, 1], rtol=1e-5)

    nb = ops.seq_metrics_blocks(H, W, R)
    partials = torch.empty((B, R, nb, ops.SEQ_NACC), device=dev, dtype=torch.float64)
    keep = [p for p in rows]
    parr, _k = _lib.ptr_array([p.data_ptr() for p in keep])
    LL, CI, CF, CD = ctypes.c_longlong * R, ctypes.c_int * R, ctypes.c_float * R, ctypes.c_double * R
    args = (parr, LL(*[p.stride(0) for p in keep]), LL(*[p.stride(1) for p in keep]), CI(*[p.shape[1] for p in keep]),
            CI(*[p.shape[2] for p in keep]), CF(*([1.0] * R)), CF(*([MAX_DISP] * R)), CD(*w), bytes([1] + [0] * K), R)
    thr = (ctypes.c_float * 2)(*THRESHOLDS)
    P = H * W
    nbytes = B * (K * P * 4 + init_hw[0] * init_hw[1] * 4 + P * 4)              # no mask here: validity from gt
    res = {"shape": [B, H, W], "K": K, "init": list(init_hw), "rows": R, "blocks_per_pair_and_row": nb,
           "seq_metrics": gpu_time(ours, a.reps, a.rounds),
           "seq_metrics_wall": wall_time(lambda: ours()[0].cpu(), a.reps, a.rounds),
           "disp_metrics_loop": gpu_time(loop, a.reps, a.rounds),
           "disp_metrics_loop_wall": wall_time(lambda: torch.stack(loop()).cpu(), a.reps, a.rounds),
           "torch_sequence_wall": wall_time(lambda: torch_sequence(init, preds, gt, mask), max(a.reps // 10, 2), 3)}
    k = kernel_time(
        lambda s: _lib.check(lib.fsmi_seq_metrics(*args, gt.data_ptr(), None, None, thr, 2, 1000.0, 1.0,
                                                  partials.data_ptr(), sums.data_ptr(), table.data_ptr(),
                                                  loss.data_ptr(), B, H, W, s), "seq_metrics"),
        a.reps, a.rounds, nbytes)
    if not bandwidth:                                                            # launch-bound: a rate would mislead
        k.pop("gb_per_s")
        k.pop("share_of_hbm_peak")
    else:
        k["tb_per_s"] = k["gb_per_s"] / 1e3
    k["note"] = f"{(R + 31) // 32} streaming launch(es) of up to 32 rows and the per-pair finalize"
    res["seq_metrics_kernels"] = k
    for key in ("seq_metrics", "seq_metrics_wall", "disp_metrics_loop", "disp_metrics_loop_wall", "torch_sequence_wall",
                "seq_metrics_kernels"):
        res[key]["median_us"] = res[key]["median_ms"] * 1e3
    res["enqueued_speedup_vs_disp_metrics_loop"] = res["disp_metrics_loop"]["median_ms"] / res["seq_metrics"]["median_ms"]
    res["wall_speedup_vs_disp_metrics_loop"] = (res["disp_metrics_loop_wall"]["median_ms"] /
                                                res["seq_metrics_wall"]["median_ms"])
    res["wall_speedup_vs_torch_sequence"] = res["torch_sequence_wall"]["median_ms"] / res["seq_metrics_wall"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seq_cfg2.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seq: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "thresholds": list(THRESHOLDS), "gamma": GAMMA, "max_disparity": MAX_DISP,
           "b1_480x640": case(1, 480, 640, 32, (120, 160), a, dev, lib, False),
           "b4_480x640": case(4, 480, 640, 32, (120, 160), a, dev, lib, False),
           "b8_1024x1536": case(8, 1024, 1536, 32, (1024, 1536), a, dev, lib, True)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
