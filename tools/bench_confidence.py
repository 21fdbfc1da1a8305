#!/usr/bin/env python3
"""The confidence stage (ops.disp_confidence, one launch) and the risk-coverage histogram
(ops.risk_coverage) against torch restatements on the same device tensors.

    python tools/bench_confidence.py [--out profiles/confidence_cfg2.json] [--reps 50] [--rounds 7]
                                     [--kernels_only] [--variant_json other.json] [--skip_model]

Shapes: 640x480 with one pair (D = 48, a 120x160 volume) and 1536x1024 with B = 8 (D = 104, 256x384),
up = 4, radius 1, the query a full-resolution disparity.  ``call`` is the median over ``rounds`` of
(device-event span of ``reps`` back-to-back calls) / reps after a warm-up, allocations included;
``wall`` the same span on the host clock, synchronised at both ends; ``kernel`` the entry point alone
into fixed outputs, ``reps`` of them captured in one graph, with the algorithmic bytes (logits once,
disp once, the four maps once) and their share of the HBM peak.  ``self_kernel`` is the same without a
query and ``mass_only_kernel`` with one output.  The 640x480 volume (3.7 MB) stays in the Infinity
Cache between calls, so its GB/s is a rate for cache-resident data.

``torch``: softmax over D, log for the entropy, the expectation and variance at quarter resolution,
then the distribution repeated to full resolution and multiplied by the trapezoid weight broadcast
over D for the mass -- what a user without the kernel writes.  It is the yardstick: the kernel must not
lose to it at any shape.

``risk``: ops.risk_coverage at 256 bins against torch.bucketize + scatter_add on the same maps, for a
uniform confidence and for one that puts every pixel into the top bin (same-address LDS atomics), and
the oracle ranking (conf = None).

``keep_logits``: run_hierachical of the hash-initialised 640x480 model (max_disp 192, 8 iterations) with
the flag off and on, host clock: the flag makes the second pass run the classifier it otherwise skips.

``--kernels_only`` times just the graph-captured entry points (for an A/B library named by FSMI_LIB);
``--variant_json`` embeds such a run's result under "variant".  Needs a HIP device.
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from foundationstereo_amd import _lib, ops  # noqa: E402
from tools.bench_frames import HBM_PEAK, gpu_time, kernel_time  # noqa: E402
from tools.bench_metrics import wall_time  # noqa: E402

RADIUS = 1.0


def torch_confidence(logits, disp, up=4, radius=RADIUS):
    B, D, h, w = logits.shape
    d = torch.arange(D, device=logits.device, dtype=torch.float32).view(1, D, 1, 1)
    p = torch.softmax(logits, dim=1)
    peak = p.amax(1)
    entropy = 1.0 + (p * torch.log(p.clamp_min(1e-38))).sum(1) / math.log(D)
    mu = (p * d).sum(1)
    var = (p * (d - mu[:, None]) ** 2).sum(1)
    big = lambda x: x.repeat_interleave(up, -2).repeat_interleave(up, -1)   # noqa: E731
    q = disp * (1.0 / up)
    wgt = (radius + 1.0 - (d - q[:, None]).abs()).clamp_(0.0, 1.0)          # (B,D,H,W)
    mass = (big(p) * wgt).sum(1)
    spread = torch.sqrt(big(var) + (big(mu) - q) ** 2)
    return mass, spread, big(peak), big(entropy)


def torch_risk(conf, pred, gt, nbins=256):
    B = pred.shape[0]
    valid = (gt > 0) & torch.isfinite(gt)
    e = (pred - gt).abs()
    sc = valid & torch.isfinite(pred) & (conf >= 0) & (conf <= 1)
    edges = torch.linspace(0, 1, nbins + 1, device=conf.device)[1:-1]
    bins = torch.bucketize(conf, edges, right=True).view(B, -1)
    q20 = (e.clamp_max(4096.0) * 1048576.0).long() * sc
    count = torch.zeros((B, nbins), device=conf.device, dtype=torch.int64).scatter_add_(1, bins, sc.view(B, -1).long())
    err = torch.zeros((B, nbins), device=conf.device, dtype=torch.int64).scatter_add_(1, bins, q20.view(B, -1))
    return count, err


def confidence_case(B, D, h, w, a, dev, lib):
    up = 4
    H, W = h * up, w * up
    g = torch.Generator(device="cpu").manual_seed(D)
    logits = (3.0 * torch.randn((B, D, h, w), generator=g)).to(dev)
    disp = (torch.rand((B, H, W), generator=g) * (D - 1) * up).to(dev)
    outs = [torch.empty((B, H, W), device=dev) for _ in range(4)]
    nbytes = 4 * (logits.numel() + 5 * B * H * W)

    def entry(query, nout):
        ptrs = [o.data_ptr() if i < nout else None for i, o in enumerate(outs)]
        return lambda s: _lib.check(lib.fsmi_disp_confidence(logits.data_ptr(), B, D, h, w,
                                                             disp.data_ptr() if query else None, up, 0.25, RADIUS, *ptrs, s),
                                    "disp_confidence")
    res = {"shape": [B, D, h, w], "up": up, "radius": RADIUS,
           "kernel": kernel_time(entry(True, 4), a.reps, a.rounds, nbytes),
           "self_kernel": kernel_time(entry(False, 4), a.reps, a.rounds, nbytes - 4 * B * H * W),
           "mass_only_kernel": kernel_time(entry(True, 1), a.reps, a.rounds, 4 * (logits.numel() + 2 * B * H * W))}
    if a.kernels_only:
        return res
    got = ops.disp_confidence(logits, disp, radius=RADIUS)
    want = torch_confidence(logits, disp)
    res["max_abs_diff_vs_torch"] = [float((x - y).abs().max()) for x, y in zip(got, want)]
    res["call"] = gpu_time(lambda: ops.disp_confidence(logits, disp, radius=RADIUS), a.reps, a.rounds)
    res["wall"] = wall_time(lambda: ops.disp_confidence(logits, disp, radius=RADIUS), a.reps, a.rounds)
    treps = max(a.reps // 10, 3)
    res["torch"] = gpu_time(lambda: torch_confidence(logits, disp), treps, min(a.rounds, 3))
    res["torch_wall"] = wall_time(lambda: torch_confidence(logits, disp), treps, min(a.rounds, 3))
    res["call_speedup_vs_torch"] = res["torch"]["median_ms"] / res["call"]["median_ms"]
    res["wall_speedup_vs_torch"] = res["torch_wall"]["median_ms"] / res["wall"]["median_ms"]
    return res


def risk_case(B, H, W, a, dev, lib, nbins=256):
    g = torch.Generator(device="cpu").manual_seed(H)
    gt = (torch.rand((B, H, W), generator=g) * 190.0 + 0.5).to(dev)
    pred = gt + torch.randn((B, H, W), generator=g).to(dev) * 2.0
    uniform = torch.rand((B, H, W), generator=g).to(dev)
    top = torch.full((B, H, W), 0.9999, device=dev)
    count = torch.empty((B, nbins), device=dev, dtype=torch.int64)
    err = torch.empty_like(count)
    dropped = torch.empty((B,), device=dev, dtype=torch.int64)
    P = B * H * W

    def entry(conf):
        return lambda s: _lib.check(lib.fsmi_risk_coverage(conf.data_ptr() if conf is not None else None, pred.data_ptr(),
                                                           gt.data_ptr(), None, B, H, W, nbins, nbins / 16.0,
                                                           count.data_ptr(), err.data_ptr(), dropped.data_ptr(), s),
                                    "risk_coverage")
    res = {"shape": [B, H, W], "nbins": nbins,
           "uniform_kernel": kernel_time(entry(uniform), a.reps, a.rounds, 12 * P + 16 * nbins * B),
           "one_bin_kernel": kernel_time(entry(top), a.reps, a.rounds, 12 * P + 16 * nbins * B),
           "oracle_kernel": kernel_time(entry(None), a.reps, a.rounds, 8 * P + 16 * nbins * B)}
    res["one_bin_over_uniform"] = res["one_bin_kernel"]["median_ms"] / res["uniform_kernel"]["median_ms"]
    if a.kernels_only:
        return res
    for name, conf in (("uniform", uniform), ("one_bin", top)):
        got, want = ops.risk_coverage(conf, pred, gt, None, nbins), torch_risk(conf, pred, gt, nbins)
        res[name + "_equals_torch"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
        res[name + "_call"] = gpu_time(lambda: ops.risk_coverage(conf, pred, gt, None, nbins), a.reps, a.rounds)
        treps = max(a.reps // 10, 3)
        res[name + "_torch"] = gpu_time(lambda: torch_risk(conf, pred, gt, nbins), treps, min(a.rounds, 3))
        res[name + "_call_speedup_vs_torch"] = res[name + "_torch"]["median_ms"] / res[name + "_call"]["median_ms"]
    return res


def keep_logits_case(a, dev):
    from foundationstereo_amd import synth
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    model = FoundationStereo(synth.make_args(max_disp=192, vit_size="vits")).eval()
    synth.init_module_(model, seed=1234)
    model = model.to(dev)
    for size in ((480, 640), (256, 320)):                # the full pass, and the half-size one padded to 32s
        fl, fr, vf = synth.backbone_features(1, size[0], size[1], "vits", shift_px=2)
        model.feature.set_features([torch.from_numpy(x).to(dev) for x in fl], [torch.from_numpy(x).to(dev) for x in fr],
                                   torch.from_numpy(vf).to(dev), size=size)
    g = torch.Generator(device="cpu").manual_seed(1)
    left, right = (torch.rand((1, 3, 480, 640), generator=g).to(dev) * 255.0 for _ in range(2))
    res = {"shape": [1, 3, 480, 640], "max_disp": 192, "iters": 8}
    with torch.no_grad():
        for flag in (False, True):
            model.keep_logits = flag
            res["hiera_wall_flag_" + ("on" if flag else "off")] = wall_time(
                lambda: model.run_hierachical(left, right, iters=8, test_mode=True), 3, 5)
            res["forward_wall_flag_" + ("on" if flag else "off")] = wall_time(
                lambda: model(left, right, iters=8, test_mode=True), 3, 5)
    res["hiera_cost_ms"] = res["hiera_wall_flag_on"]["median_ms"] - res["hiera_wall_flag_off"]["median_ms"]
    res["forward_cost_ms"] = res["forward_wall_flag_on"]["median_ms"] - res["forward_wall_flag_off"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "confidence_cfg2.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels_only", action="store_true")
    ap.add_argument("--variant_json", default=None)
    ap.add_argument("--variant_note", default="")
    ap.add_argument("--skip_model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_confidence: needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "library": os.path.basename(_lib.library_path()),
           "confidence": {"b1_480x640_d48": confidence_case(1, 48, 120, 160, a, dev, lib),
                          "b8_1024x1536_d104": confidence_case(8, 104, 256, 384, a, dev, lib)},
           "risk": {"b1_480x640": risk_case(1, 480, 640, a, dev, lib), "b8_1024x1536": risk_case(8, 1024, 1536, a, dev, lib)}}
    if not (a.kernels_only or a.skip_model):
        res["keep_logits"] = keep_logits_case(a, dev)
    if a.variant_json:
        with open(a.variant_json) as f:
            res["variant"] = {"note": a.variant_note, "result": json.load(f)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
