#!/usr/bin/env python3
"""Generate golden vectors by running the REFERENCE modules on the CPU.

Runs only in the build container (``/root/reference`` is absent on the GPU
box).  Inputs and weights come from ``foundationstereo_amd.synth`` (hash PRNG),
so only outputs and small per-op inputs are stored; tests regenerate the rest.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens.py

Writes ``tests/golden/*.npz`` and ``tests/golden/state_dict_*.json``.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from foundationstereo_amd import synth  # noqa: E402
from ref_harness import import_reference, import_reference_extractor, make_synthetic_feature_class  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
torch.set_num_threads(8)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def ops_small(sm, geo_mod, ut):
    g = {}
    # a1: gwc volume, border case D close to W
    for tag, (B, C, G, H, W, D) in {"a": (2, 32, 8, 4, 24, 8), "b": (1, 64, 8, 3, 16, 16)}.items():
        fl = synth.normal(synth.name_seed(f"gwcL{tag}"), (B, C, H, W))
        fr = synth.normal(synth.name_seed(f"gwcR{tag}"), (B, C, H, W))
        out = sm.build_gwc_volume(t(fl), t(fr), D, G)
        g[f"gwc_{tag}_fl"], g[f"gwc_{tag}_fr"], g[f"gwc_{tag}_out"] = fl, fr, out.numpy()
        g[f"gwc_{tag}_meta"] = np.array([B, C, G, H, W, D])
    # a2: concat volume
    B, C, H, W, D = 2, 12, 4, 24, 8
    pl = synth.normal(synth.name_seed("catL"), (B, C, H, W))
    pr = synth.normal(synth.name_seed("catR"), (B, C, H, W))
    g["concat_pl"], g["concat_pr"] = pl, pr
    g["concat_out"] = sm.build_concat_volume(t(pl), t(pr), D).numpy()
    g["concat_meta"] = np.array([B, C, H, W, D])
    # a4: softmax + regression
    logits = synth.normal(synth.name_seed("reg"), (2, 16, 4, 6), std=3.0)
    prob = torch.softmax(t(logits), 1)
    g["reg_logits"] = logits
    g["reg_prob"] = prob.numpy()
    g["reg_out"] = sm.disparity_regression(prob, 16).numpy()
    # a9: context upsample
    dl = synth.normal(synth.name_seed("upd"), (2, 1, 4, 6), std=5.0)
    w = torch.softmax(t(synth.normal(synth.name_seed("upw"), (2, 9, 16, 24))), 1)
    g["up_disp"], g["up_w"] = dl, w.numpy()
    g["up_out"] = sm.context_upsample(t(dl), w).numpy()
    # a5/a6: geometry encoding init + lookup, L in {2,4}; border cases in disp
    for L in (2, 4):
        B, C, Cv, D, H, W = 2, 32, 28, 16, 4, 24
        f1 = synth.normal(synth.name_seed(f"geo1_{L}"), (B, C, H, W))
        f2 = synth.normal(synth.name_seed(f"geo2_{L}"), (B, C, H, W))
        vol = synth.normal(synth.name_seed(f"geov_{L}"), (B, Cv, D, H, W))
        disp = synth.uniform(synth.name_seed(f"geod_{L}"), (B, 1, H, W), -6.0, D + 6.0)
        disp[0, 0, 0, :4] = [0.0, 3.0, D - 1.0, -4.0]     # exact integers / far outside
        disp[0, 0, 1, :3] = [D + 4.0, 0.5, 1e-3]
        dx = torch.linspace(-4, 4, 9).reshape(1, 1, 9, 1)
        ge = geo_mod.Combined_Geo_Encoding_Volume(t(f1), t(f2), t(vol), num_levels=L, dx=dx)
        coords = torch.arange(W, dtype=torch.float).reshape(1, 1, W, 1).repeat(B, H, 1, 1)
        out = ge(t(disp), coords)
        p = f"geo{L}_"
        g[p + "f1"], g[p + "f2"], g[p + "vol"], g[p + "disp"] = f1, f2, vol, disp
        g[p + "out"] = out.numpy()
        g[p + "corr"] = geo_mod.Combined_Geo_Encoding_Volume.corr(t(f1), t(f2)).numpy()
        for i, c in enumerate(ge.init_corr_pyramid):
            g[p + f"corrpyr{i}"] = c.numpy()
        g[p + "volpyr1"] = ge.geo_volume_pyramid[1].numpy()
    # bilinear_sampler 1-D (utils.py:44-55)
    img = synth.normal(synth.name_seed("bs_img"), (6, 3, 1, 11))
    x = synth.uniform(synth.name_seed("bs_x"), (6, 1, 9, 1), -2.0, 12.0)
    coords = np.concatenate([x, np.zeros_like(x)], -1)
    g["bs_img"], g["bs_coords"] = img, coords
    g["bs_out"] = ut.bilinear_sampler(t(img), t(coords)).numpy()
    np.savez_compressed(os.path.join(OUT, "ops_small.npz"), **g)
    print("ops_small", sum(v.nbytes for v in g.values()) / 1e6, "MB raw")


def update_step(up_mod):
    args = synth.make_args(max_disp=64, corr_levels=2)
    blk = up_mod.BasicSelectiveMultiUpdateBlock(args, 128, volume_dim=28).eval()
    synth.init_module_(blk, seed=77)
    B, H, W = 1, 8, 12
    cor_planes = 2 * 9 * 29
    sizes = [(H, W), (H // 2, W // 2), (H // 4, W // 4)]
    net = [synth.normal(synth.name_seed(f"net{i}"), (B, 128) + s, 0.5) for i, s in enumerate(sizes)]
    inp = [np.abs(synth.normal(synth.name_seed(f"inp{i}"), (B, 128) + s, 0.5)) for i, s in enumerate(sizes)]
    att = [synth.uniform(synth.name_seed(f"att{i}"), (B, 1) + s) for i, s in enumerate(sizes)]
    corr = synth.normal(synth.name_seed("ucorr"), (B, cor_planes, H, W), 0.5)
    disp = synth.uniform(synth.name_seed("udisp"), (B, 1, H, W), 0.0, 16.0)
    with torch.no_grad():
        onet, mask, delta = blk([t(x) for x in net], [t(x) for x in inp], t(corr), t(disp), [t(x) for x in att])
    g = {"disp": disp, "corr": corr, "mask": mask.numpy(), "delta": delta.numpy()}
    for i in range(3):
        g[f"net{i}"], g[f"inp{i}"], g[f"att{i}"], g[f"onet{i}"] = net[i], inp[i], att[i], onet[i].numpy()
    np.savez_compressed(os.path.join(OUT, "update_step.npz"), **g)
    print("update_step done")


E2E_CASES = {
    # name: (H, W, max_disp, iters, vit, corr_levels, shift)
    "e2e_tiny": (64, 96, 32, 4, "vits", 2, 2),
    "e2e_cfg1_L2": (256, 320, 64, 8, "vits", 2, 6),
    "e2e_cfg1_L4": (256, 320, 64, 8, "vits", 4, 6),
}


def e2e(fs):
    Syn = make_synthetic_feature_class(synth.feature_dims)
    fs.Feature = Syn
    for name, (H, W, md, iters, vit, L, shift) in E2E_CASES.items():
        args = synth.make_args(max_disp=md, corr_levels=L, vit_size=vit)
        model = fs.FoundationStereo(args).eval()
        synth.init_module_(model, seed=1234)
        fl, fr, vf = synth.backbone_features(1, H, W, vit, shift_px=shift)
        left, right = synth.stereo_images(1, H, W)
        model.feature.preset = ([t(x) for x in fl], [t(x) for x in fr], t(vf))
        cap = {}

        orig_call = fs.Combined_Geo_Encoding_Volume.__call__

        def hook(self, disp, coords, low_memory=False):
            out = orig_call(self, disp, coords, low_memory)
            if "geo0" not in cap:
                cap["geo0"] = out.detach().clone()
                cap["init_disp"] = disp.detach().clone()
            return out

        fs.Combined_Geo_Encoding_Volume.__call__ = hook
        try:
            with torch.no_grad():
                out = model(t(left), t(right), iters=iters, test_mode=True)
        finally:
            fs.Combined_Geo_Encoding_Volume.__call__ = orig_call
        g = {"disp": out.numpy(), "init_disp": cap["init_disp"].numpy(),
             "geo0_sum": np.float64(cap["geo0"].double().sum()),
             "geo0_abs": np.float64(cap["geo0"].double().abs().sum()),
             "geo0_row": cap["geo0"][0, :, 3, :].numpy(),
             "meta": np.array([H, W, md, iters, L, shift])}
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
        print(name, "disp mean", float(out.mean()), "init mean", float(cap["init_disp"].mean()))
        if name == "e2e_tiny":
            for v in ("vits", "vitl"):
                a2 = synth.make_args(max_disp=192, corr_levels=4, vit_size=v)
                m2 = fs.FoundationStereo(a2)
                keys = [[k, list(p.shape)] for k, p in m2.state_dict().items()]
                with open(os.path.join(OUT, f"state_dict_{v}.json"), "w") as f:
                    json.dump(keys, f)


# name: (H, W, max_disp, iters, vit, corr_levels, shift): both passes need /32 padding, so the
# reference's ``+= padder._pad[0]`` (core/foundation_stereo.py:270) is exercised (_pad[0] = 10)
HIERA_CASES = {"hiera_small": (200, 300, 64, 4, "vits", 2, 3)}


def hiera(fs):
    """run_hierachical (core/foundation_stereo.py:257-274) with the backbone stand-in synthesising
    features at each pass's padded size (as the product's SyntheticFeature does unpreset)."""
    Syn = make_synthetic_feature_class(synth.feature_dims)
    fs.Feature = Syn
    for name, (H, W, md, iters, vit, L, shift) in HIERA_CASES.items():
        args = synth.make_args(max_disp=md, corr_levels=L, vit_size=vit)
        model = fs.FoundationStereo(args).eval()
        synth.init_module_(model, seed=1234)
        model.feature.by_size = (vit, shift)
        left, right = synth.stereo_images(1, H, W)
        cap = []
        orig_fwd = fs.FoundationStereo.forward

        def fwd(self, *a, **k):
            out = orig_fwd(self, *a, **k)
            cap.append(out.detach().clone())
            return out

        fs.FoundationStereo.forward = fwd
        try:
            with torch.no_grad():
                out = model.run_hierachical(t(left), t(right), iters=iters, test_mode=True)
        finally:
            fs.FoundationStereo.forward = orig_fwd
        g = {"disp": out.numpy(), "disp_small_padded": cap[0].numpy(),
             "meta": np.array([H, W, md, iters, L, shift])}
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
        print(name, "disp", tuple(out.shape), "mean", float(out.mean()))


BACKBONE_CASES = {
    # name: (encoder, input shape) -- DepthAnythingFeature on an already /14 input
    "dav2_vits": ("vits", (2, 3, 56, 70)),
    "dav2_vitl": ("vitl", (1, 3, 28, 42)),
}
FEATURE_CASES = {"feature_vits": ("vits", (2, 3, 64, 96))}


def backbone():
    """DepthAnythingFeature (core/extractor.py:286-320) and Feature (:323-369) run by the reference,
    hash-initialised; inputs from synth (regenerated by the tests)."""
    ext = import_reference_extractor()
    for name, (enc, shape) in BACKBONE_CASES.items():
        m = ext.DepthAnythingFeature(encoder=enc).eval()
        synth.init_module_(m, seed=4321)
        x = synth.normal(synth.name_seed(name + "_x"), shape)
        with torch.no_grad():
            out = m(t(x))
        g = {k: out[k].numpy() for k in ("out", "path_1", "path_2", "path_3", "path_4", "disp")}
        for i, (tok, cls) in enumerate(out["features"]):
            g[f"feat{i}"], g[f"cls{i}"] = tok.numpy(), cls.numpy()
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
        with open(os.path.join(OUT, f"state_dict_{name}.json"), "w") as f:
            json.dump([[k, list(v.shape)] for k, v in m.state_dict().items()], f)
        print(name, {k: v.shape for k, v in g.items()})
    for name, (vit, shape) in FEATURE_CASES.items():
        args = synth.make_args(vit_size=vit)
        m = ext.Feature(args).eval()
        synth.init_module_(m, seed=4321)
        x = synth.normal(synth.name_seed(name + "_x"), shape)
        with torch.no_grad():
            feats, vit_feat = m(t(x))
        g = {f"x{4 << i}": f.numpy() for i, f in enumerate(feats)}
        g["vit_feat"] = vit_feat.numpy()
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
        with open(os.path.join(OUT, f"state_dict_{name}.json"), "w") as f:
            json.dump([[k, list(v.shape)] for k, v in m.state_dict().items()], f)
        print(name, {k: v.shape for k, v in g.items()})
    # the whole model with its real backbone: the checkpoint layout (feature.* included)
    fs, *_ = import_reference()
    fs.Feature = ext.Feature
    for vit in ("vits", "vitl"):
        m = fs.FoundationStereo(synth.make_args(max_disp=192, corr_levels=4, vit_size=vit))
        with open(os.path.join(OUT, f"state_dict_full_{vit}.json"), "w") as f:
            json.dump([[k, list(v.shape)] for k, v in m.state_dict().items()], f)


CLOUD_CASES = {"a": (5, 7), "b": (33, 70)}


def cloud():
    """depth2xyzmap (Utils.py:56-75) run by the reference on two small depth maps that include zeros
    and pixels below zmin: pins tests/cloud_oracle.py.  The rest of the demo's cloud code sits under
    ``if __name__ == "__main__"`` (scripts/run_demo.py) and cannot be called."""
    import_reference()          # installs the stubs Utils.py's imports need
    import importlib
    ref_utils = importlib.import_module("Utils")
    K = np.array([[61.5, 0.0, 33.25], [0.0, 59.75, 15.5], [0.0, 0.0, 1.0]], dtype=np.float32)
    g = {"K": K, "zmin": np.float32(0.1)}
    for tag, (H, W) in CLOUD_CASES.items():
        depth = synth.uniform(synth.name_seed(f"cloud_depth_{tag}"), (H, W), 0.02, 6.0).astype(np.float32)
        depth[0, 0] = 0.0
        depth[H // 2, W // 3] = 0.0
        depth[H - 1, W - 1] = 0.05                        # below zmin
        depth[1, 2] = 0.0999
        depth[2, 1] = 0.1001
        g[f"depth_{tag}"] = depth
        g[f"xyz_{tag}"] = ref_utils.depth2xyzmap(depth.copy(), K.copy(), zmin=0.1)
    np.savez_compressed(os.path.join(OUT, "cloud_small.npz"), **g)
    print("cloud_small", {k: (v.shape, v.dtype) for k, v in g.items()})


def frames():
    """vis_disparity (Utils.py:108-133) through its ``cmap=`` branch with matplotlib's turbo, and
    InputPadder (core/utils/utils.py:17-41), run by the reference on a 37x53 case: pins
    tests/frames_oracle.py and ``frames.TURBO``.  Needs matplotlib (here only, never in the package)."""
    import_reference()
    import importlib
    import matplotlib
    ref_utils = importlib.import_module("Utils")
    ref_core_utils = importlib.import_module("core.utils.utils")
    turbo = matplotlib.colormaps["turbo"]
    H, W = 37, 53
    disp = synth.uniform(synth.name_seed("frames_disp"), (H, W), 0.5, 60.0).astype(np.float32)
    holes = np.argsort(synth.uniform(synth.name_seed("frames_holes"), (H * W,)))[:40]
    disp.reshape(-1)[holes] = np.inf
    g = {"disp": disp,
         "lut": (turbo(np.arange(256, dtype=np.uint8))[:, :3] * 255).astype(np.uint8)}
    other = {}
    g["vis_auto"] = ref_utils.vis_disparity(disp, cmap=turbo, other_output=other)
    g["minmax_auto"] = np.array([other["min_val"], other["max_val"]], dtype=np.float32)
    g["vis_5_40"] = ref_utils.vis_disparity(disp, min_val=5, max_val=40, cmap=turbo, other_output={})
    img = synth.uniform(synth.name_seed("frames_img"), (1, 3, H, W), 0.0, 255.0).astype(np.float32)
    padder = ref_core_utils.InputPadder((H, W), divis_by=32, force_square=False)
    g["pad_in"] = img
    g["pad_out"] = padder.pad(t(img))[0].numpy()
    g["pad"] = np.array(padder._pad)
    assert g["pad"].tolist() == [5, 6, 13, 14] and g["vis_auto"].dtype == np.uint8
    np.savez_compressed(os.path.join(OUT, "frames_small.npz"), **g)
    print("frames_small", {k: (v.shape, v.dtype) for k, v in g.items()})


def _load_by_path(name, *parts):
    import importlib.util
    from ref_harness import REF_ROOT
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def metrics():
    """compute_stereo_metrics (train/utils.py:88-141), monitoring_stereo (train/losses.py:326-339) and
    depth_uint8_decoding (Utils.py:137-140) run by the reference on a (3,37,61) case whose ground truth
    is the decoded uint8 map: pins tests/metrics_oracle.py.  Pair 1's mask is empty (:122-123).  The
    inputs come from tests/metrics_oracle.py golden_case (hash PRNG); the file holds the reference's
    outputs, 8 decoded rows and checksums of the inputs."""
    import_reference()
    import importlib
    ref_utils = importlib.import_module("Utils")
    train_utils = _load_by_path("ref_train_utils", "train", "utils.py")
    train_losses = _load_by_path("ref_train_losses", "train", "losses.py")
    from tests import metrics_oracle
    case = metrics_oracle.golden_case()                     # the tests regenerate the same inputs
    gt_u8, gt, pred, mask, thresholds = (case[k] for k in ("gt_u8", "gt", "pred", "mask", "thresholds"))
    B = len(pred)
    gt64 = np.stack([ref_utils.depth_uint8_decoding(gt_u8[b], scale=1000) for b in range(B)])
    assert np.array_equal(gt, gt64.astype(np.float32))      # the inputs were built on the oracle's decode
    # the reference's float64 decode of 8 rows of pair 0 (the arithmetic is per pixel)
    g = {"gt0_decoded_f64": gt64[0, :8], "thresholds": np.array(thresholds),
         "checksums": np.array([float(gt_u8.sum()), float(pred.astype(np.float64).sum()), float(mask.sum())])}
    whole = train_utils.compute_stereo_metrics(t(pred), t(gt), t(mask), thresholds)
    keys = sorted(whole)
    g["keys"] = np.array(keys)
    g["batch"] = np.array([whole[k] for k in keys], dtype=np.float64)
    for b in range(B):
        one = train_utils.compute_stereo_metrics(t(pred[b]), t(gt[b]), t(mask[b]), thresholds)
        two = train_losses.compute_stereo_metrics(t(pred[b]), t(gt[b]), t(mask[b]), thresholds)
        assert all(one[k] == two[k] for k in two)
        g[f"pair{b}"] = np.array([one[k] for k in keys], dtype=np.float64)
        mon = train_losses.monitoring_stereo(t(pred[b]))
        g[f"monitoring{b}"] = np.array([mon[k] for k in ("disparity_mean", "disparity_std", "disparity_min",
                                                         "disparity_max")], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "metrics_small.npz"), **g)
    print("metrics_small", {k: (v.shape, v.dtype) for k, v in g.items()}, keys)


def seq():
    """foundation_stereo_loss and the three single-map losses (train/losses.py:20-187, :379-498) run by
    the reference, pair by pair, on tests/seq_oracle.py golden_case (hash PRNG): pins the oracle of the
    sequence metrics.  Two parameter sets, the initial disparity once at 10 x 16 (resized by the
    reference's own F.interpolate) and once at full size.  The file holds what the reference returned
    plus checksums of the inputs.  Also enforces the case's condition: at most 2 valid pixels of the
    resized initial row lie within the resize's rounding gap of a rate threshold."""
    import_reference()
    import torch.nn.functional as F
    ref = _load_by_path("ref_train_losses", "train", "losses.py")
    from tests import seq_oracle as so
    case = so.golden_case()
    gt, mask, preds = case["gt"], case["mask"], case["preds"]
    B, H, W = gt.shape
    keys = None
    g = {"checksums": np.array(so.checksums(case)), "params": np.array(so.GOLDEN_PARAMS)}
    for pi, (gamma, maxd) in enumerate(so.GOLDEN_PARAMS):
        for name in ("init_small", "init_full"):
            for b in range(B):
                loss, misc = ref.foundation_stereo_loss(t(case[name][b]), [t(p[b]) for p in preds], t(gt[b]),
                                                        t(mask[b]), gamma=gamma, max_disparity=maxd)
                keys = keys or sorted(misc)
                g[f"fsl_p{pi}_{name}_pair{b}"] = np.array([float(loss)] + [misc[k] for k in keys], dtype=np.float64)
        for b in range(B):
            last = t(preds[-1][b])
            outs = [ref.disparity_l1_loss(last, t(gt[b]), t(mask[b]), max_disparity=maxd),
                    ref.disparity_smooth_l1_loss(last, t(gt[b]), t(mask[b]), beta=0.5, max_disparity=maxd),
                    ref.disparity_epe_loss(last, t(gt[b]), t(mask[b]), max_disparity=maxd),
                    ref.disparity_smooth_l1_loss(t(case["init_small"][b]), t(gt[b]), t(mask[b]), beta=1.0,
                                                 max_disparity=maxd)]
            g[f"single_p{pi}_pair{b}"] = np.array([[float(l), m["epe"], m["d1_error"], m["d3_error"]] for l, m in outs],
                                                  dtype=np.float64)
    g["keys"] = np.array(keys)
    g["single_keys"] = np.array(["loss", "epe", "d1_error", "d3_error"])
    # the condition of the resized row's rate bound (tests/test_seq_host.py)
    up = F.interpolate(t(case["init_small"])[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0].numpy()
    mine = so.upsample(case["init_small"], H, W)
    measured, gap = float(np.abs(up - mine).max()), so.resize_gap_bound(np.abs(case["init_small"]).max())
    assert measured <= gap, (measured, gap)
    for _, maxd in so.GOLDEN_PARAMS:
        e = np.abs(so.row_values(case["init_small"], H, W, 1.0, maxd) - gt)[mask]
        M = int(((np.abs(e - 1.0) <= gap) | (np.abs(e - 3.0) <= gap)).sum())
        assert M <= 2, f"{M} pixels within {gap} of a threshold: change seq_oracle.GOLDEN_TAG"
    np.savez_compressed(os.path.join(OUT, "seq_small.npz"), **g)
    print("seq_small", {k: (v.shape, v.dtype) for k, v in g.items()}, keys, "resize gap", measured, "bound", gap)


def main():
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["ops", "update", "e2e", "hiera", "backbone", "cloud", "frames", "metrics", "seq"]
    if "seq" in which:
        seq()
        which = [w for w in which if w != "seq"]
        if not which:
            return
    if "cloud" in which:
        cloud()
    if "frames" in which:
        frames()
    if "metrics" in which:
        metrics()
    if set(which) <= {"cloud", "frames", "metrics"}:
        return
    fs, sm, geo_mod, up_mod, ut = import_reference()
    if "backbone" in which:
        backbone()
    if "hiera" in which:
        hiera(fs)
    if "ops" in which:
        ops_small(sm, geo_mod, ut)
    if "update" in which:
        update_step(up_mod)
    if "e2e" in which:
        e2e(fs)


if __name__ == "__main__":
    main()
