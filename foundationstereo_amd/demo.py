"""The reference's demo (scripts/run_demo.py) end to end on the device.

    python -m foundationstereo_amd.demo --left_file left.png --right_file right.png \\
        --intrinsic_file K.txt --ckpt_dir pretrained_models/model_best_bp2.pth --out_dir out

Frames in (``frames.ingest``), forward, picture (``frames.vis_disparity``), depth and clouds
(``cloud.disparity_to_cloud``): the disparity never returns to the host between them.  Writes
``vis.png``, ``depth_meter.npy`` (pinhole only), ``cloud.ply`` and ``cloud_denoise.ply`` into
``--out_dir`` next to copies of the inputs, and prints one JSON line.  The flags carry the reference's
names and defaults (run_demo.py:45-80); ``--out_dir`` is honoured (the reference replaces it with a
timestamped folder) and no viewer window opens.  ``--occlusion_check 1`` and ``--lr_check 1`` (not in the
reference; ``visibility``) draw the picture and build the clouds from the VISIBLE pixels only, write
``visibility.png`` and add the five class counts to the JSON line.  ``--photo_check 1`` (not in the reference;
``photometric``) scores the disparity against the two frames without a ground truth: it writes ``warped.png``
(the right frame in the left view) and ``photometric.png`` (the residual, 0 .. ``--photo_max`` grey levels) and
adds ``"photometric"`` and ``"row_offset"``, the rig's vertical misalignment probed over -2 .. 2 rows, to the
line.  ``--confidence 1`` (not in the reference; ``confidence``) reads the cost volume's own certainty of the
disparity: it writes ``confidence.png`` (the ``mass`` channel, 0 .. 1 over the turbo table) and adds
``"confidence": {"mass_mean", "entropy_mean", "spread_mean_px"}`` to the line; ``--min_confidence T`` drops the
pixels with ``mass < T`` from picture and clouds (ANDed with the visibility mask when a check is on).
``--synthetic`` runs without a checkpoint on the hash-initialised model the tests use.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys

import numpy as np
import torch

from . import cloud, frames

# visibility.png: one grey level per class, in code order (visible, invalid, out_of_view, occluded, mismatch)
VISIBILITY_GREY = (255, 0, 64, 128, 192)


def run_pair(model, left_u8, right_u8, K, baseline, *, scale=1.0, hiera=0, valid_iters=32, camera_type="pinhole",
             z_far=10.0, remove_invisible=1, denoise_cloud=1, denoise_nb_points=30, denoise_radius=0.03,
             get_pc=1, occlusion_check=0, lr_check=0, occlusion_tol=1.0, lr_thresh=1.0, photo_check=0,
             confidence=0, min_confidence=0.0) -> dict:
    """scripts/run_demo.py:131-275 for one pair of uint8 frames (arrays or device tensors).  Returns
    device tensors: ``disp`` (H,W), ``vis`` (H,2W,3) uint8, ``minmax`` (2), ``depth`` (H,W), ``cloud`` and
    ``cloud_denoise`` as (points (M,3), colors (M,3) uint8) -- the last three None without ``get_pc``,
    ``cloud_denoise`` None without ``denoise_cloud`` -- and ``frames``, the ingest result.  With
    ``occlusion_check`` or ``lr_check`` (the latter runs a second forward for the right view's
    disparity), ``visibility`` is ``visibility.classify``'s result, the picture is drawn from the
    disparity with every other class set to +inf, and only VISIBLE pixels enter the clouds; ``disp``
    stays the forward's.  With ``photo_check``, ``photometric`` is ``photometric.consistency``'s result (with the
    warped frame and the maps, over the VISIBLE pixels when a check is on) and ``row_probe``
    ``photometric.row_probe``'s over -2 .. 2 rows.  With ``confidence`` or ``min_confidence`` > 0 the forward
    keeps its logits (``model.keep_logits``, restored afterwards; with ``hiera`` those of the full-resolution
    pass), ``confidence`` is ``confidence.from_model``'s result unpadded to (1,H,W) maps, and with
    ``min_confidence`` = T > 0 the pixels with ``mass < T`` (NaN included) are drawn black and left out of the
    clouds, ANDed with the VISIBLE set when a check is on; ``keep`` is then that bool (1,H,W) mask."""
    check = bool(occlusion_check) or bool(lr_check)
    want_conf = bool(confidence) or min_confidence > 0
    if photo_check and camera_type != "pinhole":
        raise ValueError("run_pair: photo_check warps a rectified pinhole pair (a pixel moves along its row by its "
                         f"disparity); camera_type {camera_type!r} is refused")
    if check and camera_type != "pinhole":
        raise ValueError("run_pair: occlusion_check / lr_check model a rectified pinhole pair (a pixel moves along its "
                         f"row by its disparity); camera_type {camera_type!r} is refused")
    if lr_check and hiera:
        raise ValueError("run_pair: lr_check with hiera is refused: the right view's disparity comes from the plain forward")
    fr = frames.ingest(left_u8, right_u8, scale=scale)
    if len(fr.batch) != 1:
        raise ValueError(f"run_pair: one pair at a time, got a batch of {len(fr.batch)}")
    kept = getattr(model, "keep_logits", False)
    if want_conf:
        model.keep_logits = True
    try:
        with torch.no_grad():
            if not hiera:
                disp = model.forward(fr.left, fr.right, iters=valid_iters, test_mode=True)
            else:
                disp = model.run_hierachical(fr.left, fr.right, iters=valid_iters, test_mode=True, small_ratio=0.5)
    finally:
        if want_conf:
            model.keep_logits = kept
    conf = None
    if want_conf:
        from . import confidence as _conf
        c = _conf.from_model(model, disp.float())                           # on the padded grid, then unpadded like disp
        conf = _conf.Confidence(*[fr.padder.unpad(getattr(c, n)[:, None])[:, 0] for n in _conf.CHANNELS])
    disp = fr.padder.unpad(disp.float())                                    # run_demo.py:166
    vis_cls, drawn = None, disp
    if check:
        from . import visibility
        right = None
        if lr_check:
            right = fr.padder.unpad(visibility.right_disparity(model, fr.left, fr.right, iters=valid_iters).float())
        vis_cls = visibility.classify(disp, right, occlusion=bool(occlusion_check), occlusion_tol=occlusion_tol,
                                      lr_thresh=lr_thresh)
        drawn = visibility.invalidate(disp, vis_cls.classes)
    keep = vis_cls.visible if check else None
    if min_confidence > 0:
        sure = conf.mass >= min_confidence                                  # NaN compares false
        keep = sure if keep is None else keep & sure
        drawn = drawn.masked_fill(~sure[:, None], float("inf"))
    other = {}
    vis = frames.vis_disparity(drawn[:, 0], image=fr.image_u8, other_output=other)
    out = {"disp": disp[0, 0], "vis": vis[0], "minmax": other["minmax"][0], "frames": fr,
           "depth": None, "cloud": None, "cloud_denoise": None}
    if check:
        out["visibility"] = vis_cls
    if want_conf:
        out["confidence"], out["keep"] = conf, keep
    if photo_check:
        from . import photometric
        lv, rv, seen = fr.padder.unpad(fr.left), fr.padder.unpad(fr.right), vis_cls.visible if check else None
        out["photometric"] = photometric.consistency(disp, lv, rv, seen, want_warped=True)
        out["row_probe"] = photometric.row_probe(disp, lv, rv, seen, max_offset=2.0, step=1.0)
    if get_pc:
        c = cloud.disparity_to_cloud(disp, K, baseline, image=fr.image_u8, denoise=bool(denoise_cloud),
                                     nb_points=denoise_nb_points, radius=denoise_radius, scale=scale,
                                     camera_type=camera_type, remove_invisible=bool(remove_invisible), z_far=z_far,
                                     keep=keep)[0]
        out["depth"] = c.depth
        out["cloud"] = (c.xyz_map[c.valid], fr.image_u8[0][c.valid])
        if denoise_cloud:
            out["cloud_denoise"] = (c.points, c.colors)
    return out


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m foundationstereo_amd.demo",
                                description="FoundationStereo demo: stereo pair -> disparity picture, depth, point clouds")
    p.add_argument("--left_file", default="assets/left.png", type=str, help="Path to the left image (.npy or an image file)")
    p.add_argument("--right_file", default="assets/right.png", type=str, help="Path to the right image")
    p.add_argument("--intrinsic_file", default="assets/K.txt", type=str,
                   help="Path to camera intrinsic matrix and baseline file")
    p.add_argument("--ckpt_dir", default="pretrained_models/model_best_bp2.pth", type=str, help="Path to pretrained model")
    p.add_argument("--out_dir", default="output/", type=str, help="Directory to save results")
    p.add_argument("--camera_type", type=str, default="pinhole", choices=["pinhole", "panorama"],
                   help="Type of camera: pinhole (standard perspective) or panorama (equirectangular projection)")
    p.add_argument("--scale", default=1, type=float, help="Downsize the image by scale, must be <=1")
    p.add_argument("--hiera", default=0, type=int,
                   help="Use hierarchical inference (only needed for high-resolution images (>1K))")
    p.add_argument("--z_far", default=10, type=float, help="Maximum depth to clip in point cloud")
    p.add_argument("--valid_iters", type=int, default=32, help="Number of flow-field updates during forward pass")
    p.add_argument("--get_pc", type=int, default=1, help="Save point cloud output")
    p.add_argument("--remove_invisible", default=1, type=int,
                   help="Remove non-overlapping observations between left and right images from point cloud")
    p.add_argument("--denoise_cloud", type=int, default=1, help="Whether to denoise the point cloud")
    p.add_argument("--denoise_nb_points", type=int, default=30,
                   help="Number of points to consider for radius outlier removal")
    p.add_argument("--denoise_radius", type=float, default=0.03, help="Radius to use for outlier removal")
    p.add_argument("--occlusion_check", type=int, default=0,
                   help="Drop pixels hidden from the right camera (a z-buffer over the disparity) from picture and clouds")
    p.add_argument("--lr_check", type=int, default=0,
                   help="Drop pixels that fail the left-right consistency check (costs a second forward)")
    p.add_argument("--occlusion_tol", type=float, default=1.0,
                   help="Occluded when another pixel lands on the same right-image column with a disparity this much larger (px)")
    p.add_argument("--lr_thresh", type=float, default=1.0, help="Left-right disparity difference above which a pixel is dropped (px)")
    p.add_argument("--photo_check", type=int, default=0,
                   help="Score the disparity against the two frames: warped.png, photometric.png, residual and row offset in the JSON line")
    p.add_argument("--photo_max", type=float, default=32.0, help="Residual in grey levels at the top of photometric.png's colour range")
    p.add_argument("--confidence", type=int, default=0, nargs="?", const=1,
                   help="Read the cost volume's own certainty of the disparity: confidence.png and its means in the JSON line")
    p.add_argument("--min_confidence", type=float, default=0.0,
                   help="Drop pixels whose confidence (mass) is below this from picture and clouds (0 = off)")
    p.add_argument("--synthetic", action="store_true",
                   help="No checkpoint: the hash-initialised model of the tests (synth.make_args + synth.init_module_)")
    p.add_argument("--max_disp", type=int, default=192, help="With --synthetic: the model's max_disp")
    p.add_argument("--vit_size", type=str, default="vits", choices=["vits", "vitb", "vitl"],
                   help="With --synthetic: the backbone size")
    p.add_argument("--backbone", type=str, default="synthetic", choices=["synthetic", "real"],
                   help="real: the EdgeNeXt + DepthAnythingV2 backbone on HIP; synthetic: the seeded stand-in features")
    return p


def load_model(a, device):
    if a.synthetic:
        from . import synth
        from .foundation_stereo import FoundationStereo
        args = synth.make_args(max_disp=a.max_disp, vit_size=a.vit_size)
        args["backbone"] = a.backbone
        model = FoundationStereo(args).eval()
        synth.init_module_(model, seed=1234)
        return model.to(device)
    from . import checkpoint
    over = {k: v for k, v in vars(a).items() if k not in ("synthetic", "max_disp", "vit_size", "backbone")}
    model, _ = checkpoint.load_model(a.ckpt_dir, over, device=device, backbone=a.backbone == "real")   # run_demo.py:111-128
    return model


def photo_summary(ph, b: int = 0) -> dict:
    """The JSON object of pair ``b`` of a ``photometric.consistency`` result (one read-back)."""
    from . import photometric as pm
    row = ph.table[b, :pm.NFIXED].cpu().tolist()
    return {"l1_mean": row[pm.L1_MEAN], "l1_rms": row[pm.L1_RMS], "dssim_mean": row[pm.DSSIM_MEAN],
            "photometric": row[pm.PHOTOMETRIC], "n_scored": int(row[pm.N_SCORED]), "n_ssim": int(row[pm.N_SSIM])}


def confidence_summary(conf, b: int = 0) -> dict:
    """The JSON object of pair ``b`` of a ``confidence`` result (one read-back): the means over the finite
    pixels; ``spread`` in full-resolution pixels (4 per bin)."""
    row = torch.stack([torch.nanmean(conf.mass[b].double()), torch.nanmean(conf.entropy[b].double()),
                       4.0 * torch.nanmean(conf.spread[b].double())]).cpu().tolist()
    return {"mass_mean": row[0], "entropy_mean": row[1], "spread_mean_px": row[2]}


def main(argv=None) -> dict:
    a = parser().parse_args(argv)
    if not 0 < a.scale <= 1:
        raise SystemExit("scale must be in (0, 1]")                           # run_demo.py:149
    if not 0 <= a.min_confidence <= 1:
        raise SystemExit("demo: --min_confidence is a probability: 0 (off) .. 1")
    check = bool(a.occlusion_check) or bool(a.lr_check)
    if check and a.camera_type != "pinhole":
        raise SystemExit("demo: --occlusion_check / --lr_check model a rectified pinhole pair; "
                         "--camera_type panorama is refused with either")
    if a.photo_check and a.camera_type != "pinhole":
        raise SystemExit("demo: --photo_check warps a rectified pinhole pair; --camera_type panorama is refused with it")
    if a.lr_check and a.hiera:
        raise SystemExit("demo: --lr_check with --hiera 1 is refused: the right view's disparity comes from the plain forward")
    if not torch.cuda.is_available():
        raise SystemExit("demo: needs a HIP device")
    device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(a.out_dir, exist_ok=True)
    for src, stem in ((a.left_file, "left"), (a.right_file, "right"), (a.intrinsic_file, "K")):   # run_demo.py:106-108
        shutil.copy(src, os.path.join(a.out_dir, stem + os.path.splitext(src)[1]))
    K, baseline = cloud.read_intrinsics(a.intrinsic_file)
    model = load_model(a, device)
    left, right = frames.read_image(a.left_file), frames.read_image(a.right_file)
    out = run_pair(model, left, right, K, baseline, scale=a.scale, hiera=a.hiera, valid_iters=a.valid_iters,
                   camera_type=a.camera_type, z_far=a.z_far, remove_invisible=a.remove_invisible,
                   denoise_cloud=a.denoise_cloud, denoise_nb_points=a.denoise_nb_points,
                   denoise_radius=a.denoise_radius, get_pc=a.get_pc, occlusion_check=a.occlusion_check,
                   lr_check=a.lr_check, occlusion_tol=a.occlusion_tol, lr_thresh=a.lr_thresh,
                   photo_check=a.photo_check, confidence=a.confidence, min_confidence=a.min_confidence)
    fr = out["frames"]
    res = {"out_dir": a.out_dir, "image_size": list(out["disp"].shape), "padded_size": list(fr.batch.shape[-2:]),
           "min_disp": float(out["minmax"][0]), "max_disp": float(out["minmax"][1])}

    def path(name):
        return os.path.join(a.out_dir, name)
    frames.write_png(path("vis.png"), out["vis"])                             # run_demo.py:168-170
    res["vis"] = path("vis.png")
    if check:
        v = out["visibility"]
        grey = torch.tensor(VISIBILITY_GREY, dtype=torch.uint8, device=device)[v.classes[0].long()]
        frames.write_png(path("visibility.png"), grey[:, :, None].expand(-1, -1, 3).contiguous())
        res["visibility_png"] = path("visibility.png")
        res["visibility"] = [int(n) for n in v.counts[0].cpu().tolist()]      # pixels per class, in code order
    if a.photo_check:
        ph, probe = out["photometric"], out["row_probe"]
        frames.write_png(path("warped.png"), ph.warped[0].clamp(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous())
        frames.write_png(path("photometric.png"), frames.vis_disparity(ph.l1, min_val=0.0, max_val=a.photo_max)[0])
        res["warped_png"], res["photometric_png"] = path("warped.png"), path("photometric.png")
        res["photometric"] = photo_summary(ph)
        off = float(probe.offset[0])
        res["row_offset"] = off if off == off else None                         # NaN: the minimum is not bracketed
    if a.confidence:
        frames.write_png(path("confidence.png"), frames.vis_disparity(out["confidence"].mass, min_val=0.0, max_val=1.0)[0])
        res["confidence_png"] = path("confidence.png")
        res["confidence"] = confidence_summary(out["confidence"])
    if a.get_pc:
        cloud.write_ply(path("cloud.ply"), *out["cloud"])                     # run_demo.py:255
        res["cloud"], res["cloud_points"] = path("cloud.ply"), int(out["cloud"][0].shape[0])
        if a.camera_type == "pinhole":
            np.save(path("depth_meter.npy"), out["depth"].cpu().numpy())       # run_demo.py:259-261
            res["depth"] = path("depth_meter.npy")
        if a.denoise_cloud:
            cloud.write_ply(path("cloud_denoise.ply"), *out["cloud_denoise"])  # run_demo.py:270-274
            res["cloud_denoise"] = path("cloud_denoise.ply")
            res["cloud_denoise_points"] = int(out["cloud_denoise"][0].shape[0])
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
