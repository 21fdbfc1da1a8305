"""Score a disparity map against a ground truth: EPE, RMSE, bad-pixel rates and D1, on the device.

    # run the model on a pair, then score its disparity
    python -m foundationstereo_amd.evaluate --left_file left.png --right_file right.png \\
        --gt_file disp_gt.png --gt_scale 1000 --ckpt_dir pretrained_models/model_best_bp2.pth

    # score two stored maps, e.g. bench.py --dump-outputs' disparity.npy of --precision fast
    # against the default run's
    python -m foundationstereo_amd.evaluate --pred_file fast/disparity.npy --gt_file parity/disparity.npy

``--gt_file`` is a ``.npy`` float map (H,W), or the reference's 3 x uint8 encoding (Utils.py:137-140) as
an image file or a uint8 ``.npy`` (H,W,3), decoded with ``--gt_scale``.  A pixel is scored where the
ground truth is positive and finite; ``--all_pixels`` scores every pixel; ``--noc`` scores the non-occluded
pixels (the benchmarks' headline mask), with the occlusion derived from the ground truth itself
(``visibility.classify(gt).visible``, ``--occlusion_tol``), and adds ``"mask": "noc"`` to the line.  ``--error_png`` writes the
error map through the disparity picture's kernels (0 .. ``--error_max`` px over the turbo table,
unscored pixels black).  ``--per_iter`` scores every refinement iteration in one pass (``losses``): the model
runs ``forward(test_mode=False)``, each iteration's disparity is unpadded as a view, and the JSON line
gains a ``per_iter`` object with the convergence curve (``epe``, ``rmse``, ``d1_all``, ``bad`` per
iteration), the initial disparity's row (``init``: resized to full size and multiplied by 4), the
sequence ``loss`` and ``first_iter_within``, the first iteration whose EPE is within ``--converged_px`` of
the last one's; the other fields stay those of the last iteration.  With ``--per_iter``, ``--pred_file``
names a stored sequence (K,H,W).  The model flags are the demo's (``demo.parser``); ``--scale`` must stay 1,
because resizing a ground truth is not defined here.  ``--photometric`` and ``--row_probe N`` score the
disparity against the two frames instead (``photometric``: the right frame warped by the disparity, its
residual, and the residual with the right frame N rows up and down): they add ``"photometric"`` and
``"row_probe"`` objects to the line, need ``--left_file`` and ``--right_file`` and no ground truth (``--gt_file`` may be
left out with either; the line then has no ground-truth fields).  With ``--noc`` their mask is the visible
set.  ``--confidence`` (the demo's flag; needs the model run, so not with ``--pred_file``) adds a ``"confidence"``
object: the means of the cost volume's own confidence maps (``confidence``) and, with a ground truth, how well
each ranks the pixels by their error: ``ause_mass``, ``ause_entropy``, ``ause_peak`` (area under the sparsification
error, ``metrics.sparsification``; 0 is the oracle ranking) and ``oracle_area``, over the mask of the flags.
Prints one JSON line.
"""
from __future__ import annotations

import json
import sys

import numpy as np
import torch

from . import demo, frames, losses, metrics


def parser():
    p = demo.parser()
    p.prog = "python -m foundationstereo_amd.evaluate"
    p.description = "Score a disparity (the model's, or a stored map) against a ground truth"
    p.add_argument("--gt_file", default=None, type=str,
                   help="Ground truth: .npy float map (H,W), or the 3 x uint8 encoding as an image / uint8 .npy (H,W,3)")
    p.add_argument("--pred_file", default=None, type=str,
                   help="Score this stored .npy disparity instead of running the model on --left_file / --right_file")
    p.add_argument("--gt_scale", default=1000.0, type=float, help="Scale of the uint8 ground-truth encoding")
    p.add_argument("--thresholds", default=[1.0, 3.0, 5.0], type=float, nargs="*", help="Bad-pixel thresholds in px (up to 8)")
    p.add_argument("--all_pixels", action="store_true", help="Score every pixel (a mask of ones), not only gt > 0")
    p.add_argument("--noc", action="store_true",
                   help="Score non-occluded pixels only: gt > 0, finite and visible to the right camera by the ground truth's own z-buffer")
    p.add_argument("--error_png", default=None, type=str, help="Write the error map as a PNG here")
    p.add_argument("--error_max", default=5.0, type=float, help="Error in px at the top of the picture's colour range")
    p.add_argument("--per_iter", action="store_true",
                   help="Score every refinement iteration (forward(test_mode=False)); --pred_file then names a (K,H,W) .npy")
    p.add_argument("--converged_px", default=0.01, type=float,
                   help="With --per_iter: first_iter_within reports the first iteration whose EPE is this close to the last one's")
    p.add_argument("--gamma", default=0.9, type=float, help="With --per_iter: the sequence loss's weight factor")
    p.add_argument("--max_disparity", default=192.0, type=float, help="With --per_iter: the sequence loss clamps to [0, this]")
    p.add_argument("--photometric", action="store_true",
                   help="Score the disparity against the two frames (warp residual, SSIM); needs no --gt_file")
    p.add_argument("--row_probe", default=0, type=int,
                   help="Probe the rig's vertical misalignment over the integer row offsets -N..N (0 = off, at most 3)")
    return p


def _given(argv, flag: str) -> bool:
    """Whether ``flag`` is on the command line (the demo's defaults name files of the reference's assets)."""
    args = sys.argv[1:] if argv is None else argv
    return any(x == flag or x.startswith(flag + "=") for x in args)


def read_gt(path: str, device) -> torch.Tensor:
    """The ground truth as a device tensor: fp32 (H,W), or uint8 (H,W,3) still encoded."""
    if path.lower().endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8:
            a = np.squeeze(a)
            if a.ndim != 2:
                raise SystemExit(f"evaluate: {path}: expected a float map (H,W), got {a.shape}")
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    else:
        a = frames.read_image(path)
    if a.ndim != 3 or a.shape[2] < 3:
        raise SystemExit(f"evaluate: {path}: the uint8 encoding needs 3 channels, got {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a[:, :, :3])).to(device)


def score_mask(a, gt: torch.Tensor, device):
    """The validity mask (1,H,W) of the flags, or None for the default ``gt > 0`` and finite.  ``--noc``:
    the VISIBLE class of the ground truth itself (``visibility.classify``: positive, finite, inside the
    right image, and not behind another pixel of its row by more than ``--occlusion_tol``)."""
    if a.all_pixels:
        return torch.ones((1,) + tuple(gt.shape[:2]), dtype=torch.bool, device=device)
    if a.noc:
        from . import visibility
        g = metrics.decode_gt(gt, a.gt_scale) if gt.dtype == torch.uint8 else gt
        return visibility.classify(g, occlusion_tol=a.occlusion_tol).visible
    return None


def predict(a, device):
    """(the model's unpadded disparity (H,W) of the pair, its confidence maps or None): demo.run_pair's own
    ingest, forward and unpad, without the cloud (it reads no intrinsics then; its picture, two launches, is
    not used)."""
    model = demo.load_model(a, device)
    left, right = frames.read_image(a.left_file), frames.read_image(a.right_file)
    out = demo.run_pair(model, left, right, None, None, hiera=a.hiera, valid_iters=a.valid_iters, get_pc=0,
                        confidence=a.confidence)
    return out["disp"], out.get("confidence")


def confidence_fields(conf, pred: torch.Tensor, gt, mask, gt_scale: float) -> dict:
    """--confidence: the object it adds to the line.  ``conf`` (1,H,W) maps, ``pred`` (H,W); ``gt`` None, fp32
    (H,W) or the uint8 encoding; ``mask`` (1,H,W) or None.  One read-back."""
    res = demo.confidence_summary(conf)
    if gt is None:
        return {"confidence": res}
    g = metrics.decode_gt(gt, gt_scale) if gt.dtype == torch.uint8 else gt
    oracle = metrics.sparsification(None, pred, g, mask)
    names = ("mass", "entropy", "peak")
    ranked = [metrics.sparsification(getattr(conf, n), pred, g, mask) for n in names]
    flat = torch.stack([s.ause(oracle) for s in ranked] + [oracle.area(), ranked[0].dropped[0].double()]).cpu().tolist()
    res.update({f"ause_{n}": v for n, v in zip(names, flat)})
    res["oracle_area"], res["n_dropped"] = flat[3], int(flat[4])
    return {"confidence": res}


def predict_sequence(a, device):
    """The model's (initial disparity or None, [every iteration's unpadded disparity (1,H,W)]) of the pair:
    ``forward(test_mode=False)`` under no_grad, each map unpadded as a view.  The quarter-resolution
    initial disparity covers the PADDED frame: it goes out as it is when the frame needed no padding
    (the scoring pass resizes it), else resized to the padded size first and unpadded like the rest."""
    import torch.nn.functional as F
    model = demo.load_model(a, device)
    fr = frames.ingest(frames.read_image(a.left_file), frames.read_image(a.right_file), scale=a.scale)
    if len(fr.batch) != 1:
        raise SystemExit(f"evaluate: one pair at a time, got a batch of {len(fr.batch)}")
    with torch.no_grad():
        init, preds = model.forward(fr.left, fr.right, iters=a.valid_iters, test_mode=False)
    init = init.float()
    if any(fr.padder._pad):
        init = fr.padder.unpad(F.interpolate(init[:, None] if init.dim() == 3 else init, size=fr.left.shape[-2:],
                                             mode="bilinear", align_corners=False))
    return (init[:, 0] if init.dim() == 4 else init), [fr.padder.unpad(p.float())[:, 0] for p in preds]


def per_iter(a, device) -> dict:
    """--per_iter: the whole sequence scored in one call, one read-back."""
    if a.hiera:
        raise SystemExit("evaluate: --per_iter refuses --hiera 1: run_hierachical(test_mode=False) unpads a tuple, "
                         "in the reference as here, so its sequence is undefined")
    if a.error_png is not None:
        raise SystemExit("evaluate: --per_iter writes no error map: score the last iteration without it")
    if a.pred_file is not None:
        seq = np.load(a.pred_file)
        if seq.ndim != 3:
            raise SystemExit(f"evaluate: --per_iter --pred_file {a.pred_file}: expected a stored sequence (K,H,W), "
                             f"got {seq.shape}")
        seq = torch.from_numpy(np.ascontiguousarray(seq, dtype=np.float32)).to(device)
        init, preds = None, [seq[k][None] for k in range(len(seq))]
    else:
        init, preds = predict_sequence(a, device)
    if not 1 <= len(preds) <= losses.MAX_ROWS - 1:
        raise SystemExit(f"evaluate: --per_iter scores 1..{losses.MAX_ROWS - 1} iterations, got {len(preds)}")
    gt = read_gt(a.gt_file, device)
    H, W = preds[-1].shape[-2:]
    if tuple(gt.shape[:2]) != (H, W):
        raise SystemExit(f"evaluate: ground truth {tuple(gt.shape[:2])} against a disparity of {(H, W)}")
    mask = score_mask(a, gt, device)
    m = losses.sequence_metrics(init, preds, gt[None], mask, a.gamma, a.max_disparity, a.thresholds, init_scale=4.0,
                                gt_scale=a.gt_scale)
    # the fields of the plain call, from the unclamped last iteration: the merged single-map stage on its view
    last = metrics.stereo_metrics(preds[-1], gt, None if mask is None else mask[0], a.thresholds, a.gt_scale)
    flat = torch.cat([m.table[0].reshape(-1), m.loss, last.table[0]]).cpu().tolist()       # the one read-back
    R, n = len(preds) + int(init is not None), losses.NACC
    rows = [flat[r * n:(r + 1) * n] for r in range(R)]
    loss, row = flat[R * n], flat[R * n + 1:]
    K = len(m.thresholds)

    def pick(r):
        return {"n_valid": int(r[losses.N_VALID]), "n_nonfinite": int(r[losses.N_NONFINITE]), "epe": r[losses.EPE],
                "rmse": r[losses.RMSE], "d1_all": r[losses.D1_ALL], "bad": r[losses.BAD0:losses.BAD0 + K]}

    its = rows[1:] if init is not None else rows
    epe = [r[losses.EPE] for r in its]
    within = [k + 1 for k, e in enumerate(epe) if abs(e - epe[-1]) <= a.converged_px]
    res = {"mode": "pred_file" if a.pred_file is not None else "model", "image_size": [H, W],
           "n_valid": int(row[metrics.N_VALID]), "n_nonfinite": int(row[metrics.N_NONFINITE]),
           "epe": row[metrics.EPE], "rmse": row[metrics.RMSE], "d1_all": row[metrics.D1_ALL],
           "thresholds": list(m.thresholds), "bad": row[metrics.BAD0:metrics.BAD0 + K],
           "pred_mean": row[metrics.PRED_MEAN], "pred_std": row[metrics.PRED_STD],
           "pred_min": row[metrics.PRED_MIN], "pred_max": row[metrics.PRED_MAX],
           "per_iter": {"iters": len(its), "epe": epe, "rmse": [r[losses.RMSE] for r in its],
                        "d1_all": [r[losses.D1_ALL] for r in its],
                        "bad": [r[losses.BAD0:losses.BAD0 + K] for r in its],
                        "init": pick(rows[0]) if init is not None else None, "loss": loss, "gamma": a.gamma,
                        "max_disparity": a.max_disparity, "converged_px": a.converged_px,
                        "first_iter_within": within[0] if within else None}}
    if a.noc:
        res["mask"] = "noc"
    print(json.dumps(res))
    return res


def photo_fields(a, pred: torch.Tensor, mask, device) -> dict:
    """--photometric / --row_probe: the objects they add to the line.  ``pred`` (H,W); the frames are read
    again (as the forward's ingest did) and go in as uint8; ``mask`` (1,H,W) or None."""
    from . import photometric

    def frame(path):                                    # uint8 (H,W) or (H,W,3): alpha dropped, as the ingest does
        x = frames.read_image(path)
        if x.ndim == 3:
            x = x[:, :, :3] if x.shape[2] >= 3 else x[:, :, 0]
        return torch.from_numpy(np.ascontiguousarray(x)).to(device)
    left, right = frame(a.left_file), frame(a.right_file)
    if tuple(left.shape[:2]) != tuple(pred.shape) or left.shape != right.shape:
        raise SystemExit(f"evaluate: frames {tuple(left.shape)} and {tuple(right.shape)} against a disparity of {tuple(pred.shape)}")
    res = {}
    if a.photometric:
        res["photometric"] = demo.photo_summary(photometric.consistency(pred, left, right, mask, want_maps=False))
    if a.row_probe:
        p = photometric.row_probe(pred, left, right, mask, max_offset=float(a.row_probe), step=1.0)
        flat = torch.cat([p.l1[0], p.offset]).cpu().tolist()                       # the one read-back
        res["row_probe"] = {"offsets": [int(o) for o in p.offsets.tolist()], "l1": flat[:-1],
                            "offset": flat[-1] if flat[-1] == flat[-1] else None}
    return res


def main(argv=None) -> dict:
    a = parser().parse_args(argv)
    photo = a.photometric or a.row_probe != 0
    if a.gt_file is None and not (photo or a.confidence):
        raise SystemExit("evaluate: the following arguments are required: --gt_file (optional only with --photometric / "
                         "--row_probe / --confidence)")
    if not 0 <= a.row_probe <= 3:
        raise SystemExit("evaluate: --row_probe N probes the offsets -N..N, at most 8 of them: N in 0..3")
    if photo and a.pred_file is not None and not (_given(argv, "--left_file") and _given(argv, "--right_file")):
        raise SystemExit("evaluate: --photometric / --row_probe with --pred_file need --left_file and --right_file: the "
                         "residual is between the two frames")
    if photo and a.per_iter:
        raise SystemExit("evaluate: --photometric / --row_probe score one disparity: not with --per_iter")
    if a.confidence and (a.pred_file is not None or a.per_iter):
        raise SystemExit("evaluate: --confidence reads the cost volume of the model run: not with --pred_file or --per_iter")
    if a.min_confidence != 0:
        raise SystemExit("evaluate: --min_confidence drops pixels from the demo's picture and clouds; a score over the "
                         "confident pixels only is the sparsification curve --confidence reports")
    if a.scale != 1:
        raise SystemExit("evaluate: --scale must be 1: resizing a ground truth is not defined here")
    if a.noc and a.all_pixels:
        raise SystemExit("evaluate: --noc and --all_pixels name two different masks")
    if len(a.thresholds) > metrics.MAX_THRESHOLDS:
        raise SystemExit(f"evaluate: at most {metrics.MAX_THRESHOLDS} thresholds")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate: needs a HIP device")
    device = torch.device("cuda", torch.cuda.current_device())
    if a.per_iter:
        return per_iter(a, device)
    if a.pred_file is not None:
        pred = np.squeeze(np.load(a.pred_file))
        if pred.ndim != 2:
            raise SystemExit(f"evaluate: {a.pred_file}: expected a disparity map (H,W), got {pred.shape}")
        pred = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).to(device)
        conf = None
    else:
        pred, conf = predict(a, device)
    if a.gt_file is None:
        # no ground truth: --noc takes the visible set of the disparity itself
        if a.all_pixels or a.error_png is not None:
            raise SystemExit("evaluate: --all_pixels and --error_png need --gt_file")
        mask = None
        if a.noc:
            from . import visibility
            mask = visibility.classify(pred, occlusion_tol=a.occlusion_tol).visible
        res = {"mode": "pred_file" if a.pred_file is not None else "model", "image_size": list(pred.shape)}
        if photo:
            res.update(photo_fields(a, pred, mask, device))
        if conf is not None:
            res.update(confidence_fields(conf, pred, None, mask, a.gt_scale))
        if a.noc:
            res["mask"] = "noc"
        print(json.dumps(res))
        return res
    gt = read_gt(a.gt_file, device)
    if tuple(gt.shape[:2]) != tuple(pred.shape):
        raise SystemExit(f"evaluate: ground truth {tuple(gt.shape[:2])} against a disparity of {tuple(pred.shape)}")
    mask = score_mask(a, gt, device)
    m = metrics.stereo_metrics(pred, gt, None if mask is None else mask[0], a.thresholds, a.gt_scale, want_error=a.error_png is not None)
    if a.error_png is not None:
        frames.write_png(a.error_png, frames.vis_disparity(m.error, min_val=0.0, max_val=a.error_max)[0])
    row = m.table[0].cpu().tolist()                         # the one read-back
    res = {"mode": "pred_file" if a.pred_file is not None else "model", "image_size": list(pred.shape),
           "n_valid": int(row[metrics.N_VALID]), "n_nonfinite": int(row[metrics.N_NONFINITE]),
           "epe": row[metrics.EPE], "rmse": row[metrics.RMSE], "d1_all": row[metrics.D1_ALL],
           "thresholds": list(m.thresholds), "bad": row[metrics.BAD0:metrics.BAD0 + len(m.thresholds)],
           "pred_mean": row[metrics.PRED_MEAN], "pred_std": row[metrics.PRED_STD],
           "pred_min": row[metrics.PRED_MIN], "pred_max": row[metrics.PRED_MAX]}
    if a.error_png is not None:
        res["error_png"] = a.error_png
    if a.noc:
        res["mask"] = "noc"
    if photo:
        res.update(photo_fields(a, pred, mask, device))
    if conf is not None:
        res.update(confidence_fields(conf, pred, gt, mask, a.gt_scale))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
