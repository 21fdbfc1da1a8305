"""Which disparities belong to pixels the right camera cannot see, on the device.

The band of background next to every foreground edge is hidden from the right camera; a network still
has to put a disparity there, and those pixels become the flying points of a cloud and count against a
score that the benchmarks take over non-occluded pixels.  ``classify`` gives every pixel of a rectified
left disparity map one class (csrc/visibility.hip behind ``ops.disp_visibility``, one launch):

    INVALID       the disparity is not finite or not positive
    OUT_OF_VIEW   u - d < 0: left of the right image (the one test the reference applies, run_demo.py:173-178)
    OCCLUDED      another pixel of the row lands on the same right-image column with a disparity more than
                  ``occlusion_tol`` larger (a z-buffer over the map itself)
    MISMATCH      with a right-view disparity: it differs from the left one by more than ``lr_thresh`` where
                  the pixel lands (the left-right consistency check)
    VISIBLE       everything else

    vis = visibility.classify(disp)                                   # occlusion only, no second forward
    vis = visibility.classify(disp, visibility.right_disparity(model, left, right, iters=32))
    clouds = cloud.disparity_to_cloud(disp, K, baseline, keep=vis.visible)
    m = metrics.stereo_metrics(disp, gt, (gt > 0) & visibility.classify(gt).visible)      # "noc" scoring

Nothing in the reference pins these definitions; include/fsmi.h states them operation by operation and
tests/visibility_oracle.py restates them in numpy, bit for bit.  The 1 px defaults are the conventional
left-right threshold: parameters, not claims about this model.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import ops

Tensor = torch.Tensor

# the class codes of include/fsmi.h (FSMI_VIS_*)
VISIBLE, INVALID, OUT_OF_VIEW, OCCLUDED, MISMATCH = range(5)
NAMES = ("visible", "invalid", "out_of_view", "occluded", "mismatch")


@dataclass
class Visibility:
    """``classify``'s result: device tensors."""
    classes: Tensor             # (B,H,W) uint8, one of the five codes
    counts: Tensor              # (B,5) int64, pixels per class
    error: Optional[Tensor]     # (B,H,W) fp32 with want_error: |d - right view's d|, NaN where INVALID / OUT_OF_VIEW

    @property
    def visible(self) -> Tensor:
        """(B,H,W) bool."""
        return self.classes == VISIBLE

    @property
    def fractions(self) -> Tensor:
        """(B,5) fp64: ``counts`` over the pixels of a pair."""
        return self.counts.double() / float(self.classes.shape[1] * self.classes.shape[2])


def classify(disp: Tensor, disp_right: Optional[Tensor] = None, *, occlusion: bool = True, occlusion_tol: float = 1.0,
             lr_thresh: float = 1.0, want_error: bool = False) -> Visibility:
    """One class per pixel of ``disp`` (fp32 (H,W), (B,H,W) or (B,1,H,W) on a HIP device).  ``disp_right``,
    the right view's disparity on the right image's grid (``right_disparity``), adds the left-right
    check; ``occlusion=False`` drops the z-buffer.  ``want_error`` (needs ``disp_right``) also returns
    the left-right difference.  Widths up to 8192.  Does not synchronise."""
    d = ops._as_bhw(disp, "visibility", "disp")
    r = None if disp_right is None else ops._as_bhw(disp_right, "visibility", "disp_right")
    if want_error and r is None:
        raise ValueError("visibility.classify: want_error needs disp_right")
    classes, counts, error = ops.disp_visibility(d, r, occlusion_tol, lr_thresh, occlusion, want_error)
    return Visibility(classes=classes, counts=counts, error=error)


def right_disparity(model, left: Tensor, right: Tensor, **forward_kwargs) -> Tensor:
    """The right view's disparity, on the right image's grid: mirrored left to right, the right image
    is the left image of a rectified pair whose right image is the mirrored left one, so this is
    ``model.forward(flip(right), flip(left), **forward_kwargs)`` flipped back (plain torch flips of the
    last axis).  It costs a second forward; ``test_mode=True`` unless the caller says otherwise."""
    forward_kwargs.setdefault("test_mode", True)
    with torch.no_grad():
        out = model.forward(torch.flip(right, dims=[-1]), torch.flip(left, dims=[-1]), **forward_kwargs)
    return torch.flip(out, dims=[-1])


def invalidate(disp: Tensor, classes: Tensor, fill: float = float("inf")) -> Tensor:
    """A copy of ``disp`` with ``fill`` wherever ``classes`` is not VISIBLE.  The default +inf is what
    ``frames.vis_disparity`` draws black and ``cloud.disparity_to_xyz`` leaves out.  ``classes`` has
    ``classify``'s (B,H,W); ``disp`` may be any of the shapes ``classify`` takes."""
    bad = classes != VISIBLE
    if disp.dim() == 2:
        bad = bad[0]
    elif disp.dim() == 4:
        bad = bad[:, None]
    return disp.masked_fill(bad, fill)
