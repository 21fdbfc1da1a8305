"""How sure the network was of a disparity: per-pixel confidence from the cost volume, on the device.

The forward computes a probability distribution over disparity for every quarter-resolution pixel (the
classifier's logits, ``(B, max_disp / 4, H / 4, W / 4)``) and keeps only its mean.  With
``model.keep_logits = True`` the forward leaves those logits in ``model.last_logits`` and
``from_model`` / ``from_logits`` turn them into four maps on the grid of the disparity they judge
(csrc/confidence.hip behind ``ops.disp_confidence``, one launch):

    mass      the probability within ``radius`` bins of the disparity (a trapezoid one bin wider, so it
              is continuous in the disparity); 1 = the volume agrees with the answer
    spread    the distribution's RMS distance from the disparity, in bins (x 4 = full-resolution px)
    peak      the largest probability of the column
    entropy   1 - H / ln D: 1 for a one-hot column, 0 for a uniform one

    model.keep_logits = True
    disp = model(left, right, iters=32, test_mode=True)
    conf = confidence.from_model(model, disp)
    clouds = cloud.disparity_to_cloud(disp, K, baseline, keep=conf.mass >= 0.5)
    s = metrics.sparsification(conf.mass, disp, gt); s.ause(metrics.sparsification(None, disp, gt))

``mass`` and ``spread`` judge the refined disparity against the volume the refinement started from;
``peak`` and ``entropy`` are properties of the volume alone.  Nothing in the reference pins these
definitions; include/fsmi.h states them operation by operation and tests/confidence_oracle.py restates
them in numpy.  ``radius = 1`` bin (4 px) is a parameter, not a claim about this model.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import ops

Tensor = torch.Tensor

CHANNELS = ops.CONF_CHANNELS


@dataclass
class Confidence:
    """``from_logits``'s result: (B,H,W) fp32 device tensors, None for a channel not in ``want``."""
    mass: Optional[Tensor]
    spread: Optional[Tensor]        # in bins of the volume (``up`` full-resolution px each)
    peak: Optional[Tensor]
    entropy: Optional[Tensor]


def from_logits(logits: Tensor, disp: Optional[Tensor] = None, *, up: int = 4, radius: float = 1.0,
                want: Sequence[str] = CHANNELS) -> Confidence:
    """``logits`` fp32 (B,D,h,w), the classifier output before the softmax.  ``disp``: the disparity to
    judge, in full-resolution pixels, fp32 (H,W), (B,H,W) or (B,1,H,W) with H = h * up, W = w * up (a
    bin is ``up`` px wide); None judges every column at its own expectation, the initial disparity.
    NaN where a column holds a NaN or +inf logit, and in ``mass`` / ``spread`` where the disparity is not
    finite.  Does not synchronise."""
    d = None if disp is None else ops._as_bhw(disp, "confidence", "disp")
    out = ops.disp_confidence(logits, d, up=up, radius=radius, want=tuple(want))
    return Confidence(*out)


def from_model(model, disp: Tensor, *, radius: float = 1.0, want: Sequence[str] = CHANNELS) -> Confidence:
    """The confidence of ``disp``, the PADDED full-resolution output of the forward that just ran on
    ``model`` with ``model.keep_logits = True`` (unpad the maps as the disparity is unpadded).  After
    ``run_hierachical`` the logits are those of its full-resolution pass."""
    logits = getattr(model, "last_logits", None)
    if logits is None:
        raise RuntimeError("confidence.from_model: model.last_logits is None: set model.keep_logits = True before the "
                           "forward")
    return from_logits(logits, disp, up=4, radius=radius, want=want)
