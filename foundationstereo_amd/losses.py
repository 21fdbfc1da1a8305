"""Every refinement iteration scored in one pass: the sequence loss and the convergence curve.

``forward(test_mode=False)`` returns ``(init_disp, disp_preds)``, every iteration's upsampled
disparity.  The reference scores that pair with ``foundation_stereo_loss`` (train/losses.py:379-498,
the loss of configs/train/stereo_v1.json) and single maps with ``disparity_l1_loss``,
``disparity_smooth_l1_loss`` and ``disparity_epe_loss`` (:20-187): per map a boolean-mask gather, an
``F.interpolate`` where the size differs, and about 7 ``.item()`` read-backs.  Here the whole sequence
goes through one streaming HIP pass and a one-block-per-pair second kernel (csrc/seq_metrics.hip,
``ops.seq_metrics``): the ground truth and the mask are read once per group of 4 maps, a smaller map
is sampled bilinearly as it is read, views go in without a copy, and nothing synchronises the host.

    m = losses.sequence_metrics(init_disp, disp_preds, gt)        # device tensors, no synchronisation
    m.epe                                                          # (B, 1 + K): the convergence curve
    acc = losses.SequenceAccumulator(); acc.update(m)              # over a dataset, still on the device
    print(acc.result())                                            # one synchronisation

    loss, misc = losses.foundation_stereo_loss(init_disp, disp_preds, gt, mask)   # the reference's call

These are VALUES only: the model is inference-only, there is no backward pass, and an input that
requires grad raises (outside ``torch.no_grad()``) instead of returning a silently detached loss.

The reference's quirks are kept in the drop-ins, so their figures compare with its logs:
  * ``d1_error*`` is the rate of errors above 3 px and ``d3_error*`` the rate above 1 px (:66-67);
  * ``epe_iterative``, ``d1_error_iterative`` and ``d3_error_iterative`` are gamma-weighted SUMS over the
    iterations, not means: the rates can exceed 1 (:468-470);
  * the quarter-resolution ``init_disp`` is resized to the ground truth's size but its values are not
    multiplied by 4 (:407-418), so ``*_initial`` measure a map a quarter too small.  ``init_scale=4.0``
    is this package's opt-in for the meaningful value.
A batched input (B,H,W) returns the mean over pairs of the per-pair figures, an empty pair counting as
zeros, as ``metrics.compute_stereo_metrics`` does; the reference documents (H,W) inputs only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .metrics import _as_bhw

Tensor = torch.Tensor

NACC = ops.SEQ_NACC
MAX_ROWS = ops.SEQ_MAX_ROWS
# columns of ``table`` (and, for the counts and sums behind them, of ``sums``): include/fsmi.h
N_VALID, EPE, RMSE, SMOOTH_L1, D1_ALL, N_NONFINITE, BAD0 = range(7)


@dataclass
class SequenceMetrics:
    """``sequence_metrics``'s result: device tensors, one row per (pair, map); the named fields are
    views of ``table``.  Row 0 is the initial disparity when ``has_init``."""
    table: Tensor                   # (B,R,14) fp64: n_valid, epe, rmse, smooth_l1, d1_all, n_nonfinite, bad[0..7]
    sums: Tensor                    # (B,R,14) fp64: the raw accumulators; additive over pairs and calls
    loss: Tensor                    # (B) fp64: sum_r weights[r] * (smooth_l1 of the initial row, epe of the others)
    thresholds: Tuple[float, ...]
    weights: Tuple[float, ...]      # (R): 1 for the initial row, gamma^(K-k) for iteration k = 1..K
    has_init: bool = True

    @property
    def n_valid(self) -> Tensor:
        return self.table[:, :, N_VALID]

    @property
    def epe(self) -> Tensor:
        return self.table[:, :, EPE]

    @property
    def rmse(self) -> Tensor:
        return self.table[:, :, RMSE]

    @property
    def smooth_l1(self) -> Tensor:
        return self.table[:, :, SMOOTH_L1]

    @property
    def d1_all(self) -> Tensor:
        return self.table[:, :, D1_ALL]

    @property
    def n_nonfinite(self) -> Tensor:
        return self.table[:, :, N_NONFINITE]

    @property
    def bad(self) -> Tensor:
        """(B,R,K): the share of valid pixels with error > thresholds[k]."""
        return self.table[:, :, BAD0:BAD0 + len(self.thresholds)]


def sequence_weights(K: int, gamma: float, with_init: bool = True) -> List[float]:
    """train/losses.py:454: gamma^(K-k) for iteration k = 1..K, after a 1 for the initial row."""
    return ([1.0] if with_init else []) + [float(gamma) ** (K - (k + 1)) for k in range(K)]


def _gt_bhw(gt: Tensor) -> Tensor:
    if isinstance(gt, torch.Tensor) and gt.dtype == torch.uint8:
        return gt[None] if gt.dim() == 3 else gt
    return _as_bhw(gt, "gt")


def sequence_metrics(init_disp: Optional[Tensor], disp_preds: Sequence[Tensor], gt: Tensor,
                     mask: Optional[Tensor] = None, gamma: float = 0.9, max_disparity: float = 192.0,
                     thresholds: Sequence[float] = (1.0, 3.0, 5.0), init_scale: float = 1.0,
                     gt_scale: float = 1000.0, beta: float = 1.0) -> SequenceMetrics:
    """Score ``init_disp`` (or None) and the K maps of ``disp_preds`` against ``gt`` in one call.  Maps:
    fp32 (H,W), (B,H,W) or (B,1,H,W), views welcome; a map of another size than the ground truth's is
    resized as ``F.interpolate(mode="bilinear", align_corners=False)`` does.  ``init_disp``'s values are
    multiplied by ``init_scale`` after the resize; every map is clamped to [0, ``max_disparity``].
    ``gt``, ``mask``, ``thresholds``, ``gt_scale``: as ``metrics.stereo_metrics``.  ``loss`` is
    foundation_stereo_loss's total: the initial row's smooth-L1 mean (``beta``) plus
    sum_k gamma^(K-k) * epe_k.  Does not synchronise."""
    rows = ([] if init_disp is None else [_as_bhw(init_disp, "init_disp")]) + \
        [_as_bhw(p, f"disp_preds[{k}]") for k, p in enumerate(disp_preds)]
    has_init = init_disp is not None
    K = len(rows) - int(has_init)
    if not 1 <= len(rows) <= MAX_ROWS:
        raise ValueError(f"sequence_metrics: {len(rows)} maps, 1..{MAX_ROWS}")
    w = sequence_weights(K, gamma, has_init)
    muls = [float(init_scale) if has_init and r == 0 else 1.0 for r in range(len(rows))]
    thr = tuple(float(t) for t in thresholds)
    table, sums, loss = ops.seq_metrics(rows, _gt_bhw(gt), None if mask is None else _as_bhw(mask, "mask"), thr,
                                        max_disparity, beta, w, (0,) if has_init else (), muls, gt_scale)
    return SequenceMetrics(table=table, sums=sums, loss=loss, thresholds=thr, weights=tuple(w), has_init=has_init)


def _read(m: SequenceMetrics):
    """The mean over pairs of the table rows and of the loss, on the host: THE read-back of a drop-in."""
    flat = torch.cat([m.table.mean(dim=0).reshape(-1), m.loss.mean().reshape(1)]).cpu().numpy()
    return flat[:-1].reshape(-1, NACC), float(flat[-1])


def _single(m: SequenceMetrics, column: int):
    loss = m.table[:, 0, column].mean().float()             # 0-dim fp32, on the device
    row, _ = _read(m)
    # the thresholds are (1, 3): the reference calls the rate above 3 px "d1" and above 1 px "d3"
    return loss, {"epe": float(row[0, EPE]), "d1_error": float(row[0, BAD0 + 1]), "d3_error": float(row[0, BAD0])}


def disparity_l1_loss(pred_disparity: Tensor, gt_disparity: Tensor, mask: Tensor, max_disparity: float = 192.0,
                      **kwargs) -> Tuple[Tensor, Dict[str, float]]:
    """train/losses.py:20-79 as a drop-in: (mean |clamp(pred) - gt| over the mask as a 0-dim fp32 device
    tensor, {epe, d1_error, d3_error} as Python floats from one read-back).  A prediction of another
    size is resized; an empty mask gives zeros."""
    return _single(sequence_metrics(None, [pred_disparity], gt_disparity, mask, 1.0, max_disparity, (1.0, 3.0)), EPE)


def disparity_smooth_l1_loss(pred_disparity: Tensor, gt_disparity: Tensor, mask: Tensor, beta: float = 1.0,
                             max_disparity: float = 192.0, **kwargs) -> Tuple[Tensor, Dict[str, float]]:
    """train/losses.py:82-144 as a drop-in: the smooth-L1 mean (Fast R-CNN's, ``beta``; 0 is plain L1)."""
    return _single(sequence_metrics(None, [pred_disparity], gt_disparity, mask, 1.0, max_disparity, (1.0, 3.0),
                                    beta=beta), SMOOTH_L1)


def disparity_epe_loss(pred_disparity: Tensor, gt_disparity: Tensor, mask: Tensor, max_disparity: float = 192.0,
                       **kwargs) -> Tuple[Tensor, Dict[str, float]]:
    """train/losses.py:147-187 as a drop-in: as ``disparity_l1_loss``, but the reference does not resize
    here, so a prediction of another size than the ground truth's raises."""
    if tuple(_as_bhw(pred_disparity, "pred").shape[-2:]) != tuple(_gt_bhw(gt_disparity).shape[1:3]):
        raise ValueError(f"disparity_epe_loss: prediction {tuple(pred_disparity.shape)} against a ground truth of "
                         f"{tuple(gt_disparity.shape)} (this loss does not resize)")
    return _single(sequence_metrics(None, [pred_disparity], gt_disparity, mask, 1.0, max_disparity, (1.0, 3.0)), EPE)


def foundation_stereo_loss(pred_disparity_initial: Tensor, pred_disparity_pyramid: Sequence[Tensor],
                           gt_disparity: Tensor, mask: Tensor, gamma: float = 0.9, max_disparity: float = 192.0,
                           **kwargs) -> Tuple[Tensor, Dict[str, float]]:
    """train/losses.py:379-498 as a drop-in: L = smooth_l1(d0) + sum_k gamma^(K-k) |d_k - gt|_1 as a 0-dim
    fp32 device tensor, and the reference's eight figures as Python floats from one read-back (the
    quirks: module docstring).  ``init_scale=4.0`` (keyword) multiplies the resized initial disparity."""
    m = sequence_metrics(pred_disparity_initial, pred_disparity_pyramid, gt_disparity, mask, gamma, max_disparity,
                         (1.0, 3.0), init_scale=float(kwargs.get("init_scale", 1.0)))
    loss = m.loss.mean().float()
    rows, _ = _read(m)
    w = np.asarray(m.weights[1:], np.float64)
    it = rows[1:]
    misc = {"epe_initial": rows[0, EPE], "d1_error_initial": rows[0, BAD0 + 1], "d3_error_initial": rows[0, BAD0],
            "epe_iterative": (w * it[:, EPE]).sum(), "d1_error_iterative": (w * it[:, BAD0 + 1]).sum(),
            "d3_error_iterative": (w * it[:, BAD0]).sum(), "loss_initial": rows[0, SMOOTH_L1],
            "loss_iterative": (w * it[:, EPE]).sum()}
    return loss, {k: float(v) for k, v in misc.items()}


class SequenceAccumulator:
    """Convergence curves over a dataset, as ``metrics.MetricsAccumulator``.  ``update`` adds on the
    device the tensors live on (plain torch: CPU tensors work too) and never synchronises; ``result``
    synchronises once and returns, per row, both averages: ``per_pair`` (the mean over pairs of each
    pair's figures) and ``pooled`` (all valid pixels of all pairs as one set, from the raw sums)."""

    def __init__(self):
        self.thresholds: Optional[Tuple[float, ...]] = None
        self.weights: Optional[Tuple[float, ...]] = None
        self.n_pairs = 0
        self._pair_sum: Optional[Tensor] = None     # (R,14): sum over pairs of table rows
        self._pixel_sum: Optional[Tensor] = None    # (R,14): sum over pairs of the raw accumulators
        self._loss_sum: Optional[Tensor] = None     # (): sum over pairs of the loss

    def update(self, m: SequenceMetrics) -> None:
        if self.thresholds is None:
            self.thresholds, self.weights = tuple(m.thresholds), tuple(m.weights)
            self._pair_sum = torch.zeros(m.table.shape[1:], dtype=torch.float64, device=m.table.device)
            self._pixel_sum = torch.zeros_like(self._pair_sum)
            self._loss_sum = torch.zeros((), dtype=torch.float64, device=m.table.device)
        elif tuple(m.thresholds) != self.thresholds or tuple(m.weights) != self.weights:
            raise ValueError(f"SequenceAccumulator: thresholds {m.thresholds} and {len(m.weights)} rows after "
                             f"{self.thresholds} and {len(self.weights)} rows")
        self.n_pairs += int(m.table.shape[0])               # a shape, not a read-back
        self._pair_sum += m.table.sum(dim=0)
        self._pixel_sum += m.sums.sum(dim=0)
        self._loss_sum += m.loss.sum()

    def state(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(sum of the per-pair table rows (R,14), sum of the raw accumulators (R,14), sum of the losses)"""
        if self._pair_sum is None:
            raise RuntimeError("SequenceAccumulator: no update yet")
        return self._pair_sum, self._pixel_sum, self._loss_sum

    def result(self) -> Dict[str, object]:
        pair, pix, loss = self.state()
        flat = torch.cat([pair.reshape(-1), pix.reshape(-1), loss.reshape(1)]).cpu().numpy()     # one copy
        R = pair.shape[0]
        pair, pix = flat[:R * NACC].reshape(R, NACC), flat[R * NACC:2 * R * NACC].reshape(R, NACC)
        n = pix[:, N_VALID]
        safe = np.where(n > 0, n, 1.0)

        def pooled(col):
            return np.where(n > 0, pix[:, col] / safe, 0.0)

        per_pair = {"epe": pair[:, EPE] / self.n_pairs, "rmse": pair[:, RMSE] / self.n_pairs,
                    "smooth_l1": pair[:, SMOOTH_L1] / self.n_pairs, "d1_all": pair[:, D1_ALL] / self.n_pairs}
        pool = {"epe": pooled(EPE), "rmse": np.sqrt(pooled(RMSE)), "smooth_l1": pooled(SMOOTH_L1),
                "d1_all": pooled(D1_ALL)}
        for k, t in enumerate(self.thresholds):
            per_pair[f"bad_{t:g}"] = pair[:, BAD0 + k] / self.n_pairs
            pool[f"bad_{t:g}"] = pooled(BAD0 + k)
        return {"n_pairs": self.n_pairs, "rows": R, "n_valid": [int(v) for v in n],
                "n_nonfinite": [int(v) for v in pix[:, N_NONFINITE]], "thresholds": list(self.thresholds),
                "weights": list(self.weights), "loss": float(flat[-1]) / self.n_pairs,
                "per_pair": {k: [float(x) for x in v] for k, v in per_pair.items()},
                "pooled": {k: [float(x) for x in v] for k, v in pool.items()}}
