"""How good is a disparity map: EPE, RMSE, bad-pixel rates and KITTI's D1 against a ground truth.

The reference scores a prediction with ``compute_stereo_metrics`` (train/utils.py:88-141; the
per-pair body again in train/losses.py:342-376) and watches it with ``monitoring_stereo``
(train/losses.py:326-339): a boolean-mask gather, a Python loop over the batch and ``4 + K``
``.item()`` read-backs per pair.  Here one streaming HIP pass and a one-block-per-pair second kernel
(csrc/metrics.hip, ``ops.disp_metrics``) leave every figure of every pair in one small device
tensor; nothing synchronises the host, so the stage sits in a captured graph or a streaming
evaluation loop like the rest of the package.

    m = metrics.stereo_metrics(disp, gt)                     # device tensors, no synchronisation
    acc = metrics.MetricsAccumulator(); acc.update(m)        # over a dataset, still on the device
    print(acc.result())                                      # one synchronisation

    metrics.compute_stereo_metrics(disp, gt, gt > 0)         # the reference's function, one read-back

Sums are fp64 and added in an order fixed by the map's size alone (no float atomics): equal inputs
give equal bits, run to run and device to device.  The per-pixel error and every comparison are fp32,
as torch evaluates them.  Three things here are not pinned by the reference: ``d1_all`` follows
KITTI's published definition (error > 3 px and > 5 % of the ground truth, as a product
``0.05f * |gt|`` where the devkit divides), the default validity without a mask is ``gt > 0`` and
finite (the dataloader's ``disparity > 0``, train/dataloader.py:142-148, with NaN / inf excluded), and
``n_nonfinite`` counts the valid pixels whose error is NaN or inf.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor

NACC = ops.METRICS_NACC
MAX_THRESHOLDS = ops.METRICS_MAX_THRESHOLDS
# columns of ``table`` (and, for the counts and sums behind them, of ``sums``): include/fsmi.h
N_VALID, EPE, RMSE, D1_ALL, N_NONFINITE, PRED_MEAN, PRED_STD, PRED_MIN, PRED_MAX, BAD0 = range(10)


@dataclass
class StereoMetrics:
    """``stereo_metrics``'s result: device tensors, one row per pair; the named fields are views of
    ``table``."""
    table: Tensor                   # (B,17) fp64: n_valid, epe, rmse, d1_all, n_nonfinite, pred_*, bad[0..7]
    sums: Tensor                    # (B,17) fp64: the raw accumulators; additive over pairs and calls
    thresholds: Tuple[float, ...]
    error: Optional[Tensor] = None  # (B,H,W) fp32 with want_error: |pred - gt| on valid pixels, +inf elsewhere

    @property
    def n_valid(self) -> Tensor:
        return self.table[:, N_VALID]

    @property
    def epe(self) -> Tensor:
        return self.table[:, EPE]

    mae = epe                       # train/utils.py:130: "same as EPE for disparity"

    @property
    def rmse(self) -> Tensor:
        return self.table[:, RMSE]

    @property
    def d1_all(self) -> Tensor:
        return self.table[:, D1_ALL]

    @property
    def n_nonfinite(self) -> Tensor:
        return self.table[:, N_NONFINITE]

    @property
    def pred_mean(self) -> Tensor:
        return self.table[:, PRED_MEAN]

    @property
    def pred_std(self) -> Tensor:
        return self.table[:, PRED_STD]

    @property
    def pred_min(self) -> Tensor:
        return self.table[:, PRED_MIN]

    @property
    def pred_max(self) -> Tensor:
        return self.table[:, PRED_MAX]

    @property
    def bad(self) -> Tensor:
        """(B,K): the share of valid pixels with error > thresholds[k]."""
        return self.table[:, BAD0:BAD0 + len(self.thresholds)]


def _as_bhw(x: Tensor, name: str) -> Tensor:
    return ops._as_bhw(x, "stereo_metrics", name)


def stereo_metrics(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None,
                   thresholds: Sequence[float] = (1.0, 3.0, 5.0), gt_scale: float = 1000.0,
                   want_error: bool = False) -> StereoMetrics:
    """Score ``pred`` (fp32 (H,W), (B,H,W) or (B,1,H,W)) against ``gt``: fp32 of the same shape, or
    uint8 (..,H,W,3) in the reference's encoding, decoded with ``gt_scale`` (``decode_gt``).  ``mask``
    (bool / uint8) alone decides validity when given; otherwise a pixel is valid where ``gt > 0`` and
    finite.  Up to 8 ``thresholds``.  Does not synchronise."""
    p = _as_bhw(pred, "pred")
    if isinstance(gt, torch.Tensor) and gt.dtype == torch.uint8:
        g = gt[None] if gt.dim() == 3 else gt
    else:
        g = _as_bhw(gt, "gt")
    m = None if mask is None else _as_bhw(mask, "mask")
    thr = tuple(float(t) for t in thresholds)
    table, sums, error = ops.disp_metrics(p, g, m, thr, gt_scale, want_error)
    return StereoMetrics(table=table, sums=sums, thresholds=thr, error=error)


def decode_gt(gt_u8, scale: float = 1000.0) -> Tensor:
    """``depth_uint8_decoding`` (Utils.py:137-140) on the device: uint8 (H,W,3) or (B,H,W,3), tensor or
    numpy array (uploaded) -> fp32 (H,W) or (B,H,W); float32 of the reference's float64 result."""
    if isinstance(gt_u8, np.ndarray):
        gt_u8 = torch.from_numpy(np.ascontiguousarray(gt_u8)).to(torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(gt_u8, torch.Tensor):
        raise TypeError("decode_gt: expected a uint8 tensor or numpy array")
    single = gt_u8.dim() == 3
    out = ops.gt_decode(gt_u8[None] if single else gt_u8, scale)
    return out[0] if single else out


def error_key(threshold: float) -> str:
    """The reference's name of a bad-pixel rate, train/utils.py:139: ``d{int(t)}_error`` (so 0.5 and
    0.9 share ``d0_error``, the later one winning, as in the reference's dict)."""
    return f"d{int(threshold)}_error"


def compute_stereo_metrics(pred_disparity: Tensor, gt_disparity: Tensor, mask: Tensor,
                           thresholds: Sequence[float] = (1.0, 3.0, 5.0)) -> Dict[str, float]:
    """train/utils.py:88-141 as a drop-in: ``epe``, ``rmse``, ``mae`` and ``d{int(t)}_error`` per
    threshold as Python floats.  A 3-D input returns the mean over pairs of the per-pair values, a
    pair with an empty mask counting as zeros (:120-123).  One device-to-host copy in total."""
    m = stereo_metrics(pred_disparity, gt_disparity, mask, thresholds)
    row = m.table.mean(dim=0).cpu()                         # the only synchronisation
    out = {"epe": float(row[EPE]), "rmse": float(row[RMSE]), "mae": float(row[EPE])}
    for k, t in enumerate(m.thresholds):
        out[error_key(t)] = float(row[BAD0 + k])
    return out


def monitoring_stereo(disparity: Tensor) -> Dict[str, float]:
    """train/losses.py:326-339: mean, unbiased std, min and max of a disparity map (over every element,
    whatever its shape), with one device-to-host copy.  Any floating dtype, as in the reference (an
    autocast half map is widened to fp32 first; its statistics are then those of the fp32 values).  The
    map also goes in as its own ground truth: the statistics do not depend on it, and the error
    accumulators the same pass fills (all zero) are not read."""
    if not isinstance(disparity, torch.Tensor):
        raise TypeError("monitoring_stereo: expected a tensor")
    if not disparity.is_floating_point():
        raise RuntimeError(f"monitoring_stereo: expected a floating tensor, got {disparity.dtype}")
    d = disparity.detach().float().reshape(1, 1, -1)        # the reference runs under no_grad
    m = stereo_metrics(d, d, thresholds=())
    row = m.table[0].cpu()
    return {"disparity_mean": float(row[PRED_MEAN]), "disparity_std": float(row[PRED_STD]),
            "disparity_min": float(row[PRED_MIN]), "disparity_max": float(row[PRED_MAX])}


class MetricsAccumulator:
    """Metrics over a dataset.  ``update`` adds on the device the tensors live on (plain torch: CPU
    tensors work too) and never synchronises; ``result`` synchronises once and returns both averages
    the literature uses: ``per_pair`` (the mean over pairs of each pair's epe / rmse / d1_all / bad
    rates, what ``compute_stereo_metrics`` averages over a batch) and ``pooled`` (all valid pixels of
    all pairs as one set, from the raw sums).  The sums are additive, so pooling over ranks later is
    one all_reduce of ``state()``."""

    def __init__(self):
        self.thresholds: Optional[Tuple[float, ...]] = None
        self.n_pairs = 0
        self._pair_sum: Optional[Tensor] = None     # (17): sum over pairs of table rows
        self._pixel_sum: Optional[Tensor] = None    # (17): sum over pairs of the raw accumulators

    def update(self, m: StereoMetrics) -> None:
        if self.thresholds is None:
            self.thresholds = tuple(m.thresholds)
            self._pair_sum = torch.zeros(NACC, dtype=torch.float64, device=m.table.device)
            self._pixel_sum = torch.zeros(NACC, dtype=torch.float64, device=m.table.device)
        elif tuple(m.thresholds) != self.thresholds:
            raise ValueError(f"MetricsAccumulator: thresholds {m.thresholds} after {self.thresholds}")
        self.n_pairs += int(m.table.shape[0])               # a shape, not a read-back
        self._pair_sum += m.table.sum(dim=0)
        self._pixel_sum += m.sums.sum(dim=0)

    def state(self) -> Tuple[Tensor, Tensor]:
        """(sum of the per-pair table rows, sum of the raw accumulators): (17) fp64 each, on the device."""
        if self._pair_sum is None:
            raise RuntimeError("MetricsAccumulator: no update yet")
        return self._pair_sum, self._pixel_sum

    def result(self) -> Dict[str, object]:
        pair, pix = torch.stack(self.state()).cpu().numpy()                  # one copy
        n = float(pix[N_VALID])
        per_pair = {"epe": pair[EPE] / self.n_pairs, "rmse": pair[RMSE] / self.n_pairs,
                    "d1_all": pair[D1_ALL] / self.n_pairs}
        pooled = {"epe": pix[1] / n if n else 0.0, "rmse": float(np.sqrt(pix[2] / n)) if n else 0.0,
                  "d1_all": pix[3] / n if n else 0.0}
        for k, t in enumerate(self.thresholds):
            per_pair[f"bad_{t:g}"] = pair[BAD0 + k] / self.n_pairs
            pooled[f"bad_{t:g}"] = pix[BAD0 + k] / n if n else 0.0
        return {"n_pairs": self.n_pairs, "n_valid": int(n), "n_nonfinite": int(pix[N_NONFINITE]),
                "thresholds": list(self.thresholds),
                "per_pair": {k: float(v) for k, v in per_pair.items()},
                "pooled": {k: float(v) for k, v in pooled.items()}}


# ---------------------------------------------------------------- sparsification (risk-coverage)

ERR_Q20 = float(2 ** 20)            # err_q20 counts |pred - gt| in units of 2^-20 px (include/fsmi.h)


@dataclass
class Sparsification:
    """``sparsification``'s result: exact integers on the device, one row per pair.  Bin 0 holds the
    least confident pixels, the first to be removed."""
    count: Tensor                   # (B,nbins) int64: pixels per confidence bin
    err_q20: Tensor                 # (B,nbins) int64: their summed |pred - gt|, each capped at 4096 px, x 2^20
    dropped: Tensor                 # (B) int64: valid pixels left out (pred not finite, confidence outside [0, 1])

    def curve(self, b: int = 0):
        """(f, m) of pair ``b``, fp64 on the device: after the ``j`` lowest bins are removed, R_j pixels
        remain with mean error m_j = E_j / 2^20 / R_j at removed fraction f_j = 1 - R_j / R_0; j = 0 ..
        nbins - 1, points with R_j = 0 dropped (the boolean index synchronises)."""
        R = self.count[b].flip(0).cumsum(0).flip(0)     # R_j = sum_{k >= j} n_k, still int64
        E = self.err_q20[b].flip(0).cumsum(0).flip(0)
        keep = R > 0
        R, E = R.double(), E.double()
        R, E = R[keep], E[keep]
        return 1.0 - R / R[0] if len(R) else R, E / ERR_Q20 / R

    def area(self, b: int = 0) -> Tensor:
        """The area under ``curve(b)``, trapezoids over f: a 0-d fp64 device tensor (0 for an empty or
        one-point curve)."""
        f, m = self.curve(b)
        if len(f) < 2:
            return torch.zeros((), dtype=torch.float64, device=self.count.device)
        return ((f[1:] - f[:-1]) * (m[1:] + m[:-1]) * 0.5).sum()

    def ause(self, oracle: "Sparsification", b: int = 0) -> Tensor:
        """Area under the sparsification error: ``area - oracle.area``, the oracle being the same call
        with ``conf=None``; 0 for a confidence that ranks the pixels as their error does."""
        return self.area(b) - oracle.area(b)


def sparsification(conf: Optional[Tensor], pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None, nbins: int = 256,
                   err_cap: float = 16.0) -> Sparsification:
    """Grade a confidence map in [0, 1] (1 = sure) by the error of the pixels it would remove first:
    the risk-coverage histogram of ``ops.risk_coverage`` over ``nbins`` equal confidence bins.
    ``conf=None`` is the oracle ranking, the pixels binned by their own error over [0, ``err_cap``] px
    (``nbins / err_cap`` bins per px; larger errors share the worst bin).  conf, pred, gt fp32 (H,W),
    (B,H,W) or (B,1,H,W); validity as ``stereo_metrics``.  A map that is not a probability (``spread``,
    a photometric residual) goes in as a decreasing function of it, e.g. ``1 / (1 + x)``.  Does not
    synchronise."""
    if not float(err_cap) > 0.0:
        raise ValueError(f"sparsification: err_cap = {err_cap} must be positive")
    p, g = ops._as_bhw(pred, "sparsification", "pred"), ops._as_bhw(gt, "sparsification", "gt")
    c = None if conf is None else ops._as_bhw(conf, "sparsification", "conf")
    m = None if mask is None else ops._as_bhw(mask, "sparsification", "mask")
    count, err_q20, dropped = ops.risk_coverage(c, p, g, m, nbins, float(nbins) / float(err_cap))
    return Sparsification(count=count, err_q20=err_q20, dropped=dropped)
