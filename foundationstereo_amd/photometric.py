"""Does a disparity explain the two images?  A score that needs no ground truth, on the device.

Everything else that judges a disparity needs a ground-truth map (``metrics``, ``losses``) or a second
forward (``visibility.right_disparity``).  The classical check needs only what a forward leaves behind,
the two frames and the left disparity (csrc/photometric.hip behind ``ops.photo_consistency``, two
launches):

    warp      the right frame sampled at ``u - d`` on the pixel's own row (bilinear), in the left view
    l1        the mean absolute difference of the left frame and the warp over the channels, grey levels
    dssim     ``(1 - SSIM) / 2`` over 3x3 windows of the left frame and the warp
    row probe ``l1`` again with the right frame sampled a few rows up and down: the offset with the
              smallest residual is the rig's vertical misalignment, which a learned network does not report

    fr = frames.ingest(left_u8, right_u8)
    disp = fr.padder.unpad(model.forward(fr.left, fr.right, iters=32, test_mode=True).float())
    p = photometric.consistency(disp, fr.padder.unpad(fr.left), fr.padder.unpad(fr.right),
                                visibility.classify(disp).visible)       # occluded pixels have a residual by construction
    p.l1_mean, p.dssim_mean, p.photometric                               # (B) fp64 device tensors
    photometric.row_probe(disp, left, right).offset                      # (B) rows, NaN when the minimum is at an end

Images are the fp32 planar views of ``frames.Frames`` ((B,C,H,W) or (C,H,W); strided views go in without
a copy) or uint8 (B,H,W,C) / (H,W,C) / (H,W), C in (1, 3), grey levels 0..255 in both.  Nothing in the
reference pins these definitions; include/fsmi.h states them operation by operation and
tests/photometric_oracle.py restates them in numpy.  Nothing here synchronises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import ops

Tensor = torch.Tensor

# columns of the table (include/fsmi.h); the row probe's (n_r, mean l1) pairs follow from NFIXED on
N_SCORED, N_SSIM, N_INVALID, N_OUT_OF_VIEW, L1_MEAN, L1_RMS, DSSIM_MEAN, PHOTOMETRIC = range(8)
NFIXED = ops.PHOTO_NFIXED
MAX_OFFSETS = ops.PHOTO_MAX_OFFSETS


@dataclass
class Photometric:
    """``consistency``'s result: device tensors."""
    table: Tensor               # (B, 8 + 2R) fp64
    sums: Tensor                # (B, 8 + 2R) fp64, the raw sums in the same layout
    offsets: tuple              # the R row offsets
    warped: Optional[Tensor]    # (B,C,H,W) fp32 with want_warped: the right frame in the left view, 0 where not sampled
    l1: Optional[Tensor]        # (B,H,W) fp32 with want_maps: +inf where not scored
    dssim: Optional[Tensor]     # (B,H,W) fp32 with want_maps: +inf where SSIM is undefined

    n_scored = property(lambda s: s.table[:, N_SCORED])
    n_ssim = property(lambda s: s.table[:, N_SSIM])
    n_invalid = property(lambda s: s.table[:, N_INVALID])
    n_out_of_view = property(lambda s: s.table[:, N_OUT_OF_VIEW])
    l1_mean = property(lambda s: s.table[:, L1_MEAN])
    l1_rms = property(lambda s: s.table[:, L1_RMS])
    dssim_mean = property(lambda s: s.table[:, DSSIM_MEAN])
    photometric = property(lambda s: s.table[:, PHOTOMETRIC])
    row_n = property(lambda s: s.table[:, NFIXED::2])            # (B,R) scored pixels whose offset row is inside the image
    row_l1 = property(lambda s: s.table[:, NFIXED + 1::2])       # (B,R) mean l1 at each offset


@dataclass
class RowProbe:
    """``row_probe``'s result: device tensors."""
    offsets: Tensor             # (R) fp64
    l1: Tensor                  # (B,R) fp64, mean l1 at each offset
    n: Tensor                   # (B,R) fp64, pixels behind each mean
    offset: Tensor              # (B) fp64: the parabola's vertex, NaN when it is not bracketed


def _disp(x: Tensor) -> Tensor:
    return ops._as_bhw(x, "photometric", "disp")


def _image(x: Tensor, name: str) -> Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"photometric: {name} must be a tensor")
    if x.dtype == torch.uint8:
        if x.dim() == 2:
            return x[None, :, :, None]
        if x.dim() == 3:
            return x[None]
    elif x.dim() == 3:
        return x[None]
    if x.dim() == 4:
        return x
    raise ValueError(f"photometric: {name} must be fp32 (B,C,H,W) / (C,H,W) or uint8 (B,H,W,C) / (H,W,C) / (H,W), "
                     f"got {x.dtype} {tuple(x.shape)}")


def _mask(mask):
    return None if mask is None else ops._as_bhw(mask, "photometric", "mask")


def consistency(disp: Tensor, left: Tensor, right: Tensor, mask: Optional[Tensor] = None, *, row_offsets=(),
                alpha: float = 0.85, want_warped: bool = False, want_maps: bool = True) -> Photometric:
    """The residual between ``left`` and ``right`` warped by ``disp``, over the pixels of ``mask`` (bool /
    uint8, default all): counts, mean and rms ``l1``, mean ``dssim`` and ``photometric``, the mean of
    ``alpha * dssim + (1 - alpha) * l1 / 255``, per pair; ``row_offsets`` (up to 8 floats) adds the mean
    ``l1`` at each vertical offset of the right frame."""
    d = _disp(disp)
    table, sums, warped, l1, dssim = ops.photo_consistency(d, _image(left, "left"), _image(right, "right"), _mask(mask),
                                                           row_offsets, alpha, want_warped, want_maps, want_maps)
    return Photometric(table=table, sums=sums, offsets=tuple(float(o) for o in row_offsets), warped=warped, l1=l1,
                       dssim=dssim)


def warp_right(disp: Tensor, right: Tensor) -> Tensor:
    """``right`` in the left view: fp32 (B,C,H,W), 0 where the disparity is invalid or points left of the image."""
    r = _image(right, "right")
    return ops.photo_consistency(_disp(disp), r, r, None, (), 0.85, True, False, False, ssim=False)[2]


def row_probe(disp: Tensor, left: Tensor, right: Tensor, mask: Optional[Tensor] = None, max_offset: float = 2.0,
              step: float = 1.0) -> RowProbe:
    """Mean ``l1`` with the right frame sampled at the rows ``v + k * step``, ``|k * step| <= max_offset`` (at
    most 8 offsets), and the vertex of the parabola through the smallest mean and its two neighbours.  The
    vertex is NaN when the minimum sits at either end or a neighbour's mean has no pixel behind it."""
    if not (step > 0 and max_offset >= 0):
        raise ValueError("photometric.row_probe: step must be positive and max_offset not negative")
    k = int(max_offset / step + 1e-9)
    offs = [i * float(step) for i in range(-k, k + 1)]
    if len(offs) > MAX_OFFSETS:
        raise ValueError(f"photometric.row_probe: {len(offs)} offsets, at most {MAX_OFFSETS}")
    d = _disp(disp)
    table = ops.photo_consistency(d, _image(left, "left"), _image(right, "right"), _mask(mask), offs, 0.85, False,
                                  False, False, ssim=False)[0]
    n, l1 = table[:, NFIXED::2], table[:, NFIXED + 1::2]
    offsets = torch.tensor(offs, dtype=torch.float64, device=table.device)
    R = len(offs)
    # offsets without a pixel never win; the first smallest mean does
    i = torch.where(n > 0, l1, torch.full_like(l1, float("inf"))).argmin(dim=1)
    lo, hi = (i - 1).clamp(min=0), (i + 1).clamp(max=R - 1)

    def at(t, j):
        return t.gather(1, j[:, None])[:, 0]
    y0, y1, y2 = at(l1, lo), at(l1, i), at(l1, hi)
    ok = (i > 0) & (i < R - 1) & (at(n, lo) > 0) & (at(n, i) > 0) & (at(n, hi) > 0)
    den = y0 - 2.0 * y1 + y2
    # den > 0 at a strict minimum; a flat triple puts the vertex on the middle offset
    shift = torch.where(den > 0, 0.5 * (y0 - y2) / den.clamp(min=1e-300), torch.zeros_like(den))
    vertex = offsets[i] + float(step) * shift
    return RowProbe(offsets=offsets, l1=l1, n=n, offset=torch.where(ok, vertex, torch.full_like(vertex, float("nan"))))
