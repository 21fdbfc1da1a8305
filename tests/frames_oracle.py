"""numpy restatements of the two ends of the demo (test code; the package never imports this).

``ingest_oracle``: scripts/run_demo.py:134-159 with the resize of include/fsmi.h (fp64 blend, half up).
``vis_oracle``: Utils.py:113-133 in fp32 numpy with the table indexed directly, plus the two
definitions of csrc/frames.hip where the reference is undefined (NaN invalid, max == min -> lut[0]).
"""
import numpy as np


def sintel_pads(h, w, divis_by=32):
    """core/utils/utils.py:26-29,35 -> (left, right, top, bottom)."""
    ph = (((h // divis_by) + 1) * divis_by - h) % divis_by
    pw = (((w // divis_by) + 1) * divis_by - w) % divis_by
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def _taps(n_out, n_in, scale):
    s = (np.arange(n_out, dtype=np.float64) + 0.5) / scale - 0.5
    i0 = np.floor(s)
    w = s - i0
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), w


def resize_oracle(img, scale, return_raw=False):
    """img uint8 (H,W,C) -> uint8 (Hs,Ws,C): bilinear, half-pixel centres, no antialiasing, fp64 blend
    top = a + (b - a) wx, v = top + (bot - top) wy, floor(v + 0.5).  ``return_raw``: also v."""
    H, W = img.shape[:2]
    if scale == 1:
        return (img, img.astype(np.float64)) if return_raw else img
    Hs, Ws = round(H * scale), round(W * scale)             # half-even, as cvRound
    y0, y1, wy = _taps(Hs, H, scale)
    x0, x1, wx = _taps(Ws, W, scale)
    f = img.astype(np.float64)
    wx_, wy_ = wx[None, :, None], wy[:, None, None]
    a, b = f[y0][:, x0], f[y0][:, x1]
    c, d = f[y1][:, x0], f[y1][:, x1]
    top = a + (b - a) * wx_
    bot = c + (d - c) * wx_
    v = top + (bot - top) * wy_
    out = np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    return (out, v) if return_raw else out


def to_rgb(img):
    """run_demo.py:134-141: gray -> three channels, RGBA -> RGB.  img (H,W) or (H,W,C)."""
    if img.ndim == 2:
        img = img[:, :, None]
    if img.shape[2] == 1:
        img = np.concatenate([img, img, img], axis=2)
    return img[:, :, :3]


def ingest_oracle(left, right, scale=1.0, divis_by=32):
    """left, right uint8 (B,H,W,C) -> (batch fp32 (B,2,3,Hp,Wp), image_u8 (B,Hs,Ws,3))."""
    batch, u8 = [], []
    for l, r in zip(left, right):
        pair = []
        for k, img in enumerate((l, r)):
            s = resize_oracle(to_rgb(img), scale)
            if k == 0:
                u8.append(s)
            pl, pr, pt, pb = sintel_pads(s.shape[0], s.shape[1], divis_by)
            chw = s.astype(np.float32).transpose(2, 0, 1)
            pair.append(np.pad(chw, ((0, 0), (pt, pb), (pl, pr)), mode="edge"))
        batch.append(np.stack(pair))
    return np.stack(batch), np.stack(u8)


def vis_oracle(disp, lut, min_val=None, max_val=None, invalid_thres=np.inf, other_output=None):
    """disp fp32 (H,W) -> uint8 (H,W,3), as Utils.py:113-133 computes it in fp32."""
    disp = np.asarray(disp, dtype=np.float32)
    H, W = disp.shape
    invalid = (disp >= np.float32(invalid_thres)) | np.isnan(disp)
    if other_output is None:
        other_output = {}
    if (~invalid).sum() == 0:
        other_output["min_val"] = other_output["max_val"] = None
        return np.zeros((H, W, 3), dtype=np.uint8)
    mn = np.float32(disp[~invalid].min() if min_val is None else min_val)
    mx = np.float32(disp[~invalid].max() if max_val is None else max_val)
    other_output["min_val"], other_output["max_val"] = mn, mx
    if mx == mn:
        idx = np.zeros((H, W), dtype=np.uint8)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((disp - mn) / (mx - mn)).clip(0, 1) * np.float32(255)
            t = np.where(invalid, np.float32(0), t)
        assert t.dtype == np.float32
        idx = t.astype(np.uint8)
    vis = np.asarray(lut, dtype=np.uint8)[idx]
    vis[invalid] = 0
    return vis
