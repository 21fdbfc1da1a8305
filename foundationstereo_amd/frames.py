"""Around the forward: camera frames to model input, and the disparity picture, on the device.

The reference's demo does both on the host (scripts/run_demo.py:131-170): gray / RGBA handling,
``cv2.resize`` by ``--scale``, ``uint8 HWC -> float CHW``, ``InputPadder(divis_by=32)`` before the
forward, ``vis_disparity`` (Utils.py:108-133) after it.  Here each end is a HIP kernel
(csrc/frames.hip) behind ``ops.frames_ingest`` / ``ops.disp_minmax`` / ``ops.disp_colorize``;
nothing synchronises the host and the disparity never leaves the device.

    fr = frames.ingest(frames.read_image("left.png"), frames.read_image("right.png"))
    disp = fr.padder.unpad(model(fr.left, fr.right, iters=32, test_mode=True).float())
    vis = frames.vis_disparity(disp[:, 0], image=fr.image_u8)
    frames.write_png("vis.png", vis[0])

Parity with ``cv2`` is unpinned in two places (cv2 does not exist in this stack): the default table
is matplotlib's turbo truncated to uint8, as the reference's own ``cmap=`` branch produces it, and
``cv2.applyColorMap(COLORMAP_TURBO)`` may differ from it by a grey level in places (``lut=`` takes
any table); and for ``scale < 1`` cv2 blends uint8 with 11-bit fixed-point weights where the kernel
blends in fp32: equal on exact ties, possibly one grey level apart elsewhere.  ``scale == 1`` and the
padding are exact.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .utils import InputPadder

Tensor = torch.Tensor

# (matplotlib.colormaps['turbo'](np.arange(256, dtype=np.uint8))[:, :3] * 255).astype(np.uint8): what
# the reference's cmap= branch (Utils.py:129-130) yields for turbo.  Data; matplotlib is not imported.
TURBO = np.frombuffer(bytes.fromhex(
    "30123b31154232184a341b51351e5836215f37236538266c3929723a2c793b2f7f3c32853c358b3d37913e3a963f3d9c"
    "4040a14043a64145ab4148b0424bb5434eba4350be4353c24456c74458cb455bce455ed24560d64563d94666dd4668e0"
    "466be3466de64670e84673eb4675ed4678f0467af2467df4467ff64682f84584f94587fb4589fc448cfd438efd4291fe"
    "4193fe4096fe3f98fe3e9bfe3c9dfd3ba0fc39a2fc38a5fb36a8f934aaf833acf631aff52fb1f32db4f12bb6ef2ab9ed"
    "28bbeb26bde925c0e623c2e421c4e120c6df1ec9dc1dcbda1ccdd71bcfd41ad1d219d3cf18d5cc18d7ca17d9c717dac4"
    "17dcc217debf18e0bd18e1ba19e3b81ae4b61be5b41de7b11ee8af20e9ac22eba924eca627eda329eea02cef9d2ff09a"
    "32f19735f39438f4913bf48d3ff58a42f68746f7834af8804df97c51f97955fa7659fb725dfb6f61fc6c65fc6869fd65"
    "6dfd6271fd5f74fe5c78fe597cfe5680fe5384fe5087fe4d8bfe4b8efe4892fe4695fe4498fe429bfd409efd3ea1fc3d"
    "a4fc3ba6fb3aa9fb39acfa37aef937b1f836b3f835b6f735b9f534bbf434bef334c0f233c3f133c5ef33c8ee33caed33"
    "cdeb34cfea34d1e834d4e735d6e535d8e335dae236dde036dfde36e1dc37e3da37e5d838e7d738e8d538ead339ecd139"
    "edcf39efcd39f0cb3af2c83af3c63af4c43af6c23af7c039f8be39f9bc39f9ba38fab737fbb537fbb336fcb035fcae34"
    "fdab33fda932fda631fda330fea12ffe9e2efe9b2dfe982cfd952bfd9229fd8f28fd8c27fc8926fc8624fb8323fb8022"
    "fa7d20fa7a1ff9771ef8741cf7711bf76e1af66b18f56817f46516f36315f26014f15d13ef5a11ee5810ed550fec520e"
    "ea500de94d0de84b0ce6490be5460ae3440ae24209e04008de3e08dd3c07db3a07d93806d73606d63405d43205d23005"
    "d02f04ce2d04cb2b03c92903c72803c52602c32402c02302be2102bb1f01b91e01b61c01b41b01b11901ae1801ac1601"
    "a91501a61401a31201a011019d10019a0e01970d01940c01910b018e0a018b09018708018407018106027d05027a0402"
), dtype=np.uint8).reshape(256, 3)

_lut_on = {}        # device -> TURBO uploaded once


@dataclass
class Frames:
    """``ingest``'s result; everything is on the device."""
    batch: Tensor           # (B,2,3,Hp,Wp) fp32, [left, right] per pair: ShardedStereo's / bench.py's layout
    left: Tensor            # batch[:, 0], a view
    right: Tensor           # batch[:, 1], a view
    image_u8: Tensor        # (B,Hs,Ws,3) uint8, the resized unpadded left frame (the reference's img0_ori)
    padder: InputPadder     # padder.unpad(disp) is scripts/run_demo.py:166
    scale: float


def _as_bhwc(x, name: str) -> Tensor:
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise RuntimeError(f"ingest: {name} must be uint8, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"ingest: {name} must be a uint8 tensor or numpy array")
    if x.dim() == 2:
        return x[None, :, :, None]
    if x.dim() == 3:
        return x[None]
    if x.dim() == 4:
        return x
    raise ValueError(f"ingest: {name} must be (H,W), (H,W,C) or (B,H,W,C), got {tuple(x.shape)}")


def ingest(left, right, *, scale: float = 1.0, divis_by: int = 32) -> Frames:
    """scripts/run_demo.py:134-159 for one pair or a batch of pairs.  ``left`` / ``right``: uint8
    (H,W), (H,W,C) or (B,H,W,C) with C in {1,3,4}, device tensors or numpy arrays (uploaded)."""
    left, right = _as_bhwc(left, "left"), _as_bhwc(right, "right")
    batch, u8 = ops.frames_ingest(left, right, scale=scale, divis_by=divis_by, want_u8=True)
    return Frames(batch=batch, left=batch[:, 0], right=batch[:, 1], image_u8=u8,
                  padder=InputPadder(u8.shape[1:3], divis_by=divis_by), scale=float(scale))


def vis_disparity(disp: Tensor, min_val: Optional[float] = None, max_val: Optional[float] = None,
                  invalid_thres: float = float("inf"), lut=None, image: Optional[Tensor] = None,
                  other_output: Optional[dict] = None) -> Tensor:
    """Utils.py:108-133 on the device.  disp (H,W), (B,H,W) or (B,1,H,W) fp32 -> uint8 (H,W,3) or
    (B,H,W,3); with ``image`` uint8 (..,H,W,3) the picture is (..,H,2W,3), the image left of the
    colours (run_demo.py:169).  ``lut``: uint8 (256,3) tensor or array, default ``TURBO``.  A dict
    passed as ``other_output`` receives the (B,2) device tensor of [min, max] under ``"minmax"``
    (no synchronisation).  Where the reference is undefined: NaN is an invalid pixel, and
    ``max == min`` maps every valid pixel to ``lut[0]``."""
    d = ops._as_bhw(disp, "vis_disparity", "disp")
    single = disp.dim() == 2
    if lut is None:
        lut = _lut_on.get(d.device)
        if lut is None and d.is_cuda:
            lut = _lut_on[d.device] = torch.from_numpy(TURBO.copy()).to(d.device)
    elif isinstance(lut, np.ndarray):
        lut = torch.from_numpy(np.ascontiguousarray(lut)).to(d.device)
    if image is not None and image.dim() == 3:
        image = image[None]
    if min_val is None or max_val is None:
        minmax = ops.disp_minmax(d, invalid_thres)
    else:
        ops._check("vis_disparity", d)
        minmax = torch.empty((d.shape[0], 2), device=d.device, dtype=torch.float32)
    if min_val is not None:
        minmax[:, 0] = float(min_val)
    if max_val is not None:
        minmax[:, 1] = float(max_val)
    out = ops.disp_colorize(d, minmax, lut, invalid_thres, image)
    if isinstance(other_output, dict):
        other_output["minmax"] = minmax
    return out[0] if single else out


def read_image(path) -> np.ndarray:
    """A frame as a uint8 array (H,W) or (H,W,C): ``.npy`` through numpy, anything else through PIL."""
    path = str(path)
    if path.lower().endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8:
            raise ValueError(f"{path}: expected a uint8 array, got {a.dtype}")
        return a
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"{path}: reading image files needs Pillow (PIL), which is not installed; "
                           "pass .npy frames instead") from e
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, rgb_u8) -> None:
    """8-bit RGB PNG of an (H,W,3) uint8 tensor or array: stdlib only (zlib + struct), filter 0 rows."""
    a = rgb_u8.detach().cpu().numpy() if isinstance(rgb_u8, torch.Tensor) else np.asarray(rgb_u8)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"write_png: expected uint8 (H,W,3), got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)         # byte 0 of a row: filter type 0 (None)
    rows[:, 1:] = a.reshape(H, 3 * W)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)     # bit depth 8, colour type 2 (RGB)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
                + _chunk(b"IEND", b""))
