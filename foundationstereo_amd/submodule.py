"""Drop-in for ``core/submodule.py``: cost-volume functions on HIP, 3D filtering blocks.

Public names and module trees (hence ``state_dict`` keys) match the reference
so ``core.foundation_stereo`` can star-import this module instead
(SURVEY §8b).  The cost-volume functions, ``disparity_regression`` and
``context_upsample`` run the hand-written gfx950 kernels of ``libfsmi.so``.
Stride-1 3D conv blocks (``BasicConv``, ``Conv3dNormActReduced``,
``ResnetBasicBlock3D``) and stride-1 2D ``BasicConv``s run the halo split-precision
conv kernel with the eval BatchNorm folded into the packed weights (``conv3d_bn_act``,
``conv2d_bn_act``), the 3x3x3 stride-2 convs on its stride-2 tiles and the ConvTranspose3d
(k4, s2) on its 2x2x2 phase tiles; other strided convs (2D) stay on MIOpen through ``torch.nn``.
``FeatureAtt.logits`` gives the gate that the hourglass folds into its producing conv.
Under autocast the HIP paths still run (inputs cast up, fp32 compute).

The disparity transformer runs as one HIP kernel (``ops.disparity_transformer``); its
torch path uses PyTorch SDPA in place of the reference's third-party
``flash_attn_func`` (core/submodule.py:224): same softmax(QK^T/sqrt(d))V math, with
``window_size`` as a local-attention mask.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, torch_ops

__all__ = [
    "LayerNorm2d", "BasicConv", "Conv3dNormActReduced", "ResnetBasicBlock", "ResnetBasicBlock3D",
    "FlashMultiheadAttention", "FlashAttentionTransformerEncoderLayer", "UpsampleConv", "Conv2x",
    "BasicConv_IN", "Conv2x_IN", "groupwise_correlation", "build_gwc_volume", "build_concat_volume",
    "disparity_regression", "FeatureAtt", "context_upsample", "PositionalEmbedding",
    "CostVolumeDisparityAttention", "ChannelAttentionEnhancement", "SpatialAttentionExtractor",
    "EdgeNextConvEncoder",
]

_leaky = nn.LeakyReLU()  # slope 0.01, as the reference's nn.LeakyReLU() (core/submodule.py:85)


class LayerNorm2d(nn.LayerNorm):
    """Channels-first LayerNorm (core/submodule.py:29-47)."""

    def __init__(self, normalized_shape, eps=1e-6):
        super().__init__(normalized_shape, eps=eps)

    def forward(self, x):
        y = F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps)
        return y.permute(0, 3, 1, 2).contiguous()


# Module attributes that switch a HIP path off (set by tests, never read from the environment):
#   S2_3D      stride-2 convs on the halo kernel's stride-2 tiles; False: MIOpen (tests/test_gpu_fast.py's
#              and test_gpu_parity.py's reference for those tiles)
#   FATT_FUSE  FeatureAtt's sigmoid(gate) * cv in the producing conv's epilogue; False: ATen
#              (tests/test_gpu_fast.py)
#   DT_FAST    the disparity transformer on csrc/transformer.hip; False: the torch layers (tests/test_gpu_dt.py)
S2_3D = True
FATT_FUSE = True
DT_FAST = True


# Input dtypes the HIP paths accept.  Under the reference's fp16 autocast (scripts/run_demo.py:161)
# activations arriving from library ops are fp16 / bf16: they are cast up and the HIP kernels
# compute in fp32 (fp32 out), instead of dropping the layer to MIOpen fp16.
HIP_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _f32(x):
    return x if x.dtype == torch.float32 else x.float()


def _cached(mod, slot, tensors, build):
    """``build()`` (run under no_grad) cached in ``mod.__dict__[slot]`` until any of ``tensors`` (None
    entries skipped) is replaced or modified in place.  While none changes every call returns the same
    objects: captured graphs read the buffers a pack pins (``PackedConv.scale_bias``).  The key is
    (address, version) per tensor: a storage swapped through ``.data`` (``module.to(dtype)``), which keeps
    the version, onto an address the allocator recycled from the old storage is not seen."""
    key = tuple((t.data_ptr(), t._version) for t in tensors if t is not None)
    hit = mod.__dict__.get(slot)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = (key, build())
        mod.__dict__[slot] = hit
    return hit[1]


def _hip(x) -> bool:
    """The tensor half of every HIP-path test: a ROCm tensor of an accepted dtype, no grad (fp32
    compute, also under autocast)."""
    return x.is_cuda and x.dtype in HIP_DTYPES and not torch.is_grad_enabled()


def _bn_folds(bn, cls) -> bool:
    """No norm, or one that folds into the packed weights: an eval ``cls`` with running statistics."""
    return bn is None or isinstance(bn, nn.Identity) or (type(bn) is cls and not bn.training
                                                         and bn.track_running_stats)


def _conv_kind(conv):
    """The halo-kernel tile family a conv module runs on, from its attributes alone:
    's1'  stride-1 'same' Conv2d / Conv3d, 1x1 or 3x3 taps in the plane, any odd depth;
    's2'  Conv3d(k=3, s=2, p=1), Conv2d(k=3, s=2, p=1) or Conv2d(k=1, s=2, p=0);
    'up'  ConvTranspose2d / ConvTranspose3d(k=4, s=2, p=1), no output padding;
    None  anything else (dilated, grouped, other kernels or paddings, not a conv)."""
    if type(conv) not in (nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d):
        return None
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    n = len(k)
    if conv.dilation != (1,) * n or conv.groups != 1:
        return None
    if type(conv) in (nn.ConvTranspose2d, nn.ConvTranspose3d):
        return "up" if (k, s, p, conv.output_padding) == ((4,) * n, (2,) * n, (1,) * n, (0,) * n) else None
    if p != tuple(i // 2 for i in k):
        return None
    if s == (1,) * n:
        return "s1" if k[-2] == k[-1] and k[-1] in (1, 3) and k[0] % 2 == 1 else None
    if s == (2,) * n:
        return "s2" if k == (3,) * n or k == (1, 1) else None
    return None


def _route(x, conv, bn=None, nd=2):
    """``_conv_kind`` of an ``nd``-D conv (+ ``bn``) when act(bn(conv(x))) runs on the HIP conv engine
    (``conv2d_bn_act`` / ``conv2d_s2_bn_act`` / ``deconv2d_bn_act``; 3D: ``conv3d_bn_act``,
    ``ops.conv3d_up2``), else None: the layer stays on torch."""
    kind = _conv_kind(conv)
    if kind is None or len(conv.kernel_size) != nd or not _hip(x) or (kind == "s2" and not S2_3D):
        return None
    return kind if _bn_folds(bn, nn.BatchNorm3d if nd == 3 else nn.BatchNorm2d) else None


def conv2d_s2_bn_act(x, conv, bn, act=None, res=None, res_pre=False):
    """act(bn(conv(x)) [+ res]) for a stride-2 Conv2d (``_route`` 's2'): the volume kernel on
    (B, C, 1, H, W)."""
    pk, b = _packed_bn(conv, bn)
    r = None if res is None else _f32(res).unsqueeze(2)
    return ops.conv3d(_f32(x).unsqueeze(2), pk, bias=b, act=act, res=r, res_pre=res_pre, stride=2).squeeze(2)


def _conv2d_hip(conv, x):
    """conv(x) for a bare (no-norm) Conv2d / ConvTranspose2d: on the HIP conv engine where ``_route`` finds
    a tile for it, anything else (incl. fp16 output under autocast when the input is fp16) through torch."""
    kind = _route(x, conv)
    if kind == "s1":
        return conv2d_bn_act([x], conv, None)
    if kind == "s2":
        return conv2d_s2_bn_act(x, conv, None)
    if kind == "up":
        return deconv2d_bn_act(x, conv)
    return conv(x)


def run_seq(seq, x):
    """nn.Sequential forward with its bare Conv2d layers through ``_conv2d_hip`` and its InstanceNorm2d
    (+ a following ReLU / LeakyReLU) through ``ops.instance_norm``."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if type(m) is nn.Conv2d:
            x = _conv2d_hip(m, x)
        elif _hip_in(m, x):
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            act = "relu" if type(nxt) is nn.ReLU else ("leaky" if type(nxt) is nn.LeakyReLU
                                                       and nxt.negative_slope == 0.01 else None)
            x = ops.instance_norm(_f32(x), act=act, eps=m.eps)
            i += act is not None
        else:
            x = m(x)
        i += 1
    return x


def fast_up2d(x, conv, bn=None) -> bool:
    """ConvTranspose2d(k=4, s=2, p=1) (+ eval BatchNorm2d) that the 2x2 phase tiles run."""
    return _route(x, conv, bn) == "up"


def deconv2d_bn_act(x, conv, bn=None, act=None):
    """act(bn(conv_transpose2d(x))) on the 2x2 phase tiles (see ``fast_up2d``)."""
    packs, b = _packed_up(conv, bn)
    return ops.conv2d_up2(_f32(x), packs, bias=b, act=act)


def _hip_in(norm, x) -> bool:
    """An eval-style InstanceNorm2d (no affine, no running statistics: nn.InstanceNorm2d's defaults, as
    every InstanceNorm of the reference) that ``ops.instance_norm`` runs."""
    return (type(norm) is nn.InstanceNorm2d and not norm.affine and not norm.track_running_stats and _hip(x)
            and x.dim() == 4)


def _folded(conv, bn, slot, pack):
    """``(pack(sc), bias)`` of a conv with its eval BatchNorm folded in, in fp64: per output channel
    sc = gamma / sqrt(var + eps) (None without a BatchNorm) and bias = (b - mean) * sc + beta.  Cached
    on the conv module, rebuilt when any parameter or running statistic changes."""
    is_bn = isinstance(bn, (nn.BatchNorm2d, nn.BatchNorm3d))

    def build():
        b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(
            conv.out_channels, dtype=torch.float64, device=conv.weight.device)
        sc = None
        if is_bn:
            sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            b = (b - bn.running_mean.double()) * sc + bn.bias.double()
        return pack(sc), b.float().contiguous()

    return _cached(conv, slot, [conv.weight, conv.bias] + (
        [bn.weight, bn.bias, bn.running_mean, bn.running_var] if is_bn else []), build)


def _packed_up(conv, bn):
    """The 8 (4) phase packs of a ConvTranspose3d (2d) with its eval BatchNorm folded, and the bias."""
    pack = ops.pack_deconv2d_phases if conv.weight.dim() == 4 else ops.pack_deconv_phases
    return _folded(conv, bn, "_fsmi_pack_up", lambda sc: pack(conv.weight, sc))


def _packed_bn(conv, bn):
    """Halo-kernel weights of a Conv2d / Conv3d with its eval BatchNorm folded in, and the bias."""
    def pack(sc):
        w = conv.weight.detach().double()
        if sc is not None:
            w = w * sc.view((-1,) + (1,) * (w.dim() - 1))
        return ops.PackedConv(w.float(), mode="halo")
    return _folded(conv, bn, "_fsmi_pack_bn", pack)


def conv2d_bn_act(segs, conv, bn, act=None, **kw):
    """act(bn(conv(cat(segs)))) on the 2D halo kernel (``_route`` 's1'); ``segs`` as ops.conv2d."""
    pk, b = _packed_bn(conv, bn)
    segs = [_f32(s) if isinstance(s, torch.Tensor) else (_f32(s[0]),) + tuple(s[1:]) for s in segs]
    return ops.conv2d(segs, pk, bias=b, act=act, **kw)


def conv3d_bn_act(x, conv, bn, act=None, res=None, res_pre=False, fatt=None):
    """act(bn(conv(x)) [+ res]) [* sigmoid(fatt)] on the halo kernel (``_route`` 's1' / 's2' of a
    Conv3d; the conv's stride is taken from the module)."""
    pk, b = _packed_bn(conv, bn)
    return ops.conv3d(_f32(x), pk, bias=b, act=act, res=None if res is None else _f32(res), res_pre=res_pre,
                      stride=conv.stride[0], fatt=None if fatt is None else _f32(fatt))


def _norm(kind, ch, is_3d):
    if kind == "batch":
        return nn.BatchNorm3d(ch) if is_3d else nn.BatchNorm2d(ch)
    return nn.InstanceNorm3d(ch) if is_3d else nn.InstanceNorm2d(ch)


class BasicConv(nn.Module):
    """conv (no bias) -> BN/IN -> LeakyReLU(0.01)  (core/submodule.py:51-86)."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, bn=True, relu=True, norm="batch",
                 **kwargs):
        super().__init__()
        self.relu = relu
        self.use_bn = bn
        self.bn = nn.Identity()
        conv_t = {(False, False): nn.Conv2d, (False, True): nn.ConvTranspose2d,
                  (True, False): nn.Conv3d, (True, True): nn.ConvTranspose3d}[(is_3d, deconv)]
        self.conv = conv_t(in_channels, out_channels, bias=False, **kwargs)
        if bn:
            self.bn = _norm(norm, out_channels, is_3d)

    def forward(self, x):
        bn = self.bn if self.use_bn else None
        act = "leaky" if self.relu else None
        nd = self.conv.weight.dim() - 2
        kind = _route(x, self.conv, bn, nd)
        if nd == 3 and kind == "up":                # ConvTranspose3d k4 s2: 8 phase convs, BN folded
            packs, b = _packed_up(self.conv, bn)
            return ops.conv3d_up2(_f32(x), packs, bias=b, act=act)
        if nd == 3 and kind:                        # 3D conv (stride 1 / 2) + folded BN + LeakyReLU
            return conv3d_bn_act(x, self.conv, bn, act)
        if kind == "s1":
            return conv2d_bn_act([x], self.conv, bn, act)
        if kind == "up":                            # ConvTranspose2d k4 s2: 4 phase convs, BN folded
            return deconv2d_bn_act(x, self.conv, bn, act)
        # (a stride-2 Conv2d + BatchNorm stays on MIOpen here; ResidualBlock runs the context net's)
        if bn is not None and _hip_in(bn, x) and _route(x, self.conv):
            # norm='instance': conv, then InstanceNorm + LeakyReLU
            return ops.instance_norm(_conv2d_hip(self.conv, x), act=act, eps=bn.eps)
        x = self.bn(self.conv(x)) if self.use_bn else self.conv(x)
        return F.leaky_relu(x, 0.01) if self.relu else x


class Conv3dNormActReduced(nn.Module):
    """Axial-planar conv: (1,k,k)+BN+ReLU then (kd,1,1)+BN+ReLU (core/submodule.py:89-114)."""

    def __init__(self, C_in, C_out, hidden=None, kernel_size=3, kernel_disp=None, stride=1, norm=nn.BatchNorm3d):
        super().__init__()
        kd = kernel_size if kernel_disp is None else kernel_disp
        hidden = C_out if hidden is None else hidden
        k = kernel_size
        self.conv1 = nn.Sequential(
            nn.Conv3d(C_in, hidden, kernel_size=(1, k, k), padding=(0, k // 2, k // 2), stride=(1, stride, stride)),
            norm(hidden), nn.ReLU())
        self.conv2 = nn.Sequential(
            nn.Conv3d(hidden, C_out, kernel_size=(kd, 1, 1), padding=(kd // 2, 0, 0), stride=(stride, 1, 1)),
            norm(C_out), nn.ReLU())

    def forward(self, x, fatt=None):
        """``fatt``: a following FeatureAtt's pre-sigmoid gate (``FeatureAtt.logits``), applied in the
        second conv's epilogue (returns sigmoid(fatt).unsqueeze(2) * block(x))."""
        c1, c2 = self.conv1, self.conv2
        if _route(x, c1[0], c1[1], 3) == "s1" and _route(x, c2[0], c2[1], 3) == "s1" \
                and isinstance(c1[2], nn.ReLU) and isinstance(c2[2], nn.ReLU):
            y = conv3d_bn_act(x, c1[0], c1[1], "relu")
            return conv3d_bn_act(y, c2[0], c2[1], "relu", fatt=fatt)
        y = self.conv2(self.conv1(x))
        return y if fatt is None else torch.sigmoid(fatt).unsqueeze(2) * y


class _ResBlock(nn.Module):
    _conv = nn.Conv2d
    _bn = nn.BatchNorm2d

    def __init__(self, inplanes, planes, kernel_size=3, stride=1, padding=1, downsample=None, groups=1,
                 base_width=64, dilation=1, norm_layer="default", bias=False):
        super().__init__()
        norm_layer = self._bn if norm_layer == "default" else norm_layer
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        if dilation > 1:
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock")
        self.norm_layer = norm_layer
        self.conv1 = self._conv(inplanes, planes, kernel_size=kernel_size, stride=stride, bias=bias, padding=padding)
        if norm_layer is not None:
            self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = self._conv(planes, planes, kernel_size=kernel_size, stride=stride, bias=bias, padding=padding)
        if norm_layer is not None:
            self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x, fatt=None):
        """``fatt`` (3D blocks): a following FeatureAtt's pre-sigmoid gate, applied in conv2's epilogue
        (returns sigmoid(fatt).unsqueeze(2) * block(x))."""
        bn1 = self.bn1 if self.norm_layer is not None else None
        bn2 = self.bn2 if self.norm_layer is not None else None
        if self.downsample is None and _route(x, self.conv1, bn1, 3) == "s1" \
                and _route(x, self.conv2, bn2, 3) == "s1":
            y = conv3d_bn_act(x, self.conv1, bn1, "relu")
            # relu(bn2(conv2) + x) [* sigmoid(fatt)]
            return conv3d_bn_act(y, self.conv2, bn2, "relu", res=x, res_pre=True, fatt=fatt)
        if (self.downsample is None and fatt is None and bn1 is not None and _hip_in(bn1, x) and _hip_in(bn2, x)
                and _route(x, self.conv1) == "s1" and _route(x, self.conv2) == "s1"):
            # InstanceNorm variant (Conv2x_IN's conv2): relu(IN(conv2(relu(IN(conv1 x)))) + x)
            x = _f32(x)
            y = ops.instance_norm(conv2d_bn_act([x], self.conv1, None), act="relu", eps=bn1.eps)
            return ops.instance_norm(conv2d_bn_act([y], self.conv2, None), res=x, act2="relu", eps=bn2.eps)
        if fatt is not None:
            return torch.sigmoid(fatt).unsqueeze(2) * self.forward(x)
        y = self.conv1(x)
        if self.norm_layer is not None:
            y = self.bn1(y)
        y = F.relu(y)
        y = self.conv2(y)
        if self.norm_layer is not None:
            y = self.bn2(y)
        skip = x if self.downsample is None else self.downsample(x)
        return F.relu(y + skip)


class ResnetBasicBlock(_ResBlock):
    """core/submodule.py:119-156."""


class ResnetBasicBlock3D(_ResBlock):
    """core/submodule.py:159-195."""
    _conv = nn.Conv3d
    _bn = nn.BatchNorm3d


class FlashMultiheadAttention(nn.Module):
    """core/submodule.py:198-229 with SDPA as the attention kernel."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.embed_dim = embed_dim
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == self.embed_dim, "embed_dim must be divisible by num_heads"
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)

    def forward(self, query, key, value, attn_mask=None, window_size=(-1, -1)):
        B, L, C = query.shape

        def heads(t):
            return t.view(B, -1, self.num_heads, self.head_dim).transpose(1, 2)

        mask = None
        if tuple(window_size) != (-1, -1):
            # flash_attn_func(window_size=(left, right)) (core/submodule.py:224): query i sees keys
            # j with i - left <= j <= i + right; -1 leaves that side unbounded
            left, right = window_size
            i = torch.arange(L, device=query.device)[:, None]
            j = torch.arange(key.shape[1], device=query.device)[None, :]
            mask = torch.ones(L, key.shape[1], dtype=torch.bool, device=query.device)
            if left >= 0:
                mask &= j >= i - left
            if right >= 0:
                mask &= j <= i + right
        o = F.scaled_dot_product_attention(heads(self.q_proj(query)), heads(self.k_proj(key)),
                                           heads(self.v_proj(value)), attn_mask=mask)
        return self.out_proj(o.transpose(1, 2).reshape(B, L, C))


class FlashAttentionTransformerEncoderLayer(nn.Module):
    """Post-norm encoder layer (core/submodule.py:233-257); dropout is identity in eval."""

    def __init__(self, embed_dim, num_heads, dim_feedforward, dropout=0.1, act=nn.GELU, norm=nn.LayerNorm):
        super().__init__()
        self.self_attn = FlashMultiheadAttention(embed_dim, num_heads)
        self.act = act()
        self.linear1 = nn.Linear(embed_dim, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, embed_dim)
        self.norm1 = norm(embed_dim)
        self.norm2 = norm(embed_dim)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, src, src_mask=None, window_size=(-1, -1)):
        src = self.norm1(src + self.dropout1(self.self_attn(src, src, src, src_mask, window_size=window_size)))
        ff = self.linear2(self.dropout(self.act(self.linear1(src))))
        return self.norm2(src + self.dropout2(ff))


class UpsampleConv(nn.Module):
    """core/submodule.py:261-277."""

    def __init__(self, C_in, C_out, is_3d=False, kernel_size=3, bias=True, stride=1, padding=1):
        super().__init__()
        self.is_3d = is_3d
        conv = nn.Conv3d if is_3d else nn.Conv2d
        self.conv = conv(C_in, C_out, kernel_size=kernel_size, stride=1, padding=kernel_size // 2, bias=bias)

    def forward(self, x):
        mode = "trilinear" if self.is_3d else "bilinear"
        return self.conv(F.interpolate(x, scale_factor=2, align_corners=False, mode=mode))


class Conv2x(nn.Module):
    """core/submodule.py:281-317."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, concat=True, keep_concat=True, bn=True,
                 relu=True, keep_dispc=False):
        super().__init__()
        self.concat = concat
        self.is_3d = is_3d
        kernel = (4, 4, 4) if (deconv and is_3d) else (4 if deconv else 3)
        if deconv and is_3d and keep_dispc:
            self.conv1 = BasicConv(in_channels, out_channels, deconv, is_3d, bn=bn, relu=True, kernel_size=(1, 4, 4),
                                   stride=(1, 2, 2), padding=(0, 1, 1))
        else:
            self.conv1 = BasicConv(in_channels, out_channels, deconv, is_3d, bn=bn, relu=True, kernel_size=kernel,
                                   stride=2, padding=1)
        if concat:
            mul = 2 if keep_concat else 1
            self.conv2 = BasicConv(out_channels * 2, out_channels * mul, False, is_3d, bn, relu, kernel_size=3,
                                   stride=1, padding=1)
        else:
            self.conv2 = BasicConv(out_channels, out_channels, False, is_3d, bn, relu, kernel_size=3, stride=1,
                                   padding=1)

    def forward(self, x, rem):
        x = self.conv1(x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="bilinear")
        c2 = self.conv2
        bn2 = c2.bn if c2.use_bn else None
        if self.concat and not self.is_3d and x.shape[1] % 8 == 0 and _route(x, c2.conv, bn2) == "s1":
            # the cat read in place: conv2's input is the two segments (x, rem)
            return conv2d_bn_act([x, rem], c2.conv, bn2, "leaky" if c2.relu else None)
        x = torch.cat((x, rem), 1) if self.concat else x + rem
        return self.conv2(x)


class BasicConv_IN(nn.Module):
    """conv -> InstanceNorm -> LeakyReLU (core/submodule.py:320-346)."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, IN=True, relu=True, **kwargs):
        super().__init__()
        self.relu = relu
        self.use_in = IN
        conv_t = {(False, False): nn.Conv2d, (False, True): nn.ConvTranspose2d,
                  (True, False): nn.Conv3d, (True, True): nn.ConvTranspose3d}[(is_3d, deconv)]
        self.conv = conv_t(in_channels, out_channels, bias=False, **kwargs)
        self.IN = nn.InstanceNorm3d(out_channels) if is_3d else nn.InstanceNorm2d(out_channels)

    def forward(self, x):
        if self.use_in and _hip_in(self.IN, x) and _route(x, self.conv):
            return ops.instance_norm(_conv2d_hip(self.conv, x), act="leaky" if self.relu else None, eps=self.IN.eps)
        x = _conv2d_hip(self.conv, x)
        if self.use_in:
            x = self.IN(x)
        return F.leaky_relu(x, 0.01) if self.relu else x


class Conv2x_IN(nn.Module):
    """core/submodule.py:349-385."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, concat=True, keep_concat=True, IN=True,
                 relu=True, keep_dispc=False):
        super().__init__()
        self.concat = concat
        self.is_3d = is_3d
        kernel = (4, 4, 4) if (deconv and is_3d) else (4 if deconv else 3)
        if deconv and is_3d and keep_dispc:
            self.conv1 = BasicConv_IN(in_channels, out_channels, deconv, is_3d, IN=True, relu=True,
                                      kernel_size=(1, 4, 4), stride=(1, 2, 2), padding=(0, 1, 1))
        else:
            self.conv1 = BasicConv_IN(in_channels, out_channels, deconv, is_3d, IN=True, relu=True,
                                      kernel_size=kernel, stride=2, padding=1)
        if concat:
            mul = 2 if keep_concat else 1
            self.conv2 = ResnetBasicBlock(out_channels * 2, out_channels * mul, kernel_size=3, stride=1, padding=1,
                                          norm_layer=nn.InstanceNorm2d)
        else:
            self.conv2 = BasicConv_IN(out_channels, out_channels, False, is_3d, IN, relu, kernel_size=3, stride=1,
                                      padding=1)

    def forward(self, x, rem):
        x = self.conv1(x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="bilinear")
        x = torch.cat((x, rem), 1) if self.concat else x + rem
        return self.conv2(x)


# ---------------------------------------------------------------- HIP hot path
# The reference-API functions below dispatch through the registered operators torch.ops.fsmi.*
# (csrc/torch_ops.cpp); the fused model internals call the C ABI through ops.py.

def groupwise_correlation(fea1, fea2, num_groups):
    """core/submodule.py:388-397: the d=0 slice of the gwc volume, (B,G,H,W)."""
    B, C, H, W = fea1.shape
    assert C % num_groups == 0, f"C:{C}, num_groups:{num_groups}"
    fea1, fea2 = fea1.float(), fea2.float()
    return torch_ops.op("gwc_volume", fea1, fea2)(fea1, fea2, 1, num_groups)[:, :, 0]


def build_gwc_volume(refimg_fea, targetimg_fea, maxdisp, num_groups, stride=1):
    """core/submodule.py:399-412 on the gfx950 kernel; fp32 out (the reference
    computes the correlation in fp32 and stores it in the input dtype)."""
    B, C, H, W = refimg_fea.shape
    assert C % num_groups == 0, f"C:{C}, num_groups:{num_groups}"
    fl, fr = refimg_fea.float(), targetimg_fea.float()
    out = torch_ops.op("gwc_volume", fl, fr)(fl, fr, maxdisp, num_groups)
    return out if refimg_fea.dtype == torch.float32 else out.to(refimg_fea.dtype)


def build_concat_volume(refimg_fea, targetimg_fea, maxdisp):
    """core/submodule.py:416-427 on the gfx950 kernel."""
    pl, pr = refimg_fea.float(), targetimg_fea.float()
    out = torch_ops.op("concat_volume", pl, pr)(pl, pr, maxdisp)
    return out if refimg_fea.dtype == torch.float32 else out.to(refimg_fea.dtype)


def disparity_regression(x, maxdisp):
    """core/submodule.py:431-435."""
    assert len(x.shape) == 4
    xf = x.float()
    out = torch_ops.op("disparity_regression", xf)(xf, maxdisp)
    return out if x.dtype == torch.float32 else out.to(x.dtype)


def context_upsample(disp_low, up_weights):
    """core/submodule.py:456-468."""
    d, w = disp_low.float(), up_weights.float()
    return torch_ops.op("context_upsample", d, w)(d, w)


class FeatureAtt(nn.Module):
    """sigmoid(conv1x1(LReLU(BN(conv1x1 feat)))) * cv  (core/submodule.py:438-454)."""

    def __init__(self, cv_chan, feat_chan):
        super().__init__()
        self.feat_att = nn.Sequential(BasicConv(feat_chan, feat_chan // 2, kernel_size=1, stride=1, padding=0),
                                      nn.Conv2d(feat_chan // 2, cv_chan, 1))

    def logits(self, feat):
        """feat_att(feat): the pre-sigmoid gate (B, cv_chan, H, W); both 1x1 convs on the halo kernel
        when they qualify (the hourglass folds sigmoid(gate) * cv into the producing conv)."""
        c0, c1 = self.feat_att
        h = c0(feat)
        return conv2d_bn_act([h], c1, None) if _route(h, c1) == "s1" else c1(h)

    def forward(self, cv, feat):
        return torch.sigmoid(self.logits(feat)).unsqueeze(2) * cv


class PositionalEmbedding(nn.Module):
    """Fixed sin/cos table (core/submodule.py:472-502); not a buffer, as in the reference."""

    def __init__(self, d_model, max_len=512):
        super().__init__()
        pos = torch.arange(0, max_len).float().unsqueeze(1)
        div = (torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model)).exp()[None]
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self.pe = pe.unsqueeze(0)

    def forward(self, x, resize_embed=False):
        self.pe = self.pe.to(x.device).to(x.dtype)
        pe = self.pe
        if pe.shape[1] < x.shape[1]:
            if not resize_embed:
                raise RuntimeError(f"x:{x.shape}, pe:{pe.shape}")
            pe = F.interpolate(pe.permute(0, 2, 1), size=x.shape[1], mode="linear", align_corners=False).permute(0, 2, 1)
        return x + pe[:, :x.size(1)]


class CostVolumeDisparityAttention(nn.Module):
    """Transformer over disparity tokens (core/submodule.py:506-528)."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout=0.1, act=nn.GELU, norm_first=False, num_transformer=6,
                 max_len=512, resize_embed=False):
        super().__init__()
        self.resize_embed = resize_embed
        self.sa = nn.ModuleList([FlashAttentionTransformerEncoderLayer(embed_dim=d_model, num_heads=nhead,
                                                                       dim_feedforward=dim_feedforward, act=act,
                                                                       dropout=dropout)
                                 for _ in range(num_transformer)])
        self.pos_embed0 = PositionalEmbedding(d_model, max_len=max_len)

    def _fast(self, cv, window_size=(-1, -1)) -> bool:
        if not (DT_FAST and _hip(cv) and window_size == (-1, -1)) or self.training:
            return False
        a = self.sa[0].self_attn if len(self.sa) else None
        return (a is not None and cv.shape[1] == 28 and a.num_heads == 4 and self.sa[0].linear1.out_features == 28
                and type(self.sa[0].act) is nn.GELU and self.sa[0].act.approximate == "none"
                and 1 <= cv.shape[2] <= 64 and all(m.norm1.eps == m.norm2.eps == self.sa[0].norm1.eps
                                                   for m in self.sa))

    def _packed(self):
        return _cached(self, "_fsmi_pack", [t for m in self.sa for t in m.parameters()],
                       lambda: ops.pack_dt_layers(list(self.sa)))

    def forward(self, cv, window_size=(-1, -1)):
        B, C, D, H, W = cv.shape
        if self._fast(cv, tuple(window_size)):
            # one HIP kernel for PE + all encoder layers (csrc/transformer.hip), fp32
            cv = _f32(cv)
            pe = self.pos_embed0.pe.to(cv.device, cv.dtype)
            self.pos_embed0.pe = pe
            if pe.shape[1] < D:
                if not self.resize_embed:
                    raise RuntimeError(f"x:{(B * H * W, D, C)}, pe:{tuple(pe.shape)}")
                pe = F.interpolate(pe.permute(0, 2, 1), size=D, mode="linear", align_corners=False).permute(0, 2, 1)
            eps = self.sa[0].norm1.eps
            return ops.disparity_transformer(cv, self._packed(), pe[0, :D].contiguous(), 4, 28, len(self.sa), eps)
        x = cv.permute(0, 3, 4, 2, 1).reshape(B * H * W, D, C)
        x = self.pos_embed0(x, resize_embed=self.resize_embed)
        for layer in self.sa:
            x = layer(x, window_size=window_size)
        return x.reshape(B, H, W, D, C).permute(0, 4, 3, 1, 2)


class ChannelAttentionEnhancement(nn.Module):
    """core/submodule.py:532-547."""

    def __init__(self, in_planes, ratio=16):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.fc = nn.Sequential(nn.Conv2d(in_planes, in_planes // 16, 1, bias=False), nn.ReLU(),
                                nn.Conv2d(in_planes // 16, in_planes, 1, bias=False))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        # global pools as plain reductions: identical values to AdaptiveAvg/MaxPool2d(1), and
        # the ROCm adaptive-max kernel takes ~0.7 ms on a (1,128,120,160) map
        return self.sigmoid(self.fc(x.mean((2, 3), keepdim=True)) + self.fc(x.amax((2, 3), keepdim=True)))


class SpatialAttentionExtractor(nn.Module):
    """core/submodule.py:549-561."""

    def __init__(self, kernel_size=7):
        super().__init__()
        self.samconv = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        t = torch.cat([x.mean(1, keepdim=True), x.amax(1, keepdim=True)], 1)
        return self.sigmoid(self.samconv(t))


class EdgeNextConvEncoder(nn.Module):
    """Depthwise 7x7 + inverted-bottleneck MLP, residual (core/submodule.py:565-591)."""

    def __init__(self, dim, layer_scale_init_value=1e-6, expan_ratio=4, kernel_size=7, norm="layer"):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=kernel_size, padding=kernel_size // 2, groups=dim)
        self.norm = LayerNorm2d(dim, eps=1e-6) if norm == "layer" else nn.Identity()
        self.pwconv1 = nn.Linear(dim, expan_ratio * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(expan_ratio * dim, dim)
        self.gamma = (nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True)
                      if layer_scale_init_value > 0 else None)

    def forward(self, x):
        y = self.norm(self.dwconv(x)).permute(0, 2, 3, 1)
        y = self.pwconv2(self.act(self.pwconv1(y)))
        if self.gamma is not None:
            y = self.gamma * y
        return x + y.permute(0, 3, 1, 2)
