"""fp64 restatements of the non-conv backbone kernels (csrc/backbone.hip) and the small heads (csrc/heads.hip),
the synthetic inputs their kernel tests run on, and the tolerances.

CPU only, plain torch: shared by tests/test_gpu_backbone_kernels.py (the device comparison) and
tests/test_backbone_kernels_host.py (which pins this file to torch's own functionals, shows that a plain fp32
restatement of each operation stays inside its tolerance on these inputs, and that the comparison refuses the
faults such kernels could have).  Every function restates the operation from the reference lines the kernel
headers cite, not from the kernels.

Tolerances (``err`` is max |device - fp64| over the written extent), with the largest error of the plain fp32
restatement over the GPU test's case lists (tests/test_backbone_kernels_host.py asserts that it is inside
and prints it):

* norms (``norm_tol``): the project's 1e-5 + 2e-5 max|ref| (tests/test_gpu_backbone.py's ``_close``).  The
  inputs at mean 64 / std 1 are what tells a centred variance from E[x^2] - mean^2: the centred fp32 form
  stays within 0.23 of the tolerance (LayerNorm) and 0.11 (InstanceNorm) there, the one-pass fp32 form is
  refused on every such case.  Mean 256 would put the centred form itself at the tolerance (the mean's own
  rounding, 2^-24 * 256, is then 1.5e-5 of a unit-variance value), so 64 it is.
* attention, XCA (``attn_tol``): the project's 3e-6 + 3e-6 max|ref|.  fp32 restatement: at most 0.35 of it
  (attention), 0.34 (XCA).
* layout kernels, token assembly, elementwise: exact (``torch.equal``); one rounding or none per element.
* soft-argmin over D planes (``softargmin_tol``): (D - 1)(D + 8) 2^-24 + 1e-6.  The result is at most D - 1;
  every p_d carries a few ulp from expf and the division (8 ulp allowed) plus the D-term sum's rounding
  (D ulp).  2.1e-5 at D = 16, the figure of tests/test_gpu_parity.py's golden test.  fp32 restatement: at
  most 0.12 of it.  ``regression_tol`` for the plain sum_d d p_d on given probabilities: D products and D
  additions of partial sums below D - 1, (D - 1)(D + 1) 2^-24; fp32 restatement at most 0.18 of it.
* convex upsampling (``upsample_tol``): 1e-5 (weights given) and 2e-5 (softmax of logits, disparity times 4),
  the figures of tests/test_gpu_parity.py, at its magnitudes (disparities of std 7).  fp32 restatement:
  1.7e-6 and 8.4e-6.
* bicubic: two-sided, as tests/test_gpu_backbone.py has it (``F.interpolate`` in fp32 and fp64).
"""
import functools

import torch
import torch.nn.functional as F

from foundationstereo_amd import synth
from tests.helpers import t

ACTS = {None: lambda v: v, "relu": F.relu, "leaky": lambda v: F.leaky_relu(v, 0.01)}


def _n(name, shape, std=1.0):
    return t(synth.normal(synth.name_seed("bbk_" + name), shape, std))


# ---------------------------------------------------------------- tolerances

def norm_tol(ref):
    return 1e-5 + 2e-5 * float(ref.abs().max())


def attn_tol(ref):
    return 3e-6 + 3e-6 * float(ref.abs().max())


def softargmin_tol(D):
    return (D - 1) * (D + 8) * 2.0 ** -24 + 1e-6


def regression_tol(D):
    return (D - 1) * (D + 1) * 2.0 ** -24


def upsample_tol(softmax):
    return 2e-5 if softmax else 1e-5


# ---------------------------------------------------------------- references (fp64)

def layernorm_ref(x, w=None, b=None, eps=1e-6, n=None, x_offset=0, dtype=torch.double):
    """nn.LayerNorm over the C channels of tokens [x_offset, x_offset + n) of x (B, C, Tx) -> (B, C, n):
    biased variance of the centred values (dinov2 layers/block.py:63,75)."""
    n = x.shape[2] - x_offset if n is None else n
    v = x.to(dtype)[:, :, x_offset:x_offset + n]
    mean = v.mean(1, keepdim=True)
    d = v - mean
    y = d / ((d * d).mean(1, keepdim=True) + eps).sqrt()
    if w is not None:
        y = y * w.to(dtype).view(1, -1, 1)
    if b is not None:
        y = y + b.to(dtype).view(1, -1, 1)
    return y


def instnorm_ref(x, act=None, res=None, act2=None, eps=1e-5, dtype=torch.double):
    """act2(act(InstanceNorm2d(x)) + res) per (b, c) plane: no affine, biased variance of the centred values
    (core/submodule.py:320-385, core/extractor.py:20-80); act2 only applies with a residual."""
    v = x.to(dtype)
    mean = v.mean((2, 3), keepdim=True)
    d = v - mean
    y = ACTS[act](d / ((d * d).mean((2, 3), keepdim=True) + eps).sqrt())
    if res is not None:
        y = ACTS[act2](y + res.to(dtype))
    return y


def split_qkv(qkv, heads):
    """(q, k, v), each (B, heads, hd, Tp), of the channel-major qkv (B, 3 * heads * hd, Tp)."""
    B, C3, Tp = qkv.shape
    return qkv.view(B, 3, heads, C3 // (3 * heads), Tp).unbind(1)


def sdpa_ref(qkv, heads, T, scale, dtype=torch.double):
    """softmax(q k^T * scale) v per head over the keys < T, every one of the Tp query columns computed
    (dinov2 layers/attention.py:69-79) -> (B, heads * hd, Tp)."""
    B, C3, Tp = qkv.shape
    q, k, v = split_qkv(qkv.to(dtype), heads)
    s = torch.einsum("bhdi,bhdj->bhij", q, k[..., :T]) * scale
    p = torch.softmax(s, -1)
    return torch.einsum("bhij,bhdj->bhdi", p, v[..., :T]).reshape(B, C3 // 3, Tp)


def xca_ref(qkv, temp, heads, dtype=torch.double):
    """timm edgenext CrossCovarianceAttn's core: rows of q and k (one per channel, over the N tokens)
    normalised as F.normalize does (divided by max(|row|, 1e-12)), attn = softmax(q k^T * temperature) over
    the key channels, out = attn v.  qkv (B, 3C, N), temp (heads, 1, 1) -> (B, C, N)."""
    B, C3, N = qkv.shape
    C = C3 // 3
    q, k, v = qkv.to(dtype).view(B, 3, heads, C // heads, N).unbind(1)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    a = torch.softmax(q @ k.transpose(-2, -1) * temp.to(dtype).view(1, heads, 1, 1), -1)
    return (a @ v).reshape(B, C, N)


def tokens_ref(emb, cls, pos, Tp):
    """vision_transformer.py:214-233 with the class token stored after the N patch tokens: columns < N hold
    emb + pos, column N cls + pos, the padding columns past it exact zeros.  emb (B, C, N), cls (C,),
    pos (C, Tp) -> (B, C, Tp) in fp32 (one fp32 addition per element: exact to compare)."""
    B, C, N = emb.shape
    out = torch.zeros(B, C, Tp, dtype=torch.double)
    out[:, :, :N] = emb.double() + pos.double()[None, :, :N]
    out[:, :, N] = (cls.double().view(-1) + pos.double()[:, N])[None]
    return out.float()


def depth_to_space_ref(x, k):
    """out[b, c, y k + ky, x k + kx] = in[b, (ky k + kx) C + c, y, x] (a stride == kernel transposed conv run
    as a 1x1 conv, depth_anything/dpt.py:41-53)."""
    B, CK, H, W = x.shape
    C = CK // (k * k)
    out = torch.empty(B, C, H * k, W * k, dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            out[:, :, ky::k, kx::k] = x[:, (ky * k + kx) * C:(ky * k + kx + 1) * C]
    return out


def softargmin_ref(vol, softmax=True, dtype=torch.double):
    """sum_d d p_d over dim 1 (core/submodule.py:431-435), p = softmax(vol) (core/foundation_stereo.py:
    218-220) or vol itself -> (B, 1, H, W)."""
    p = vol.to(dtype)
    if softmax:
        p = torch.softmax(p, 1)
    d = torch.arange(vol.shape[1], dtype=dtype).view(1, -1, 1, 1)
    return (p * d).sum(1, keepdim=True)


def upsample_ref(disp, wts, softmax=False, scale=1.0, dtype=torch.double, padding="zeros"):
    """core/submodule.py:456-468: the 3x3 neighbourhood of every low-resolution disparity (zero padded),
    repeated over its 4x4 block, weighted by the 9 planes of ``wts`` (B, 9, 4h, 4w) and summed; with
    ``softmax`` the planes are logits and the disparity is scaled first (core/foundation_stereo.py:187-189).
    disp (B, 1, h, w) -> (B, 4h, 4w)."""
    b, _, h, w = disp.shape
    d = disp.to(dtype) * scale
    d = F.pad(d, (1, 1, 1, 1), mode="replicate" if padding == "replicate" else "constant")
    un = F.unfold(d, 3).reshape(b, 9, h, w)
    un = un.repeat_interleave(4, 2).repeat_interleave(4, 3)
    p = wts.to(dtype)
    if softmax:
        p = torch.softmax(p, 1)
    return (un * p).sum(1)


def _cubic_matrix(n_in, n_out, border, dtype):
    """(n_out, n_in) weights of 1D cubic convolution, A = -0.75, source (dst + 0.5) in/out - 0.5, taps
    clamped to the border (``border`` "clamp") or dropped outside it ("zero")."""
    A = -0.75
    src = (torch.arange(n_out, dtype=dtype) + 0.5) * (n_in / n_out) - 0.5
    i0 = src.floor()
    f = src - i0
    ws = [((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A,
          ((A + 2) * f - (A + 3)) * f * f + 1,
          ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1,
          ((A * (2 - f) - 5 * A) * (2 - f) + 8 * A) * (2 - f) - 4 * A]
    M = torch.zeros(n_out, n_in, dtype=dtype)
    rows = torch.arange(n_out)
    for a, wa in enumerate(ws):
        idx = i0.long() - 1 + a
        if border == "zero":
            wa = wa * ((idx >= 0) & (idx < n_in)).to(dtype)
        M.index_put_((rows, idx.clamp(0, n_in - 1)), wa, accumulate=True)
    return M


def bicubic_ref(x, size, border="clamp", dtype=torch.double):
    """F.interpolate(mode="bicubic", align_corners=False) (core/extractor.py:352) as two 1D cubic
    convolutions."""
    My = _cubic_matrix(x.shape[2], size[0], border, dtype)
    Mx = _cubic_matrix(x.shape[3], size[1], border, dtype)
    return My @ x.to(dtype) @ Mx.t()


# ---------------------------------------------------------------- dispatch, restated

IN_REG_MAX = 256 * 80          # instnorm_kernel<true>: planes held in registers


def instnorm_path(HW):
    return "reg" if HW <= IN_REG_MAX else "three_pass"


def attn_splits(B, heads, T, Tp):
    """Key ranges per (image, head, 128-query tile) and key blocks per range (``vit_attn_splits``): enough
    blocks for two per CU, at least 4 key blocks of 64 each, at most 8 ranges, none empty."""
    nkb = (T + 63) // 64
    nb = B * heads * ((Tp + 127) // 128)
    ns = min(8, (512 + nb - 1) // nb)
    ns = max(1, min(ns, nkb // 4))
    per = (nkb + ns - 1) // ns
    return (nkb + per - 1) // per, per


def attn_ws_floats(B, heads, T, Tp):
    ns, _ = attn_splits(B, heads, T, Tp)
    return ns * B * heads * 66 * Tp if ns > 1 else 0


# ---------------------------------------------------------------- inputs
# Cached: callers must not write to what they get.

@functools.lru_cache(maxsize=None)
def layernorm_inputs(C, Tx, n, off, stats, affine):
    """stats "mean64": mean 64 / std 1; "mean0.5": mean 0.5 / std 3 (tests/test_gpu_backbone.py's);
    "outlier": mean 0 / std 1 with channel 5 at 500 (the ViT's outlier channel).  affine "wb" / "w" / None."""
    tag = f"ln_{C}_{Tx}_{stats}"
    x = _n(tag + "_x", (2, C, Tx), 3.0 if stats == "mean0.5" else 1.0)
    if stats == "mean64":
        x = x + 64.0
    elif stats == "mean0.5":
        x = x + 0.5
    else:
        x[:, 5] = 500.0 + x[:, 5]
    w = _n(tag + "_w", (C,), 0.3) + 1 if affine in ("wb", "w") else None
    b = _n(tag + "_b", (C,), 0.1) if affine == "wb" else None
    c = {"C": C, "Tx": Tx, "n": n, "off": off, "stats": stats, "affine": affine, "x": x, "w": w, "b": b, "eps": 1e-6}
    c["ref"] = layernorm_ref(x, w, b, 1e-6, n, off)
    c["tol"] = norm_tol(c["ref"])
    return c


INSTNORM_PLANES = (1, 3)       # (B, C): three planes


@functools.lru_cache(maxsize=None)
def instnorm_inputs(HW, stats):
    """x (1, 3, 1, HW) at mean 64 / std 1 ("mean64") or mean 1 / std 2 ("mean1"), and a residual of std 1."""
    shape = INSTNORM_PLANES + (1, HW)
    x = _n(f"in_{HW}_{stats}_x", shape, 1.0 if stats == "mean64" else 2.0) + (64.0 if stats == "mean64" else 1.0)
    return {"HW": HW, "stats": stats, "path": instnorm_path(HW), "x": x, "res": _n(f"in_{HW}_res", shape)}


@functools.lru_cache(maxsize=None)
def attention_inputs(B, heads, T, Tp, variant=None):
    """qkv (B, 3 * heads * 64, Tp) of std 1.5, noise in the padding columns too.

    Variant "dominant": q and the keys < 256 times 6, so that the key range holding them outweighs the
    others by more than fp32's range (2^-126) for nearly every query.  That takes scores of up to ~260
    (370 in the log2 units a kernel may keep them in), where fp32 itself resolves a score to 3e-5 only: a
    score that went through four roundings is off by up to 6e-5 log2 units = 4.2e-5, and where two such
    keys nearly tie the output moves by a quarter of that times their values' difference.  No fp32 code
    could hold 3e-6 there on values of std 1.5 (the fp32 restatement measures 7e-5), so this variant's q and
    k have std 1.25 and its v std 1/32: two values differ by at most 8 / 32, the move stays below
    4.2e-5 / 4 * 0.25 = 2.6e-6, inside the absolute part of the tolerance, while a wrong or missing range
    weight still moves outputs by the values' own size, 1e4 times the tolerance."""
    qkv = _n(f"att_{B}_{heads}_{T}_{Tp}", (B, 3 * heads * 64, Tp), 1.5)
    if variant == "dominant":
        qkv = qkv * (1.25 / 1.5)
        qkv[:, 2 * heads * 64:] *= 1.5 / 1.25 / 48
        qkv[:, :heads * 64] *= 6.0
        qkv[:, heads * 64:2 * heads * 64, :256] *= 6.0
    c = {"B": B, "heads": heads, "T": T, "Tp": Tp, "variant": variant, "qkv": qkv, "scale": 0.125}
    c["ref"] = sdpa_ref(qkv, heads, T, 0.125)
    c["tol"] = attn_tol(c["ref"])
    return c


def attention_padding(c, value):
    """Case c's qkv with every column >= T at ``value`` times the sign of the noise that was there."""
    qkv = c["qkv"].clone()
    T = c["T"]
    qkv[..., T:] = torch.sign(qkv[..., T:]) * value
    return qkv


@functools.lru_cache(maxsize=None)
def xca_inputs(C, heads, N, variant=None):
    """qkv (2, 3C, N) of std 1 and temperatures around 1.  Variant "rows": in every head q's row 0 and k's
    row 1 are zero (the 1e-12 clamp) and q's row 2 is scaled by 1e-9 (a norm between the clamp and its square
    root); "temp30": temperature 30, a softmax near one-hot where the rows correlate."""
    ch = C // heads
    qkv = _n(f"xca_{C}_{heads}_{N}", (2, 3 * C, N)).clone()
    temp = _n(f"xca_{C}_{heads}_t", (heads, 1, 1), 0.5) + 1.0
    if variant == "rows":
        q, k, _ = qkv.view(2, 3, heads, ch, N).unbind(1)
        q[:, :, 0] = 0.0
        k[:, :, 1] = 0.0
        q[:, :, 2] *= 1e-9
    elif variant == "temp30":
        temp = torch.full((heads, 1, 1), 30.0)
    c = {"C": C, "heads": heads, "N": N, "variant": variant, "qkv": qkv, "temp": temp}
    c["ref"] = xca_ref(qkv, temp, heads)
    c["tol"] = attn_tol(c["ref"])
    return c


@functools.lru_cache(maxsize=None)
def tokens_inputs(B, C, N, Tp):
    """Patch embeddings, a class token, and a position table that is random in every column, the padding
    columns past N included."""
    tag = f"tok_{B}_{C}_{N}_{Tp}"
    c = {"emb": _n(tag + "_e", (B, C, N)), "cls": _n(tag + "_c", (C,)), "pos": _n(tag + "_p", (C, Tp)), "N": N, "Tp": Tp}
    c["ref"] = tokens_ref(c["emb"], c["cls"], c["pos"], Tp)
    return c


@functools.lru_cache(maxsize=None)
def softargmin_inputs(D, variant=None):
    """Logits (2, D, 3, 70) of std 2.  Variant "pm88": +88 and -88 alternating over depth (from plane 1 on
    where D > 1) under the noise, so every column holds both; "onehot": -1e4 everywhere but one plane per
    pixel at 0, where the softmax is exactly one-hot and the result exactly that plane's index."""
    shape = (2, D, 3, 70)
    x = _n(f"sa_{D}", shape, 2.0)
    hot = None
    if variant == "pm88":
        sign = torch.where(torch.arange(D) % 2 == 0, 88.0, -88.0).view(1, D, 1, 1)
        x = x * 0.01 + sign
    elif variant == "onehot":
        hot = (torch.arange(2 * 3 * 70).view(2, 1, 3, 70) * 7 + 3) % D
        x = torch.full(shape, -1e4).scatter_(1, hot, 0.0)
    c = {"D": D, "variant": variant, "x": x, "hot": hot}
    c["ref"] = softargmin_ref(x, True)
    c["prob"] = torch.softmax(x, 1)                                    # fp32 probabilities: the plain sum's input
    c["ref_prob"] = softargmin_ref(c["prob"], False)
    return c


@functools.lru_cache(maxsize=None)
def upsample_inputs(h, w, variant=None):
    """disp (2, 1, h, w) of std 7 and logits (2, 9, 4h, 4w) of std 2 (tests/test_gpu_parity.py's magnitudes);
    the weights of the plain variant are their fp32 softmax.  Variant "pm80": logits of +80 on one plane per
    pixel and -80 on the others, under noise of std 0.5."""
    tag = f"up_{h}_{w}"
    disp = _n(tag + "_d", (2, 1, h, w), 7.0)
    lg = _n(tag + "_l", (2, 9, 4 * h, 4 * w), 2.0)
    if variant == "pm80":
        hot = (torch.arange(2 * 16 * h * w).view(2, 1, 4 * h, 4 * w) * 5 + 1) % 9
        lg = lg * 0.25 + torch.full_like(lg, -80.0).scatter_(1, hot, 80.0)
    c = {"h": h, "w": w, "variant": variant, "disp": disp, "logits": lg, "wts": torch.softmax(lg, 1)}
    c["ref_plain"] = upsample_ref(disp, c["wts"])
    c["ref_softmax"] = upsample_ref(disp, lg, True, 4.0)
    return c


def bicubic_input(Hi, Wi):
    return _n(f"bic_{Hi}_{Wi}", (2, 3, Hi, Wi), 2.0)


def d2s_input(k):
    return _n(f"d2s_{k}", (2, k * k * 3, 5, 7))
