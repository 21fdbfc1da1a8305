"""The non-conv backbone kernels (csrc/backbone.hip) and the small heads (csrc/heads.hip) on every code path
and guard branch vs fp64 (tests/backbone_reference.py: references, inputs, tolerances with their derivations).

* InstanceNorm: both kernels (planes in registers up to 20480 px, three passes above), the boundary, planes
  under one block, inputs whose mean is 64 standard deviations (a one-pass variance fails there), every
  (act, res, act2) the product uses, ``eps``, ``out=`` and in place, constant planes;
* channel LayerNorm: channel counts that are no multiple of the 16 channel groups, one channel, the 1024
  limit and its refusal, token windows, the affine arms, ``out=`` wider than ``n``, in place;
* attention: 1, 2, 5 and 8 key ranges, ``T == Tp``, one live key in a block / in the last range's last
  block, one key, a range that outweighs the others beyond fp32's range, the padding contract;
* XCA: 1 and 40 channels per head and the refusal at 41, fewer tokens than key splits, a 1-token tail chunk,
  zero and tiny rows, temperature 30;
* token assembly, depth-to-space and the elementwise kernel exactly; bicubic at identity size, a 4x
  downscale and sources narrower than the 4 taps; soft-argmin with the depth tail, with +-88 logits and
  one-hot; convex upsampling from one pixel up, with +-80 logits.

The case lists are module constants: tests/test_backbone_kernels_host.py checks them against the restated
dispatch and shows that ``_check`` / ``_check_exact`` / ``_check_bicubic`` refuse faulted results on them.
The worst err / tol per kernel family goes to $FSMI_PARITY_LOG.
"""
import pytest
import torch
import torch.nn.functional as F

from foundationstereo_amd import ops
from tests import backbone_reference as br

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from foundationstereo_amd import _lib
    return _lib.load()


WORST = {}       # family -> (err / tol, err, tol, case)


@pytest.fixture(scope="module", autouse=True)
def _log_worst():
    """After the module: the worst err / tol per kernel family to $FSMI_PARITY_LOG (JSON lines, the shape
    tests/test_gpu_volume.py writes)."""
    import json
    import os
    yield
    path = os.environ.get("FSMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            for fam, (ratio, err, tol, case) in sorted(WORST.items()):
                f.write(json.dumps({"test": f"backbone_kernel_{fam}", "max_abs_diff_px": err, "bound": tol,
                                    "err_over_tol": ratio, "case": case}) + "\n")


def _check(out, ref, tol, what, fam=None):
    """Every element finite and within ``tol`` of the fp64 ``ref``; returns the max error."""
    out = out.detach().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite values in the written extent"
    err = float((out.double() - ref.double()).abs().max())
    print(f"{what}: max |diff| {err:.3g} (bound {tol:.3g})")
    if fam is not None and tol > 0 and (fam not in WORST or err / tol > WORST[fam][0]):
        WORST[fam] = (err / tol, err, tol, what)
    assert err <= tol, f"{what}: max |diff| {err:.3g} > {tol:.3g}"
    return err


def _check_exact(out, ref, what):
    """Bit-for-bit the values of ``ref`` (fp32)."""
    out = out.detach().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    bad = int((out != ref).sum())
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ"


def _check_bicubic(out, x, size, what, fam=None):
    """tests/test_gpu_backbone.py's two-sided check: the reference runs the resize in fp32 (source coordinates
    from the fp32 in/out scale, one fma rounding): agree with that to rounding; against the fp64
    interpolation, be no further than the reference's own fp32 result is."""
    out = out.detach().cpu()
    ref32 = F.interpolate(x, size=size, mode="bicubic", align_corners=False)
    ref = F.interpolate(x.double(), size=size, mode="bicubic", align_corners=False)
    m = float(ref.abs().max())
    _check(out, ref32, 1e-6 + 5e-6 * float(ref32.abs().max()), what + " vs fp32", fam)
    e32 = float((ref32.double() - ref).abs().max())
    _check(out, ref, 1.1 * e32 + 2e-6 * m, what + " vs fp64")


def g(x):
    return None if x is None else x.to(DEV)


# ---------------------------------------------------------------- InstanceNorm

IN_REG, IN_3P = "reg", "three_pass"                 # instnorm_kernel<true> / <false>
# (HW, input statistics, the kernel it takes)
IN_CASES = [(hw, stats, IN_REG if hw <= 20480 else IN_3P)
            for hw in (1, 2, 63, 255, 256, 257, 20480, 20481, 76800)
            for stats in ("mean1",) + (("mean64",) if hw >= 63 else ())]
# the product's (act, res, act2): submodule.py (BasicConv_IN, Conv2x_IN, ResnetBasicBlock), extractor.py
# (ResidualBlock), backbone.py (the fusion conv); and LeakyReLU after the residual
IN_TRIPLES = [(None, False, None), ("relu", False, None), ("leaky", False, None), (None, True, "relu"),
              ("relu", True, "relu"), ("leaky", True, "leaky")]


def _in_ref(c, act, res, act2, eps=1e-5):
    return br.instnorm_ref(c["x"], act, c["res"] if res else None, act2, eps)


@pytest.mark.parametrize("HW,stats,path", IN_CASES)
def test_instance_norm(HW, stats, path):
    c = br.instnorm_inputs(HW, stats)
    x, r = g(c["x"]), g(c["res"])
    for act, res, act2 in IN_TRIPLES:
        out = ops.instance_norm(x, act=act, res=r if res else None, act2=act2)
        ref = _in_ref(c, act, res, act2)
        _check(out, ref, br.norm_tol(ref), f"instance norm HW {HW} {stats} {act}/{res}/{act2}", "instnorm_" + path)
    assert torch.equal(x.cpu(), c["x"]) and torch.equal(r.cpu(), c["res"]), "an operand was modified"


@pytest.mark.parametrize("HW", [63, 20481])
def test_instance_norm_eps(HW):
    c = br.instnorm_inputs(HW, "mean1")
    x = c["x"] * 0.01                                     # variance 4e-4: eps 1e-3 is most of the denominator
    out = ops.instance_norm(g(x), act="relu", res=g(c["res"]), act2="relu", eps=1e-3)
    ref = br.instnorm_ref(x, "relu", c["res"], "relu", 1e-3)
    assert float((ref - br.instnorm_ref(x, "relu", c["res"], "relu", 1e-5)).abs().max()) > 0.1
    _check(out, ref, br.norm_tol(ref), f"instance norm HW {HW} eps 1e-3", "instnorm_" + c["path"])


@pytest.mark.parametrize("HW", [257, 20481])
def test_instance_norm_out_and_in_place(HW):
    c = br.instnorm_inputs(HW, "mean64")
    ref = _in_ref(c, "leaky", True, "relu")
    x, r = g(c["x"]), g(c["res"])
    full = torch.full((3,) + tuple(c["x"].shape[1:]), NAN, device=DEV)       # guard images around the output
    got = ops.instance_norm(x, act="leaky", res=r, act2="relu", out=full[1:2])
    assert got.data_ptr() == full[1:2].data_ptr()
    _check(full[1:2], ref, br.norm_tol(ref), f"instance norm HW {HW} out=", "instnorm_" + c["path"])
    assert bool(torch.isnan(full[0]).all()) and bool(torch.isnan(full[2]).all()), "written outside out"
    ops.instance_norm(x, act="leaky", res=r, act2="relu", out=x)
    _check(x, ref, br.norm_tol(ref), f"instance norm HW {HW} in place", "instnorm_" + c["path"])


@pytest.mark.parametrize("HW", [1024, 32768])
def test_instance_norm_constant_plane(HW):
    """A plane of 2.0: every partial sum is an integer below 2^24, so the mean is exactly 2 and the output
    exactly 0 on both kernels."""
    out = ops.instance_norm(torch.full((1, 3, 1, HW), 2.0, device=DEV))
    _check_exact(out, torch.zeros(1, 3, 1, HW), f"constant plane HW {HW}")


# ---------------------------------------------------------------- LayerNorm

LN_WINDOWS = [(48, 48, 0), (50, 21, 7), (20, 1, 5), (37, 37, 0)]       # (Tx, n, x_offset)
# (C, Tx, n, x_offset, input statistics, affine)
LN_CASES = ([(C, Tx, n, off, "mean64" if C >= 17 else "mean0.5", "wb")
             for C in (1, 17, 48, 1000, 1024) for Tx, n, off in LN_WINDOWS]
            + [(C, 50, 21, 7, "mean64", aff) for C in (17, 1000) for aff in ("w", None)]
            + [(384, 48, 48, 0, "outlier", "wb"), (384, 50, 21, 7, "outlier", None)])


@pytest.mark.parametrize("C,Tx,n,off,stats,affine", LN_CASES)
def test_channel_layernorm(C, Tx, n, off, stats, affine):
    c = br.layernorm_inputs(C, Tx, n, off, stats, affine)
    out = ops.channel_layernorm(g(c["x"]), g(c["w"]), g(c["b"]), c["eps"], n=n, x_offset=off)
    _check(out, c["ref"], c["tol"], f"layernorm C {C} Tx {Tx} n {n} off {off} {stats} {affine}", "layernorm")


@pytest.mark.parametrize("C", [17, 1000])
def test_channel_layernorm_wider_out(C):
    """``out`` (B, C, To) with To > n: the columns >= n keep what they held, bit for bit."""
    c = br.layernorm_inputs(C, 50, 21, 7, "mean64", "wb")
    out = torch.full((2, C, 29), -7.25, device=DEV)
    ops.channel_layernorm(g(c["x"]), g(c["w"]), g(c["b"]), c["eps"], n=21, x_offset=7, out=out)
    _check(out[:, :, :21], c["ref"], c["tol"], f"layernorm C {C} To 29", "layernorm")
    _check_exact(out[:, :, 21:], torch.full((2, C, 8), -7.25), f"layernorm C {C}: columns past n")


@pytest.mark.parametrize("Tx,n", [(37, 37), (50, 21)])
def test_channel_layernorm_in_place(Tx, n):
    c = br.layernorm_inputs(48, Tx, n, 0, "mean64", "wb")
    x = g(c["x"]).clone()
    got = ops.channel_layernorm(x, g(c["w"]), g(c["b"]), c["eps"], n=n, out=x)
    assert got.data_ptr() == x.data_ptr()
    _check(x[:, :, :n], c["ref"], c["tol"], f"layernorm in place Tx {Tx} n {n}", "layernorm")
    _check_exact(x[:, :, n:], c["x"][:, :, n:], "layernorm in place: columns past n")


def test_channel_layernorm_refuses_1025_channels():
    from foundationstereo_amd import _lib
    out = torch.full((1, 1025, 4), NAN, device=DEV)
    with pytest.raises(_lib.FsmiError, match="C 1025 > 1024"):
        ops.channel_layernorm(torch.zeros((1, 1025, 4), device=DEV), out=out)
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------- attention

# (B, heads, T, Tp, key ranges, variant)
ATTN_CASES = [(1, 1, 1, 64, 1, None),                 # one live key
              (1, 2, 65, 128, 1, None),               # the second block holds one live key
              (1, 1, 448, 448, 1, None),              # T == Tp: the masking branch is never taken
              (1, 1, 449, 512, 2, None),              # one live key in the last range's last block
              (1, 1, 449, 512, 2, "dominant"),        # the second range's weight underflows in the combine
              (1, 1, 1600, 1600, 5, None),            # 6 ranges asked for, 5 returned; unmasked
              (1, 1, 1985, 2048, 8, None)]            # the maximum; one live key in the last block
ATTN_PADDING_CASES = [(1, 2, 65, 128), (1, 1, 449, 512)]


@pytest.mark.parametrize("B,heads,T,Tp,ns,variant", ATTN_CASES)
def test_vit_attention(lib, B, heads, T, Tp, ns, variant):
    assert lib.fsmi_vit_attention_ws_floats(B, heads, T, Tp) == (ns * B * heads * 66 * Tp if ns > 1 else 0)
    c = br.attention_inputs(B, heads, T, Tp, variant)
    qkv = g(c["qkv"])
    out = ops.vit_attention(qkv, heads, T, c["scale"])
    _check(out, c["ref"], c["tol"], f"attention B {B} heads {heads} T {T} Tp {Tp} {variant}", "attention")
    assert torch.equal(qkv.cpu(), c["qkv"]), "qkv was modified"


@pytest.mark.parametrize("B,heads,T,Tp", ATTN_PADDING_CASES)
def test_vit_attention_padding_contract(B, heads, T, Tp):
    """Keys >= T are masked whatever finite values the padding columns hold: with them at zero and at +-1e3
    the outputs at the queries < T are equal (a masked key's probability is an exact zero), and every output
    column, padding included, is finite.  Non-finite padding is outside the contract: the kernel's header
    says the padding stays finite, and the product guarantees it (the token assembly writes zeros there and
    every layer maps finite columns to finite columns), so none is fed here."""
    c = br.attention_inputs(B, heads, T, Tp)
    outs = [ops.vit_attention(g(br.attention_padding(c, v)), heads, T, c["scale"]).cpu() for v in (0.0, 1e3)]
    for o in outs:
        assert bool(torch.isfinite(o).all()), "non-finite output columns"
        _check(o[..., :T], c["ref"][..., :T], c["tol"], f"attention T {T} Tp {Tp}, padding replaced", "attention")
    _check_exact(outs[1][..., :T], outs[0][..., :T], "attention with padding at +-1e3 vs at zero")


# ---------------------------------------------------------------- XCA

# (C, heads, N, variant)
XCA_CASES = [(40, 1, 300, None),                      # XCA_MAXCH channels per head
             (8, 8, 64, None),                        # one channel per head
             (96, 8, 1, None), (96, 8, 5, None),      # fewer tokens than the 16 key splits: empty ranges
             (96, 8, 129, None),                      # 9 tokens per split, 15 splits used
             (24, 2, 2049, None),                     # splits of 129 tokens: a 128-token chunk and a 1-token tail
             (96, 8, 129, "rows"), (96, 8, 5, "temp30"), (40, 1, 300, "temp30")]


@pytest.mark.parametrize("C,heads,N,variant", XCA_CASES)
def test_xca(C, heads, N, variant):
    c = br.xca_inputs(C, heads, N, variant)
    out = ops.xca(g(c["qkv"]), g(c["temp"]), heads)
    _check(out, c["ref"], c["tol"], f"xca C {C} heads {heads} N {N} {variant}", "xca")


def test_xca_refuses_41_channels_per_head():
    from foundationstereo_amd import _lib
    with pytest.raises(_lib.FsmiError, match="<= 40 channels per head"):
        ops.xca(torch.zeros((1, 3 * 41, 8), device=DEV), torch.ones((1, 1, 1), device=DEV), 1)


# ---------------------------------------------------------------- token assembly, layout, elementwise

TOKEN_CASES = [(2, 5, 7, 64), (1, 3, 63, 64), (2, 4, 64, 128)]        # (B, C, N, Tp)


@pytest.mark.parametrize("B,C,N,Tp", TOKEN_CASES)
def test_vit_tokens(B, C, N, Tp):
    c = br.tokens_inputs(B, C, N, Tp)
    out = ops.vit_tokens(g(c["emb"]), g(c["cls"]), g(c["pos"]), Tp)
    _check_exact(out, c["ref"], f"tokens B {B} C {C} N {N} Tp {Tp}")


@pytest.mark.parametrize("k", [2, 4])
def test_depth_to_space(k):
    x = br.d2s_input(k)
    assert (x.numel() % 256) != 0
    _check_exact(ops.depth_to_space(g(x), k), br.depth_to_space_ref(x, k), f"depth to space k {k}")


def test_elementwise_mul_broadcast_in_place():
    a, b, b1 = br._n("ew_a", (3, 5, 7, 9)), br._n("ew_b", (3, 5, 7, 9)), br._n("ew_b1", (1, 5, 7, 9))
    _check_exact(ops.elementwise(g(a), g(b), "mul"), a * b, "mul")
    _check_exact(ops.elementwise(g(a), g(b1), "mul", broadcast=True), a * b1, "mul, broadcast")
    _check_exact(ops.elementwise(g(a), g(b1), "add", broadcast=True), a + b1, "add, broadcast at batch 3")
    _check_exact(ops.elementwise(g(a), g(b1), "add_relu", broadcast=True), F.relu(a + b1), "add_relu, broadcast")
    ad = g(a)
    got = ops.elementwise(ad, g(b), "add", out=ad)
    assert got.data_ptr() == ad.data_ptr()
    _check_exact(ad, a + b, "add in place")
    full = torch.full((3,) + tuple(a.shape), NAN, device=DEV)
    ops.elementwise(g(a), g(b), "mul", out=full[1])
    _check_exact(full[1], a * b, "mul, out=")
    assert bool(torch.isnan(full[0]).all()) and bool(torch.isnan(full[2]).all()), "written outside out"


@pytest.mark.parametrize("n", [1, 257])
def test_elementwise_sizes(n):
    a, b = br._n(f"ew_a{n}", (1, 1, 1, n)), br._n(f"ew_b{n}", (1, 1, 1, n))
    _check_exact(ops.elementwise(g(a), g(b), "mul"), a * b, f"mul n {n}")
    _check_exact(ops.elementwise(g(a), g(b), "add_relu"), F.relu(a + b), f"add_relu n {n}")
    _check_exact(ops.elementwise(g(a), op="relu"), F.relu(a), f"relu n {n}")


# ---------------------------------------------------------------- bicubic

# identity; a 4x downscale; a 1x1 source (every tap the same pixel); a 2x3 source (every tap clamped)
BICUBIC_CASES = [(32, 40, 32, 40), (64, 64, 16, 16), (1, 1, 5, 7), (2, 3, 9, 11)]


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", BICUBIC_CASES)
def test_resize_bicubic(Hi, Wi, Ho, Wo):
    x = br.bicubic_input(Hi, Wi)
    out = ops.resize_bicubic(g(x), (Ho, Wo))
    _check_bicubic(out, x, (Ho, Wo), f"bicubic {Hi}x{Wi} -> {Ho}x{Wo}", "bicubic")
    if (Hi, Wi) == (Ho, Wo):
        # at scale 1 the source coordinate is the pixel and the weights evaluate to 0, 1, 0, 0 in fp32
        _check_exact(out, x, "bicubic at identity size")
    if (Hi, Wi) == (1, 1):
        const = x.expand(-1, -1, Ho, Wo)
        _check(out, const, 1e-6 + 5e-6 * float(x.abs().max()), "bicubic of one pixel vs that pixel")


# ---------------------------------------------------------------- soft-argmin, upsampling

# (D, variant): the 8-wide main loop alone, the scalar tail alone, both
SOFTARGMIN_CASES = [(1, None), (7, None), (8, None), (9, None), (20, None), (9, "pm88"), (20, "pm88"),
                    (9, "onehot"), (20, "onehot")]


@pytest.mark.parametrize("D,variant", SOFTARGMIN_CASES)
def test_softmax_regression(D, variant):
    c = br.softargmin_inputs(D, variant)
    out = ops.softmax_regression(g(c["x"]))
    _check(out, c["ref"], br.softargmin_tol(D), f"soft-argmin D {D} {variant}", "softargmin")
    if variant == "onehot":
        _check_exact(out, c["hot"].float(), f"soft-argmin of a one-hot column D {D}")


@pytest.mark.parametrize("D,variant", SOFTARGMIN_CASES)
def test_disparity_regression(D, variant):
    c = br.softargmin_inputs(D, variant)
    out = ops.disparity_regression(g(c["prob"]), D)
    tol = br.regression_tol(D)
    if tol == 0:
        _check_exact(out, torch.zeros_like(c["ref_prob"]).float(), "regression over one plane")
    else:
        _check(out, c["ref_prob"], tol, f"regression D {D} {variant}", "regression")


# (h, w, variant)
UPSAMPLE_CASES = [(1, 1, None), (3, 5, None), (6, 10, None), (3, 5, "pm80")]


@pytest.mark.parametrize("h,w,variant", UPSAMPLE_CASES)
def test_context_upsample(h, w, variant):
    c = br.upsample_inputs(h, w, variant)
    out = ops.context_upsample(g(c["disp"]), g(c["wts"]))
    _check(out, c["ref_plain"], br.upsample_tol(False), f"upsample {h}x{w} {variant}", "upsample")
    out = ops.softmax_context_upsample(g(c["disp"]), g(c["logits"]), 4.0)
    _check(out, c["ref_softmax"], br.upsample_tol(True), f"softmax upsample {h}x{w} {variant}", "upsample_softmax")
