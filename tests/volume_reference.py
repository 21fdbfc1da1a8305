"""fp64 restatement of the stride-1 volume conv (``fsmi_conv3d_halo_x3_ex``: the ``D3`` instantiation of
csrc/conv_halo.h) with its epilogues, the synthetic inputs the volume tests run on, and their tolerances.

CPU only, plain torch: shared by tests/test_gpu_volume.py (the device comparison) and
tests/test_volume_host.py (which pins this file to the product's own torch modules and shows that the
comparison discriminates).

Epilogue order, as ``store_frag_c`` documents it: with ``res_pre`` (ResnetBasicBlock3D's tail) act(pre +
res), otherwise act(pre) + res; then times sigmoid(fatt) broadcast over depth (FeatureAtt folded into the
producing conv).

Tolerance, derived: the project's bound for a split-precision conv holds for the pre-activation,
e = 2e-5 + 1e-5 max|pre_ref|.  Every epilogue here is 1-Lipschitz in ``pre`` (ReLU, LeakyReLU, identity,
a residual added on either side) and the gate factor is at most 1, so the output moves by at most e; the
device's few fp32 operations after the conv sum (residual add, expf, one product) add 8 * 2^-24 max|ref|,
the same fp32 term as ``gate_reference.gate_tol``.

Ladder inputs exercise range mode 1 (a block exponent per (kd, 32-channel chunk) pair, ``rescale_acc`` on
the accumulators when a chunk does not fit the current one): depth plane d is scaled by 2^(6 d) ("asc"),
2^(-6 d) ("desc") or 2^(-6 |d - D // 2|) ("peak"), and with 72 input channels channel chunk c by
2^(6 c) on top, so the exponent moves both inside one kd plane and from plane to plane, and the partial sum
in the accumulators at a rescale is 2^-6 of the output, not below its rounding.  Their bound is taken per
(batch, output depth) plane, 3e-6 max|ref over that plane| -- the project's figure for the split's range
tests (``test_conv3d_halo_range``), per plane so that a small plane cannot hide behind a large one.
"""
import functools
import math

import torch
import torch.nn.functional as F

from foundationstereo_amd import synth
from tests.helpers import t

B = 2
# name -> (act, residual: None / "post" / "pre", FeatureAtt gate)
EPILOGUES = {
    "leaky": ("leaky", None, False),
    "none_res_post": (None, "post", False),
    "relu_res_pre": ("relu", "pre", False),
    "relu_fatt": ("relu", None, True),
    "relu_res_pre_fatt": ("relu", "pre", True),
    # a residual after a nonlinearity: with act None the two residual orders are the same function
    "leaky_res_post": ("leaky", "post", False),
}
ACTS = {None: lambda v: v, "relu": F.relu, "leaky": lambda v: F.leaky_relu(v, 0.01)}
LADDER_KINDS = ("asc", "desc", "peak")
LADDER_STEP = 6          # log2 of the scale step between neighbouring planes / channel chunks
PLANE_RTOL = 3e-6


def volume_reference(x, w, bias=None, act=None, res=None, res_pre=False, fatt=None):
    """(pre, ref) of a 'same' stride-1 Conv3d in fp64: ``pre`` = conv3d(x, w) + bias, ``ref`` the epilogue
    on it (module docstring).  ``fatt`` (B, Cout, H, W) is the pre-sigmoid gate."""
    d = torch.double
    pad = tuple(k // 2 for k in w.shape[2:])
    pre = F.conv3d(x.to(d), w.to(d), None if bias is None else bias.to(d), padding=pad)
    if res is not None and res_pre:
        ref = ACTS[act](pre + res.to(d))
    else:
        ref = ACTS[act](pre)
        if res is not None:
            ref = ref + res.to(d)
    if fatt is not None:
        ref = ref * torch.sigmoid(fatt.to(d)).unsqueeze(2)
    return pre, ref


def volume_tol(pre_ref, ref):
    return 2e-5 + 1e-5 * float(pre_ref.abs().max()) + 8 * 2.0 ** -24 * float(ref.abs().max())


def _n(name, shape, std=1.0):
    return t(synth.normal(synth.name_seed(name), shape, std))


def _tag(kern, cin, cout, D, H, W):
    return f"k{kern[0]}{kern[1]}{kern[2]}_ci{cin}_co{cout}_{D}x{H}x{W}"


@functools.lru_cache(maxsize=None)
def _base(kern, cin, cout, D, H, W):
    """What every epilogue of one shape shares: x, w, bias, the fp64 conv, a residual of the conv's own
    std and a gate of std 1.5."""
    tag = "vol_" + _tag(kern, cin, cout, D, H, W)
    taps = kern[0] * kern[1] * kern[2]
    c = {"kern": kern, "cin": cin, "cout": cout, "shape": (D, H, W),
         "x": _n(tag + "_x", (B, cin, D, H, W)),
         "w": _n(tag + "_w", (cout, cin) + tuple(kern), 1 / math.sqrt(cin * taps)),
         "bias": _n(tag + "_b", (cout,), 0.1)}
    c["pre"], _ = volume_reference(c["x"], c["w"], c["bias"])
    c["res"] = _n(tag + "_res", (B, cout, D, H, W), float(c["pre"].std()))
    c["fatt"] = _n(tag + "_fatt", (B, cout, H, W), 1.5)
    return c


@functools.lru_cache(maxsize=None)
def volume_inputs(kern, cin, cout, D, H, W, epi):
    """The synthetic operands of one volume conv (fp32, CPU), its fp64 reference under epilogue ``epi``
    (a key of EPILOGUES) and the tolerance.  Weights of std 1/sqrt(Cin taps) and a bias of std 0.1 keep
    the pre-activation around zero at unit scale.  Cached: every tile / split of a shape shares one
    reference (and the epilogues of a shape one conv); callers must not write to what they get."""
    act, rmode, gated = EPILOGUES[epi]
    base = _base(tuple(kern), cin, cout, D, H, W)
    c = {k: v for k, v in base.items() if k not in ("res", "fatt")}
    c.update(epi=epi, act=act, res_pre=rmode == "pre",
             res=base["res"] if rmode else None, fatt=base["fatt"] if gated else None)
    _, c["ref"] = volume_reference(c["x"], c["w"], c["bias"], act, c["res"], c["res_pre"], c["fatt"])
    c["tol"] = volume_tol(c["pre"], c["ref"])
    arg = c["pre"] + c["res"].double() if c["res_pre"] else c["pre"]
    c["pos_share"] = float((arg > 0).double().mean())
    c["gate_sat"] = float((c["fatt"].abs() > 4).double().mean()) if gated else 0.0
    return c


def assert_exercised(c):
    """The activation must see both signs and the gate its slope: a ReLU that is all on / all off, or a
    saturated sigmoid, hides a wrong sum."""
    assert 0.3 <= c["pos_share"] <= 0.7, f"share of positive activation arguments {c['pos_share']:.3g}"
    assert c["gate_sat"] < 0.01, f"share of |gate| > 4: {c['gate_sat']:.3g}"


def ladder_scales(kind, cin, D):
    """log2 of the scale of (depth plane d, input channel ci): (D, cin) integers."""
    d = torch.arange(D)
    plane = {"asc": d, "desc": -d, "peak": -(d - D // 2).abs()}[kind] * LADDER_STEP
    chunk = (torch.arange(cin) // 32) * LADDER_STEP if cin == 72 else torch.zeros(cin, dtype=torch.long)
    return plane.view(D, 1) + chunk.view(1, cin)


@functools.lru_cache(maxsize=None)
def ladder_inputs(kind, kern, cin, cout, D, H, W):
    """A conv without bias or epilogue whose input planes and channel chunks step by 2^6 (module
    docstring), and its fp64 reference.  Scaling by exact powers of two keeps x an fp32 tensor."""
    assert kind in LADDER_KINDS
    tag = f"ladder_{kind}_" + _tag(kern, cin, cout, D, H, W)
    taps = kern[0] * kern[1] * kern[2]
    s = torch.pow(2.0, ladder_scales(kind, cin, D).double()).float()           # (D, cin)
    x = _n(tag + "_x", (B, cin, D, H, W)) * s.t().reshape(1, cin, D, 1, 1)
    c = {"kind": kind, "kern": tuple(kern), "cin": cin, "cout": cout, "shape": (D, H, W), "x": x,
         "w": _n(tag + "_w", (cout, cin) + tuple(kern), 1 / math.sqrt(cin * taps))}
    _, c["ref"] = volume_reference(x, c["w"])
    return c


def plane_bounds(ref):
    """The ladder bound per (batch, output depth) plane of ``ref`` (B, Cout, D, H, W): (B, D)."""
    return PLANE_RTOL * ref.abs().amax((1, 3, 4))
