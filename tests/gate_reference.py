"""fp64 restatement of the SelectiveConvGRU gate epilogues (``ops.conv2d_gate``, act 3-5 of the halo
conv; core/update.py:83-95,117), the synthetic inputs the gate tests run on, and their tolerance.

CPU only, plain torch: shared by tests/test_gpu_gate.py (the device comparison) and
tests/test_gate_host.py (which pins this file to the oracle and shows that the comparison
discriminates).

Tolerance, derived: the halo conv's bound holds for the pre-activation, e = 2e-5 + 1e-5 max|pre_ref|;
an output moves by at most its Lipschitz factor in the pre-activation times that -- sigmoid' <= 1/4 for
z, max|h|/4 for rh = sigmoid(r) h, z (1 - tanh^2) att <= 1 for both blends -- plus 8 * 2^-24 max|ref| for
the device's expf / tanhf and the few fp32 products after them.
"""
import functools
import math

import torch
import torch.nn.functional as F

from foundationstereo_amd import synth
from tests.helpers import t

MODES = ("zr", "blend_small", "blend_large")
B = 2
CIN_ZR = 72          # zr input: one segment, 3 chunks of 32 with a ragged last one
XC, XC0, XCN = 40, 5, 29   # blend input: [rh (Hd channels), xc[:, 5:34]]


def gate_reference(mode, x, w, bias, h, z=None, att=None, out0=None):
    """``mode`` "zr": ``w`` = [convz; convr] stacked -> (pre, {"z": sigmoid(pre[:Hd]), "rh": sigmoid(pre[Hd:]) h});
    "blend_small": (pre, {"out": ((1-z) h + z tanh(pre)) att}); "blend_large": (pre, {"out": out0 + (...)(1-att)}).
    ``x`` is the conv's whole input (the segments concatenated); everything in fp64."""
    d = torch.double
    k = w.shape[-1]
    pre = F.conv2d(x.to(d), w.to(d), bias.to(d), padding=k // 2)
    h = h.to(d)
    Hd = h.shape[1]
    if mode == "zr":
        assert pre.shape[1] == 2 * Hd
        s = torch.sigmoid(pre)
        return pre, {"z": s[:, :Hd], "rh": s[:, Hd:] * h}
    assert pre.shape[1] == Hd
    z, att = z.to(d), att.to(d)
    hn = (1 - z) * h + z * torch.tanh(pre)
    if mode == "blend_small":
        return pre, {"out": hn * att}
    assert mode == "blend_large"
    return pre, {"out": out0.to(d) + hn * (1 - att)}


def lipschitz(mode, name, h):
    """Bound on |d output / d pre-activation| (see the module docstring)."""
    if mode == "zr":
        return 0.25 if name == "z" else float(h.abs().max()) / 4
    return 1.0


def gate_tol(pre_ref, ref, lip):
    return (2e-5 + 1e-5 * float(pre_ref.abs().max())) * lip + 8 * 2.0 ** -24 * float(ref.abs().max())


def _n(name, shape, std=1.0):
    return t(synth.normal(synth.name_seed(name), shape, std))


def _u(name, shape):
    u = synth.uniform(synth.name_seed(name), shape, 0.0, 1.0)
    return t(u).clamp(2.0 ** -24, 1 - 2.0 ** -24)      # (0, 1), both ends open


@functools.lru_cache(maxsize=None)
def gate_inputs(mode, k, Hd, H, W):
    """The synthetic operands of one gate conv (fp32, CPU) and its fp64 reference.  Own inputs per mode:
    an error in one mode never feeds the next.  Weights of std 1/sqrt(Cin k^2) and a bias of std 0.1 keep
    the gates off saturation.  Cached: every tile / split of a shape shares one reference; callers must
    not write to what they get."""
    tag = f"gate_{mode}_k{k}_hd{Hd}_{H}x{W}"
    cout = 2 * Hd if mode == "zr" else Hd
    cin = CIN_ZR if mode == "zr" else Hd + XCN
    c = {"mode": mode, "k": k, "Hd": Hd,
         "w": _n(tag + "_w", (cout, cin, k, k), 1 / math.sqrt(cin * k * k)),
         "bias": _n(tag + "_b", (cout,), 0.1),
         "h": _n(tag + "_h", (B, Hd, H, W))}
    if mode == "zr":
        c["hx"] = _n(tag + "_hx", (B, CIN_ZR, H, W))
        x = c["hx"]
    else:
        c["rh"] = _n(tag + "_rh", (B, Hd, H, W), 0.5)
        c["xc"] = _n(tag + "_xc", (B, XC, H, W))
        c["z"] = _u(tag + "_z", (B, Hd, H, W))
        c["att"] = _u(tag + "_att", (B, 1, H, W))
        x = torch.cat([c["rh"], c["xc"][:, XC0:XC0 + XCN]], 1)
    if mode == "blend_large":
        c["out0"] = _n(tag + "_out0", (B, Hd + 3, H, W))
    c["x"] = x
    c["pre"], c["ref"] = gate_reference(mode, x, c["w"], c["bias"], c["h"], c.get("z"), c.get("att"),
                                        c["out0"][:, :Hd] if mode == "blend_large" else None)
    c["tol"] = {n: gate_tol(c["pre"], v, lipschitz(mode, n, c["h"])) for n, v in c["ref"].items()}
    c["pre_std"] = float(c["pre"].std())
    c["pre_sat"] = float((c["pre"].abs() > 4).double().mean())
    return c


def assert_unsaturated(c):
    """The gates must be exercised on their slopes: a saturated sigmoid / tanh hides a wrong pre-activation."""
    assert 0.5 <= c["pre_std"] <= 2.0, f"pre-activation std {c['pre_std']:.3g} outside [0.5, 2]"
    assert c["pre_sat"] < 0.01, f"share of |pre| > 4: {c['pre_sat']:.3g}"
