"""CPU side of the gate-epilogue tests (tests/test_gpu_gate.py):

* tests/gate_reference.py, the fp64 reference those tests compare against, restates the oracle's
  SelectiveConvGRU (core/update.py:83-119);
* the comparison discriminates: reference-made "device results" carrying the faults a tile's epilogue
  could have are refused by the GPU test's own check, the unfaulted result passes;
* the tuning table selects no 2D tile the gate matrix does not run.
"""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import oracle
from foundationstereo_amd import synth
from tests.conv_tiles import HALO_2D, POLICY_DEFAULTS, PW_2D
from tests.gate_reference import assert_unsaturated, gate_inputs, gate_reference
from tests.helpers import t
from tests.test_gpu_gate import _check_outputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_reference_matches_oracle():
    from foundationstereo_amd.update import SelectiveConvGRU
    B, Hd, Ci, H, W = 1, 32, 32, 9, 14
    mod = SelectiveConvGRU(Hd, 2 * Ci)
    synth.init_module_(mod, seed=511)
    P = {"m." + k: v.detach() for k, v in mod.state_dict().items()}
    h = t(synth.normal(512, (B, Hd, H, W)))
    xs = [t(synth.normal(513 + i, (B, Ci, H, W))).clip(0, None) for i in range(2)]
    att = t(synth.uniform(517, (B, 1, H, W), 0.0, 1.0))
    _conv = oracle.stereo_oracle._conv
    x = F.relu(_conv(P, "m.conv0.0", torch.cat(xs, 1), 1, 1))
    hx = F.relu(_conv(P, "m.conv1.0", torch.cat([x, h], 1), 1, 1))
    out = None
    for gru, mode in (("small_gru", "blend_small"), ("large_gru", "blend_large")):
        w = {n: P[f"m.{gru}.conv{n}.weight"] for n in "zrq"}
        b = {n: P[f"m.{gru}.conv{n}.bias"] for n in "zrq"}
        _, zr = gate_reference("zr", hx, torch.cat([w["z"], w["r"]], 0), torch.cat([b["z"], b["r"]], 0), h)
        _, o = gate_reference(mode, torch.cat([zr["rh"], x.double()], 1), w["q"], b["q"], h, zr["z"], att, out)
        out = o["out"]
    ref = oracle.stereo_oracle.selective_gru(P, "m", att, h, *xs)
    err = float((out - ref.double()).abs().max())
    assert err <= 1e-5, err            # the oracle is fp32: the suite's per-op figure for summation order


FAULT_SHAPES = [(3, 40, 19, 45), (1, 128, 12, 40)]


def _parts(c):
    """The pieces of case c's reference, to assemble faulted results from."""
    pre, h, Hd = c["pre"], c["h"].double(), c["Hd"]
    if c["mode"] == "zr":
        return pre, h, Hd, None, None
    z, att = c["z"].double(), c["att"].double()
    return pre, h, Hd, (1 - z) * h + z * torch.tanh(pre), att


def _faults(c):
    pre, h, Hd, hn, att = _parts(c)
    ref = {n: v.clone() for n, v in c["ref"].items()}
    if c["mode"] == "zr":
        s = torch.sigmoid(pre)
        yield "z and r rows swapped", {"z": s[:, Hd:], "rh": s[:, :Hd] * h}
        yield "co % Hd clamped to Hd - 1", {"z": ref["z"], "rh": s[:, Hd:] * h[:, Hd - 1:Hd]}
        rh = ref["rh"].clone()
        rh[:, Hd - 1] = rh[:, Hd - 2]
        yield "last cout row copied from its neighbour", {"z": ref["z"], "rh": rh}
    else:
        if c["mode"] == "blend_large":
            out0 = c["out0"][:, :Hd].double()
            yield "att in place of 1 - att", {"out": out0 + hn * att}
            yield "blend_large overwrites", {"out": hn * (1 - att)}
        else:
            yield "1 - att in place of att", {"out": hn * (1 - att)}
        out = ref["out"].clone()
        out[:, Hd - 1] = out[:, Hd - 2]
        yield "last cout row copied from its neighbour", {"out": out}
    # one fp16 product per MAC: inputs and weights rounded to fp16 before the conv
    _, half = gate_reference(c["mode"], c["x"].half(), c["w"].half(), c["bias"], c["h"], c.get("z"), c.get("att"),
                             c["out0"][:, :Hd] if c["mode"] == "blend_large" else None)
    yield "operands rounded to fp16", half


@pytest.mark.parametrize("k,Hd,H,W", FAULT_SHAPES)
@pytest.mark.parametrize("mode", ["zr", "blend_small", "blend_large"])
def test_check_discriminates(mode, k, Hd, H, W):
    c = gate_inputs(mode, k, Hd, H, W)
    assert_unsaturated(c)
    _check_outputs(c, {n: v.float() for n, v in c["ref"].items()}, "unfaulted")
    n = 0
    for what, got in _faults(c):
        with pytest.raises(AssertionError, match="max .diff."):
            _check_outputs(c, {name: v.float() for name, v in got.items()}, what)
        n += 1
    assert n >= 3


def test_check_refuses_nonfinite():
    c = gate_inputs("blend_small", 1, 40, 12, 40)
    out = c["ref"]["out"].float().clone()
    out[1, 7, 3, 5] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        _check_outputs(c, {"out": out}, "one NaN")


def test_tuning_table_inside_gate_matrix():
    """A re-tune that picks a 2D tile the gate matrix does not run fails here."""
    assert set(POLICY_DEFAULTS) <= set(HALO_2D)
    assert not set(HALO_2D) & set(PW_2D)
    with open(os.path.join(REPO, "tuning", "fsmi_conv.json")) as f:
        entries = json.load(f)["entries"]
    seen = 0
    for key, e in entries.items():
        if "_d1_" not in key or "_D1_" not in key:
            continue
        seen += 1
        ks = re.match(r"k(\w+?)_d1_", key).group(1)
        assert e["cfg"] in HALO_2D + PW_2D, f"{key}: tile {e['cfg']} is not in the gate matrix"
        assert e["cfg"] not in PW_2D or ks == "1", f"{key}: pointwise tile {e['cfg']} on a {ks}x{ks} conv"
    assert seen > 0
