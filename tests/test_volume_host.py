"""CPU side of the volume-conv tests (tests/test_gpu_volume.py):

* tests/volume_reference.py, the fp64 reference those tests compare against, restates the product's own
  torch path: ResnetBasicBlock3D with and without a gate, BasicConv(is_3d) + FeatureAtt, BatchNorm folded
  as ``submodule.conv3d_bn_act`` folds it;
* the comparison discriminates: reference-made "device results" carrying the faults a volume tile could
  have are refused by the GPU test's own checks, the unfaulted result rounded to fp32 passes;
* the tuning table selects no volume or stride-2 tile outside tests/conv_tiles.py's lists.
"""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

from foundationstereo_amd import synth
from tests.conv_tiles import DEPTH_TILE, S2_3D, VOLUME_3D
from tests.helpers import t
from tests.test_gpu_volume import _check, _check_planes
from tests.volume_reference import (ACTS, B, EPILOGUES, LADDER_KINDS, LADDER_STEP, assert_exercised, ladder_inputs,
                                    ladder_scales, volume_inputs, volume_reference)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fold(conv, bn):
    """(w, b) of conv + eval BatchNorm through the product's own fold (``submodule._folded``): fp64 weights
    scaled per output channel, the bias rounded to fp32 as the packed conv gets it."""
    from foundationstereo_amd.submodule import _folded
    return _folded(conv, bn, "_volume_host_fold",
                   lambda sc: conv.weight.detach().double() * sc.view(-1, 1, 1, 1, 1))


def _fold_tol(b, ref):
    # the folded bias is rounded to fp32 (half an ulp of its largest entry); fp64 summation order beside it
    return 2.0 ** -24 * float(b.abs().max()) + 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("gated", [False, True])
def test_reference_matches_resnet_block(gated):
    from foundationstereo_amd.submodule import ResnetBasicBlock3D
    C, D, H, W = 12, 4, 6, 9
    m = ResnetBasicBlock3D(C, C, kernel_size=3, stride=1, padding=1).eval()
    synth.init_module_(m, seed=731)
    m = m.double()
    x = t(synth.normal(732, (B, C, D, H, W))).double()
    fatt = t(synth.normal(733, (B, C, H, W), 1.5)).double() if gated else None
    with torch.no_grad():
        want = m(x, fatt=fatt)
        y = F.relu(m.bn1(m.conv1(x)))
        w, b = _fold(m.conv2, m.bn2)
    _, ref = volume_reference(y, w, b, "relu", res=x, res_pre=True, fatt=fatt)
    err = float((ref - want).abs().max())
    assert err <= _fold_tol(b, want), err


def test_reference_matches_basicconv_feature_att():
    from foundationstereo_amd.submodule import BasicConv, FeatureAtt
    Ci, Co, Cf, D, H, W = 10, 12, 16, 4, 6, 9
    conv = BasicConv(Ci, Co, is_3d=True, kernel_size=3, padding=1, stride=1).eval()
    att = FeatureAtt(Co, Cf).eval()
    synth.init_module_(conv, seed=741)
    synth.init_module_(att, seed=742)
    conv, att = conv.double(), att.double()
    x = t(synth.normal(743, (B, Ci, D, H, W))).double()
    feat = t(synth.normal(744, (B, Cf, H, W))).double()
    with torch.no_grad():
        want = att(conv(x), feat)
        w, b = _fold(conv.conv, conv.bn)
        _, ref = volume_reference(x, w, b, "leaky", fatt=att.logits(feat))
    err = float((ref - want).abs().max())
    assert err <= _fold_tol(b, want), err


# (3,3,3) with a second 128-cout tile; (17,1,1) deeper than the volume (most taps read padding)
FAULT_SHAPES = [((3, 3, 3), 72, 136, 5, 9, 37), ((17, 1, 1), 40, 37, 5, 9, 37)]


def _epilogue(c, pre, res_pre=None, fatt=None, res=None):
    """Case c's epilogue on ``pre`` with some of its pieces replaced."""
    res_pre = c["res_pre"] if res_pre is None else res_pre
    res = c["res"] if res is None else res
    fatt = c["fatt"] if fatt is None else fatt
    if res is not None and res_pre:
        out = ACTS[c["act"]](pre + res.double())
    else:
        out = ACTS[c["act"]](pre)
        if res is not None:
            out = out + res.double()
    if fatt is not None:
        g = torch.sigmoid(fatt.double())
        out = out * (g.unsqueeze(2) if g.dim() == 4 else g)
    return out


def _faults(c):
    x, w, bias, pre = c["x"].double(), c["w"].double(), c["bias"].double(), c["pre"]
    kd, ks = c["kern"][0], c["kern"][2]
    D, H, W = c["shape"]
    cout = c["cout"]
    if kd > 1:
        p = kd // 2
        idx = torch.arange(-p, D + p) % D                 # plane -1 reads plane D - 1
        wrapped = F.conv3d(x[:, :, idx], w, bias, padding=(0, ks // 2, ks // 2))
        yield "depth padding wraps", _epilogue(c, wrapped)
        yield "kd taps reversed", _epilogue(c, F.conv3d(x, w.flip(2), bias, padding=(p, ks // 2, ks // 2)))
    if c["fatt"] is not None:
        # gate read at hw = d * P + hw2 without % P: channel (b * Cout + co + d) of the flattened gate
        fl = c["fatt"].reshape(B * cout, H, W)
        idx = (torch.arange(B * cout).view(-1, 1) + torch.arange(D).view(1, -1)).clamp(max=B * cout - 1)
        yield "gate indexed without % P", _epilogue(c, pre, fatt=fl[idx].reshape(B, cout, D, H, W))
        yield "gate taken from batch 0", _epilogue(c, pre, fatt=c["fatt"][:1].expand(B, -1, -1, -1))
    if c["res"] is not None and c["act"] is not None:
        yield "residual on the other side of the activation", _epilogue(c, pre, res_pre=not c["res_pre"])
    ref = c["ref"]
    out = ref.clone()
    out[:, cout - 1] = out[:, cout - 2]
    yield "last cout row copied from its neighbour", out
    if cout > 128:
        out = ref.clone()
        out[:, 128:] = out[:, :cout - 128]
        yield "couts past 128 taken from the first cout tile", out
    _, half = volume_reference(c["x"].half(), c["w"].half(), c["bias"], c["act"], c["res"], c["res_pre"], c["fatt"])
    yield "operands rounded to fp16", half
    out = ref.clone()
    out[1] = out[0]
    yield "batch 1 equal to batch 0", out


@pytest.mark.parametrize("kern,cin,cout,D,H,W", FAULT_SHAPES)
@pytest.mark.parametrize("epi", list(EPILOGUES))
def test_check_discriminates(epi, kern, cin, cout, D, H, W):
    c = volume_inputs(kern, cin, cout, D, H, W, epi)
    assert_exercised(c)
    _check(c["ref"].float(), c["ref"], c["tol"], "unfaulted")
    seen = set()
    for what, got in _faults(c):
        with pytest.raises(AssertionError, match="max .diff."):
            _check(got.float(), c["ref"], c["tol"], what)
        seen.add(what)
    want = {"last cout row copied from its neighbour", "operands rounded to fp16", "batch 1 equal to batch 0"}
    if kern[0] > 1:
        want |= {"depth padding wraps", "kd taps reversed"}
    if c["fatt"] is not None:
        want |= {"gate indexed without % P", "gate taken from batch 0"}
    if epi in ("relu_res_pre", "relu_res_pre_fatt", "leaky_res_post"):
        want |= {"residual on the other side of the activation"}
    if cout > 128:
        want |= {"couts past 128 taken from the first cout tile"}
    assert want <= seen, want - seen


def test_check_refuses_nonfinite():
    c = volume_inputs((17, 1, 1), 40, 37, 5, 9, 37, "leaky")
    out = c["ref"].float().clone()
    out[1, 7, 3, 5, 11] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        _check(out, c["ref"], c["tol"], "one NaN")


def _rescale_points(kind, kern, cin, D, d):
    """Chunks (kd, channel chunk), in the kernel's kd-major order, of output plane d, and the indices of
    those before which the accumulators are rescaled: a chunk that does not fit the current exponent, which
    was aimed kHeadroom1 = 4 bits below the fit of the chunk that set it, i.e. one more than 2^5 times it
    (a 2^6 step, random maxima within a factor of 2 of each other)."""
    log2s = ladder_scales(kind, cin, D)
    pd, nck = kern[0] // 2, (cin + 31) // 32
    chunks, points, top = [], [], None
    for kd in range(kern[0]):
        p = d + kd - pd
        for ck in range(nck):
            chunks.append((kd, ck))
            if not 0 <= p < D:
                continue                                   # a zero padding plane never moves the exponent
            s = int(log2s[p, 32 * ck])
            if top is None:
                top = s
            elif s > top + 5:
                points.append(len(chunks) - 1)
                top = s
    return chunks, points


@pytest.mark.parametrize("kern", [(3, 3, 3), (1, 1, 1)])
@pytest.mark.parametrize("kind", LADDER_KINDS)
def test_ladder_check_refuses_skipped_rescale(kind, kern):
    """One rescale skipped: the partial sum accumulated before one chunk is off by 2^4 (the re-aim's
    headroom) in the output plane it belongs to.  The per-plane bound refuses it wherever that partial
    sum is the 2^-6 share the ladder is built to give (the last rescale of a plane's chunk sequence)."""
    cin, cout, D, H, W = 72, 37, 5, 9, 37
    c = ladder_inputs(kind, kern, cin, cout, D, H, W)
    ref = c["ref"]
    _check_planes(ref.float(), ref, "unfaulted")
    x, w = c["x"].double(), c["w"].double()
    pd, ks = kern[0] // 2, kern[2]
    refused = 0
    for d in range(D):
        chunks, points = _rescale_points(kind, kern, cin, D, d)
        if not points:
            continue
        before = torch.zeros(B, cout, H, W, dtype=torch.double)
        for kd, ck in chunks[:points[-1]]:
            p = d + kd - pd
            if 0 <= p < D:
                ch = slice(32 * ck, min(32 * ck + 32, cin))
                before += F.conv2d(x[:, ch, p], w[:, ch, kd], padding=ks // 2)
        share = float(before.abs().max() / ref[:, :, d].abs().max())
        assert share >= 2.0 ** -(LADDER_STEP + 3), (d, share)     # measurable: about 2^-6 of the plane
        for f in (2.0 ** 4, 2.0 ** -4):
            out = ref.clone()
            out[:, :, d] += (f - 1) * before
            with pytest.raises(AssertionError, match=f"plane \\(b ., d {d}\\)"):
                _check_planes(out.float(), ref, f"rescale skipped at plane {d} ({f})")
            refused += 1
    assert refused >= 2 * (D - 1)
    # one wrong plane must not hide behind a larger one: the whole-tensor figure would pass this
    d_small = int(ref.abs().amax((0, 1, 3, 4)).argmin())
    out = ref.clone()
    out[:, :, d_small] *= 1 + 1e-4
    assert float((out - ref).abs().max()) < 3e-6 * float(ref.abs().max())
    with pytest.raises(AssertionError, match="plane"):
        _check_planes(out.float(), ref, "smallest plane off by 1e-4")


def test_tuning_table_inside_volume_lists():
    """A re-tune that picks a volume or stride-2 tile the volume matrix / the stride-2 tests do not run
    fails here (2D entries: tests/test_gate_host.py)."""
    assert DEPTH_TILE not in VOLUME_3D
    with open(os.path.join(REPO, "tuning", "fsmi_conv.json")) as f:
        entries = json.load(f)["entries"]
    seen = {"volume": 0, "d17": 0, "s2": 0}
    for key, e in entries.items():
        m = re.match(r"k(\d)(s2)?_d(\d+)_ci\d+_co\d+_b\d+_D(\d+)_h\d+_w\d+$", key)
        assert m, f"{key}: not a tuning key"
        ks, s2, kd, D = int(m.group(1)), bool(m.group(2)), int(m.group(3)), int(m.group(4))
        assert 1 <= e["nsplit"] <= 8, f"{key}: nsplit {e['nsplit']}"
        if s2:
            seen["s2"] += 1
            assert e["cfg"] in S2_3D, f"{key}: stride-2 tile {e['cfg']}"
        elif kd > 1 or D > 1:
            seen["volume"] += 1
            d17 = ks == 1 and kd == 17
            seen["d17"] += d17
            assert e["cfg"] in VOLUME_3D or (d17 and e["cfg"] == DEPTH_TILE), \
                f"{key}: tile {e['cfg']} is not in the volume matrix"
    assert all(seen.values()), seen
