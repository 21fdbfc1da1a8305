"""The SelectiveConvGRU gate epilogues of the halo conv (``ops.conv2d_gate`` -> ``fsmi_conv2d_halo_x3_gate``)
on every 2D tile family vs fp64.

act 3 ("zr": z = sigmoid(.), rh = sigmoid(r) h from the stacked convz|convr conv), act 4 ("blend_small":
out = ((1-z) h + z tanh(q)) att) and act 5 ("blend_large": out += (...)(1-att)) exist four times: in
``store_frag_c`` (every register / LDS / pipelined / K-group tile, and the pointwise tiles), in the scalar
and the float4 split-K reduce, and in the volume instantiation 2D convs take in safe range mode.  Checked
here, per tile and per gate:

* every tile id a stride-1 2D conv may take (tests/conv_tiles.py) x k in {1, 3} x split-K 1 / 2 / 3, at
  B = 2, Hd in {128 (the product's; the z|r boundary on a 128-cout tile edge), 40 (z|r boundary inside a
  32-row fragment, partial last fragment)}, maps 19x45 (ragged 2- / 4- / 5- / 8-row and 32-column tiles,
  H*W % 4 != 0: the scalar reduce) and 12x40 (the float4 reduce; the pointwise tiles), vs the fp64
  reference of tests/gate_reference.py within its derived tolerance (not tuned; see that file);
* written extents (NaN guard batches, the channels of ``out`` past Hd), read-only operands, bit-equal
  repeat runs, a clear range flag, and that the tile asked for is the tile that ran;
* the same in safe range mode;
* the zr -> blend_small -> blend_large chain of ``SelectiveConvGRU.forward`` vs the fp64 chain and vs the
  unfused ``ops.gru_reset`` / ``ops.gru_blend`` kernels;
* the refusals of ``ops.conv2d_gate`` and of the C entry.

The worst error per (mode, tile family) goes to $FSMI_PARITY_LOG.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from foundationstereo_amd import synth
from tests.conv_tiles import HALO_2D, PW_2D
from tests.gate_reference import (B, MODES, XC0, XCN, assert_unsaturated, gate_inputs, gate_reference, gate_tol,
                                  lipschitz)
from tests.helpers import t

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")


@pytest.fixture(scope="module")
def ops_mod():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from foundationstereo_amd import _lib, ops
    _lib.load()
    return ops


@pytest.fixture
def range_clear(ops_mod):
    ops_mod.set_range_safe(False)
    ops_mod.range_overflowed(reset=True)
    yield
    ops_mod.set_range_safe(False)          # sticky: never leak safe mode into other tests
    ops_mod.range_overflowed(reset=True)


WORST = {}       # (mode, output, family) -> (err / tol, err, tol, case)


@pytest.fixture(scope="module", autouse=True)
def _log_worst():
    """After the module: the worst error per (mode, output, tile family) to $FSMI_PARITY_LOG (JSON lines, the
    figure under test_gpu_parity.record's key, plus its bound and the case it came from)."""
    import json
    import os
    yield
    path = os.environ.get("FSMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            for (mode, name, fam), (_, err, tol, case) in sorted(WORST.items()):
                f.write(json.dumps({"test": f"gate_{mode}_{name}_{fam}", "max_abs_diff_px": err, "bound": tol,
                                    "case": case}) + "\n")


def family(cfg, safe=False):
    f = ("policy" if cfg < 0 else "lds" if cfg <= 1 else "reg" if cfg <= 11 else "kgroup" if cfg <= 23 else
         "pw" if cfg <= 29 else "pipe")
    return ("safe_" if safe else "") + f


def _check(out, ref, tol, what):
    """Every element finite and within ``tol`` of the fp64 ``ref``; returns the max error."""
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite values in the written extent"
    err = float((out.double() - ref.to(out.device)).abs().max())
    print(f"{what}: max |diff| {err:.3g} (bound {tol:.3g})")
    assert err <= tol, f"{what}: max |diff| {err:.3g} > {tol:.3g}"
    return err


def _check_outputs(c, got, what, fam=None):
    """``got`` (name -> tensor) of case ``c``'s mode against its reference, each output under its own bound."""
    assert set(got) == set(c["ref"])
    for name, ref in c["ref"].items():
        tol = c["tol"][name]
        err = _check(got[name], ref, tol, f"{what} {name}")
        if fam is not None:
            key = (c["mode"], name, fam)
            if key not in WORST or err / tol > WORST[key][0]:
                WORST[key] = (err / tol, err, tol, what)


_DEV_CASES = {}


def dev_case(ops, mode, k, Hd, H, W):
    """gate_inputs on the device: fp32 operands with pristine copies, the packed conv, the fp64 reference."""
    key = (mode, k, Hd, H, W)
    if key not in _DEV_CASES:
        c = gate_inputs(mode, k, Hd, H, W)
        d = {n: v for n, v in c.items() if not isinstance(v, (torch.Tensor, dict))}
        for n, v in c.items():
            if isinstance(v, torch.Tensor) and v.dtype == torch.float32:
                d[n] = v.to(DEV)
                d[n + "_copy"] = v.to(DEV)
        d["ref"] = {n: v.to(DEV) for n, v in c["ref"].items()}
        d["tol"] = c["tol"]
        d["pk"] = ops.PackedConv(d["w"], mode="halo")
        d["shape"] = (H, W)
        _DEV_CASES[key] = d
    return _DEV_CASES[key]


def _bits(x):
    return x.view(torch.int32)


def _launch(ops, d, cfg, nsplit):
    """One gate conv of case ``d`` into fresh guarded buffers: the outputs are the middle batch slice
    [1 : B+1] of (B + 2, ...) tensors prefilled with NaN (blend_large: the slice holds out0).  Asserts the
    written extents and returns the written slices."""
    mode, Hd, (H, W) = d["mode"], d["Hd"], d["shape"]
    what = f"{mode} k{d['k']} cfg {cfg} split {nsplit} Hd {Hd} {H}x{W}"
    if mode == "zr":
        fulls = {"z": torch.full((B + 2, Hd, H, W), NAN, device=DEV),
                 "rh": torch.full((B + 2, Hd, H, W), NAN, device=DEV)}
        ops.conv2d_gate([d["hx"]], d["pk"], d["bias"], "zr", h=d["h"], z=fulls["z"][1:B + 1],
                        rh=fulls["rh"][1:B + 1], cfg=cfg, nsplit=nsplit)
    else:
        fulls = {"out": torch.full((B + 2, Hd + 3, H, W), NAN, device=DEV)}
        if mode == "blend_large":
            fulls["out"][1:B + 1] = d["out0"]
        before = fulls["out"].clone()
        ops.conv2d_gate([d["rh"], (d["xc"], XC0, XCN)], d["pk"], d["bias"], mode, h=d["h"], z=d["z"],
                        att=d["att"], out=fulls["out"][1:B + 1], cfg=cfg, nsplit=nsplit)
        assert torch.equal(_bits(fulls["out"][1:B + 1, Hd:]), _bits(before[1:B + 1, Hd:])), \
            f"{what}: channels of out past Hd were written"
    for name, full in fulls.items():
        assert bool(torch.isnan(full[0]).all()) and bool(torch.isnan(full[B + 1]).all()), \
            f"{what}: {name} written outside its batch slice"
    # read-only operands (z only for the blends: zr writes it)
    for name in ("h", "att", "z", "rh", "xc", "hx", "bias"):
        if name in d and not (mode == "zr" and name in ("z", "rh")):
            assert torch.equal(_bits(d[name]), _bits(d[name + "_copy"])), f"{what}: operand {name} was modified"
    return {name: full[1:B + 1, :Hd] for name, full in fulls.items()}, what


def _run_modes(ops, k, cfg, nsplit, Hd, HW, fam):
    for mode in MODES:
        d = dev_case(ops, mode, k, Hd, *HW)
        assert_unsaturated(d)
        if cfg >= 0:
            ops.conv_launch_counts(reset=True)
        got, what = _launch(ops, d, cfg, nsplit)
        assert not ops.range_overflowed(), f"{what}: range flag set"
        if cfg >= 0 and not fam.startswith("safe_"):
            assert ops.conv_launch_counts()[cfg] == 1, f"{what}: tile {cfg} did not run"
        _check_outputs(d, got, what, fam)
        # split-K sums its partials in order and the K groups sum through LDS: repeat runs are bit-equal
        again, _ = _launch(ops, d, cfg, nsplit)
        for name in got:
            assert torch.equal(got[name], again[name]), f"{what}: {name} differs between two runs"
        assert not ops.range_overflowed(), f"{what}: range flag set"


def _matrix():
    for (H, W), Hd, k, nsplit in itertools.product([(19, 45), (12, 40)], [128, 40], [1, 3], [1, 2, 3]):
        for cfg in HALO_2D + (PW_2D if k == 1 and (H, W) == (12, 40) else []):
            yield pytest.param(k, cfg, nsplit, Hd, (H, W), id=f"k{k}-cfg{cfg}-s{nsplit}-hd{Hd}-{H}x{W}")


@pytest.mark.parametrize("k,cfg,nsplit,Hd,HW", list(_matrix()))
def test_gate_epilogues_vs_fp64(ops_mod, range_clear, k, cfg, nsplit, Hd, HW):
    """The three gate modes, one after another, on tile ``cfg`` with split-K ``nsplit``.  (cfg -1 takes the
    policy's tile, and ops._SPLIT_CAP holds an auto-chosen tile's split at 2: its nsplit 3 case repeats 2.)"""
    _run_modes(ops_mod, k, cfg, nsplit, Hd, HW, family(cfg))


@pytest.mark.parametrize("nsplit", [1, 2])
@pytest.mark.parametrize("k,cfg", [(k, cfg) for cfg in [-1, 9, 11, 43, 19, 24, 28] for k in (1, 3)
                                   if k == 1 or cfg not in PW_2D])
def test_gate_epilogues_safe_mode(ops_mod, range_clear, k, cfg, nsplit):
    """Safe range mode: 2D convs run the volume instantiation (per-chunk exponent) of the same epilogues;
    tiles 11 / 43 fall back to 9, the pointwise tiles to 4."""
    ops_mod.set_range_safe(True)
    _run_modes(ops_mod, k, cfg, nsplit, 40, (12, 40), family(cfg, safe=True))


def test_gate_chain_matches_unfused_kernels(ops_mod, range_clear):
    """zr -> blend_small -> blend_large for the small (1x1) and the large (3x3) branch, in the order of
    SelectiveConvGRU.forward, vs the fp64 chain -- and vs ops.gru_reset / ops.gru_blend fed with the fp64
    convs' pre-activations rounded to fp32, which ties the fused epilogues to the unfused kernels."""
    ops = ops_mod
    Hd, H, W, Chx, Cx = 128, 12, 40, 72, 40

    def n(name, shape, std=1.0):
        return t(synth.normal(synth.name_seed("gate_chain_" + name), shape, std))

    h, hx, xc = n("h", (B, Hd, H, W)), n("hx", (B, Chx, H, W)), n("xc", (B, Cx, H, W))
    att = t(synth.uniform(synth.name_seed("gate_chain_att"), (B, 1, H, W), 0.0, 1.0))
    P = {}
    for br, k in (("s", 1), ("l", 3)):
        P[br] = (k, n(f"wzr_{br}", (2 * Hd, Chx, k, k), (Chx * k * k) ** -0.5), n(f"bzr_{br}", (2 * Hd,), 0.1),
                 n(f"wq_{br}", (Hd, Hd + Cx, k, k), ((Hd + Cx) * k * k) ** -0.5), n(f"bq_{br}", (Hd,), 0.1))
    # fp64 chain
    ref, out_ref = {}, torch.zeros(B, Hd, H, W, dtype=torch.double)
    for br, mode in (("s", "blend_small"), ("l", "blend_large")):
        k, wzr, bzr, wq, bq = P[br]
        pre_zr, zr = gate_reference("zr", hx, wzr, bzr, h)
        pre_q, o = gate_reference(mode, torch.cat([zr["rh"], xc.double()], 1), wq, bq, h, zr["z"], att, out_ref)
        out_ref = o["out"]
        ref[br] = (pre_zr, zr, pre_q)
    # fused kernels
    hd, hxd, xcd, attd = h.to(DEV), hx.to(DEV), xc.to(DEV), att.to(DEV)
    out = torch.full((B, Hd, H, W), NAN, device=DEV)
    for br, mode in (("s", "blend_small"), ("l", "blend_large")):
        k, wzr, bzr, wq, bq = P[br]
        z, rh = torch.full_like(out, NAN), torch.full_like(out, NAN)
        ops.conv2d_gate([hxd], ops.PackedConv(wzr.to(DEV), mode="halo"), bzr.to(DEV), "zr", h=hd, z=z, rh=rh)
        ops.conv2d_gate([rh, xcd], ops.PackedConv(wq.to(DEV), mode="halo"), bq.to(DEV), mode, h=hd, z=z, att=attd,
                        out=out)
        pre_zr, zr, _ = ref[br]
        _check(z, zr["z"], gate_tol(pre_zr, zr["z"], lipschitz("zr", "z", h)), f"chain {br} z")
        _check(rh, zr["rh"], gate_tol(pre_zr, zr["rh"], lipschitz("zr", "rh", h)), f"chain {br} rh")
    assert not ops.range_overflowed()
    pre_q = torch.cat([ref["s"][2], ref["l"][2]], 1)
    tol = gate_tol(pre_q, out_ref, 1.0)
    _check(out, out_ref, tol, "chain out vs fp64")
    # unfused kernels on the fp64 convs' pre-activations
    zr_s, zr_l = (ref[br][0].float().to(DEV) for br in ("s", "l"))
    qs_in, ql_in = ops.gru_reset(zr_s, zr_l, hd, xcd)
    q = [F.conv2d(qin.double().cpu(), P[br][3].double(), P[br][4].double(), padding=P[br][0] // 2).float().to(DEV)
         for br, qin in (("s", qs_in), ("l", ql_in))]
    unfused = ops.gru_blend(zr_s, zr_l, q[0], q[1], hd, attd)
    _check(unfused, out_ref, tol, "chain unfused kernels vs fp64")
    _check(out, unfused.double(), tol, "chain out vs unfused kernels")


def test_gate_refusals(ops_mod, range_clear):
    ops = ops_mod
    from foundationstereo_amd import _lib
    k, Hd, H, W = 1, 40, 12, 40
    zr, bl = dev_case(ops, "zr", k, Hd, H, W), dev_case(ops, "blend_small", k, Hd, H, W)
    z, rh, out = (torch.empty(B, Hd, H, W, device=DEV) for _ in range(3))
    with pytest.raises(AssertionError):          # zr with a conv of Hd couts
        ops.conv2d_gate([bl["rh"], (bl["xc"], XC0, XCN)], bl["pk"], bl["bias"], "zr", h=bl["h"], z=z, rh=rh)
    with pytest.raises(AssertionError):          # blend without att
        ops.conv2d_gate([bl["rh"], (bl["xc"], XC0, XCN)], bl["pk"], bl["bias"], "blend_small", h=bl["h"], z=bl["z"],
                        out=out)
    with pytest.raises(AssertionError):          # blend without out
        ops.conv2d_gate([bl["rh"], (bl["xc"], XC0, XCN)], bl["pk"], bl["bias"], "blend_large", h=bl["h"], z=bl["z"],
                        att=bl["att"])

    # the C entry, with the pointer arrays ops.conv2d_gate passes: refused before any launch
    _, (pp, chs, tots, keep), _ = ops._segments([zr["hx"]])
    pk = zr["pk"]
    sb = pk.scale_bias(zr["bias"])
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def raw(mode, h_ptr, hd):
        rc = _lib.load().fsmi_conv2d_halo_x3_gate(pp, chs, tots, 1, pk.whi.data_ptr(), pk.wlo.data_ptr(),
                                                  sb.data_ptr(), mode, h_ptr, z.data_ptr(), None, rh.data_ptr(), hd,
                                                  None, 0, 0, B, pk.cout, k, H, W, 4, 1, None, 0, stream)
        _lib.check(rc, "conv2d_gate")

    ops.conv_launch_counts(reset=True)
    with pytest.raises(_lib.FsmiError, match="mode 3"):
        raw(3, zr["h"].data_ptr(), Hd)
    with pytest.raises(_lib.FsmiError, match="null h"):
        raw(0, None, Hd)
    with pytest.raises(_lib.FsmiError, match="Cout == 2\\*Hd"):
        raw(0, zr["h"].data_ptr(), Hd + 1)
    assert sum(ops.conv_launch_counts()) == 0, "a refused call launched a conv"
    raw(0, zr["h"].data_ptr(), Hd)               # the same call, legal: accepted
    assert ops.conv_launch_counts()[4] == 1
    del keep
    _check(z, zr["ref"]["z"], zr["tol"]["z"], "raw zr z")
