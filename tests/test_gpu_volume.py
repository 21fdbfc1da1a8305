"""The volume instantiation of the halo conv (``fsmi_conv3d_halo_x3_ex``, ``launch_cfg<KS, true>``) on every
stride-1 volume tile and epilogue vs fp64.

It shares the MFMA core with the 2D kernels; its own are the (kd, 32-channel chunk) chunk order with zero
depth-padding planes, the depth-fastest tile decode, range mode 1 (a block exponent per chunk with
``rescale_acc``), the ``RESPRE`` epilogue (``res_pre``, the FeatureAtt gate indexed by ``hw2`` /
``(hw + k) % P``) and split-K over KD * CinP / 32 chunks.  Checked here, per tile:

* every tile id a stride-1 volume conv may take (tests/conv_tiles.py) x kernels (3,3,3), (1,3,3), (1,1,1),
  (17,1,1) x split-K 1 / 2 / 3, at B = 2, channels (40 -> 37: two chunks with a ragged last one, a ragged
  32-row fragment) and (72 -> 136: three chunks, a second 128-cout tile of 8 rows, ragged inside the
  256-cout tile), volumes 5x9x37 (every row tile ragged, a ragged second column tile, D*H*W % 4 != 0: the
  scalar reduce) and 4x9x37 (the float4 reduce with quads that cross a depth plane); (17,1,1) at D = 5
  (shallower than the kernel) and D = 20; each with the epilogues of tests/volume_reference.py one after
  another, vs its fp64 reference within its derived tolerance (not tuned; see that file);
* written extents (NaN guard batches), read-only operands, bit-equal repeat runs, a clear range flag, and
  that the tile asked for is the tile that ran, once;
* split-K with more splits than fit evenly ("no empty splits": 17 chunks at nsplit 8 run 6 splits of 3) and
  with more than 8 partials (the scalar reduce although D*H*W % 4 == 0); the depth tile 30 on the same cases;
* the exponent ladder: planes and channel chunks 2^6 apart, so that the accumulators are rescaled inside a
  kd plane and across planes, under a bound per (batch, output depth) plane;
* the refusals of the C entry (nothing launched) and the 32 + c fallback to the plain tile c.

The worst err / tol per (epilogue or ladder kind, tile family) goes to $FSMI_PARITY_LOG.
"""
import itertools

import pytest
import torch

from tests.conv_tiles import DEPTH_TILE, VOLUME_3D
from tests.volume_reference import (B, EPILOGUES, LADDER_KINDS, assert_exercised, ladder_inputs, plane_bounds,
                                    volume_inputs)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
ACT_CODE = {None: 0, "relu": 1, "leaky": 6}


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
    ops_mod.range_overflowed(reset=True)


WORST = {}       # (epilogue / ladder kind, family) -> (err / tol, err, tol, case)


@pytest.fixture(scope="module", autouse=True)
def _log_worst():
    """After the module: the worst err / tol per (epilogue or ladder kind, tile family) to $FSMI_PARITY_LOG
    (JSON lines, the shape tests/test_gpu_gate.py writes)."""
    import json
    import os
    yield
    path = os.environ.get("FSMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            for (name, fam), (ratio, err, tol, case) in sorted(WORST.items()):
                f.write(json.dumps({"test": f"volume_{name}_{fam}", "max_abs_diff_px": err, "bound": tol,
                                    "err_over_tol": ratio, "case": case}) + "\n")


def family(cfg):
    return "policy" if cfg < 0 else "lds" if cfg <= 1 else "reg" if cfg <= 11 else "kgroup" if cfg <= 23 else "depth"


def _worst(name, fam, ratio, err, tol, what):
    if fam is not None and ((name, fam) not in WORST or ratio > WORST[(name, fam)][0]):
        WORST[(name, fam)] = (ratio, err, tol, what)


def _check(out, ref, tol, what):
    """Every element finite and within ``tol`` of the fp64 ``ref``; returns the max error."""
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite values in the written extent"
    err = float((out.double() - ref.to(out.device)).abs().max())
    print(f"{what}: max |diff| {err:.3g} (bound {tol:.3g})")
    assert err <= tol, f"{what}: max |diff| {err:.3g} > {tol:.3g}"
    return err


def _check_planes(out, ref, what):
    """The ladder's check: every (batch, output depth) plane within 3e-6 of its own largest reference
    value.  Returns (worst err / bound, that plane's err, its bound)."""
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite values in the written extent"
    ref = ref.to(out.device)
    err = (out.double() - ref).abs().amax((1, 3, 4))
    bound = plane_bounds(ref)
    ratio = err / bound
    i = int(ratio.argmax())
    b, d = divmod(i, ref.shape[2])
    worst, e, bd = float(ratio.flatten()[i]), float(err.flatten()[i]), float(bound.flatten()[i])
    print(f"{what}: worst plane (b {b}, d {d}) max |diff| {e:.3g} (bound {bd:.3g}, ratio {worst:.3g})")
    assert worst <= 1.0, f"{what}: plane (b {b}, d {d}) max |diff| {e:.3g} > {bd:.3g}"
    return worst, e, bd


_DEV_CASES = {}


def _to_dev(ops, key, c):
    """Case ``c`` on the device: fp32 operands with pristine copies, the packed conv, the fp64 reference."""
    if key not in _DEV_CASES:
        d = {n: v for n, v in c.items() if not isinstance(v, torch.Tensor)}
        for n in ("x", "bias", "res", "fatt"):
            v = c.get(n)
            d[n] = None if v is None else v.to(DEV)
            d[n + "_copy"] = None if v is None else v.to(DEV)
        d["ref"] = c["ref"].to(DEV)
        d["pk"] = ops.PackedConv(c["w"].to(DEV), mode="halo")
        d["sb"] = d["pk"].scale_bias(d["bias"])
        _DEV_CASES[key] = d
    return _DEV_CASES[key]


def dev_case(ops, kern, cin, cout, D, H, W, epi):
    key = (tuple(kern), cin, cout, D, H, W, epi)
    return _to_dev(ops, key, volume_inputs(*key))


def dev_ladder(ops, kind, kern, cin, cout, D, H, W):
    key = (kind, tuple(kern), cin, cout, D, H, W)
    return _to_dev(ops, key, ladder_inputs(*key))


def _bits(x):
    return x.view(torch.int32)


def _ptr(x):
    return None if x is None else x.data_ptr()


def _raw(ops, d, out, cfg, nsplit, D=None):
    """``fsmi_conv3d_halo_x3_ex`` (stride 1) on case ``d`` as ops.conv3d calls it, into ``out``; returns its
    status.  ``D``: a depth other than the case's (the refusals)."""
    from foundationstereo_amd import _lib
    D0, H, W = d["shape"]
    D = D0 if D is None else D
    kd, ks = d["kern"][0], d["kern"][2]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    floats = max(nsplit, 8) * B * d["cout"] * D * H * W
    ws = ops._split_workspace(DEV, stream, floats)
    pk = d["pk"]
    return _lib.load().fsmi_conv3d_halo_x3_ex(
        d["x"].data_ptr(), d["cin"], pk.whi.data_ptr(), pk.wlo.data_ptr(), d["sb"].data_ptr(), _ptr(d["res"]),
        _ptr(d["fatt"]), out.data_ptr(), B, d["cout"], D, H, W, kd, ks, 1, ACT_CODE[d.get("act")],
        int(d.get("res_pre", False)), cfg, nsplit, ws.data_ptr(), ws.numel(), stream)


def _launch(ops, d, cfg, nsplit, what):
    """One volume conv of case ``d`` into a fresh guarded buffer: the output is the middle batch slice
    [1 : B+1] of a (B + 2, Cout, D, H, W) tensor prefilled with NaN.  Asserts the launch counters, the
    written extent, the read-only operands and the range flag; returns the written slice."""
    from foundationstereo_amd import _lib
    full = torch.full((B + 2, d["cout"]) + tuple(d["shape"]), NAN, device=DEV)
    ops.conv_launch_counts(reset=True)
    _lib.check(_raw(ops, d, full[1:B + 1], cfg, nsplit), "conv3d")
    counts = ops.conv_launch_counts(reset=True)
    assert sum(counts) == 1, f"{what}: launches {[(i, n) for i, n in enumerate(counts) if n]}"
    if cfg >= 0:
        assert counts[cfg] == 1, f"{what}: tile {cfg} did not run: {[(i, n) for i, n in enumerate(counts) if n]}"
    assert not ops.range_overflowed(), f"{what}: range flag set"
    assert bool(torch.isnan(full[0]).all()) and bool(torch.isnan(full[B + 1]).all()), \
        f"{what}: written outside the batch slice"
    for name in ("x", "res", "fatt", "bias"):
        if d[name] is not None:
            assert torch.equal(_bits(d[name]), _bits(d[name + "_copy"])), f"{what}: operand {name} was modified"
    return full[1:B + 1]


def _run_epilogues(ops, kern, cfg, nsplit, cin, cout, DHW, fam, epilogues=tuple(EPILOGUES)):
    for epi in epilogues:
        d = dev_case(ops, kern, cin, cout, *DHW, epi)
        assert_exercised(d)
        what = f"{epi} k{kern} cfg {cfg} split {nsplit} {cin}->{cout} {DHW}"
        got = _launch(ops, d, cfg, nsplit, what)
        err = _check(got, d["ref"], d["tol"], what)
        _worst(epi, fam, err / d["tol"], err, d["tol"], what)
        # split-K sums its partials in order and the K groups sum through LDS: repeat runs are bit-equal
        again = _launch(ops, d, cfg, nsplit, what)
        assert torch.equal(_bits(got), _bits(again)), f"{what}: output differs between two runs"


KERNELS = [(3, 3, 3), (1, 3, 3), (1, 1, 1), (17, 1, 1)]
CHANNELS = [(40, 37), (72, 136)]
H, W = 9, 37


def _depths(kern):
    # 5: D*H*W % 4 != 0 (scalar reduce), shallower than the (17,1,1) kernel; 4 / 20: the float4 reduce
    return [5, 20] if kern[0] == 17 else [5, 4]


def _matrix():
    for kern in KERNELS:
        for D, (cin, cout), nsplit, cfg in itertools.product(_depths(kern), CHANNELS, [1, 2, 3], VOLUME_3D):
            yield pytest.param(kern, cfg, nsplit, cin, cout, (D, H, W),
                               id=f"k{kern[0]}{kern[1]}{kern[2]}-cfg{cfg}-s{nsplit}-{cin}to{cout}-D{D}")


@pytest.mark.parametrize("kern,cfg,nsplit,cin,cout,DHW", list(_matrix()))
def test_volume_epilogues_vs_fp64(ops_mod, range_clear, kern, cfg, nsplit, cin, cout, DHW):
    """Every epilogue, one after another, on tile ``cfg`` with split-K ``nsplit``.  (cfg -1 takes the
    policy's tile -- the depth tile, which never splits, for (17,1,1); a split-K beyond the number of
    chunks, 2 for (1,1,1) at 40 channels, runs one split per chunk.)"""
    _run_epilogues(ops_mod, kern, cfg, nsplit, cin, cout, DHW, family(cfg))


@pytest.mark.parametrize("cfg,nsplit", [(c, n) for n in (8, 17) for c in (0, 4, 7, 9, 21)] + [(DEPTH_TILE, 1)])
@pytest.mark.parametrize("D", [5, 20])
def test_volume_depth_kernel_splits(ops_mod, range_clear, cfg, nsplit, D):
    """(17,1,1) on 28 channels: 17 chunks.  nsplit 8 -> 3 chunks per split -> 6 splits, none empty; nsplit 17
    -> more than the float4 reduce's 8 partials: the scalar reduce although D*H*W % 4 == 0 at D = 20.  The
    depth tile on the same cases."""
    _run_epilogues(ops_mod, (17, 1, 1), cfg, nsplit, 28, 37, (D, H, W), family(cfg))


@pytest.mark.parametrize("nsplit", [1, 2])
@pytest.mark.parametrize("kern", [(3, 3, 3), (1, 1, 1)])
@pytest.mark.parametrize("kind", LADDER_KINDS)
@pytest.mark.parametrize("cfg", VOLUME_3D)
def test_volume_exponent_ladder(ops_mod, range_clear, cfg, kind, kern, nsplit):
    """Planes and channel chunks 2^6 apart: every chunk larger than all before it re-aims the block exponent
    and rescales the accumulators, whose content is then 2^-6 of the output.  Per-plane bound."""
    d = dev_ladder(ops_mod, kind, kern, 72, 37, 5, H, W)
    what = f"ladder {kind} k{kern} cfg {cfg} split {nsplit}"
    got = _launch(ops_mod, d, cfg, nsplit, what)
    ratio, err, bound = _check_planes(got, d["ref"], what)
    _worst("ladder_" + kind, family(cfg), ratio, err, bound, what)
    again = _launch(ops_mod, d, cfg, nsplit, what)
    assert torch.equal(_bits(got), _bits(again)), f"{what}: output differs between two runs"


def test_volume_refusals_and_fallback(ops_mod, range_clear):
    """Argument checks of the C entry: each returns an error before any launch.  32 + c on a volume is
    accepted and runs the plain tile c."""
    ops = ops_mod
    from foundationstereo_amd import _lib
    k333 = dev_case(ops, (3, 3, 3), 40, 37, 5, H, W, "relu_res_pre")
    k111 = dev_case(ops, (1, 1, 1), 40, 37, 4, H, W, "relu_res_pre")
    out = torch.full((B, 37, 5, H, W), NAN, device=DEV)

    def refused(d, cfg, match, **kw):
        with pytest.raises(_lib.FsmiError, match=match):
            _lib.check(_raw(ops, d, out, cfg, 1, **kw), "conv3d")

    ops.conv_launch_counts(reset=True)
    refused(k333, 11, "cfg 11")                            # the 5-row tile is 2D only
    for cfg in range(24, 30):
        refused(k111, cfg, "pointwise tile")               # 1x1, but a volume
    refused(k333, DEPTH_TILE, "tile 30")                   # the depth tile on a (3,3,3) kernel
    refused(k111, 4, "res_pre needs a volume", D=1)        # res_pre at D = KD = 1, stride 1
    refused(k333, 22, "no K-group variant")                # 16 + 6
    assert sum(ops.conv_launch_counts()) == 0, "a refused call launched a conv"
    assert bool(torch.isnan(out).all())

    plain = _launch(ops, k333, 3, 1, "cfg 3")
    full = torch.full((B + 2, 37, 5, H, W), NAN, device=DEV)
    _lib.check(_raw(ops, k333, full[1:B + 1], 35, 1), "conv3d")
    counts = ops.conv_launch_counts(reset=True)
    assert counts[3] == 1 and sum(counts) == 1, [(i, n) for i, n in enumerate(counts) if n]
    assert torch.equal(_bits(full[1:B + 1]), _bits(plain)), "cfg 32 + 3 on a volume differs from cfg 3"
    _check(plain, k333["ref"], k333["tol"], "cfg 3")
