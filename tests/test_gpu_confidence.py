"""ops.disp_confidence (csrc/confidence.hip) on the GPU against the fp64 oracle of
tests/confidence_oracle.py, within the tolerances derived there: every path of the kernel (the three
register tiers 16 / 64 / 128 and the streaming path above, at each boundary and one past it; up == 4
with its 16-byte accesses and the other factors), query given and self mode, three radii, each output
alone and all four together, the three logit families, exact one-hot columns, planted non-finite
values, and the torch.ops front end."""
import functools

import numpy as np
import pytest
import torch

from tests import confidence_oracle as co

pytestmark = pytest.mark.gpu

# (B, D, h, w, up): the issue's shapes, then D at and one past every path boundary, and the cap
SHAPES = [(1, 1, 1, 1, 1), (1, 2, 3, 5, 4), (2, 7, 5, 37, 3), (1, 48, 4, 70, 4), (2, 104, 3, 65, 1), (1, 8, 2, 257, 2),
          (300, 3, 2, 3, 1),
          (1, 16, 2, 9, 4), (1, 17, 2, 9, 4), (1, 64, 2, 9, 2), (1, 65, 2, 9, 4), (1, 128, 1, 67, 4), (1, 129, 1, 67, 4),
          (1, 136, 2, 5, 3), (1, 1024, 1, 3, 1)]
RADII = (0.0, 1.0, 2.5)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind="std2"):
    B, D, h, w, up = shape
    logits = co.make_logits(kind, B, D, h, w, seed=D * 7 + w)
    rng = np.random.default_rng(D * 13 + h)
    disp = (rng.uniform(-2.0, D + 1.0, (B, h * up, w * up)) * up).astype(np.float32)    # q in [-2, D + 1]
    return logits, disp


@functools.lru_cache(maxsize=None)
def _ref(shape, self_mode, radius, kind="std2"):
    logits, disp = _inputs(shape, kind)
    return co.confidence_ref(logits, None if self_mode else disp, up=shape[4], radius=radius)


def _run(dev, logits, disp, up, radius, want=co.CHANNELS, **kw):
    from foundationstereo_amd import ops
    outs = ops.disp_confidence(torch.from_numpy(logits).to(dev), None if disp is None else torch.from_numpy(disp).to(dev),
                               up=up, radius=radius, want=want, **kw)
    return {c: None if o is None else o.cpu().numpy() for c, o in zip(co.CHANNELS, outs)}


def _check(got, ref, D, self_mode, what):
    tol = co.tolerances(D, ref, self_mode)
    used = {c: co.fraction_used(got[c], ref[c], tol[c]) for c in co.CHANNELS}
    print(what, " ".join(f"{c}={v:.3f}" for c, v in used.items()))
    assert max(used.values()) <= 1.0, (what, used)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("self_mode", [False, True], ids=["query", "self"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64_each_output_alone_and_all_together(shape, self_mode, radius):
    dev = _gpu()
    B, D, h, w, up = shape
    logits, disp = _inputs(shape)
    d = None if self_mode else disp
    got = _run(dev, logits, d, up, radius)
    for c in co.CHANNELS:
        assert got[c].shape == (B, h * up, w * up) and got[c].dtype == np.float32
    _check(got, _ref(shape, self_mode, radius), D, self_mode, f"{shape} self={self_mode} r={radius}")
    for c in ("peak", "entropy", "mass"):
        assert np.all((got[c] >= 0) & (got[c] <= 1)), c                     # what risk_coverage accepts
    for c in co.CHANNELS:                                                   # a map alone: the same bits
        alone = _run(dev, logits, d, up, radius, want=(c,))
        assert all(alone[o] is None for o in co.CHANNELS if o != c)
        assert np.array_equal(alone[c], got[c]), c


@pytest.mark.parametrize("kind", ["std12", "alt88"])
@pytest.mark.parametrize("shape", [(1, 7, 5, 37, 3), (1, 48, 4, 70, 4), (1, 104, 3, 65, 1), (1, 200, 2, 33, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_peaked_and_underflowing_logits(shape, kind):
    dev = _gpu()
    logits, disp = _inputs(shape, kind)
    for self_mode in (False, True):
        for radius in RADII:
            got = _run(dev, logits, None if self_mode else disp, shape[4], radius)
            _check(got, _ref(shape, self_mode, radius, kind), shape[1], self_mode, f"{kind} {shape} self={self_mode} r={radius}")


@pytest.mark.parametrize("D,up", [(1, 1), (2, 4), (7, 3), (48, 4), (104, 4), (130, 2)])
def test_one_hot_columns_are_exact(D, up):
    dev = _gpu()
    h, w = 3, 5
    k = (np.arange(h * w).reshape(h, w) * 5) % D                            # the hot bin of every column
    logits = np.full((1, D, h, w), -np.inf, np.float32)
    logits[0, :, 1] = -200.0                                                # expf(-200 - 3) is 0 in fp32 too
    np.put_along_axis(logits[0], k[None], 3.0, axis=0)
    disp = (np.repeat(np.repeat(k, up, 0), up, 1)[None] * up).astype(np.float32)        # q = k
    for radius in RADII:
        for d in (disp, None):
            got = _run(dev, logits, d, up, radius)
            assert np.all(got["mass"] == 1.0) and np.all(got["peak"] == 1.0) and np.all(got["entropy"] == 1.0)
            assert np.all(got["spread"] == 0.0)
    # one bin off: mass is 1 with radius >= 1 and 0 with radius 0, spread exactly 1
    if D > 1:
        off = disp + np.where(disp / up + 1 < D, up, -up).astype(np.float32)
        got = _run(dev, logits, off, up, 0.0)
        assert np.all(got["mass"] == 0.0) and np.all(got["spread"] == 1.0)
        got = _run(dev, logits, off, up, 1.0)
        assert np.all(got["mass"] == 1.0) and np.all(got["spread"] == 1.0)


@pytest.mark.parametrize("shape", [(1, 7, 5, 37, 3), (1, 48, 4, 70, 4), (1, 130, 2, 11, 4)], ids=lambda s: "x".join(map(str, s)))
def test_planted_non_finite_values(shape):
    dev = _gpu()
    B, D, h, w, up = shape
    logits, disp = (a.copy() for a in _inputs(shape))
    logits[0, D // 2, 0, 0] = np.nan
    logits[0, 0, 1, 2] = np.inf
    logits[0, D - 1, 1, 3] = np.inf
    logits[0, :, 0, 4] = -np.inf                                            # no distribution at all
    logits[0, D // 3, 1, 5] = -np.inf                                       # probability 0
    logits[0, 1:, 1, 6] = -np.inf                                           # one bin left
    disp[0, 0, up * 7] = np.nan
    disp[0, 1, up * 8] = np.inf
    disp[0, 2, up * 8 + 1] = -np.inf
    disp[0, 0, up * 9] = 1.0e6                                             # finite, far outside the volume
    disp[0, 0, up * 9 + 1] = -1.0e6
    ref = co.confidence_ref(logits, disp, up=up, radius=1.0)
    bad_cols = [(0, 0), (1, 2), (1, 3), (0, 4)]
    for (y, x) in bad_cols:                                                 # the oracle itself says what the issue states
        for c in co.CHANNELS:
            assert np.isnan(ref[c][0, y * up:(y + 1) * up, x * up:(x + 1) * up]).all()
    for c in ("peak", "entropy"):
        assert np.isfinite(ref[c][0, :up, up * 7:up * 10]).all()
    assert np.isnan(ref["mass"][0, 0, up * 7]) and np.isnan(ref["spread"][0, 1, up * 8])
    assert ref["mass"][0, 0, up * 9] == 0.0 and np.isfinite(ref["spread"][0, 0, up * 9])
    got = _run(dev, logits, disp, up, 1.0)
    _check(got, ref, D, False, f"planted {shape}")                          # same NaN pattern, the rest within tolerance
    self_ref = co.confidence_ref(logits, None, up=up, radius=1.0)
    _check(_run(dev, logits, None, up, 1.0), self_ref, D, True, f"planted {shape} self")


def test_disp_scale_and_views():
    """An explicit disp_scale, a non-contiguous logits view and a (B,1,H,W) disparity through
    confidence.from_logits."""
    dev = _gpu()
    from foundationstereo_amd import confidence
    shape = (2, 7, 5, 37, 3)
    logits, disp = _inputs(shape)
    got = _run(dev, logits, disp * 2.0, 3, 1.0, disp_scale=1.0 / 6.0)
    ref = co.confidence_ref(logits, disp * 2.0, up=3, disp_scale=1.0 / 6.0, radius=1.0)
    _check(got, ref, 7, False, "disp_scale")
    wide = torch.from_numpy(np.concatenate([logits, logits], axis=3)).to(dev)[..., :37]
    c = confidence.from_logits(wide, torch.from_numpy(disp).to(dev)[:, None], up=3, radius=2.5, want=("mass", "spread"))
    assert c.peak is None and c.entropy is None
    full = _run(dev, logits, disp, 3, 2.5)
    assert np.array_equal(c.mass.cpu().numpy(), full["mass"]) and np.array_equal(c.spread.cpu().numpy(), full["spread"])


@pytest.mark.parametrize("shape", [(2, 7, 5, 37, 3), (1, 48, 4, 70, 4), (1, 129, 1, 67, 4)], ids=lambda s: "x".join(map(str, s)))
def test_views_that_are_not_16_byte_aligned(shape):
    """A contiguous view whose base is a multiple of 4 bytes only (a slice of a larger buffer) goes in
    without a copy and takes the one-float-at-a-time kernel, up == 4 included: the aligned call's bits."""
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    logits, disp = (torch.from_numpy(a).to(dev) for a in _inputs(shape))
    want = ops.disp_confidence(logits, disp, up=shape[4], radius=2.5)

    def shifted(t, k):
        buf = torch.empty(t.numel() + k, device=dev)
        v = buf[k:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 * k) % 16
        return v
    for kl, kd in ((1, 0), (0, 1), (3, 2)):
        lg, dp = shifted(logits, kl), shifted(disp, kd)
        for got in (ops.disp_confidence(lg, dp, up=shape[4], radius=2.5),
                    torch.ops.fsmi.disp_confidence(lg, dp, shape[4], None, 2.5)):
            for x, y in zip(got, want):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_torch_op_equals_ctypes_front_end():
    dev = _gpu()
    from foundationstereo_amd import ops, torch_ops
    torch_ops.load()
    for shape in [(2, 7, 5, 37, 3), (1, 48, 4, 70, 4), (1, 129, 1, 67, 4)]:
        logits, disp = (torch.from_numpy(a).to(dev) for a in _inputs(shape))
        a = torch.ops.fsmi.disp_confidence(logits, disp, shape[4], None, 2.5)
        b = ops.disp_confidence(logits, disp, up=shape[4], radius=2.5)
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
        a = torch.ops.fsmi.disp_confidence(logits, None, shape[4], None, 1.0, False, True, False, True)
        b = ops.disp_confidence(logits, None, up=shape[4], want=("spread", "entropy"))
        assert a[0].numel() == 0 and a[2].numel() == 0 and b[0] is None and b[2] is None
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
    with pytest.raises(RuntimeError, match="up"):
        torch.ops.fsmi.disp_confidence(logits, None, 9)


def test_front_end_refusals_on_device_tensors():
    dev = _gpu()
    from foundationstereo_amd import ops
    logits = torch.zeros(1, 8, 2, 4, device=dev)
    with pytest.raises(RuntimeError, match="disp must be"):
        ops.disp_confidence(logits, torch.zeros(1, 8, 15, device=dev))
    with pytest.raises(RuntimeError, match="D in 1"):
        ops.disp_confidence(torch.zeros(1, 1025, 1, 1, device=dev))
    with pytest.raises(RuntimeError, match="float32"):
        ops.disp_confidence(logits.half())
    with pytest.raises(RuntimeError, match=r"\(B,D,h,w\)"):
        ops.disp_confidence(logits[0])


def test_does_not_synchronise_and_is_capturable():
    """The call sits in a captured graph: replays on new logits give the eager result's bits."""
    dev = _gpu()
    from foundationstereo_amd import ops
    shape = (1, 48, 4, 70, 4)
    logits, disp = (torch.from_numpy(a).to(dev) for a in _inputs(shape))
    eager = ops.disp_confidence(logits, disp)
    static_l, static_d = torch.zeros_like(logits), torch.zeros_like(disp)
    ops.disp_confidence(static_l, static_d)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.disp_confidence(static_l, static_d)
    static_l.copy_(logits)
    static_d.copy_(disp)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
