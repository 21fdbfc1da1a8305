"""Host-side checks of the module layer's dispatch and of its weight-pack caches (CPU only).

The classification table drives the eligibility predicates with a stub tensor (only ``is_cuda``, ``dtype``,
``shape`` and ``dim()`` are read); every expected route was taken from the six hand-written predicates
``submodule._route`` replaced (``_fast3d``, ``_fast_s2_3d``, ``_fast_s2_2d``, ``_fast_up3d``, ``fast_up2d``,
``_fast2d``): the table was written against them and passed there before it was ported.  The cache tests build
real packs on CPU tensors."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from foundationstereo_amd import ops, submodule as sub, update


def stub(nd=2, is_cuda=True, dtype=torch.float32):
    shape = (1, 8) + (8,) * nd
    return SimpleNamespace(is_cuda=is_cuda, dtype=dtype, shape=shape, dim=lambda: len(shape))


def route(x, conv, bn=None):
    """(kind, spatial dims) of the HIP path ``conv`` (+ ``bn``) takes on ``x``, or None."""
    hits = [(sub._route(x, conv, bn, nd), nd) for nd in (2, 3) if sub._route(x, conv, bn, nd)]
    assert len(hits) <= 1, hits
    return hits[0] if hits else None


C2, C3, T2, T3 = nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d
ACCEPTED = [
    ("conv3d_k3_p1", lambda: C3(8, 8, 3, padding=1), ("s1", 3)),
    ("conv3d_1x3x3", lambda: C3(8, 8, (1, 3, 3), padding=(0, 1, 1)), ("s1", 3)),
    ("conv3d_17x1x1", lambda: C3(8, 8, (17, 1, 1), padding=(8, 0, 0)), ("s1", 3)),
    ("conv3d_k1", lambda: C3(8, 8, 1), ("s1", 3)),
    ("conv3d_k3_s2_p1", lambda: C3(8, 8, 3, stride=2, padding=1), ("s2", 3)),
    ("conv2d_k1", lambda: C2(8, 8, 1), ("s1", 2)),
    ("conv2d_k3_p1", lambda: C2(8, 8, 3, padding=1), ("s1", 2)),
    ("conv2d_k3_s2_p1", lambda: C2(8, 8, 3, stride=2, padding=1), ("s2", 2)),
    ("conv2d_k1_s2_p0", lambda: C2(8, 8, 1, stride=2), ("s2", 2)),
    ("deconv3d_k4_s2_p1", lambda: T3(8, 8, 4, stride=2, padding=1), ("up", 3)),
    ("deconv2d_k4_s2_p1", lambda: T2(8, 8, 4, stride=2, padding=1), ("up", 2)),
]
REJECTED = [
    ("conv2d_dilation2", lambda: C2(8, 8, 3, padding=1, dilation=2)),
    ("conv2d_dilation2_same", lambda: C2(8, 8, 3, padding=2, dilation=2)),
    ("conv3d_dilation2", lambda: C3(8, 8, 3, padding=1, dilation=2)),
    ("deconv2d_dilation2", lambda: T2(8, 8, 4, stride=2, padding=1, dilation=2)),
    ("conv2d_groups2", lambda: C2(8, 8, 3, padding=1, groups=2)),
    ("conv3d_groups2", lambda: C3(8, 8, 3, padding=1, groups=2)),
    ("conv3d_s2_groups2", lambda: C3(8, 8, 3, stride=2, padding=1, groups=2)),
    ("deconv3d_groups2", lambda: T3(8, 8, 4, stride=2, padding=1, groups=2)),
    ("conv3d_even_kd", lambda: C3(8, 8, (2, 3, 3), padding=(1, 1, 1))),
    ("conv3d_even_kd_p0", lambda: C3(8, 8, (2, 1, 1), padding=(0, 0, 0))),
    ("conv2d_k3_p0", lambda: C2(8, 8, 3)),
    ("conv2d_k1_p1", lambda: C2(8, 8, 1, padding=1)),
    ("conv3d_k3_p0", lambda: C3(8, 8, 3)),
    ("conv2d_k3_s2_p0", lambda: C2(8, 8, 3, stride=2)),
    ("conv3d_17x1x1_p0", lambda: C3(8, 8, (17, 1, 1))),
    ("conv2d_k5_p2", lambda: C2(8, 8, 5, padding=2)),
    ("conv2d_1x3", lambda: C2(8, 8, (1, 3), padding=(0, 1))),
    ("conv3d_1x3x3_s122", lambda: C3(8, 8, (1, 3, 3), padding=(0, 1, 1), stride=(1, 2, 2))),
    ("conv3d_k1_s2", lambda: C3(8, 8, 1, stride=2)),
    ("deconv2d_output_padding1", lambda: T2(8, 8, 4, stride=2, padding=1, output_padding=1)),
    ("deconv3d_output_padding1", lambda: T3(8, 8, 4, stride=2, padding=1, output_padding=1)),
    ("deconv3d_1x4x4", lambda: T3(8, 8, (1, 4, 4), stride=(1, 2, 2), padding=(0, 1, 1))),
    ("deconv2d_k2_s2", lambda: T2(8, 8, 2, stride=2)),
    ("linear", lambda: nn.Linear(8, 8)),
]


def _nd(conv):
    return conv.weight.dim() - 2


def _bn(conv):
    return (nn.BatchNorm3d if _nd(conv) == 3 else nn.BatchNorm2d)(8)


@pytest.mark.parametrize("norm", ["none", "eval_bn", "identity"])
@pytest.mark.parametrize("name,make,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_accepted(name, make, want, norm):
    conv = make()
    bn = {"none": None, "eval_bn": _bn(conv).eval(), "identity": nn.Identity()}[norm]
    with torch.no_grad():
        assert route(stub(_nd(conv)), conv, bn) == want
        for dt in (torch.float16, torch.bfloat16):
            assert route(stub(_nd(conv), dtype=dt), conv, bn) == want


@pytest.mark.parametrize("norm", ["none", "eval_bn", "identity"])
@pytest.mark.parametrize("name,make", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_conv(name, make, norm):
    conv = make()
    bn = {"none": None, "eval_bn": _bn(conv).eval(), "identity": nn.Identity()}[norm]
    with torch.no_grad():
        assert route(stub(_nd(conv)), conv, bn) is None


@pytest.mark.parametrize("name,make,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_rejected_norm_and_tensor(name, make, want):
    conv = make()
    nd = _nd(conv)
    good = _bn(conv).eval()
    wrong_dim = (nn.BatchNorm2d if nd == 3 else nn.BatchNorm3d)(8).eval()
    with torch.no_grad():
        assert route(stub(nd), conv, good) == want
        assert route(stub(nd), conv, _bn(conv).train()) is None
        assert route(stub(nd), conv, type(good)(8, track_running_stats=False).eval()) is None
        assert route(stub(nd), conv, wrong_dim) is None
        assert route(stub(nd), conv, nn.InstanceNorm2d(8)) is None
        assert route(stub(nd, is_cuda=False), conv, good) is None
        assert route(stub(nd, dtype=torch.int32), conv, good) is None
        assert route(stub(nd, dtype=torch.float64), conv, None) is None
    with torch.enable_grad():
        assert route(stub(nd), conv, good) is None
        assert route(stub(nd), conv, None) is None


@pytest.mark.parametrize("name,make,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_s2_knob(name, make, want, monkeypatch):
    """``S2_3D = False`` (the off-path the stride-2 tests use as their reference) drops the stride-2
    routes and nothing else."""
    monkeypatch.setattr(sub, "S2_3D", False)
    conv = make()
    with torch.no_grad():
        assert route(stub(_nd(conv)), conv, None) == (None if want[0] == "s2" else want)


def test_hip_in():
    with torch.no_grad():
        assert sub._hip_in(nn.InstanceNorm2d(8), stub(2))
        assert sub._hip_in(nn.InstanceNorm2d(8), stub(2, dtype=torch.float16))
        assert not sub._hip_in(nn.InstanceNorm2d(8, affine=True), stub(2))
        assert not sub._hip_in(nn.InstanceNorm2d(8, track_running_stats=True), stub(2))
        assert not sub._hip_in(nn.InstanceNorm2d(8), stub(3))               # a 5-D input
        assert not sub._hip_in(nn.InstanceNorm3d(8), stub(3))
        assert not sub._hip_in(nn.BatchNorm2d(8).eval(), stub(2))
        assert not sub._hip_in(nn.InstanceNorm2d(8), stub(2, is_cuda=False))
        assert not sub._hip_in(nn.InstanceNorm2d(8), stub(2, dtype=torch.int32))
    with torch.enable_grad():
        assert not sub._hip_in(nn.InstanceNorm2d(8), stub(2))


def test_conv_kind_reads_attributes_only():
    """The classifier half sees no tensor: same kinds as the routed table."""
    for _, make, want in ACCEPTED:
        assert sub._conv_kind(make()) == want[0]
    for _, make in REJECTED:
        assert sub._conv_kind(make()) is None


def test_tensor_half_shared():
    """``_hip`` is the tensor test of the remaining predicates; ``update._fast`` adds CONV_ENGINE."""
    with torch.no_grad():
        assert sub._hip(stub()) and update._fast(stub())
        assert not sub._hip(stub(is_cuda=False)) and not update._fast(stub(is_cuda=False))
        assert not sub._hip(stub(dtype=torch.int32)) and not update._fast(stub(dtype=torch.int32))
        up = nn.ConvTranspose2d(8, 8, 4, stride=2, padding=1)
        assert sub.fast_up2d(stub(), up) and sub.fast_up2d(stub(), up, nn.BatchNorm2d(8).eval())
        assert not sub.fast_up2d(stub(), nn.Conv2d(8, 8, 3, padding=1))
    with torch.enable_grad():
        assert not sub._hip(stub()) and not update._fast(stub())


def test_update_fast_conv_engine(monkeypatch):
    monkeypatch.setattr(update, "CONV_ENGINE", "miopen")
    with torch.no_grad():
        assert not update._fast(stub())


# ---------------------------------------------------------------- pack caches

def _tensors(pack):
    """The device-side content of a cached pack: PackedConv halves and scales, plain tensors, nested."""
    if isinstance(pack, torch.Tensor):
        return [pack]
    if isinstance(pack, ops.PackedConv):
        return [pack.whi, pack.wlo, pack.wscale]
    return [t for p in pack for t in _tensors(p)]


def _leaves(pack):
    return [pack] if isinstance(pack, (torch.Tensor, ops.PackedConv)) else [x for p in pack for x in _leaves(p)]


def _same_objects(a, b):
    la, lb = _leaves(a), _leaves(b)
    return len(la) == len(lb) and all(x is y for x, y in zip(la, lb))


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))


def _randomize_(bn):
    with torch.no_grad():
        bn.weight.uniform_(0.5, 2.0)
        bn.bias.normal_()
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    return bn.eval()


def _check_cache(get, mods, weights, biases=(), stats=()):
    """``get()`` -> (weights pack, bias): same objects until a keyed tensor changes, then a rebuild whose
    weights pack (``weights`` / ``stats`` changes) or bias (``biases``) differs."""
    first = get()
    assert _same_objects(get(), first)
    with torch.no_grad():
        for kind, ts in (("w", weights), ("b", biases), ("w", stats)):
            for t in ts:
                old = get()
                t.copy_(torch.rand_like(t) + 0.5)
                new = get()
                assert not any(x is y for x, y in zip(_leaves(new), _leaves(old)))
                assert not _equal(new[0] if kind == "w" else new[1], old[0] if kind == "w" else old[1])
                assert _same_objects(get(), new)
    # the parameters' storage replaced: a dtype round trip (same values), then fresh tensors (new values)
    # ``keep`` holds the old storages (``.data`` aliases them): a freed one could hand its address to the new
    # tensor, and a swap onto a recycled address with an unchanged version is invisible to the key
    old, keep = get(), [t.data for m in mods for t in list(m.parameters()) + list(m.buffers())]
    for m in mods:
        m.to(torch.float64).to(torch.float32)
    new = get()
    assert not any(x is y for x, y in zip(_leaves(new), _leaves(old))) and _equal(new, old)
    keep += [t.data for m in mods for t in list(m.parameters()) + list(m.buffers())]
    for m in mods:
        m.load_state_dict({k: torch.rand_like(v) + 0.5 if v.is_floating_point() else v.clone()
                           for k, v in m.state_dict().items()}, assign=True)
    newer = get()
    assert not any(x is y for x, y in zip(_leaves(newer), _leaves(new))) and not _equal(newer[0], new[0])
    assert _same_objects(get(), newer)
    del keep


def _no_grad_fn(pack):
    return all(t.grad_fn is None and not t.requires_grad for t in _tensors(pack))


@pytest.mark.parametrize("nd", [2, 3])
def test_packed_bn_cache(nd):
    conv = (nn.Conv3d if nd == 3 else nn.Conv2d)(8, 12, 3, padding=1)
    bn = _randomize_((nn.BatchNorm3d if nd == 3 else nn.BatchNorm2d)(12))
    with torch.enable_grad():
        assert _no_grad_fn(sub._packed_bn(conv, bn))
    _check_cache(lambda: sub._packed_bn(conv, bn), [conv, bn], [conv.weight, bn.weight], [conv.bias, bn.bias, bn.running_mean],
                 [bn.running_var])


@pytest.mark.parametrize("bias", [True, False])
def test_packed_bn_is_the_fp64_fold(bias):
    conv = nn.Conv2d(8, 12, 3, padding=1, bias=bias)
    bn = _randomize_(nn.BatchNorm2d(12))
    pk, b = sub._packed_bn(conv, bn)
    with torch.no_grad():
        sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        ref = ops.PackedConv((conv.weight.double() * sc.view(-1, 1, 1, 1)).float())
        b0 = conv.bias.double() if bias else torch.zeros(12, dtype=torch.float64)
        rb = ((b0 - bn.running_mean.double()) * sc + bn.bias.double()).float()
    assert _equal(pk, ref) and torch.equal(b, rb)
    # no norm / Identity: the plain weights and bias
    conv2 = nn.Conv2d(8, 12, 3, padding=1)
    for norm in (None, nn.Identity()):
        pk, b = sub._packed_bn(conv2, norm)
        assert _equal(pk, ops.PackedConv(conv2.weight)) and torch.equal(b, conv2.bias.detach())
        conv2.__dict__.pop("_fsmi_pack_bn")


@pytest.mark.parametrize("nd", [2, 3])
def test_packed_up_cache(nd):
    conv = (nn.ConvTranspose3d if nd == 3 else nn.ConvTranspose2d)(8, 12, 4, stride=2, padding=1)
    bn = _randomize_((nn.BatchNorm3d if nd == 3 else nn.BatchNorm2d)(12))
    packs, b = sub._packed_up(conv, bn)
    assert len(packs) == 2 ** nd
    with torch.no_grad():
        sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        ref = (ops.pack_deconv_phases if nd == 3 else ops.pack_deconv2d_phases)(conv.weight, sc)
        rb = ((conv.bias.double() - bn.running_mean.double()) * sc + bn.bias.double()).float()
    assert _equal(packs, ref) and torch.equal(b, rb)
    with torch.enable_grad():
        assert _no_grad_fn(sub._packed_up(conv, bn))
    _check_cache(lambda: sub._packed_up(conv, bn), [conv, bn], [conv.weight, bn.weight], [conv.bias, bn.bias, bn.running_mean],
                 [bn.running_var])


def test_update_packed_cache():
    conv = nn.Conv2d(16, 8, 3, padding=1)
    with torch.enable_grad():
        assert _no_grad_fn(update._packed(conv))
    _check_cache(lambda: update._packed(conv), [conv], [conv.weight], [conv.bias])
    lin = nn.Linear(16, 8)                                  # a Linear packs as a 1x1 conv
    assert _equal(update._packed(lin)[0], ops.PackedConv(lin.weight[:, :, None, None]))


def test_update_packed_stacked_zr():
    gru = update.RaftConvGRU(8, 16, 3)
    pk, b = update._packed(gru.convz, gru.convr)
    assert pk.cout == 16 and _equal(pk, ops.PackedConv(gru.convz.weight, gru.convr.weight))
    assert torch.equal(b, torch.cat([gru.convz.bias, gru.convr.bias]).detach())
    _check_cache(lambda: update._packed(gru.convz, gru.convr), [gru.convz, gru.convr],
                 [gru.convz.weight, gru.convr.weight], [gru.convz.bias, gru.convr.bias])
    # the torch path's stacked weights: a slot on the GRU module, no side dict
    assert not hasattr(gru, "_zr_cache")
    _check_cache(lambda: update._stacked_zr(gru), [gru.convz, gru.convr], [gru.convz.weight, gru.convr.weight],
                 [gru.convz.bias, gru.convr.bias])
    w, b = update._stacked_zr(gru)
    assert torch.equal(w, torch.cat([gru.convz.weight, gru.convr.weight]).detach())


def test_update_packed_cin_orders():
    conv = nn.Conv2d(16, 8, 3, padding=1)
    swapped = tuple(range(8, 16)) + tuple(range(8))
    head = tuple(range(8))
    with torch.enable_grad():
        a, b, plain = (update._packed(conv, cin_order=swapped), update._packed(conv, cin_order=head),
                       update._packed(conv))
    assert _no_grad_fn(a) and _no_grad_fn(b)
    # one slot per order: none evicts another
    assert _same_objects(update._packed(conv, cin_order=swapped), a)
    assert _same_objects(update._packed(conv, cin_order=head), b)
    assert _same_objects(update._packed(conv), plain)
    assert _equal(a[0], ops.PackedConv(conv.weight[:, list(swapped)]))
    assert _equal(b[0], ops.PackedConv(conv.weight[:, :8])) and b[0].cin == 8
    for order in (swapped, head):
        _check_cache(lambda: update._packed(conv, cin_order=order), [conv], [conv.weight], [conv.bias])
    assert _same_objects(update._packed(conv, cin_order=swapped), update._packed(conv, cin_order=list(swapped)))


def test_disparity_transformer_pack_cache():
    att = sub.CostVolumeDisparityAttention(d_model=28, nhead=4, dim_feedforward=28, num_transformer=2, max_len=16)
    with torch.enable_grad():
        first = att._packed()
    assert first.grad_fn is None and not first.requires_grad
    assert att._packed() is first
    lin = att.sa[1].linear1
    for t in (lin.weight, lin.bias, att.sa[0].norm2.weight):
        old = att._packed()
        with torch.no_grad():
            t.copy_(torch.rand_like(t) + 0.5)
        new = att._packed()
        assert new is not old and not torch.equal(new, old) and att._packed() is new
    old, keep = att._packed(), [t.data for t in att.parameters()]      # old storages stay alive
    att.to(torch.float64).to(torch.float32)
    new = att._packed()
    assert new is not old and torch.equal(new, old)
    keep += [t.data for t in att.parameters()]
    att.load_state_dict({k: torch.rand_like(v) for k, v in att.state_dict().items()}, assign=True)
    assert not torch.equal(att._packed(), new)
    del keep


def test_patch_fold_cache():
    from foundationstereo_amd.foundation_stereo import hourglass
    hg = hourglass({"max_disp": 64}, 8, feat_dims=[16, 16, 16, 16]).eval()
    pc, bn = hg.conv_patch[0], _randomize_(hg.conv_patch[1])
    scale, shift = hg._patch_fold()
    with torch.no_grad():
        inv = (bn.running_var.double() + bn.eps).rsqrt() * bn.weight.double()
        ref = (pc.bias.double() - bn.running_mean.double()) * inv + bn.bias.double()
    assert torch.equal(scale, inv.float()) and torch.equal(shift, ref.float())
    again = hg._patch_fold()
    assert again[0] is scale and again[1] is shift
    with torch.no_grad():
        bn.running_var.copy_(torch.rand_like(bn.running_var) + 0.5)
    assert not torch.equal(hg._patch_fold()[0], scale)
