"""Which tile ids (``cfg``) each conv entry point accepts, probed through the C ABI on the CPU, against the
hand-written lists of tests/conv_tiles.py.

No call here reaches a launch.  The stride-1 and stride-2 entries are called with ``nsplit = 2`` and no
workspace on 40 input channels (two 32-channel chunks): a tile that passes every tile check then stops at the
"split-K 2 needs N workspace floats" argument check, which follows all tile validation and precedes the launch;
a tile that is refused stops earlier with another message.  The entries that cannot be stopped that way -- the
transposed-conv phase launches (they fix ``nsplit = 1``) and the depth tile 30 (it never splits) -- are probed
only with ids they must refuse; the ids they accept are run by tests/test_gpu_parity.py and
tests/test_gpu_volume.py.  The pointers are host buffers that no host code reads through.

Skipped where a GPU is visible, so that a regression can never launch a kernel on those buffers.
"""
import ctypes

import pytest
import torch

from tests.conv_tiles import DEPTH_TILE, HALO_2D, PW_2D, S2_3D, UP2, VOLUME_3D

ERR_ARG = 1001
CIN, COUT, B = 40, 37, 2
SWEEP = range(-1, 64)
PIPE_ON_VOLUME = list(range(34, 42))       # 32 + c, c in 2..9: accepted on a volume, runs the plain tile c


@pytest.fixture(scope="module")
def lib():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: this probe passes host buffers as device pointers")
    from foundationstereo_amd import _lib
    lib = _lib.load()
    yield lib
    lib.fsmi_set_range_safe(0)


_BUF = (ctypes.c_char * 4096)()
PTR = (ctypes.addressof(_BUF) + 63) // 64 * 64     # 64-B aligned: the pointwise tiles want 16, scale_bias 8


def _outcome(lib, rc):
    """"accepted" (stopped at the split-K workspace check) or the refusal's message."""
    msg = lib.fsmi_last_error().decode()
    assert rc == ERR_ARG, f"status {rc} ({msg!r}): the call went past the argument checks"
    return "accepted" if "split-K 2 needs" in msg and "workspace floats" in msg else msg


def _conv2d(lib, cfg, ks, H, W, gate=False):
    from foundationstereo_amd import _lib
    seg, keep = _lib.ptr_array([PTR])
    ch, tot = (ctypes.c_int * 1)(CIN), (ctypes.c_int * 1)(CIN)
    if gate:        # mode 1: the small GRU's blend, Cout == Hd
        rc = lib.fsmi_conv2d_halo_x3_gate(seg, ch, tot, 1, PTR, PTR, PTR, 1, PTR, PTR, PTR, PTR, COUT, PTR, COUT, 0,
                                          B, COUT, ks, H, W, cfg, 2, None, 0, None)
    else:
        rc = lib.fsmi_conv2d_halo_x3(seg, ch, tot, 1, PTR, PTR, PTR, None, None, 0, PTR, COUT, 0, B, COUT, ks, H, W,
                                     1, 1.0, cfg, 2, None, 0, None)
    del keep
    return _outcome(lib, rc)


def _conv3d(lib, cfg, kd, ks, D, H, W, stride=1):
    return _outcome(lib, lib.fsmi_conv3d_halo_x3_ex(PTR, CIN, PTR, PTR, PTR, None, None, PTR, B, COUT, D, H, W, kd, ks,
                                                    stride, 1, 0, cfg, 2, None, 0, None))


def _accepted(probe, ids=SWEEP):
    return [c for c in ids if probe(c) == "accepted"]


@pytest.mark.parametrize("gate", [False, True])
def test_2d_tiles(lib, gate):
    lib.fsmi_set_range_safe(0)
    assert _accepted(lambda c: _conv2d(lib, c, 3, 9, 37, gate)) == sorted(HALO_2D)
    assert _accepted(lambda c: _conv2d(lib, c, 1, 9, 37, gate)) == sorted(HALO_2D)            # H*W % 4 != 0
    assert _accepted(lambda c: _conv2d(lib, c, 1, 8, 37, gate)) == sorted(HALO_2D + PW_2D)
    for c in PW_2D:
        assert "pointwise tile" in _conv2d(lib, c, 3, 8, 37, gate)
        assert "pointwise tile" in _conv2d(lib, c, 1, 9, 37, gate)
    assert "no K-group variant" in _conv2d(lib, 22, 3, 9, 37, gate)
    assert "tile 30" in _conv2d(lib, DEPTH_TILE, 1, 8, 37, gate)


def test_2d_tiles_safe_range(lib):
    """Safe range mode runs 2D maps on the volume instantiation: 11 / 43 become 9 and 24..29 become 4 before any
    tile check, on either kernel size and whatever H*W is; every other id as on a 2D map."""
    lib.fsmi_set_range_safe(1)
    try:
        for ks in (1, 3):
            assert _accepted(lambda c: _conv2d(lib, c, ks, 9, 37)) == sorted(HALO_2D + PW_2D)
    finally:
        lib.fsmi_set_range_safe(0)


@pytest.mark.parametrize("kd,ks", [(3, 3), (1, 1)])
def test_volume_tiles(lib, kd, ks):
    lib.fsmi_set_range_safe(0)
    assert _accepted(lambda c: _conv3d(lib, c, kd, ks, 5, 9, 37)) == sorted(VOLUME_3D + PIPE_ON_VOLUME)
    assert "cfg 11" in _conv3d(lib, 11, kd, ks, 5, 9, 37)
    assert "cfg 11" in _conv3d(lib, 43, kd, ks, 5, 9, 37)
    for c in PW_2D:
        assert "pointwise tile" in _conv3d(lib, c, kd, ks, 4, 9, 37)
    assert "tile 30" in _conv3d(lib, DEPTH_TILE, kd, ks, 5, 9, 37)
    assert "no K-group variant" in _conv3d(lib, 22, kd, ks, 5, 9, 37)


def test_depth_kernel_tiles(lib):
    """(17, 1, 1): the generic volume tiles.  -1 and 30 are the depth tile, which never splits: not probed."""
    lib.fsmi_set_range_safe(0)
    ids = [c for c in SWEEP if c not in (-1, DEPTH_TILE)]
    want = sorted(c for c in VOLUME_3D + PIPE_ON_VOLUME if c != -1)
    assert _accepted(lambda c: _conv3d(lib, c, 17, 1, 5, 9, 37), ids) == want


def test_2d_map_through_the_volume_entry(lib):
    """D = KD = 1 at stride 1 is the 2D instantiation: the 2D-only tiles 11 / 43 and the pointwise tiles too."""
    lib.fsmi_set_range_safe(0)
    assert _accepted(lambda c: _conv3d(lib, c, 1, 3, 1, 9, 37)) == sorted(HALO_2D)
    assert _accepted(lambda c: _conv3d(lib, c, 1, 1, 1, 8, 37)) == sorted(HALO_2D + PW_2D)


@pytest.mark.parametrize("kd,ks,D", [(3, 3, 5), (1, 1, 1)])
def test_stride2_tiles(lib, kd, ks, D):
    lib.fsmi_set_range_safe(0)
    assert _accepted(lambda c: _conv3d(lib, c, kd, ks, D, 9, 37, stride=2)) == sorted([-1] + S2_3D)


@pytest.mark.parametrize("phases", [8, 4])
def test_up2_refuses_every_other_tile(lib, phases):
    from foundationstereo_amd import _lib
    packs, keep = _lib.ptr_array([PTR] * phases)
    for c in SWEEP:
        if c == -1 or c in UP2:
            continue
        if phases == 8:
            rc = lib.fsmi_conv3d_up2_halo_x3(PTR, CIN, packs, packs, packs, PTR, B, COUT, 2, 5, 33, 1, c, None)
        else:
            rc = lib.fsmi_conv2d_up2_halo_x3(PTR, CIN, packs, packs, packs, PTR, B, COUT, 5, 33, 1, c, None)
        msg = _outcome(lib, rc)
        assert f"tile {c} " in msg, (c, msg)
    del keep
