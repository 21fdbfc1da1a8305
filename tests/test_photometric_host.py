"""CPU-only checks of the photometric consistency stage: the exported entry points and their refusals
(made before any HIP call), the front ends' refusals, the new flags' defaults, and the numpy oracle
itself on closed forms and on the coverage the GPU tests' fuzz inputs must have."""
import ctypes

import numpy as np
import pytest
import torch

from tests import photometric_oracle as po


def _lib():
    from foundationstereo_amd import _lib
    return _lib, _lib.load()


def test_entry_points_are_exported_and_declared():
    _l, lib = _lib()
    assert len(_l.SIGNATURES["fsmi_photo_consistency"]) == 28 and len(_l.SIGNATURES["fsmi_photo_consistency_ws_bytes"]) == 4
    assert hasattr(lib, "fsmi_photo_consistency") and hasattr(lib, "fsmi_photo_consistency_ws_bytes")
    from foundationstereo_amd import ops, photometric, torch_ops
    assert "photo_consistency" in torch_ops.OPS
    assert (photometric.NFIXED, photometric.MAX_OFFSETS) == (8, 8) == (ops.PHOTO_NFIXED, ops.PHOTO_MAX_OFFSETS)
    assert (photometric.N_SCORED, photometric.N_SSIM, photometric.N_INVALID, photometric.N_OUT_OF_VIEW, photometric.L1_MEAN,
            photometric.L1_RMS, photometric.DSSIM_MEAN, photometric.PHOTOMETRIC) == tuple(range(8))
    # one row of 8 + 2R doubles per 64 x 12 tile and pair; 0 for arguments the call refuses
    assert lib.fsmi_photo_consistency_ws_bytes(2, 13, 65, 3) == 2 * (2 * 2) * 14 * 8
    assert lib.fsmi_photo_consistency_ws_bytes(1, 1, 1, 0) == 64
    assert lib.fsmi_photo_consistency_ws_bytes(0, 4, 4, 0) == 0 and lib.fsmi_photo_consistency_ws_bytes(1, 4, 4, 9) == 0


def _call(lib, B=1, C=3, H=4, W=8, fmt=0, offsets=(), alpha=0.85, ssim=1, null=(), shift=None, strides=None, n=None):
    """Pointer values are never dereferenced (``offsets`` is host memory): every refusal happens before a HIP call."""
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    names = ("disp", "left", "right", "mask", "warped", "l1", "dssim", "table", "sums", "ws")
    ptrs = [None if k in null else p + (shift or {}).get(k, 0) for k in names]
    offs = (ctypes.c_float * 9)(*offsets)
    st = strides or (H * W, W, C * H * W, H * W, W, C * H * W, H * W, W)
    return lib.fsmi_photo_consistency(*ptrs, B, C, H, W, fmt, *st, offs, len(offsets) if n is None else n, alpha, ssim, None)


@pytest.mark.parametrize("shape", [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3)])
def test_empty_and_negative_shapes_are_refused(shape):
    _, lib = _lib()
    B, H, W = shape
    assert _call(lib, B=B, H=H, W=W) == 1001 and b"shape" in lib.fsmi_last_error()


def test_channels_format_offsets_and_alpha_are_refused():
    _, lib = _lib()
    for C in (0, 2, 4):
        assert _call(lib, C=C) == 1001 and b"channels" in lib.fsmi_last_error()
    assert _call(lib, fmt=2) == 1001 and b"image_format" in lib.fsmi_last_error()
    assert _call(lib, offsets=(0.0,) * 9) == 1001 and b"n_offsets = 9" in lib.fsmi_last_error()
    assert _call(lib, n=-1) == 1001 and b"n_offsets" in lib.fsmi_last_error()
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _call(lib, offsets=(0.0, bad)) == 1001 and b"row offset 1 is not finite" in lib.fsmi_last_error()
    for alpha in (-0.01, 1.01, float("nan"), float("inf")):
        assert _call(lib, alpha=alpha) == 1001 and b"alpha" in lib.fsmi_last_error()


def test_null_pointers_misalignment_and_strides_are_refused():
    _, lib = _lib()
    for k in ("disp", "left", "right", "table", "sums", "ws"):
        assert _call(lib, null=(k,)) == 1001 and b"null" in lib.fsmi_last_error(), k
    for k in ("warped", "l1", "dssim"):
        assert _call(lib, shift={k: 4}) == 1001 and b"16-byte aligned" in lib.fsmi_last_error(), k
    assert _call(lib, shift={"disp": 2}) == 1001 and b"4-byte aligned" in lib.fsmi_last_error()
    assert _call(lib, shift={"table": 4}) == 1001 and b"8-byte aligned" in lib.fsmi_last_error()
    assert _call(lib, ssim=0) == 1001 and b"dssim map needs ssim" in lib.fsmi_last_error()
    assert _call(lib, strides=(32, 7, 96, 32, 8, 96, 32, 8)) == 1001 and b"disp strides" in lib.fsmi_last_error()
    assert _call(lib, strides=(32, 8, 96, 32, 7, 96, 32, 8)) == 1001 and b"row strides" in lib.fsmi_last_error()
    assert _call(lib, strides=(32, 8, 96, 32, 8, 96, -1, 8)) == 1001 and b"row strides" in lib.fsmi_last_error()
    # the uint8 format ignores the image strides
    assert _call(lib, fmt=1, strides=(32, 8, 0, 0, 0, 0, 0, 0), null=("disp",)) == 1001 and b"null" in lib.fsmi_last_error()


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    from foundationstereo_amd import ops, photometric
    d, img = torch.ones(1, 4, 8), torch.ones(1, 3, 4, 8)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.photo_consistency(d, img, img)
    with pytest.raises(RuntimeError, match="ROCm"):
        photometric.consistency(d[0], img[0], img[0])
    with pytest.raises(RuntimeError, match="ROCm"):
        photometric.warp_right(d, torch.ones(4, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm"):
        photometric.row_probe(d, img, img)
    with pytest.raises(ValueError, match=r"\(H,W\)"):
        photometric.consistency(torch.ones(8), img, img)
    with pytest.raises(ValueError, match="left must be"):
        photometric.consistency(d, torch.ones(8), img)
    with pytest.raises(ValueError, match="at most 8"):
        photometric.row_probe(d, img, img, max_offset=4.0, step=1.0)
    with pytest.raises(ValueError, match="step"):
        photometric.row_probe(d, img, img, step=0.0)


def test_demo_and_evaluate_flags_default_off_and_refuse():
    from foundationstereo_amd import demo, evaluate
    a = demo.parser().parse_args([])
    assert (a.photo_check, a.photo_max) == (0, 32.0)
    e = evaluate.parser().parse_args(["--gt_file", "x"])
    assert e.photometric is False and e.row_probe == 0
    assert evaluate.parser().parse_args(["--photometric"]).gt_file is None
    with pytest.raises(SystemExit, match="panorama"):
        demo.main(["--photo_check", "1", "--camera_type", "panorama"])
    with pytest.raises(ValueError, match="photo_check"):
        demo.run_pair(None, None, None, None, None, photo_check=1, camera_type="panorama")
    for flags in (["--photometric"], ["--row_probe", "2"]):
        with pytest.raises(SystemExit, match="--left_file and --right_file"):
            evaluate.main(flags + ["--pred_file", "p.npy"])
        with pytest.raises(SystemExit, match="--left_file and --right_file"):
            evaluate.main(flags + ["--pred_file", "p.npy", "--left_file", "l.png"])
    with pytest.raises(SystemExit, match="--gt_file"):
        evaluate.main(["--pred_file", "p.npy"])
    with pytest.raises(SystemExit, match="row_probe"):
        evaluate.main(["--row_probe", "4"])


def test_oracle_on_the_shift_scene():
    H, W, d = 6, 11, 3
    disp, left, right = po.shift_scene(H, W, d, 0)
    o = po.oracle32(disp, left, right)
    L = po.planar(left, np.float32)
    assert not o["invalid"].any() and o["out_of_view"][0, :, :d].all() and o["sampled"][0, :, d:].all()
    assert np.array_equal(o["warped"][:, :, :, d:], L[:, :, :, d:]) and not o["warped"][:, :, :, :d].any()
    assert (o["l1"][0, :, d:] == 0).all() and np.isinf(o["l1"][0, :, :d]).all()
    # SSIM: rows 1 .. H-2, columns d+1 .. W-2 (the window's left column must be sampled too); identical windows give 1
    has = np.zeros((1, H, W), bool)
    has[0, 1:H - 1, d + 1:W - 1] = True
    assert np.array_equal(o["has_ssim"], has) and (o["dssim"][has] == 0).all() and np.isinf(o["dssim"][~has]).all()
    assert o["table"][0].tolist() == [H * (W - d), (H - 2) * (W - d - 2), 0, H * d, 0, 0, 0, 0]
    # a mask takes pixels out of the scores, not out of the windows
    mask = np.ones((1, H, W), np.uint8)
    mask[0, 2, 5] = 0
    m = po.oracle32(disp, left, right, mask)
    assert m["table"][0, :2].tolist() == [H * (W - d) - 1, (H - 2) * (W - d - 2) - 1] and m["has_ssim"][0, 2, 6]
    assert np.array_equal(m["warped"], o["warped"])


def test_oracle_row_probe_finds_the_row_shift():
    disp, left, right = po.shift_scene(9, 14, 3, 1)
    offs = (-2, -1, 0, 1, 2)
    o = po.oracle32(disp, left, right, None, offs)
    n, l1 = o["table"][0, 8::2], o["table"][0, 9::2]
    assert n.tolist() == [7 * 11, 8 * 11, 9 * 11, 8 * 11, 7 * 11]          # rows whose offset row exists x sampled columns
    assert l1[3] == 0 and (np.delete(l1, 3) > 0).all()
    half = po.oracle32(disp, left, right, None, (0.5, 1.0))                  # ty = 0.5: the mean of two rows, not a match
    assert half["table"][0, 9] > 0 and half["table"][0, 11] == 0


def test_oracle_interpolates_a_ramp_exactly():
    H, W = 3, 12
    right = np.broadcast_to((np.arange(W, dtype=np.float32) * 4 + 10)[None, None, None, :], (1, 1, H, W)).copy()
    left = np.zeros_like(right)
    disp = np.full((1, H, W), 2.5, np.float32)
    o = po.oracle32(disp, left, right)
    want = 4 * (np.arange(W, dtype=np.float32) - 2.5) + 10                   # exact in fp32: xr = u - 2.5, t = 0.5
    assert np.array_equal(o["warped"][0, 0, :, 3:], np.broadcast_to(want[3:], (H, W - 3)))
    assert not o["warped"][0, 0, :, :3].any() and o["out_of_view"][0, :, :3].all()
    assert np.array_equal(o["l1"][0, :, 3:], np.broadcast_to(want[3:], (H, W - 3)))
    edge = po.oracle32(np.full((1, H, W), 0.5, np.float32), left, right)
    assert edge["warped"][0, 0, 0, W - 1] == 4 * (W - 1.5) + 10 and edge["warped"][0, 0, 0, 1] == 4 * 0.5 + 10


@pytest.mark.parametrize("shape", po.GPU_SHAPES)
def test_fuzz_reaches_every_kind_of_pixel(shape):
    B, H, W = shape
    d, left, right, mask = po.gpu_fuzz(shape, 3, "u8")
    for C, fmt in ((1, "f32"), (3, "f32"), (1, "u8")):                       # disparities and mask do not depend on the images
        d2, _, _, m2 = po.gpu_fuzz(shape, C, fmt)
        assert np.array_equal(d, d2, equal_nan=True) and np.array_equal(mask, m2)
    o = po.oracle32(d, left, right, mask)
    xr = np.arange(W, dtype=np.float32) - d
    assert (d == np.floor(d))[o["sampled"]].any() and (d != np.floor(d))[o["sampled"]].any()     # t == 0 and t != 0
    assert np.isnan(d).any() or np.isinf(d).any() or (d <= 0).any()
    if W >= 9:
        assert (xr == 0)[o["sampled"]].any() and ((xr < 0) & (xr > -1e-4)).any()
        assert np.isnan(d).any() and np.isposinf(d).any() and (d == 0).any() and (d < 0).any()
    for b in range(B):
        kinds = [o["invalid"][b], o["out_of_view"][b], o["sampled"][b] & ~o["scored"][b], o["scored"][b] & ~o["has_ssim"][b]]
        assert all(k.any() for k in kinds)
        # column 0 is never sampled, so windows exist from width 5 on only (the oracle's docstring)
        assert o["has_ssim"][b].any() == (W >= 5 and H >= 3)
        assert 2 * o["scored"][b].sum() >= H * W


def test_the_recorded_dssim_tolerance_covers_the_oracles_on_every_gpu_input():
    worst = 0.0
    for shape, C, fmt in po.GPU_CASES:
        d, left, right, mask = po.gpu_fuzz(shape, C, fmt)
        for m in (None, mask):
            a, b = po.oracle32(d, left, right, m), po.oracle64(d, left, right, m)
            assert np.array_equal(a["has_ssim"], b["has_ssim"]) and np.array_equal(a["table"][:, :4], b["table"][:, :4])
            if a["has_ssim"].any():
                worst = max(worst, float(np.abs(a["dssim"][a["has_ssim"]].astype(np.float64) - b["dssim"][b["has_ssim"]]).max()))
    assert 0.5 * po.DSSIM_O32_O64_MAX < worst <= po.DSSIM_O32_O64_MAX and po.DSSIM_TOL == 4 * po.DSSIM_O32_O64_MAX
