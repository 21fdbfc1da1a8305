"""CPU-only checks of the visibility stage: the exported entry point and its refusals (made before any
HIP call), the front ends' refusals, and the numpy oracle itself on the closed-form scene."""
import ctypes

import numpy as np
import pytest
import torch

from tests import visibility_oracle as vo


def _lib():
    from foundationstereo_amd import _lib
    return _lib, _lib.load()


def test_entry_point_is_exported_and_declared():
    _l, lib = _lib()
    assert "fsmi_disp_visibility" in _l.SIGNATURES and len(_l.SIGNATURES["fsmi_disp_visibility"]) == 12
    assert hasattr(lib, "fsmi_disp_visibility")
    from foundationstereo_amd import torch_ops, visibility
    assert "disp_visibility" in torch_ops.OPS
    assert (visibility.VISIBLE, visibility.INVALID, visibility.OUT_OF_VIEW, visibility.OCCLUDED,
            visibility.MISMATCH) == (0, 1, 2, 3, 4) == (vo.VISIBLE, vo.INVALID, vo.OUT_OF_VIEW, vo.OCCLUDED, vo.MISMATCH)


def _call(lib, B, H, W, disp=1, right=None, classes=1, err=None, counts=1):
    # pointer values are never dereferenced: every refusal below happens before a HIP call
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf) & ~15
    return lib.fsmi_disp_visibility(p if disp else None, p if right else None, p if classes else None,
                                    p if err else None, p if counts else None, B, H, W, 1.0, 1.0, 1, None)


def test_width_beyond_the_lds_cap_is_refused():
    _, lib = _lib()
    assert _call(lib, 1, 1, 8193) == 1001
    msg = lib.fsmi_last_error()
    assert b"W = 8193" in msg and b"8192" in msg


@pytest.mark.parametrize("shape", [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -2, 4), (4, 4, -3)])
def test_empty_and_negative_shapes_are_refused(shape):
    _, lib = _lib()
    assert _call(lib, *shape) == 1001 and b"shape" in lib.fsmi_last_error()


def test_null_pointers_and_error_map_without_right_view_are_refused():
    _, lib = _lib()
    assert _call(lib, 1, 2, 8, disp=0) == 1001 and b"null" in lib.fsmi_last_error()
    assert _call(lib, 1, 2, 8, counts=0) == 1001 and b"null" in lib.fsmi_last_error()
    assert _call(lib, 1, 2, 8, err=1) == 1001 and b"disp_right" in lib.fsmi_last_error()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf) & ~15
    assert lib.fsmi_disp_visibility(p, None, p, None, p, 1, 2, 8, float("nan"), 1.0, 1, None) == 1001
    assert lib.fsmi_disp_visibility(p + 4, None, p, None, p, 1, 2, 8, 1.0, 1.0, 1, None) == 1001
    assert b"aligned" in lib.fsmi_last_error()


def test_front_ends_refuse_cpu_tensors_and_bad_arguments():
    from foundationstereo_amd import ops, visibility
    d = torch.ones(1, 2, 8)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_visibility(d)
    with pytest.raises(RuntimeError, match="ROCm"):
        visibility.classify(d[0])
    with pytest.raises(ValueError, match="want_error"):
        visibility.classify(d, want_error=True)
    with pytest.raises(ValueError, match=r"\(H,W\)"):
        visibility.classify(torch.ones(8))

def test_invalidate_fills_every_other_class():
    from foundationstereo_amd import visibility
    d = torch.arange(10, dtype=torch.float32).reshape(1, 2, 5)
    cls = torch.tensor([[[0, 1, 2, 3, 4], [0, 0, 4, 0, 1]]], dtype=torch.uint8)
    want = d.clone()
    want[cls != 0] = float("inf")
    assert torch.equal(visibility.invalidate(d, cls), want) and d[0, 0, 1] == 1.0       # a copy
    assert torch.equal(visibility.invalidate(d[0], cls), want[0])
    assert torch.equal(visibility.invalidate(d[:, None], cls, fill=-1.0), want[:, None].nan_to_num(posinf=-1.0))


def test_demo_and_evaluate_flags_default_off():
    from foundationstereo_amd import demo, evaluate
    a = demo.parser().parse_args([])
    assert (a.occlusion_check, a.lr_check, a.occlusion_tol, a.lr_thresh) == (0, 0, 1.0, 1.0)
    assert evaluate.parser().parse_args(["--gt_file", "x"]).noc is False
    with pytest.raises(SystemExit, match="panorama"):
        demo.main(["--occlusion_check", "1", "--camera_type", "panorama"])
    with pytest.raises(SystemExit, match="panorama"):
        demo.main(["--lr_check", "1", "--camera_type", "panorama"])
    with pytest.raises(SystemExit, match="two different masks"):
        evaluate.main(["--gt_file", "x", "--noc", "--all_pixels"])


@pytest.mark.parametrize("H", [1, 2])
def test_oracle_gives_the_closed_form_classes(H):
    left, right, occ, lr = vo.analytic_scene(H)
    cls, counts, err = vo.classify_oracle(left)
    assert np.array_equal(cls, occ) and err is None
    assert counts.tolist() == [[44 * H, 0, 4 * H, 16 * H, 0]]
    cls, counts, err = vo.classify_oracle(left, right, occlusion=False)
    assert np.array_equal(cls, lr) and counts.tolist() == [[44 * H, 0, 4 * H, 0, 16 * H]]
    assert np.isnan(err[..., :4]).all() and (err[..., 14:30] == 16).all()
    assert not err[..., 4:14].any() and not err[..., 30:].any()
    # both detectors on: occlusion takes precedence, the sets are the same
    cls, counts, _ = vo.classify_oracle(left, right)
    assert np.array_equal(cls, occ)


def test_oracle_ties_interpolation_and_threads():
    # d = u: every pixel of the row lands on column 0 (u = 0 has d = 0: INVALID); the largest d hides
    # whoever is more than the tolerance below it
    d = np.arange(8, dtype=np.float32)[None, None]
    assert vo.classify_oracle(d)[0].tolist() == [[[1, 3, 3, 3, 3, 3, 0, 0]]]              # 7 - d > 1
    assert vo.classify_oracle(d, occlusion_tol=6.0)[0].tolist() == [[[1, 0, 0, 0, 0, 0, 0, 0]]]
    d = np.array([[[0.25, 0.75, 1.75, 2.75]]], np.float32)          # xr = -0.25, then 0.25 three times
    assert vo.classify_oracle(d)[0].tolist() == [[[2, 3, 0, 0]]]    # 2.75 - d > 1 for d = 0.75 only
    # t != 0: r = dR[0] + 0.25 * (dR[1] - dR[0]);  t == 0 skips the product, so an inf neighbour is harmless
    right = np.array([[[1.0, 3.0, np.inf, 0.0]]], np.float32)
    left = np.array([[[np.nan, 0.75, 1.0, 2.0]]], np.float32)       # xr = -, 0.25, 1, 1
    cls, _, err = vo.classify_oracle(left, right, occlusion=False, lr_thresh=0.8)
    assert np.isnan(err[0, 0, 0]) and err[0, 0, 1:].tolist() == [0.75, 2.0, 1.0]
    assert cls.tolist() == [[[1, 0, 4, 4]]]
    left, right = vo.fuzz_maps((3, 37, 61), seed=5, with_right=True)
    one = vo.classify_oracle(left, right, workers=1)
    many = vo.classify_oracle(left, right, workers=16)
    for a, b in zip(one, many):
        assert np.array_equal(a, b, equal_nan=True)
    assert (one[1] > 0).all()                                       # the fuzz reaches every class
