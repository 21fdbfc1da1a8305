"""The frame / picture stage on the GPU (csrc/frames.hip) against tests/frames_oracle.py.

Every comparison is exact.  scale == 1 and the padding involve no arithmetic.  At scale 0.5 the tap
weights are exactly 1/2, every blend an exact quarter sum and a quarter of the pixels exact ties, so
equality pins the half-up rounding.  At scale 0.6 the weights are multiples of 1/3, every blend a
multiple of 1/9 and so at least 1/18 from a rounding boundary: four orders above the fp32 error of the
blend (about 255 * 2^-21), hence equality with the fp64 oracle, no pixel skipped.  The picture is
fp32 arithmetic with IEEE division on both sides.
"""
import os

import numpy as np
import pytest
import torch

from tests import frames_oracle

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _frames(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


def _ingest_equals_oracle(left, right, scale=1.0):
    dev = _gpu()
    from foundationstereo_amd import frames
    fr = frames.ingest(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev), scale=scale)
    l4 = left.reshape((-1,) + left.shape[-3:]) if left.ndim >= 3 else left[None, :, :, None]
    r4 = right.reshape((-1,) + right.shape[-3:]) if right.ndim >= 3 else right[None, :, :, None]
    batch, u8 = frames_oracle.ingest_oracle(l4, r4, scale)
    assert fr.batch.dtype == torch.float32 and fr.batch.shape == batch.shape
    assert fr.image_u8.dtype == torch.uint8 and fr.image_u8.shape == u8.shape
    assert np.array_equal(fr.batch.cpu().numpy(), batch)
    assert np.array_equal(fr.image_u8.cpu().numpy(), u8)
    assert fr.left.data_ptr() == fr.batch[:, 0].data_ptr() and fr.right.data_ptr() == fr.batch[:, 1].data_ptr()
    assert fr.padder._pad == list(frames_oracle.sintel_pads(u8.shape[1], u8.shape[2]))
    assert fr.scale == scale
    return fr, batch, u8


# ------------------------------------------------------------------ ingest

def test_ingest_odd_pads_ragged_rows():
    dev = _gpu()
    from foundationstereo_amd.utils import InputPadder
    left, right = _frames((2, 37, 53, 3), 1)
    fr, batch, _ = _ingest_equals_oracle(left, right)
    assert fr.batch.shape == (2, 2, 3, 64, 64) and fr.padder._pad == [5, 6, 13, 14]
    assert np.array_equal(fr.image_u8.cpu().numpy(), left)
    for k, img in enumerate((left, right)):                    # scripts/run_demo.py:156-159 with torch on the device
        x = torch.as_tensor(img).to(dev).float().permute(0, 3, 1, 2)
        want = InputPadder(x.shape, divis_by=32).pad(x)[0]
        assert torch.equal(fr.batch[:, k], want)
    assert torch.equal(fr.padder.unpad(fr.left), torch.as_tensor(left).to(dev).float().permute(0, 3, 1, 2))


@pytest.mark.parametrize("C", [1, 4])
def test_ingest_gray_and_rgba(C):
    left, right = _frames((1, 33, 40, C), 2 + C)
    fr, batch, u8 = _ingest_equals_oracle(left, right)
    assert fr.batch.shape == (1, 2, 3, 64, 64)
    got = fr.image_u8.cpu().numpy()
    if C == 1:
        assert np.array_equal(got, np.repeat(left, 3, axis=3))
    else:
        assert np.array_equal(got, left[..., :3])


def test_ingest_2d_gray_and_hwc():
    left, right = _frames((33, 40), 7)
    fr, _, _ = _ingest_equals_oracle(left, right)
    assert fr.batch.shape == (1, 2, 3, 64, 64)
    left, right = _frames((33, 40, 3), 8)
    _ingest_equals_oracle(left, right)


def test_ingest_numpy_input_is_uploaded():
    _gpu()
    from foundationstereo_amd import frames
    left, right = _frames((33, 40, 3), 9)
    fr = frames.ingest(left, right)
    assert fr.batch.is_cuda and np.array_equal(fr.image_u8[0].cpu().numpy(), left)


def test_ingest_no_padding():
    left, right = _frames((1, 64, 96, 3), 10)
    fr, _, _ = _ingest_equals_oracle(left, right)
    assert fr.padder._pad == [0, 0, 0, 0] and fr.batch.shape == (1, 2, 3, 64, 96)
    assert np.array_equal(fr.batch[:, 0].cpu().numpy(), left.astype(np.float32).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("hw,want", [((43, 86), (22, 43)), ((45, 90), (22, 45))])
def test_ingest_exact_half_scale(hw, want):
    left, right = _frames((2,) + hw + (3,), 11)
    _, raw = frames_oracle.resize_oracle(left[0], 0.5, return_raw=True)
    assert raw.shape[:2] == want and (raw % 1 == 0.5).mean() > 0.15          # exact ties: rounding is pinned
    fr, _, u8 = _ingest_equals_oracle(left, right, 0.5)
    assert u8.shape[1:3] == want


def test_ingest_scale_0p6():
    left, right = _frames((1, 45, 75, 3), 12)
    for img in (left[0], right[0]):
        out, raw = frames_oracle.resize_oracle(img, 0.6, return_raw=True)
        assert out.shape[:2] == (27, 45)
        assert (np.abs(raw - np.floor(raw) - 0.5) >= 0.05).all()             # no value near a rounding boundary
    _ingest_equals_oracle(left, right, 0.6)
    gray = _frames((1, 45, 75, 1), 13)
    _ingest_equals_oracle(*gray, 0.6)


def test_ingest_non_contiguous_input():
    dev = _gpu()
    from foundationstereo_amd import frames
    big_l, big_r = _frames((2, 40, 60, 4), 14)
    tl, tr = torch.from_numpy(big_l).to(dev)[:, 2:39, 3:56, :3], torch.from_numpy(big_r).to(dev)[:, 2:39, 3:56, :3]
    assert not tl.is_contiguous()
    a = frames.ingest(tl, tr)
    b = frames.ingest(tl.contiguous(), tr.contiguous())
    assert torch.equal(a.batch, b.batch) and torch.equal(a.image_u8, b.image_u8)
    assert np.array_equal(a.image_u8.cpu().numpy(), big_l[:, 2:39, 3:56, :3])


# ------------------------------------------------------------------ the picture

@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "frames_small.npz"))


def test_vis_reference_golden(golden):
    dev = _gpu()
    from foundationstereo_amd import frames
    disp = torch.from_numpy(golden["disp"]).to(dev)
    other = {}
    vis = frames.vis_disparity(disp, other_output=other)
    assert vis.dtype == torch.uint8 and vis.shape == (37, 53, 3)
    assert np.array_equal(vis.cpu().numpy(), golden["vis_auto"])
    assert other["minmax"].shape == (1, 2) and np.array_equal(other["minmax"][0].cpu().numpy(), golden["minmax_auto"])
    vis = frames.vis_disparity(disp, min_val=5, max_val=40, other_output=other)
    assert np.array_equal(vis.cpu().numpy(), golden["vis_5_40"])
    assert other["minmax"].tolist() == [[5.0, 40.0]]
    lo = frames.vis_disparity(disp, min_val=5)                                # one of the two explicit
    assert np.array_equal(lo.cpu().numpy(), frames_oracle.vis_oracle(golden["disp"], frames.TURBO, min_val=5))


def _vis_equals_oracle(disp, lut=None, **kw):
    dev = _gpu()
    from foundationstereo_amd import frames
    other = {}
    got = frames.vis_disparity(torch.from_numpy(disp).to(dev), lut=lut, other_output=other, **kw).cpu().numpy()
    table = frames.TURBO if lut is None else lut
    mm = other["minmax"].cpu().numpy()
    for b in range(len(disp)):
        o = {}
        assert np.array_equal(got[b], frames_oracle.vis_oracle(disp[b], table, other_output=o, **kw)), b
        if o["min_val"] is None:
            assert mm[b].tolist() == [np.inf, -np.inf]
        else:
            assert mm[b].tolist() == [o["min_val"], o["max_val"]]
    return got, mm


def test_vis_per_image_range_and_ragged_tail():
    rng = np.random.default_rng(20)
    disp = np.stack([rng.uniform(2, 9, (9, 37)), rng.uniform(-30, 80, (9, 37))]).astype(np.float32)   # 333 px: P % 4 = 1
    got, mm = _vis_equals_oracle(disp)
    assert mm[0, 1] < 9.0 < mm[1, 1] and mm[1, 0] < 0 < mm[0, 0]
    three = np.concatenate([disp, -disp[:1]])                                  # B = 3: image starts at 333 and 666 floats
    _vis_equals_oracle(three)
    _vis_equals_oracle(rng.uniform(0, 50, (1, 3, 2)).astype(np.float32))        # W < 4, a single partial quad
    _vis_equals_oracle(rng.uniform(0, 50, (2, 40, 52)).astype(np.float32))      # more than one block


def test_vis_degenerate_images():
    from foundationstereo_amd import frames
    disp = np.full((3, 6, 10), 7.5, np.float32)
    disp[0] = np.inf                                                           # no valid pixel
    disp[1, 2, 3] = np.nan                                                     # constant where valid
    disp[2, 0, :5] = -0.0                                                      # two values, one of them -0
    disp[2, 0, 5:] = 0.0
    disp[2, 1:] = -3.0
    got, mm = _vis_equals_oracle(disp)
    assert not got[0].any()
    assert (got[1][~np.isnan(disp[1])] == frames.TURBO[0]).all() and not got[1, 2, 3].any()
    assert mm[2].tolist() == [-3.0, 0.0] and (got[2, 0] == frames.TURBO[255]).all()


def test_vis_invalid_pixels_and_threshold():
    rng = np.random.default_rng(21)
    disp = rng.uniform(1, 60, (2, 17, 23)).astype(np.float32)
    disp[0, 3, 4] = np.nan
    disp[0, 5, 6] = np.inf
    disp[1, 0, 0] = np.nan
    disp[1, 16, 22] = 30.0                                                     # >= thres is invalid: the boundary itself
    got, mm = _vis_equals_oracle(disp, invalid_thres=30.0)
    bad = np.isnan(disp) | (disp >= 30)
    assert bad.sum() > 100 and not got[bad].any() and (mm[:, 1] < 30).all()
    assert got[~bad].reshape(-1, 3).any(1).all()                               # no turbo entry is black


def test_vis_side_by_side_and_custom_lut():
    dev = _gpu()
    from foundationstereo_amd import frames
    rng = np.random.default_rng(22)
    for shape in ((2, 9, 37), (1, 12, 40)):                                     # W % 4 != 0 and == 0
        disp = rng.uniform(1, 60, shape).astype(np.float32)
        disp[0, 1, 2] = np.inf
        img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        d, im = torch.from_numpy(disp).to(dev), torch.from_numpy(img).to(dev)
        plain = frames.vis_disparity(d)
        both = frames.vis_disparity(d, image=im)
        W = shape[2]
        assert both.shape == shape[:2] + (2 * W, 3)
        assert torch.equal(both[:, :, :W], im) and torch.equal(both[:, :, W:], plain)
    one = frames.vis_disparity(d[0], image=im[0])                              # (H,W) with (H,W,3)
    assert one.shape == (12, 80, 3) and torch.equal(one, both[0])
    rev = np.ascontiguousarray(frames.TURBO[::-1])
    got, _ = _vis_equals_oracle(disp, lut=rev)
    assert not np.array_equal(got, plain.cpu().numpy())
    lut_t = torch.from_numpy(rev).to(dev)
    assert np.array_equal(frames.vis_disparity(d, lut=lut_t).cpu().numpy(), got)


# ------------------------------------------------------------------ operators, capture, refusals

def test_torch_operators_equal_ctypes(golden):
    dev = _gpu()
    from foundationstereo_amd import frames, ops, torch_ops
    torch_ops.load()
    left, right = (torch.from_numpy(a).to(dev) for a in _frames((2, 45, 75, 3), 30))
    for scale in (1.0, 0.6):
        a = torch.ops.fsmi.frames_ingest(left, right, scale, 32)
        b = ops.frames_ingest(left, right, scale=scale)
        assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))
    disp = torch.from_numpy(np.stack([golden["disp"], 2 * golden["disp"]])).to(dev)
    lut = torch.from_numpy(frames.TURBO.copy()).to(dev)
    img = left[:, :37, :53].contiguous()
    pic, mm = torch.ops.fsmi.vis_disparity(disp, lut)
    assert torch.equal(mm, ops.disp_minmax(disp)) and torch.equal(pic, ops.disp_colorize(disp, mm, lut))
    pic, mm = torch.ops.fsmi.vis_disparity(disp, lut, 5.0, 40.0, 50.0, img)
    assert mm.tolist() == [[5.0, 40.0]] * 2
    assert torch.equal(pic, ops.disp_colorize(disp, mm, lut, 50.0, img))
    pic, mm = torch.ops.fsmi.vis_disparity(disp, lut, None, 40.0)
    assert torch.equal(pic, frames.vis_disparity(disp, max_val=40.0))


def test_graph_capture_of_the_whole_stage():
    """ingest -> minmax -> colorize captured on one stream and replayed on new frames: the min / max
    buffer is re-initialised inside the captured work and nothing synchronises."""
    dev = _gpu()
    from foundationstereo_amd import frames, ops
    a, b = _frames((1, 37, 53, 3), 40)
    left, right = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    lut = torch.from_numpy(frames.TURBO.copy()).to(dev)

    def stage():
        batch, u8 = ops.frames_ingest(left, right)
        disp = batch[:, 1, 2]                                                   # a channel as the disparity
        mm = ops.disp_minmax(disp)
        return ops.disp_colorize(disp, mm, lut), mm
    stage()                                                                     # library load, first launches
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            pic, mm = stage()
    torch.cuda.current_stream().wait_stream(side)
    c, d = _frames((1, 37, 53, 3), 41)
    d[0, :, :, 2] = np.clip(d[0, :, :, 2], 60, 190)                             # a narrower range than before
    left.copy_(torch.from_numpy(c).to(dev))
    right.copy_(torch.from_numpy(d).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    want_pic, want_mm = stage()
    assert want_mm.tolist() == [[60.0, 190.0]]
    assert torch.equal(mm, want_mm) and torch.equal(pic, want_pic)


def test_refusals():
    dev = _gpu()
    from foundationstereo_amd import frames, ops
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.frames_ingest(u8.cpu(), u8.cpu())
    with pytest.raises(RuntimeError, match="uint8"):
        ops.frames_ingest(u8.float(), u8.float())
    with pytest.raises(RuntimeError, match="uint8"):
        frames.ingest(u8.float(), u8.float())
    with pytest.raises(RuntimeError, match="alike"):
        ops.frames_ingest(u8, u8[:, :4])
    with pytest.raises(Exception, match="C = 2"):
        ops.frames_ingest(u8[..., :2], u8[..., :2])
    with pytest.raises(Exception, match="scale"):
        ops.frames_ingest(u8, u8, scale=1.5)
    d = torch.ones((1, 8, 8), device=dev)
    with pytest.raises(RuntimeError, match="ROCm"):
        frames.vis_disparity(d.cpu())
    with pytest.raises(RuntimeError, match="float32"):
        frames.vis_disparity(d.double())
    with pytest.raises(RuntimeError, match="uint8"):
        frames.vis_disparity(d, lut=torch.zeros((256, 3), device=dev))
    with pytest.raises(RuntimeError, match="image"):
        frames.vis_disparity(d, image=u8[:, :4])
