"""A mask, or an encoded ground truth, that starts at an odd byte gives the bits its aligned copy gives.

The three scoring ops normalise a mask through one helper (ops._mask_arg, mask_arg in torch_ops.cpp):
fsmi_disp_metrics reads it a word at a time and gets a 4-byte aligned copy, fsmi_seq_metrics reads bytes
and fsmi_photo_consistency tests each quad's address, so both take the odd view as it is.  Either way
the table and the sums must not depend on where the bytes lie.  Exact equality: no tolerance.
  (2,3,5)    the scoring ops: H*W = 15 is odd, so pair 1 starts off a 16-byte boundary (head, quad, tail)
  (2,13,65)  the photometric op, C = 3 uint8 frames: a full 64 x 12 tile, a one-column and a one-row
             remainder, four tiles in all
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _odd(t):
    """The bytes of uint8 / bool ``t`` as a view that starts one byte into a fresh buffer."""
    n = t.numel()
    buf = torch.zeros(n + 1, dtype=torch.uint8, device=t.device)
    view = buf[1:1 + n].view(t.shape)
    view.copy_(t.view(torch.uint8))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _call(path, name):
    from foundationstereo_amd import ops, torch_ops
    if path == "ctypes":
        return getattr(ops, name)
    torch_ops.load()
    return getattr(torch.ops.fsmi, name)


@pytest.mark.parametrize("path", ["ctypes", "torch_ops"])
def test_scoring_ops_ignore_where_the_mask_and_the_ground_truth_start(path):
    dev = _gpu()
    g = torch.Generator().manual_seed(71)
    shape = (2, 3, 5)
    gt = (torch.rand(shape, generator=g) * 40.0 + 0.5).to(dev)
    preds = [(gt.cpu() + torch.randn(shape, generator=g) * 3.0).to(dev) for _ in range(2)]
    mask = (torch.rand(shape, generator=g) < 0.7).to(torch.uint8).to(dev)
    gt_u8 = torch.randint(0, 256, shape + (3,), generator=g, dtype=torch.uint8)
    gt_u8[..., 0] = 0                                                    # (g * 255 + b) / 1000: up to 65 px
    gt_u8 = gt_u8.to(dev)
    disp_metrics, seq_metrics = _call(path, "disp_metrics"), _call(path, "seq_metrics")
    for m_view, m_copy in ((_odd(mask), mask.clone()), (_odd(mask).view(torch.bool), mask.bool())):
        a, b = disp_metrics(preds[0], gt, m_view), disp_metrics(preds[0], gt, m_copy)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
        a, b = seq_metrics(preds, gt, m_view), seq_metrics(preds, gt, m_copy)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and _same_bits(a[2], b[2])
        assert float(a[0][:, :, 0].min()) > 0                               # pixels were scored
    u_view, u_copy = _odd(gt_u8), gt_u8.clone()
    assert u_copy.data_ptr() % 4 == 0
    for m in (None, _odd(mask)):
        a, b = disp_metrics(preds[0], u_view, m), disp_metrics(preds[0], u_copy, m)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
        a, b = seq_metrics(preds, u_view, m), seq_metrics(preds, u_copy, m)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and _same_bits(a[2], b[2])
        assert float(a[0][:, :, 0].min()) > 0


@pytest.mark.parametrize("path", ["ctypes", "torch_ops"])
def test_photo_consistency_ignores_where_the_mask_starts(path):
    dev = _gpu()
    g = torch.Generator().manual_seed(72)
    B, H, W = 2, 13, 65
    disp = (torch.rand((B, H, W), generator=g) * 6.0 + 0.25).to(dev)
    left = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    right = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    mask = (torch.rand((B, H, W), generator=g) < 0.7).to(torch.uint8).to(dev)
    photo = _call(path, "photo_consistency")
    for m_view, m_copy in ((_odd(mask), mask.clone()), (_odd(mask).view(torch.bool), mask.bool())):
        a, b = photo(disp, left, right, m_view, [-1.0, 0.0, 1.0]), photo(disp, left, right, m_copy, [-1.0, 0.0, 1.0])
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
        assert float(a[0][:, 0].min()) > 0 and float(a[0][:, 1].min()) > 0      # scored pixels, SSIM pixels
        unmasked = photo(disp, left, right, None, [-1.0, 0.0, 1.0])
        assert float((unmasked[0][:, 0] - a[0][:, 0]).min()) > 0                 # the mask was read
