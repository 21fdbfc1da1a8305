"""``update.OVERLAP`` on vs off: the same kernels on the same inputs, forked onto side streams or in order on
the calling stream (every call site writes its sequence once and picks the stream, streams.fork / join), so
the whole forward is bit-identical in the two configurations.  ``update.CTX_PRE`` is off for the comparison:
the in-order loop (``BasicSelectiveMultiUpdateBlock.forward``) convolves conv0 whole while the overlapped one
splits off ``context_pre``, a different fp32 summation order, not a different schedule.

The smallest model the schedule code still walks fully: 64x96 images, max_disp 32, two correlation levels,
three GRU levels (the pipelined loop in test mode, the per-iteration loop otherwise).
"""
import pytest
import torch

from foundationstereo_amd import synth
from tests.helpers import t

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from foundationstereo_amd import _lib
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    _lib.load()
    H, W = 64, 96
    args = synth.make_args(max_disp=32, corr_levels=2, vit_size="vits")
    assert args.n_gru_layers == 3
    m = FoundationStereo(args).eval()
    synth.init_module_(m, seed=1234)
    m = m.to(DEV)
    fl, fr, vf = synth.backbone_features(1, H, W, args.vit_size, shift_px=2)
    m.feature.set_features([t(a).to(DEV) for a in fl], [t(a).to(DEV) for a in fr], t(vf).to(DEV))
    left, right = synth.stereo_images(1, H, W)
    return m, t(left).to(DEV), t(right).to(DEV)


def _both(model, monkeypatch, **kw):
    from foundationstereo_amd import update
    m, left, right = model
    monkeypatch.setattr(update, "CTX_PRE", False)
    outs = {}
    for on in (True, False):
        monkeypatch.setattr(update, "OVERLAP", on)
        with torch.no_grad():
            outs[on] = m(left, right, **kw)
        torch.cuda.synchronize()
    return outs[True], outs[False]


def test_test_mode_disparity_equal(model, monkeypatch):
    """(a) the pipelined loop against the in-order per-iteration loop."""
    fork, inorder = _both(model, monkeypatch, iters=3, test_mode=True)
    assert torch.isfinite(fork).all()
    assert torch.equal(fork, inorder), f"max |d| {float((fork - inorder).abs().max())}"


def test_sequence_equal(model, monkeypatch):
    """(b) ``init_disp`` and every prediction of the per-iteration loop."""
    (init_f, preds_f), (init_i, preds_i) = _both(model, monkeypatch, iters=2, test_mode=False)
    assert torch.equal(init_f, init_i), f"init_disp: max |d| {float((init_f - init_i).abs().max())}"
    assert len(preds_f) == len(preds_i) == 2
    for k, (a, b) in enumerate(zip(preds_f, preds_i)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"prediction {k}: max |d| {float((a - b).abs().max())}"
