"""keep_logits, confidence.from_model and the demo / evaluate flags on the GPU: the 64x96 hash-initialised
model of tests/test_gpu_demo.py (max_disp 32, so D = 8 and a 16x24 volume, 4 iterations)."""
import json
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, MAX_DISP, ITERS = 64, 96, 32, 4
K = np.array([[80.0, 0, 47.5], [0, 80.0, 31.5], [0, 0, 1]], dtype=np.float32)
BASELINE = 0.1
CLOUD = dict(z_far=20.0, denoise_radius=0.4, denoise_nb_points=10)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _frames(h=H, w=W):
    rng = np.random.default_rng(51)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def model():
    dev = _gpu()
    from foundationstereo_amd import synth
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    args = synth.make_args(max_disp=MAX_DISP, corr_levels=2, vit_size="vits")
    m = FoundationStereo(args).eval()
    synth.init_module_(m, seed=1234)
    return m.to(dev)


@pytest.fixture(scope="module")
def images():
    dev = _gpu()
    left, right = _frames()
    return tuple(torch.from_numpy(a).to(dev).float().permute(2, 0, 1)[None].contiguous() for a in (left, right))


@pytest.fixture(scope="module")
def runs(model, images):
    """Every forward of this file, once: flag off and on, test_mode on and off, run_hierachical."""
    left, right = images
    out = {}
    with torch.no_grad():
        assert model.keep_logits is False and model.last_logits is None
        out["off_test"] = model(left, right, iters=ITERS, test_mode=True)
        out["off_train"] = model(left, right, iters=ITERS, test_mode=False)
        out["off_hiera"] = model.run_hierachical(left, right, iters=ITERS, test_mode=True)
        out["none_after_off"] = model.last_logits is None
        model.keep_logits = True
        try:
            out["on_test"] = model(left, right, iters=ITERS, test_mode=True)
            out["logits_test"] = model.last_logits
            out["on_train"] = model(left, right, iters=ITERS, test_mode=False)
            out["logits_train"] = model.last_logits
            out["on_hiera"] = model.run_hierachical(left, right, iters=ITERS, test_mode=True)
            out["logits_hiera"] = model.last_logits
        finally:
            model.keep_logits = False
    return out


def test_flag_off_keeps_nothing(runs):
    assert runs["none_after_off"]


def test_disparity_is_unchanged_by_the_flag(runs):
    assert torch.equal(runs["on_test"], runs["off_test"])
    assert torch.equal(runs["on_train"][0], runs["off_train"][0])
    assert len(runs["on_train"][1]) == len(runs["off_train"][1]) == ITERS
    for a, b in zip(runs["on_train"][1], runs["off_train"][1]):
        assert torch.equal(a, b)
    assert torch.equal(runs["on_hiera"], runs["off_hiera"]) and torch.isfinite(runs["on_hiera"]).all()


def test_kept_logits_are_the_classifier_output(runs):
    from foundationstereo_amd import ops
    for key in ("logits_test", "logits_train", "logits_hiera"):                # hiera: the full pass's shape, not the half-size one's
        lg = runs[key]
        assert lg.shape == (1, MAX_DISP // 4, H // 4, W // 4) and lg.dtype == torch.float32 and lg.is_contiguous()
        assert torch.isfinite(lg).all()
    assert torch.equal(ops.softmax_regression(runs["logits_train"]), runs["on_train"][0])
    assert torch.equal(runs["logits_test"], runs["logits_train"])           # the same volume, whatever the mode


def test_from_model_is_from_logits_on_the_kept_tensor(model, runs):
    from foundationstereo_amd import confidence
    model.last_logits = runs["logits_test"]
    disp = runs["on_test"]
    a = confidence.from_model(model, disp)
    b = confidence.from_logits(runs["logits_test"], disp, up=4)
    for n in confidence.CHANNELS:
        x, y = getattr(a, n), getattr(b, n)
        assert x.shape == (1, H, W) and torch.equal(x, y)
    assert torch.isfinite(a.mass).all() and float(a.mass.min()) >= 0 and float(a.mass.max()) <= 1
    # the initial disparity judged against its own volume is self mode
    init4 = torch.nn.functional.interpolate(runs["on_train"][0], scale_factor=4, mode="nearest") * 4.0
    c = confidence.from_logits(runs["logits_train"], init4, up=4, want=("spread",))
    s = confidence.from_logits(runs["logits_train"], None, up=4, want=("spread",))
    np.testing.assert_allclose(c.spread.cpu().numpy(), s.spread.cpu().numpy(), atol=2e-5)


def test_run_pair_confidence_and_min_confidence(model):
    from foundationstereo_amd import cloud, confidence, demo
    left, right = _frames(50, 90)                                            # padded to 64x96 with pads 3/3 and 7/7
    plain = demo.run_pair(model, left, right, K, BASELINE, valid_iters=ITERS, **CLOUD)
    assert "confidence" not in plain and model.keep_logits is False
    seen = demo.run_pair(model, left, right, K, BASELINE, valid_iters=ITERS, confidence=1, **CLOUD)
    conf = seen["confidence"]
    assert isinstance(conf, confidence.Confidence) and seen["keep"] is None and model.keep_logits is False
    for n in confidence.CHANNELS:
        assert getattr(conf, n).shape == (1, 50, 90)
    assert torch.equal(seen["disp"], plain["disp"]) and torch.equal(seen["vis"], plain["vis"])
    assert torch.equal(seen["cloud"][0], plain["cloud"][0])
    T = float(conf.mass.median())                                           # drops about half the pixels
    cut = demo.run_pair(model, left, right, K, BASELINE, valid_iters=ITERS, confidence=1, min_confidence=T, **CLOUD)
    sure = cut["confidence"].mass >= T
    assert torch.equal(cut["keep"], sure) and 0 < int(sure.sum()) < 50 * 90
    assert torch.equal(cut["disp"], plain["disp"])
    img = torch.from_numpy(left).to(sure.device)
    c = cloud.disparity_to_cloud(plain["disp"], K, BASELINE, image=img, nb_points=CLOUD["denoise_nb_points"],
                                 radius=CLOUD["denoise_radius"], z_far=CLOUD["z_far"], keep=sure)[0]
    assert torch.equal(cut["cloud"][0], c.xyz_map[c.valid]) and torch.equal(cut["cloud_denoise"][0], c.points)
    assert len(cut["cloud"][0]) < len(plain["cloud"][0])
    both = demo.run_pair(model, left, right, K, BASELINE, valid_iters=ITERS, occlusion_check=1, min_confidence=T, **CLOUD)
    assert torch.equal(both["keep"], both["visibility"].visible & sure)
    hiera = demo.run_pair(model, left, right, K, BASELINE, valid_iters=ITERS, hiera=1, confidence=1, get_pc=0)
    assert hiera["confidence"].mass.shape == (1, 50, 90) and torch.isfinite(hiera["confidence"].mass).all()


def _files(tmp_path):
    left, right = _frames(50, 90)
    np.save(tmp_path / "L.npy", left)
    np.save(tmp_path / "R.npy", right)
    (tmp_path / "K.txt").write_text(" ".join(str(float(v)) for v in K.reshape(-1)) + f"\n{BASELINE}\n")
    return ["--synthetic", "--max_disp", str(MAX_DISP), "--left_file", str(tmp_path / "L.npy"), "--right_file",
            str(tmp_path / "R.npy"), "--valid_iters", str(ITERS)]


def test_demo_main_writes_confidence_png_and_json(tmp_path, capsys):
    _gpu()
    from foundationstereo_amd import demo
    common = _files(tmp_path) + ["--intrinsic_file", str(tmp_path / "K.txt"), "--z_far", str(CLOUD["z_far"]),
                                 "--denoise_radius", str(CLOUD["denoise_radius"]), "--denoise_nb_points",
                                 str(CLOUD["denoise_nb_points"])]
    out = tmp_path / "out"
    res = demo.main(common + ["--out_dir", str(out), "--confidence", "1"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and sorted(res["confidence"]) == ["entropy_mean", "mass_mean", "spread_mean_px"]
    assert all(np.isfinite(v) for v in res["confidence"].values())
    assert 0 <= res["confidence"]["mass_mean"] <= 1 and 0 <= res["confidence"]["entropy_mean"] <= 1
    raw = open(out / "confidence.png", "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (90, 50)
    cut = demo.main(common + ["--out_dir", str(tmp_path / "cut"), "--min_confidence", "0.5"])
    assert "confidence" not in cut and not os.path.exists(tmp_path / "cut" / "confidence.png")
    assert cut["cloud_points"] <= res["cloud_points"]
    with pytest.raises(SystemExit, match="min_confidence"):
        demo.main(common + ["--out_dir", str(out), "--min_confidence", "1.5"])


def test_evaluate_confidence_prints_finite_auses(tmp_path, capsys, model):
    _gpu()
    from foundationstereo_amd import demo, evaluate
    args = _files(tmp_path)
    left, right = _frames(50, 90)
    disp = demo.run_pair(model, left, right, None, None, valid_iters=ITERS, get_pc=0)["disp"].cpu().numpy()
    rng = np.random.default_rng(9)
    gt = np.abs(disp + rng.normal(0, 1.0, disp.shape)).astype(np.float32) + 0.5
    np.save(tmp_path / "gt.npy", gt)
    res = evaluate.main(args + ["--gt_file", str(tmp_path / "gt.npy"), "--confidence"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    c = res["confidence"]
    assert sorted(c) == ["ause_entropy", "ause_mass", "ause_peak", "entropy_mean", "mass_mean", "n_dropped", "oracle_area",
                         "spread_mean_px"]
    assert all(np.isfinite(c[k]) for k in c) and c["oracle_area"] > 0 and c["n_dropped"] == 0
    assert res["n_valid"] == 50 * 90 and np.isfinite(res["epe"])
    nogt = evaluate.main(args + ["--confidence", "1"])
    assert sorted(nogt["confidence"]) == ["entropy_mean", "mass_mean", "spread_mean_px"]
    with pytest.raises(SystemExit, match="pred_file"):
        evaluate.main(args + ["--gt_file", str(tmp_path / "gt.npy"), "--pred_file", str(tmp_path / "gt.npy"), "--confidence"])


def test_last_logits_are_cleared_by_a_forward_with_the_flag_off(model, images, runs):
    left, right = images
    model.last_logits = runs["logits_test"]                                 # what an earlier flag-on forward left
    with torch.no_grad():
        out = model(left, right, iters=ITERS, test_mode=True)
    assert model.keep_logits is False and model.last_logits is None         # from_model now refuses instead of judging stale logits
    assert torch.equal(out, runs["off_test"])


CAPTURE_CHILD = r'''
import faulthandler, json, os, sys
faulthandler.enable()
sys.path.insert(0, os.environ["REPO"])
import torch
from foundationstereo_amd import _lib, confidence, synth
from foundationstereo_amd.foundation_stereo import FoundationStereo
_lib.load()
H, W, md, iters = 64, 96, 32, 4
model = FoundationStereo(synth.make_args(max_disp=md, corr_levels=2, vit_size="vits")).eval()
synth.init_module_(model, seed=1234)
fl, fr, vf = synth.backbone_features(1, H, W, "vits", shift_px=2)
left, right = synth.stereo_images(1, H, W)
dev = torch.device("cuda:0")
model = model.to(dev)
model.feature.set_features([torch.from_numpy(a).to(dev) for a in fl], [torch.from_numpy(a).to(dev) for a in fr],
                           torch.from_numpy(vf).to(dev))
L, R = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
model.keep_logits = True
with torch.no_grad():
    eager = model(L, R, iters=iters, test_mode=True).clone()
    eager_logits = model.last_logits.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = model(L, R, iters=iters, test_mode=True)
    kept = model.last_logits                       # graph-static memory
g.replay()
torch.cuda.synchronize()
first = bool(torch.equal(kept, eager_logits)) and bool(torch.equal(out, eager))
ptr = kept.data_ptr()
kept.zero_()                                       # the next replay writes the same memory again
g.replay()
torch.cuda.synchronize()
second = bool(torch.equal(kept, eager_logits)) and model.last_logits.data_ptr() == ptr
conf = confidence.from_model(model, out)
print(json.dumps({"first": first, "second": second, "shape": list(kept.shape),
                  "finite": bool(torch.isfinite(conf.mass).all()), "contiguous": kept.is_contiguous()}))
'''


def test_captured_forward_keeps_graph_static_logits():
    """Under capture last_logits is memory of the graph's pool: each replay rewrites it with the bits of
    the eager forward, and the poison node that follows it leaves a clean forward's logits alone."""
    _gpu()
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CAPTURE_CHILD], env=dict(os.environ, REPO=repo), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stderr[-3000:]}"
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == {"first": True, "second": True, "shape": [1, MAX_DISP // 4, H // 4, W // 4], "finite": True,
                   "contiguous": True}, res
