"""The scoring CLI on the GPU (foundationstereo_amd/evaluate.py) with the shapes of tests/test_gpu_demo.py:
50x90 frames, max_disp 32, 4 iterations, the hash-initialised model.  The ground truth is the model's own
unpadded disparity plus a known perturbation, with some pixels zeroed; the CLI's JSON must equal
tests/metrics_oracle.py on those arrays within the bounds of tests/test_gpu_metrics.py."""
import json
import struct

import numpy as np
import pytest
import torch

from tests import metrics_oracle as mo

pytestmark = pytest.mark.gpu

H, W, MAX_DISP, ITERS = 50, 90, 32, 4
THR = (0.5, 1.0, 3.0)
EPS = 2.0 ** -52


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Frames, the model's disparity, the ground truth derived from it, all as files; computed once."""
    dev = _gpu()
    from foundationstereo_amd import demo, synth
    from foundationstereo_amd.foundation_stereo import FoundationStereo
    d = tmp_path_factory.mktemp("evaluate")
    rng = np.random.default_rng(50)
    left, right = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    model = FoundationStereo(synth.make_args(max_disp=MAX_DISP, corr_levels=2, vit_size="vits")).eval()
    synth.init_module_(model, seed=1234)
    K = np.array([[80.0, 0, 44.5], [0, 80.0, 24.5], [0, 0, 1]], dtype=np.float32)
    disp = demo.run_pair(model.to(dev), left, right, K, 0.1, valid_iters=ITERS, get_pc=0)["disp"].cpu().numpy()
    assert disp.shape == (H, W) and np.isfinite(disp).all()
    # a known perturbation: +-0.25 px on most pixels, 2 px on every 7th, 6 px on every 11th; 1 in 13 unscored
    idx = np.arange(H * W).reshape(H, W)
    delta = np.where(idx % 2 == 0, 0.25, -0.25).astype(np.float32)
    delta[idx % 7 == 0] = 2.0
    delta[idx % 11 == 0] = -6.0
    gt = (disp + delta).astype(np.float32)                                  # <= 0 somewhere: unscored there as well
    gt[idx % 13 == 0] = 0.0
    np.save(d / "L.npy", left)
    np.save(d / "R.npy", right)
    np.save(d / "gt.npy", gt)
    np.save(d / "pred.npy", disp)
    return {"dir": d, "disp": disp, "gt": gt}


def _against_oracle(res, pred, gt, mask, thr):
    wt, ws, _ = mo.metrics(pred[None], gt[None], None if mask is None else mask[None], thr)
    t, N, P = wt[0], ws[0, 0], pred.size
    assert res["image_size"] == [H, W] and res["n_valid"] == N and res["n_nonfinite"] == 0
    assert res["thresholds"] == list(thr) and res["bad"] == t[9:9 + len(thr)].tolist() and res["d1_all"] == t[3]
    assert abs(res["epe"] - t[1]) <= (N + 4) * EPS * t[1] and abs(res["rmse"] - t[2]) <= (N + 4) * EPS * t[2]
    assert res["pred_min"] == t[7] and res["pred_max"] == t[8]
    assert abs(res["pred_mean"] - t[5]) <= (P + 4) * EPS * mo.abs_dev(pred) / P
    bvar = (P + 4) * EPS * ws[0, 6] / (P - 1)
    assert abs(res["pred_std"] - t[6]) <= bvar / t[6] + EPS * t[6]
    return t, N


def test_model_mode_and_pred_file_mode(case, capsys):
    _gpu()
    from foundationstereo_amd import evaluate
    d = case["dir"]
    model_flags = ["--synthetic", "--max_disp", str(MAX_DISP), "--valid_iters", str(ITERS), "--left_file", str(d / "L.npy"),
                   "--right_file", str(d / "R.npy")]
    score_flags = ["--gt_file", str(d / "gt.npy"), "--thresholds", *[str(t) for t in THR]]
    res = evaluate.main(model_flags + score_flags)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and res["mode"] == "model"
    t, N = _against_oracle(res, case["disp"], case["gt"], None, THR)
    assert N == np.count_nonzero(case["gt"] > 0) and 0 < N < H * W
    assert 0.2 < t[1] < 6.0 and t[9] >= t[10] >= t[11] and t[2] > t[1]         # the perturbation shows in the figures

    stored = evaluate.main(["--pred_file", str(d / "pred.npy")] + score_flags)
    assert stored["mode"] == "pred_file"
    assert {k: v for k, v in stored.items() if k != "mode"} == {k: v for k, v in res.items() if k != "mode"}
    capsys.readouterr()


def test_all_pixels_and_error_png(case, capsys):
    _gpu()
    from foundationstereo_amd import evaluate
    d = case["dir"]
    png = d / "error.png"
    res = evaluate.main(["--pred_file", str(d / "pred.npy"), "--gt_file", str(d / "gt.npy"), "--all_pixels",
                         "--thresholds", "1", "3", "--error_png", str(png), "--error_max", "3"])
    capsys.readouterr()
    _against_oracle(res, case["disp"], case["gt"], np.ones((H, W), bool), (1.0, 3.0))
    assert res["n_valid"] == H * W and res["error_png"] == str(png)
    raw = open(png, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and struct.unpack(">II", raw[16:24]) == (W, H)


def test_u8_ground_truth_file(case, capsys):
    _gpu()
    from foundationstereo_amd import evaluate
    d = case["dir"]
    n = np.round(np.maximum(case["gt"], 0).astype(np.float64) * 100).astype(np.int64)   # scale 100: 0.01 px steps
    u8 = np.stack([n // 65025, (n % 65025) // 255, n % 255], axis=-1).astype(np.uint8)
    np.save(d / "gt_u8.npy", u8)
    res = evaluate.main(["--pred_file", str(d / "pred.npy"), "--gt_file", str(d / "gt_u8.npy"), "--gt_scale", "100",
                         "--thresholds", *[str(t) for t in THR]])
    capsys.readouterr()
    _against_oracle(res, case["disp"], mo.decode(u8, 100.0), None, THR)


def test_scale_is_refused(case):
    from foundationstereo_amd import evaluate
    d = case["dir"]
    with pytest.raises(SystemExit, match="resizing a ground truth"):
        evaluate.main(["--pred_file", str(d / "pred.npy"), "--gt_file", str(d / "gt.npy"), "--scale", "0.5"])
