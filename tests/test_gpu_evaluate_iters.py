"""``python -m foundationstereo_amd.evaluate --per_iter`` on the GPU: the demo tests' tiny pair (50x90
frames padded to 64x96, the hash-initialised model) at 3 iterations.  This is the first GPU test that
reaches the per-iteration loop (``forward(test_mode=False)``, UpdateBlock.forward_overlapped) through
the model's own ``forward``; plain ``evaluate`` takes the pipelined test-mode path."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W, MAX_DISP, ITERS = 50, 90, 32, 3
THR = (1.0, 3.0, 5.0)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("evaluate_iters")
    rng = np.random.default_rng(50)
    np.save(d / "L.npy", rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    np.save(d / "R.npy", rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    gt = rng.uniform(0.5, 30.0, (H, W)).astype(np.float32)
    gt[rng.random((H, W)) < 0.1] = 0.0
    np.save(d / "gt.npy", gt)
    return d


def _flags(d):
    return ["--synthetic", "--max_disp", str(MAX_DISP), "--valid_iters", str(ITERS), "--left_file", str(d / "L.npy"),
            "--right_file", str(d / "R.npy"), "--gt_file", str(d / "gt.npy"), "--thresholds", *[str(t) for t in THR]]


def test_per_iter_against_the_plain_call(files, capsys):
    _gpu()
    from foundationstereo_amd import evaluate
    plain = evaluate.main(_flags(files))
    capsys.readouterr()
    res = evaluate.main(_flags(files) + ["--per_iter"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res
    # the old fields: the same keys, the last iteration's values ("same kernels, same inputs": 1e-3 px)
    assert [k for k in res if k != "per_iter"] == list(plain)
    assert res["mode"] == "model" and res["image_size"] == [H, W] and res["thresholds"] == list(THR)
    assert res["n_valid"] == plain["n_valid"] > 0 and res["n_nonfinite"] == 0
    assert abs(res["epe"] - plain["epe"]) <= 1e-3
    p = res["per_iter"]
    assert p["iters"] == ITERS and len(p["epe"]) == len(p["rmse"]) == len(p["d1_all"]) == len(p["bad"]) == ITERS
    assert all(len(b) == len(THR) for b in p["bad"]) and all(np.isfinite(p["epe"]))
    assert p["init"] is not None and p["init"]["n_valid"] == res["n_valid"] and np.isfinite(p["init"]["epe"])
    # 3 + 1 rows; the last row is the plain call's figure (the sequence clamps to [0, 192]: nothing there here)
    assert abs(p["epe"][-1] - plain["epe"]) <= 1e-3
    assert abs(p["epe"][-1] - res["epe"]) <= 1e-9 * res["epe"] and p["bad"][-1] == res["bad"]
    w = [0.9 ** (ITERS - k) for k in range(1, ITERS + 1)]
    assert p["loss"] > sum(wk * e for wk, e in zip(w, p["epe"])) > 0       # plus the initial row's smooth-L1
    assert p["first_iter_within"] in (1, 2, 3)
    assert all(abs(e - p["epe"][-1]) > p["converged_px"] for e in p["epe"][:p["first_iter_within"] - 1])


def test_stored_sequence_and_refusals(files, capsys):
    dev = _gpu()
    from foundationstereo_amd import evaluate
    gt = np.load(files / "gt.npy")
    seq = np.stack([gt + np.float32(d) for d in (2.0, 0.5, 0.004)]).astype(np.float32)
    np.save(files / "seq.npy", seq)
    res = evaluate.main(["--pred_file", str(files / "seq.npy"), "--gt_file", str(files / "gt.npy"), "--per_iter"])
    capsys.readouterr()
    p = res["per_iter"]
    assert res["mode"] == "pred_file" and p["iters"] == 3 and p["init"] is None and p["first_iter_within"] == 3
    assert p["epe"] == pytest.approx([2.0, 0.5, 0.004], rel=1e-4) and p["bad"][0][0] == 1.0 and p["bad"][1][0] == 0.0
    with pytest.raises(SystemExit, match="hiera"):
        evaluate.main(_flags(files) + ["--per_iter", "--hiera", "1"])
    np.save(files / "one.npy", seq[0])
    with pytest.raises(SystemExit, match="stored sequence"):
        evaluate.main(["--pred_file", str(files / "one.npy"), "--gt_file", str(files / "gt.npy"), "--per_iter"])
