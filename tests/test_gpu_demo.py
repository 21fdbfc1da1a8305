"""The demo end to end on the GPU (foundationstereo_amd/demo.py): one hash-initialised model with the
arguments and iteration count of the 64x96 end-to-end tests, on 50x90 frames (padded to 64x96 with
pads 3/3 and 7/7)."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import frames_oracle

pytestmark = pytest.mark.gpu

H, W, MAX_DISP, ITERS = 50, 90, 32, 4
K = np.array([[80.0, 0, 44.5], [0, 80.0, 24.5], [0, 0, 1]], dtype=np.float32)
BASELINE = 0.1
CLOUD = dict(z_far=20.0, denoise_radius=0.4, denoise_nb_points=10)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _frames():
    rng = np.random.default_rng(50)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


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
def pair(model):
    from foundationstereo_amd import demo
    left, right = _frames()
    return demo.run_pair(model, left, right, K, BASELINE, valid_iters=ITERS, **CLOUD)


def test_run_pair_disparity_is_the_forward_on_torch_padded_inputs(model, pair):
    dev = _gpu()
    from foundationstereo_amd.utils import InputPadder
    left, right = _frames()
    x0 = torch.as_tensor(left).to(dev).float()[None].permute(0, 3, 1, 2)        # scripts/run_demo.py:156-159
    x1 = torch.as_tensor(right).to(dev).float()[None].permute(0, 3, 1, 2)
    padder = InputPadder(x0.shape, divis_by=32)
    assert padder._pad == [3, 3, 7, 7]
    p0, p1 = padder.pad(x0, x1)
    assert torch.equal(pair["frames"].left, p0) and torch.equal(pair["frames"].right, p1)
    with torch.no_grad():
        disp = padder.unpad(model.forward(p0, p1, iters=ITERS, test_mode=True).float())
    assert pair["disp"].shape == (H, W) and torch.isfinite(pair["disp"]).all()
    assert torch.equal(pair["disp"], disp[0, 0])                               # same kernels, same input bytes


def test_run_pair_outputs_match_the_direct_calls(pair):
    from foundationstereo_amd import cloud, frames
    left, _ = _frames()
    disp = pair["disp"]
    o = {}
    vis = frames_oracle.vis_oracle(disp.cpu().numpy(), frames.TURBO, other_output=o)
    assert pair["vis"].shape == (H, 2 * W, 3)
    assert np.array_equal(pair["vis"].cpu().numpy(), np.concatenate([left, vis], axis=1))
    assert pair["minmax"].tolist() == [o["min_val"], o["max_val"]]
    img = torch.from_numpy(left).to(disp.device)
    c = cloud.disparity_to_cloud(disp, K, BASELINE, image=img, nb_points=CLOUD["denoise_nb_points"],
                                 radius=CLOUD["denoise_radius"], z_far=CLOUD["z_far"])[0]
    assert torch.equal(pair["depth"], c.depth)
    assert torch.equal(pair["cloud"][0], c.xyz_map[c.valid]) and torch.equal(pair["cloud"][1], img[c.valid])
    assert torch.equal(pair["cloud_denoise"][0], c.points) and torch.equal(pair["cloud_denoise"][1], c.colors)
    assert 0 < len(c.points) <= int(c.valid.sum())


def _ply_vertices(path):
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").splitlines()
    n = next(int(ln.split()[2]) for ln in head if ln.startswith("element vertex"))
    assert len(raw) - raw.index(b"end_header\n") - len(b"end_header\n") == n * 15     # float xyz + uchar rgb
    return n


def test_demo_main_writes_the_demo_files(pair, tmp_path, capsys):
    _gpu()
    from foundationstereo_amd import demo
    left, right = _frames()
    np.save(tmp_path / "L.npy", left)
    np.save(tmp_path / "R.npy", right)
    (tmp_path / "K.txt").write_text(" ".join(str(float(v)) for v in K.reshape(-1)) + f"\n{BASELINE}\n")
    common = ["--synthetic", "--max_disp", str(MAX_DISP), "--left_file", str(tmp_path / "L.npy"), "--right_file",
              str(tmp_path / "R.npy"), "--intrinsic_file", str(tmp_path / "K.txt"), "--valid_iters", str(ITERS),
              "--z_far", str(CLOUD["z_far"]), "--denoise_radius", str(CLOUD["denoise_radius"]),
              "--denoise_nb_points", str(CLOUD["denoise_nb_points"])]
    out = tmp_path / "out"
    res = demo.main(common + ["--out_dir", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and res["image_size"] == [H, W] and res["padded_size"] == [64, 96]
    assert sorted(os.listdir(out)) == ["K.txt", "cloud.ply", "cloud_denoise.ply", "depth_meter.npy", "left.npy",
                                       "right.npy", "vis.png"]
    raw = open(out / "vis.png", "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR"
    assert struct.unpack(">II", raw[16:24]) == (2 * W, H)                       # 50 rows of 180 pixels
    assert _ply_vertices(out / "cloud.ply") == res["cloud_points"] == len(pair["cloud"][0])
    assert _ply_vertices(out / "cloud_denoise.ply") == res["cloud_denoise_points"] == len(pair["cloud_denoise"][0])
    assert np.array_equal(np.load(out / "depth_meter.npy"), pair["depth"].cpu().numpy(), equal_nan=True)
    assert [res["min_disp"], res["max_disp"]] == pair["minmax"].tolist()

    pano = tmp_path / "pano"
    res = demo.main(common + ["--out_dir", str(pano), "--camera_type", "panorama"])
    assert "depth" not in res and not os.path.exists(pano / "depth_meter.npy")
    assert os.path.exists(pano / "vis.png") and _ply_vertices(pano / "cloud.ply") == res["cloud_points"]
