"""bench.py's ``--dump-outputs`` helper (CPU): ``dump_outputs`` writes the step's disparities as
float32, whole or -- beyond its size limit -- as the same seeded sample every time."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_dump_outputs_whole(tmp_path):
    import bench
    out = torch.arange(2 * 6 * 8, dtype=torch.float64).reshape(2, 1, 6, 8) / 7
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["disparity.npy"]
    got = np.load(tmp_path / "d" / "disparity.npy")
    assert got.dtype == np.float32 and got.shape == (2, 1, 6, 8)
    assert np.array_equal(got, out.float().numpy())


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096)
    g = torch.Generator().manual_seed(3)
    out = torch.rand(3, 1, 40, 50, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out.clone())
    a, b = np.load(tmp_path / "a" / "disparity.npy"), np.load(tmp_path / "b" / "disparity.npy")
    assert a.dtype == np.float32 and a.nbytes <= 4096 and a.size == 4096 // 8
    assert np.array_equal(a, b)
    assert np.isin(a, out.numpy()).all()


def test_plain_and_full_options_parse():
    """``--help`` lists ``--full`` and ``--dump-outputs DIR``."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
