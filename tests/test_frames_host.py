"""CPU-only checks of the frame / picture stage: the oracle against the reference's golden, the
committed colour table, the PNG writer, the image reader, the argument checks of the three new entry
points and the demo's command line."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import frames_oracle


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "frames_small.npz"))


def test_vis_oracle_reproduces_reference(golden):
    """tests/golden/frames_small.npz holds the reference's own vis_disparity(cmap=turbo) output
    (tools/make_goldens.py frames): bit for bit, with computed and with explicit min / max."""
    disp, lut = golden["disp"], golden["lut"]
    assert disp.shape == (37, 53) and np.isinf(disp).sum() == 40
    other = {}
    got = frames_oracle.vis_oracle(disp, lut, other_output=other)
    assert got.dtype == np.uint8 and np.array_equal(got, golden["vis_auto"])
    assert np.array_equal(np.array([other["min_val"], other["max_val"]], np.float32), golden["minmax_auto"])
    assert not got[np.isinf(disp)].any() and got[~np.isinf(disp)].any()
    assert np.array_equal(frames_oracle.vis_oracle(disp, lut, min_val=5, max_val=40), golden["vis_5_40"])
    assert not np.array_equal(golden["vis_5_40"], golden["vis_auto"])


def test_ingest_oracle_reproduces_reference_padder(golden):
    """The reference's InputPadder((37, 53), divis_by=32): pads [5, 6, 13, 14], replicate values."""
    assert golden["pad"].tolist() == [5, 6, 13, 14] == list(frames_oracle.sintel_pads(37, 53))
    from foundationstereo_amd.utils import InputPadder
    assert InputPadder((37, 53), divis_by=32)._pad == [5, 6, 13, 14]
    img = np.floor(golden["pad_in"][0]).astype(np.uint8).transpose(1, 2, 0)          # (37,53,3) uint8
    batch, u8 = frames_oracle.ingest_oracle(img[None], img[None, ::-1])
    assert batch.shape == (1, 2, 3, 64, 64) and batch.dtype == np.float32 and np.array_equal(u8[0], img)
    want = np.floor(golden["pad_out"][0])            # floor commutes with replicate padding
    assert np.array_equal(batch[0, 0], want)
    assert np.array_equal(batch[0, 1, :, 13:50, 5:58], img[::-1].transpose(2, 0, 1))


def test_resize_oracle_sizes_and_ties():
    rng = np.random.default_rng(0)
    for (H, W), want in (((43, 86), (22, 43)), ((45, 90), (22, 45))):                # 21.5 -> 22, 22.5 -> 22
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out, raw = frames_oracle.resize_oracle(img, 0.5, return_raw=True)
        assert out.shape[:2] == want
        assert np.array_equal(raw * 4, np.round(raw * 4))                            # exact quarter sums
        assert (raw % 1 == 0.5).mean() > 0.15                                        # ties are common
        i = img.astype(np.int64)
        h, w = want[0] - 1, want[1] - 1                                              # outputs whose four taps exist
        box = i[0:2 * h:2, 0:2 * w:2] + i[0:2 * h:2, 1:2 * w:2] + i[1:2 * h:2, 0:2 * w:2] + i[1:2 * h:2, 1:2 * w:2]
        assert np.array_equal(out[:h, :w], (box + 2) // 4)                           # 2x2 mean, half up


def test_turbo_table_is_the_goldens(golden):
    from foundationstereo_amd import frames
    assert frames.TURBO.dtype == np.uint8 and frames.TURBO.shape == (256, 3)
    assert np.array_equal(frames.TURBO, golden["lut"])
    assert "import matplotlib" not in open(frames.__file__).read()


def _chunks(raw):
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        out.append((tag, data))
        pos += 12 + n
    assert pos == len(raw)
    return out


def test_write_png_structure(tmp_path):
    from foundationstereo_amd import frames
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    frames.write_png(tmp_path / "a.png", torch.from_numpy(img))
    ch = _chunks(open(tmp_path / "a.png", "rb").read())
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (13, 7, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(ch[1][1]), np.uint8).reshape(7, 1 + 39)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(7, 13, 3), img)
    with pytest.raises(ValueError):
        frames.write_png(tmp_path / "b.png", img[..., 0])
    with pytest.raises(ValueError):
        frames.write_png(tmp_path / "b.png", img.astype(np.float32))


def test_write_png_decodes_with_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from foundationstereo_amd import frames
    img = np.random.default_rng(2).integers(0, 256, (21, 34, 3), dtype=np.uint8)
    frames.write_png(tmp_path / "a.png", img)
    with Image.open(tmp_path / "a.png") as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)
    assert np.array_equal(frames.read_image(tmp_path / "a.png"), img)


def test_read_image_npy(tmp_path):
    from foundationstereo_amd import frames
    img = np.random.default_rng(3).integers(0, 256, (5, 6, 4), dtype=np.uint8)
    np.save(tmp_path / "f.npy", img)
    got = frames.read_image(tmp_path / "f.npy")
    assert got.dtype == np.uint8 and np.array_equal(got, img)
    np.save(tmp_path / "g.npy", img.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        frames.read_image(tmp_path / "g.npy")


def test_frame_entry_points_reject_bad_args_without_gpu():
    """Argument validation happens before any HIP call, so it is testable on the CPU."""
    from foundationstereo_amd import _lib
    lib = _lib.load()

    def ingest(left=16, right=16, out=16, u8=None, B=1, H=37, W=53, C=3, scale=1.0, Hs=37, Ws=53, pl=5, pr=6, pt=13,
               pb=14, d=32):
        return lib.fsmi_frames_ingest(left, right, out, u8, B, H, W, C, scale, Hs, Ws, pl, pr, pt, pb, d, None)
    assert ingest(C=2) == 1001 and b"C = 2" in lib.fsmi_last_error()
    assert ingest(scale=0.0) == 1001 and b"scale" in lib.fsmi_last_error()
    assert ingest(scale=1.5) == 1001 and b"scale" in lib.fsmi_last_error()
    assert ingest(scale=-0.5) == 1001
    assert ingest(scale=float("nan")) == 1001
    assert ingest(pb=13) == 1001 and b"divis_by" in lib.fsmi_last_error()          # Hp = 63
    assert ingest(pr=5) == 1001                                                      # Wp = 63
    assert ingest(Hs=36) == 1001                                                     # scale 1 but resized != source
    assert ingest(scale=0.5, Hs=40, Ws=26, pt=12, pb=12, pl=3, pr=3) == 1001         # resized larger than the source
    assert ingest(pl=-1, pr=12) == 1001
    assert ingest(d=0) == 1001
    assert ingest(B=0) == 1001
    assert ingest(left=None) == 1001 and b"null" in lib.fsmi_last_error()
    assert ingest(out=20) == 1001 and b"aligned" in lib.fsmi_last_error()
    assert ingest(pl=0, pr=1, pt=0, pb=1, d=2) == 1001                               # Wp = 54: even, not a float4
    assert b"multiple of 4" in lib.fsmi_last_error()

    inf = float("inf")
    assert lib.fsmi_disp_minmax(None, 16, 1, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_minmax(16, None, 1, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_minmax(16, 16, 0, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_minmax(20, 16, 1, 4, 4, inf, None) == 1001                  # unaligned disp
    assert lib.fsmi_disp_minmax(16, 16, 1, 4, 4, float("nan"), None) == 1001

    assert lib.fsmi_disp_colorize(None, 16, 16, None, 16, 1, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_colorize(16, None, 16, None, 16, 1, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_colorize(16, 16, None, None, 16, 1, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_colorize(16, 16, 16, None, None, 1, 4, 4, inf, None) == 1001
    assert lib.fsmi_disp_colorize(16, 16, 16, None, 16, 1, 4, 0, inf, None) == 1001
    assert lib.fsmi_disp_colorize(16, 16, 16, None, 18, 1, 4, 4, inf, None) == 1001  # unaligned out
    assert lib.fsmi_disp_colorize(16, 16, 16, None, 16, 1, 1 << 15, 1 << 15, inf, None) == 1001
    assert b"2^31" in lib.fsmi_last_error()


def test_frame_ops_refuse_cpu_tensors_and_floats():
    from foundationstereo_amd import frames, ops
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.frames_ingest(u8, u8)
    with pytest.raises(RuntimeError, match="ROCm"):
        frames.ingest(u8[0], u8[0])
    with pytest.raises(RuntimeError, match="ROCm"):
        ops.disp_minmax(torch.ones(1, 4, 8))
    with pytest.raises(RuntimeError, match="ROCm"):
        frames.vis_disparity(torch.ones(4, 8))
    with pytest.raises(RuntimeError, match="ROCm"):
        frames.vis_disparity(torch.ones(4, 8), min_val=0.0, max_val=1.0)
    with pytest.raises(RuntimeError, match="uint8"):
        frames.ingest(np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.float32))


def test_frame_torch_operators_registered_without_cpu_kernel():
    from foundationstereo_amd import torch_ops
    torch_ops.load()
    assert "frames_ingest" in torch_ops.OPS and "vis_disparity" in torch_ops.OPS
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        torch.ops.fsmi.frames_ingest(u8, u8)
    with pytest.raises(NotImplementedError):
        torch.ops.fsmi.vis_disparity(torch.ones(1, 4, 8), torch.zeros((256, 3), dtype=torch.uint8))


def test_demo_command_line_lists_the_reference_flags(capsys):
    from foundationstereo_amd import demo
    with pytest.raises(SystemExit) as e:
        demo.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--left_file", "--right_file", "--intrinsic_file", "--ckpt_dir", "--out_dir", "--camera_type", "--scale",
                 "--hiera", "--z_far", "--valid_iters", "--get_pc", "--remove_invisible", "--denoise_cloud",
                 "--denoise_nb_points", "--denoise_radius", "--synthetic", "--backbone", "--max_disp", "--vit_size"):
        assert flag in text, flag
    a = demo.parser().parse_args([])
    assert (a.camera_type, a.scale, a.hiera, a.z_far, a.valid_iters, a.get_pc, a.remove_invisible, a.denoise_cloud,
            a.denoise_nb_points, a.denoise_radius) == ("pinhole", 1, 0, 10, 32, 1, 1, 1, 30, 0.03)
