"""CPU: overlap statistics (return_uncertainty) and pseudo labels -- the prv2_blend_*_stats entry points are declared, bound and
exported and reject bad arguments without a GPU, their torch ops have schemas, Tester.generate_pl writes exactly the five files of a
pseudo label in the encodings the semi-supervised loader reads, and tools/test.py offers --generate-pl / --count-thr."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_SYMBOLS = ("prv2_blend_paste_stats", "prv2_blend_update_stats", "prv2_blend_resize_stats")
STATS_OPS = ("blend_init_stats", "blend_update_stats", "blend_resize_stats")


def test_stats_entry_points_declared_bound_and_exported():
    from patchrefinerv2_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    lib = L.load()
    assert lib.prv2_abi_version() == 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in STATS_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in L.SIGNATURES and hasattr(raw, name), name


def _err(lib):
    return lib.prv2_last_error().decode()


def test_stats_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument check before a launch
    paste, update, resize = lib.prv2_blend_paste_stats, lib.prv2_blend_update_stats, lib.prv2_blend_resize_stats
    # null m2 / ntiles (and the maps the *_frames checks already cover)
    for fn in (paste, update):
        assert fn(p, p, None, p, 1, 32, 32, p, 8, 8, 64, p, p, 1, 1, 8, 8, None) != 0 and "null" in _err(lib)
        assert fn(p, p, p, None, 1, 32, 32, p, 8, 8, 64, p, p, 1, 1, 8, 8, None) != 0 and "null" in _err(lib)
        assert fn(None, p, p, p, 1, 32, 32, p, 8, 8, 64, p, p, 1, 1, 8, 8, None) != 0 and "null" in _err(lib)
    assert resize(p, p, None, p, 1, 8, 8, p, p, p, p, 16, 16, None) != 0 and "null" in _err(lib)
    assert resize(p, p, p, p, 1, 8, 8, p, p, p, None, 16, 16, None) != 0 and "null" in _err(lib)
    # n_frames out of [1, 65535]
    for b in (0, -1):
        assert paste(p, p, p, p, b, 32, 32, p, 8, 8, 64, p, p, 1, 1, 8, 8, None) != 0 and "n_frames" in _err(lib)
        assert update(p, p, p, p, b, 32, 32, p, 8, 8, 64, p, p, 1, 1, 8, 8, None) != 0 and "n_frames" in _err(lib)
        assert resize(p, p, p, p, b, 8, 8, p, p, p, p, 16, 16, None) != 0 and "n_frames" in _err(lib)
    assert update(p, p, p, p, 70000, 32, 32, p, 8, 8, 4 * 64, p, p, 4, 4, 8, 8, None) != 0 and "frame count" in _err(lib)
    assert resize(p, p, p, p, 70000, 8, 8, p, p, p, p, 16, 16, None) != 0
    # overlapping frame strides: tile stride < k, prediction stride < k * ph * pw
    assert update(p, p, p, p, 2, 32, 32, p, 8, 8, 4 * 64, p, p, 3, 4, 8, 8, None) != 0 and "stride" in _err(lib)
    assert paste(p, p, p, p, 2, 32, 32, p, 8, 8, 4 * 64 - 1, p, p, 4, 4, 8, 8, None) != 0 and "stride" in _err(lib)
    # geometry: a tile larger than the map, k < 1, empty resize
    assert update(p, p, p, p, 1, 32, 32, p, 8, 8, 64, p, p, 1, 1, 40, 8, None) != 0 and "geometry" in _err(lib)
    assert paste(p, p, p, p, 1, 32, 32, p, 8, 8, 64, p, p, 1, 0, 8, 8, None) != 0 and "geometry" in _err(lib)
    assert resize(p, p, p, p, 1, 8, 8, p, p, p, p, 0, 16, None) != 0
    with pytest.raises(RuntimeError):
        L.check(resize(p, p, p, p, 0, 8, 8, p, p, p, p, 16, 16, None), "blend_resize_stats")


def test_stats_torch_ops_registered_and_reject_cpu_tensors():
    from patchrefinerv2_amd import torch_ops
    ops = torch_ops.load()
    for name in STATS_OPS:
        assert name in torch_ops.OPS
        getattr(ops, name).default._schema  # registered with a schema
    s = str(ops.blend_update_stats.default._schema)
    for frag in ("Tensor(a!) avg", "Tensor(b!) cnt", "Tensor(c!) m2", "Tensor(d!) ntiles", "Tensor pred", "Tensor tiles", "int th"):
        assert frag in s, (frag, s)
    assert "-> (Tensor, Tensor, Tensor, Tensor)" in str(ops.blend_resize_stats.default._schema)
    z = torch.zeros
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.blend_init_stats(z(1, 8, 8), z(1, 8, 8), z(1, 8, 8), z(1, 8, 8), z(1, 1, 4, 4), z(4, 4), z(1, 1, 2, dtype=torch.int32), 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.blend_update_stats(z(1, 8, 8), z(1, 8, 8), z(1, 8, 8), z(1, 8, 8), z(1, 1, 4, 4), z(4, 4), z(1, 1, 2, dtype=torch.int32), 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.blend_resize_stats(z(1, 8, 8), z(1, 8, 8), z(1, 8, 8), z(1, 8, 8), 16, 16)


# ------------------------------------------------------------------------------------------------------------------------------
# Tester.generate_pl on a stub model (host tensors)
# ------------------------------------------------------------------------------------------------------------------------------
H, W = 12, 20
N_TILES = 40  # the stub plan's tile count: the low-coverage threshold is count_thr * 40


def _frame_maps(i):
    """known depth / uncertainty / count of frame i: a count ramp from 0 to 299 tiles (low coverage at the left, saturation at the right)"""
    g = np.random.RandomState(30 + i)
    depth = (g.rand(H, W) * 40 + 1).astype(np.float32)
    unc = (g.rand(H, W) * 3).astype(np.float32)
    count = np.floor(np.linspace(0, 299, H * W)).reshape(H, W).astype(np.float32)
    return depth, unc, count


class _StubModel:
    """what generate_pl needs of a model: device, resizer, the call contract with return_uncertainty, last_plan"""
    device = torch.device("cpu")
    needs_coarse = False

    def __init__(self):
        self.calls = []

    def resizer(self, hr):
        return hr[:, :, ::2, ::2]

    def __call__(self, mode=None, image_hr=None, return_uncertainty=False, **kw):
        assert mode == "infer" and return_uncertainty
        idx = [int(v) for v in image_hr[:, 0, 0, 0]]  # the stub dataset writes the frame index into pixel (0, 0)
        self.calls.append(idx)
        maps = [_frame_maps(i) for i in idx]
        t = lambda k: torch.from_numpy(np.stack([m[k] for m in maps]))[:, None]  # noqa: E731
        self.last_plan = [dict(kind="init", raw=[(0, 0)] * 4), dict(kind="random", raw=[(0, 0)] * (N_TILES - 4))]
        return t(0), dict(uncertainty=t(1), count_map=t(2))


class _StubDataset:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        hr = torch.zeros(3, H, W)
        hr[0, 0, 0] = i
        return dict(image_hr=hr, img_file_basename=f"img{i}")


@pytest.mark.parametrize("frame_batch", [1, 2])
def test_generate_pl_writes_the_five_pseudo_label_files(tmp_path, frame_batch):
    from PIL import Image
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    model = _StubModel()
    runner = RunnerInfo(rank=0, world_size=1, save=True, work_dir=str(tmp_path))
    res = Tester(None, runner, _StubDataset(3), model).generate_pl(cai_mode="r32", process_num=4, image_raw_shape=(H, W),
                                                                   patch_split_num=(2, 2), count_thr=0.25, frame_batch=frame_batch)
    assert model.calls == ([[0], [1], [2]] if frame_batch == 1 else [[0, 1], [2]])
    assert [r["name"] for r in res] == ["img0", "img1", "img2"] and all(r["n_tiles"] == N_TILES for r in res)
    suffixes = (".png", "_uint16.png", "_uncert_uint16.png", "_uncert.png", "_count_uint16.png")
    assert sorted(os.listdir(tmp_path)) == sorted(f"img{i}{s}" for i in range(3) for s in suffixes)
    for i in range(3):
        depth, unc, count = _frame_maps(i)
        png = lambda s: np.asarray(Image.open(str(tmp_path / f"img{i}{s}")))  # noqa: E731
        d16, u16, c16 = png("_uint16.png"), png("_uncert_uint16.png"), png("_count_uint16.png")
        assert d16.dtype == u16.dtype == c16.dtype == np.uint16 and d16.shape == u16.shape == c16.shape == (H, W)
        assert np.array_equal(d16, (depth * 256).astype(np.uint16))
        # uncertainty: min-max to [0, 1], then 1 where fewer than count_thr * tiles = 10 tiles cover the pixel; floor(u * 256)
        u = (unc.astype(np.float64) - unc.min()) / (float(unc.max()) - float(unc.min()))
        low = count < 0.25 * N_TILES
        assert low.sum() > 0 and (~low).sum() > 0
        u[low] = 1.0
        assert np.array_equal(u16, np.floor(u * 256).astype(np.uint16))
        assert np.all(u16[low] == 256) and u16.max() == 256
        # tile counts x 256, saturating at 65535 (256 tiles or more)
        assert np.array_equal(c16, np.clip(count.astype(np.float64) * 256, 0, 65535).astype(np.uint16))
        assert np.all(c16[count >= 256] == 65535) and (count >= 256).sum() > 0
        assert np.array_equal(c16[count < 256], (count[count < 256] * 256).astype(np.uint16))
        for s in (".png", "_uncert.png"):  # colour maps
            c = png(s)
            assert c.dtype == np.uint8 and c.shape == (H, W, 3) and c.std() > 0


def test_generate_pl_gray_scale_flat_uncertainty_and_no_save(tmp_path):
    """a flat uncertainty map normalises to 0 (only the low-coverage override remains); without save nothing is written"""
    from PIL import Image
    from patchrefinerv2_amd.tester import RunnerInfo, Tester, pseudo_label_uncertainty
    u, count = pseudo_label_uncertainty(np.full((2, 3), 0.7, np.float32), np.array([[1, 5, 9], [2, 2, 40]], np.float32), 40, 0.1)
    assert np.array_equal(u, [[1, 0, 0], [1, 1, 0]]) and count.dtype == np.float64
    runner = RunnerInfo(rank=0, world_size=1, save=False, work_dir=str(tmp_path / "none"))
    Tester(None, runner, _StubDataset(1), _StubModel()).generate_pl(image_raw_shape=(H, W), patch_split_num=(2, 2))
    assert not (tmp_path / "none").exists()
    runner = RunnerInfo(rank=0, world_size=1, save=True, gray_scale=True, work_dir=str(tmp_path / "g"))
    Tester(None, runner, _StubDataset(1), _StubModel()).generate_pl(image_raw_shape=(H, W), patch_split_num=(2, 2))
    c = np.asarray(Image.open(str(tmp_path / "g" / "img0.png")))
    assert np.array_equal(c[..., 0], c[..., 1]) and np.array_equal(c[..., 1], c[..., 2])  # gray_r


def test_generate_pl_frame_sharded_over_ranks(tmp_path):
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    model = _StubModel()
    runner = RunnerInfo(rank=1, world_size=2, save=True, work_dir=str(tmp_path))
    res = Tester(None, runner, _StubDataset(5), model).generate_pl(image_raw_shape=(H, W), patch_split_num=(2, 2), frame_batch=2)
    assert model.calls == [[1, 3]] and [r["name"] for r in res] == ["img1", "img3"]
    assert sorted(n for n in os.listdir(tmp_path) if n.endswith("_count_uint16.png")) == ["img1_count_uint16.png", "img3_count_uint16.png"]


def test_cli_lists_generate_pl_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--generate-pl" in r.stdout and "--count-thr" in r.stdout
