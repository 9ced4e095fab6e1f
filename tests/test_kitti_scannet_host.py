"""CPU: KittiDataset and ScanNetDataset without a GPU -- the specification of their device work (metrics.depth16_decode_spec,
metrics.pil_nearest_index) against PIL itself (``Image.crop``, ``Image.resize(NEAREST)``, ``np.asarray``) and against the reference's
numpy expressions, and the host half of the two classes: split parsing, the basename rules, the reader, the unbuilt modes, the command
line's two test types, the C entry point.  Parity with the reference classes themselves is unpinned (they need mmengine, kornia, cv2):
what is not PIL is a line-by-line restatement.  The generators of the synthetic trees are shared with tests/test_kitti_scannet_gpu.py."""
import argparse
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from test_cityscapes_host import image_scene
from test_general_gt_host import bit_equal, boundaries_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS10 = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")  # kitti_dataset.py:236-245
KEYS30 = tuple(pre + k for pre in ("edge_", "noedge_", "") for k in KEYS10)                     # scannet_dataset.py:258-289
KB = (352, 1216)
KITTI_SHAPE, KITTI_FRAMES = (360, 1224), 2   # the source of the kb-crop: top margin 8, left margin 4; frame 1 has an empty Garg crop
SCANNET_IMG, SCANNET_DEPTH, SCANNET_FRAMES = (30, 40), (12, 16), 2
SCANNET_CLI_IMG, SCANNET_CLI_DEPTH = (64, 128), (27, 50)  # the CLI's tree: a frame the model can tile (divisible by 2 x the split)
SCANNET_SEED, SCANNET_CLI_SEED = 1, 0  # (frame i of a tree is scannet_samples(seed + i))
SCANNET_SCENE = "1ada7a0617"


# ------------------------------------------------------------------------------------------------------------------ scenes
def kitti_dense(h, w, seed=0):
    """a dense metric depth map of a road scene, float64 metres: far at the top, near at the bottom, two boxes"""
    y, x = np.mgrid[0:h, 0:w]
    d = 6.0 + 60.0 * (1.0 - y / h) ** 2 + 0.002 * x
    d[(y > 0.55 * h) & (y < 0.8 * h) & (x > 0.2 * w + 7 * seed) & (x < 0.3 * w + 7 * seed)] = 9.0 + seed
    d[(y > 0.45 * h) & (y < 0.7 * h) & (x > 0.6 * w) & (x < 0.72 * w)] = 17.5
    return d


def kitti_samples(h, w, seed=0, empty_crop=False):
    """the uint16 samples of a KITTI depth PNG (metres x 256): sparse LiDAR returns -- about a third of the pixels, none in the top
    third --, zeros elsewhere; ``empty_crop``: no return below row 0.4 h, so that nothing valid lies inside the Garg crop"""
    rs = np.random.RandomState(50 + seed)
    raw = np.round(kitti_dense(h, w, seed) * 256).astype(np.uint16)
    raw[rs.rand(h, w) > 0.35] = 0
    raw[:h // 3] = 0
    if empty_crop:
        raw[int(0.38 * h):] = 0
        raw[h // 8:h // 6, ::3] = 2000  # (returns above the crop: the frame is not empty)
    return raw


def scannet_samples(h, w, seed=0):
    """the uint16 samples of a ScanNet depth PNG (millimetres): a tilted floor, a wall 1.5 m nearer and a pillar, a few zeros"""
    y, x = np.mgrid[0:h, 0:w]
    d = 3200.0 + (3.0 + seed) * x + 2.0 * y
    wall = x < (5 * w) // 16 + seed
    d[wall] = 1500.0 + 100.0 * seed + 2.0 * y[wall]
    d[(y >= (2 * h) // 3 - seed) & (x >= (5 * w) // 8) & (x < (7 * w) // 8)] = 2100.0
    raw = np.round(d).astype(np.uint16)
    raw[0, w - 1] = raw[h - 1, 0] = 0
    return raw


# ------------------------------------------------------------------------------------------------------------------ trees and configs
def write_kitti_tree(root, n=KITTI_FRAMES, shape=KITTI_SHAPE, seed=0):
    """a synthetic KITTI tree under ``root``: raw/<date>/<drive>/image_02/data/<frame>.png and depth/<drive>/proj_depth/groundtruth/
    image_02/<frame>.png, a split file of 'img depth' lines relative to raw/ and depth/ in REVERSE order plus one 'None' line ->
    (split path, [dict(img, depth: absolute paths; rel; pixels, raw: the arrays)] sorted by image path)"""
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    drive = "2011_09_26_drive_0002_sync"
    items = []
    for i in range(n):
        rel_img = f"2011_09_26/{drive}/image_02/data/{i:010d}.png"
        rel_depth = f"{drive}/proj_depth/groundtruth/image_02/{i:010d}.png"
        it = dict(rel=rel_img, rel_depth=rel_depth, img=os.path.join(root, "raw", rel_img), depth=os.path.join(root, "depth", rel_depth))
        it["pixels"], it["raw"] = image_scene(*shape, seed=seed + i), kitti_samples(*shape, seed=seed + i, empty_crop=(i == 1))
        for p in (it["img"], it["depth"]):
            os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(it["pixels"]).save(it["img"])
        write_png16(it["depth"], it["raw"])
        items.append(it)
    split = os.path.join(root, "eigen_test.txt")
    with open(split, "w") as f:
        f.write(f"2011_09_26/{drive}/image_02/data/{99:010d}.png None 721.5377\n")
        for it in reversed(items):
            f.write(f"{it['rel']} {it['rel_depth']} 721.5377\n")
    return split, sorted(items, key=lambda it: it["img"])


def write_scannet_tree(root, n=SCANNET_FRAMES, img_shape=SCANNET_IMG, depth_shape=SCANNET_DEPTH, seed=SCANNET_SEED):
    """a synthetic ScanNet++ tree under ``root``: data/<scene>/iphone/rgb/frame_<n>.png beside .../render_depth/frame_<n>.png of ANOTHER
    size, a split file of absolute 'img depth' lines in REVERSE order -> (split path, [dict(img, depth, pixels, raw)] sorted)"""
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    items = []
    for i in range(n):
        stem = f"frame_{120 * i:06d}"
        it = dict(img=os.path.join(root, "data", SCANNET_SCENE, "iphone", "rgb", stem + ".png"),
                  depth=os.path.join(root, "data", SCANNET_SCENE, "iphone", "render_depth", stem + ".png"))
        it["pixels"], it["raw"] = image_scene(*img_shape, seed=seed + i), scannet_samples(*depth_shape, seed=seed + i)
        for p in (it["img"], it["depth"]):
            os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(it["pixels"]).save(it["img"])
        write_png16(it["depth"], it["raw"])
        items.append(it)
    split = os.path.join(root, "nvs_sem_val.txt")
    with open(split, "w") as f:
        for it in reversed(items):
            f.write(f"{it['img']} {it['depth']}\n")
    return split, sorted(items, key=lambda it: it["img"])


TC = "transform_cfg=dict(degree=1.0, network_process_size=[384, 512])"


def kitti_config_text(root, split, extra=""):
    """the project's small config with configs/_base_/datasets/kitti.py's val_dataloader"""
    return (f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n{extra}"
            f"val_dataloader = dict(_delete_=True, batch_size=1, num_workers=1, dataset=dict(type='KittiDataset', mode='infer', "
            f"data_root={root!r}, split={split!r}, min_depth=1e-3, max_depth=80, {TC}))\n")


def scannet_config_text(split, extra=""):
    """the project's small config with configs/_base_/datasets/scannet.py's val_dataloader"""
    return (f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n{extra}"
            f"val_dataloader = dict(_delete_=True, batch_size=1, num_workers=2, dataset=dict(type='ScanNetDataset', mode='infer', "
            f"split={split!r}, min_depth=1e-3, max_depth=80, {TC}))\n")


def cli_module():
    spec = importlib.util.spec_from_file_location("prv2_tools_test_kitti_scannet", os.path.join(ROOT, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def cli_dataset(cfg_path, test_type, **ns):
    """the dataset ``tools/test.py CONFIG --test-type kitti|scannet`` builds"""
    from patchrefinerv2_amd.registry import Config
    cli = cli_module()
    args = argparse.Namespace(**dict(dict(test_type=test_type, config=str(cfg_path), image_raw_shape=[8, 16], edge_metrics=False), **ns))
    return cli.build_dataset(cli.dataset_config(Config.fromfile(str(cfg_path)), args))


def _tc():
    return dict(degree=1.0, network_process_size=[384, 512])


def _kitti(root, split, **kw):
    from patchrefinerv2_amd import tester
    cfg = dict(mode="infer", data_root=root, split=split, transform_cfg=_tc(), min_depth=1e-3, max_depth=80)
    cfg.update(kw)
    return tester.KittiDataset(**cfg)


def _scannet(split, **kw):
    from patchrefinerv2_amd import tester
    cfg = dict(mode="infer", split=split, transform_cfg=_tc(), min_depth=1e-3, max_depth=80)
    cfg.update(kw)
    return tester.ScanNetDataset(**cfg)


def host_slot(shape, img_shape=None):
    """a staging slot in plain host memory (the datasets' own are pinned, which needs a GPU)"""
    ih, iw = img_shape or shape
    return dict(img=torch.empty(ih * iw * 3, dtype=torch.uint8), depth=torch.empty(shape[0] * shape[1] * 2, dtype=torch.uint8), shape=None,
                img_shape=None)


# ------------------------------------------------------------------------------------------------------------------ host routes (PIL + numpy)
def pil_u16(raw):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(raw, np.uint16))
    assert im.mode == "I;16"
    return im


def kitti_host_route(raw, do_kb_crop=True):
    """kitti_dataset.py:117, :123-131, :142, :203 with PIL and numpy -> (depth float32, boundary uint8)"""
    depth_gt = pil_u16(raw)
    if do_kb_crop:
        height, width = depth_gt.height, depth_gt.width
        top_margin = int(height - 352)
        left_margin = int((width - 1216) / 2)
        depth_gt = depth_gt.crop((left_margin, top_margin, left_margin + 1216, top_margin + 352))
    depth = np.asarray(depth_gt, dtype=np.float32) / 256.0
    return depth, boundaries_spec(depth, 1.0)


def scannet_host_route(raw, img_hw):
    """scannet_dataset.py:112-118, :132, :188 with PIL and numpy -> (depth float32, boundary uint8)"""
    from PIL import Image
    depth_gt = pil_u16(raw).resize((img_hw[1], img_hw[0]), Image.NEAREST)
    depth = np.asarray(depth_gt).astype(np.float32).copy() / 1000.0
    return depth, boundaries_spec(depth, 1.0)


def pil_nearest(n_in, n_out):
    """the source index PIL's NEAREST resize picks for every output index along one axis"""
    from PIL import Image
    row = np.arange(n_in, dtype=np.uint16)[None, :]
    got = np.asarray(pil_u16(row).resize((n_out, 1), Image.NEAREST))[0].astype(np.int64)
    col = np.asarray(pil_u16(row.T.copy()).resize((1, n_out), Image.NEAREST))[:, 0].astype(np.int64)
    assert np.array_equal(got, col)  # rows and columns follow one rule
    return got


def canny_margin(log_depth):
    """how far the host detector's decisions on this map are from flipping: the smallest distance of a pixel's gradient magnitude from
    the two thresholds (metrics.canny's own smoothing and Sobel)"""
    from scipy import ndimage as ndi
    image = np.asarray(log_depth, np.float32)
    bleed = ndi.gaussian_filter(np.ones(image.shape, np.float32), 1.0, mode="constant", cval=0.0) + np.finfo(np.float32).eps
    sm = ndi.gaussian_filter(image, 1.0, mode="constant", cval=0.0) / bleed
    mag = np.hypot(ndi.sobel(sm, axis=0), ndi.sobel(sm, axis=1))[1:-1, 1:-1]
    return float(min(np.abs(mag - 0.1).min(), np.abs(mag - 0.2).min()))


# ------------------------------------------------------------------------------------------------------------------ the spec against PIL
PAIRS = [(i, o) for i in range(1, 24) for o in range(1, 24)] + [(640, 1296), (480, 968), (1440, 1440), (1920, 1920), (4, 6), (12, 30), (16, 40),
                                                                 (27, 64), (50, 128), (1296, 640), (2, 49), (4, 14), (6, 47), (2, 7)]


def test_pil_nearest_index_equals_pillow():
    from patchrefinerv2_amd import metrics as M
    for n_in, n_out in PAIRS:
        got = M.pil_nearest_index(n_out, n_in)
        assert got.dtype == np.int64 and got.shape == (n_out,) and np.array_equal(got, pil_nearest(n_in, n_out)), (n_in, n_out)
    for n in (1, 7, 1440):
        assert np.array_equal(M.pil_nearest_index(n, n), np.arange(n))  # equal sizes: the identity
    with pytest.raises(ValueError):
        M.pil_nearest_index(0, 4)


def test_exact_ties_take_the_upper_pixel_and_adding_the_step_up_does_not_reproduce_pillow():
    """(2x + 1) n_in divisible by 2 n_out: the product lands on an integer, which belongs to the upper pixel"""
    from patchrefinerv2_amd import metrics as M
    assert list(M.pil_nearest_index(6, 4)) == [0, 1, 1, 2, 3, 3] == list(pil_nearest(4, 6))  # x = 1: 1.5 * 4 / 6 = 1 exactly
    assert (2 * 40 + 1) * 640 % (2 * 1296) == 0 and M.pil_nearest_index(1296, 640)[40] == 20 == pil_nearest(640, 1296)[40]
    assert M.pil_nearest_index(1296, 640)[39] == 19

    def accumulated(n_in, n_out):
        s = np.float64(n_in) / np.float64(n_out)
        xo, out = s * 0.5, []
        for _ in range(n_out):
            out.append(int(xo))
            xo += s
        return np.array(out)
    differ = sum(not np.array_equal(accumulated(i, o), pil_nearest(i, o)) for i, o in PAIRS)
    assert differ > 10  # the rule that multiplies is the one to build


@pytest.mark.parametrize("shape", [(375, 1242), (376, 1240)])
def test_window_offsets_equal_image_crop(shape):
    """an odd and an even margin: top = h - 352, left = int((w - 1216) / 2) against PIL's crop of the same box"""
    from patchrefinerv2_amd import metrics as M
    h, w = shape
    raw = ((np.arange(h, dtype=np.uint32)[:, None] * 1543 + np.arange(w, dtype=np.uint32)[None, :] * 7) % 65536).astype(np.uint16)
    top, left = int(h - 352), int((w - 1216) / 2)
    assert (top, left) == ((23, 13) if shape == (375, 1242) else (24, 12))
    want_d, want_b = kitti_host_route(raw)
    depth, boundary = M.depth16_decode_spec(raw, 256.0, window=(top, left) + KB)
    assert depth.shape == KB and depth.dtype == np.float32 and boundary.dtype == np.uint8
    assert bit_equal(depth, want_d) and np.array_equal(boundary, want_b)
    assert depth[0, 0] == np.float32(raw[top, left]) / np.float32(256) and depth[-1, -1] == np.float32(raw[h - 1, left + 1215]) / np.float32(256)
    whole_d, whole_b = M.depth16_decode_spec(raw, 256.0)
    assert bit_equal(whole_d, kitti_host_route(raw, do_kb_crop=False)[0]) and np.array_equal(whole_b, kitti_host_route(raw, False)[1])


@pytest.mark.parametrize("src,out", [((5, 7), (13, 15)), ((4, 4), (6, 6)), ((2, 640), (3, 1296)), ((9, 12), (4, 5)), ((7, 9), (7, 9)),
                                     ((1, 1), (3, 3)), (SCANNET_DEPTH, SCANNET_IMG), (SCANNET_CLI_DEPTH, SCANNET_CLI_IMG)])
def test_nearest_decode_equals_image_resize(src, out):
    from patchrefinerv2_amd import metrics as M
    rs = np.random.RandomState(src[0] * 100 + out[1])
    raw = rs.randint(0, 65536, src).astype(np.uint16)
    raw.flat[0], raw.flat[-1] = 0, 65535  # (one pixel: 65535)
    want_d, want_b = scannet_host_route(raw, out)
    depth, boundary = M.depth16_decode_spec(raw, 1000.0, out_hw=out)
    assert depth.shape == out and bit_equal(depth, want_d) and np.array_equal(boundary, want_b)
    if out[0] >= src[0] and out[1] >= src[1]:  # (an upscale reads every source pixel)
        assert depth.max() == np.float32(65535) / np.float32(1000) and (depth.min() == 0 or raw.size == 1)


def test_decode_is_the_references_numpy_expression():
    from PIL import Image
    from patchrefinerv2_amd import metrics as M
    raw = np.arange(65536, dtype=np.uint16).reshape(256, 256)  # every sample value
    im = pil_u16(raw)
    assert np.array_equal(np.asarray(im), raw)
    d_k, _ = M.depth16_decode_spec(raw, 256.0)
    d_s, _ = M.depth16_decode_spec(raw, 1000.0)
    assert bit_equal(d_k, np.asarray(im, dtype=np.float32) / 256.0)                    # kitti_dataset.py:142
    assert bit_equal(d_s, np.asarray(im).astype(np.float32).copy() / 1000.0)           # scannet_dataset.py:132
    assert bit_equal(d_s, np.asarray(im.resize((256, 256), Image.NEAREST)).astype(np.float32) / 1000.0)
    # a multiply by the reciprocal is another function: 1 / 1000 is no float32
    assert not bit_equal(d_s, raw.astype(np.float32) * np.float32(1.0 / 1000.0))
    with pytest.raises(ValueError, match="uint16"):
        M.depth16_decode_spec(raw.astype(np.int32), 256.0)
    with pytest.raises(ValueError, match="not both"):
        M.depth16_decode_spec(raw, 256.0, window=(0, 0, 2, 2), out_hw=(4, 4))
    with pytest.raises(ValueError, match="outside"):
        M.depth16_decode_spec(raw, 256.0, window=(250, 0, 8, 8))


def test_hand_checkable_boundary_rows():
    """a difference of exactly 1.0 m is no boundary, one raw unit more is"""
    from patchrefinerv2_amd import metrics as M
    raw = np.array([[1000, 1256, 1513, 1513, 0]], np.uint16)  # 256 apart: 1.0 m; 257 apart: more; equal; a step to zero
    depth, boundary = M.depth16_decode_spec(raw, 256.0)
    assert float(depth[0, 1] - depth[0, 0]) == 1.0 and list(boundary[0]) == [0, 1, 1, 1, 1]
    raw = np.array([[2000], [3000], [4001], [4001]], np.uint16)  # 1000 apart: 1.0 m; 1001 apart
    depth, boundary = M.depth16_decode_spec(raw, 1000.0)
    assert float(depth[1, 0] - depth[0, 0]) == 1.0 and list(boundary[:, 0]) == [0, 1, 1, 0]
    # through the nearest grid: the boundary is taken between OUTPUT neighbours, so a repeated source pixel has none inside its block
    raw = np.array([[1000, 3000]], np.uint16)
    depth, boundary = M.depth16_decode_spec(raw, 1000.0, out_hw=(1, 6))
    assert list(depth[0]) == [1.0] * 3 + [3.0] * 3 and list(boundary[0]) == [0, 0, 1, 1, 0, 0]
    # through a window: a step at the window's edge is outside it
    raw = np.array([[9000, 1000, 1000, 9000]], np.uint16)
    assert list(M.depth16_decode_spec(raw, 256.0, window=(0, 1, 1, 2))[1][0]) == [0, 0]
    assert list(M.depth16_decode_spec(raw, 256.0)[1][0]) == [1, 1, 1, 1]


def test_scenes_hold_what_the_tests_need():
    from patchrefinerv2_amd import metrics as M
    for i in range(KITTI_FRAMES):
        raw = kitti_samples(*KITTI_SHAPE, seed=i, empty_crop=(i == 1))
        depth, boundary = kitti_host_route(raw)
        y0, y1, x0, x1 = M._eval_crop(*KB, True, False, "kitti")
        valid = (depth > 1e-3) & (depth < 80)
        assert valid.any() and boundary.any() and (depth == 0).mean() > 0.5  # sparse
        assert bool(valid[y0:y1, x0:x1].any()) == (i != 1)                   # frame 1: nothing valid inside the Garg crop
    for shape, out, seed in ((SCANNET_DEPTH, SCANNET_IMG, SCANNET_SEED), (SCANNET_CLI_DEPTH, SCANNET_CLI_IMG, SCANNET_CLI_SEED)):
        for i in range(SCANNET_FRAMES):
            depth, boundary = scannet_host_route(scannet_samples(*shape, seed=seed + i), out)
            region = M.edge_split_masks(depth)
            valid = (depth > 1e-3) & (depth < 80)
            assert boundary.any() and (region & valid).sum() > 50 and (~region & valid).sum() > 50 and (depth == 0).any()


def test_no_scannet_scene_has_a_pixel_near_a_canny_threshold():
    """the condition under which the device's edge area equals the host's pixel for pixel: the device's logarithm may differ from
    torch's in the last bit, so no gradient magnitude of the log ground truth may lie near 0.1 or 0.2, and the host detector must give
    the same edges for maps one ulp away"""
    from patchrefinerv2_amd import metrics as M
    rs = np.random.RandomState(0)
    for shape, out, seed in ((SCANNET_DEPTH, SCANNET_IMG, SCANNET_SEED), (SCANNET_CLI_DEPTH, SCANNET_CLI_IMG, SCANNET_CLI_SEED)):
        for i in range(SCANNET_FRAMES):
            depth, _ = scannet_host_route(scannet_samples(*shape, seed=seed + i), out)
            log = M.preprocess_depth(depth, "log")
            # one ulp of a log below 4 is 2.4e-7; the smoothing's weights sum to one and Sobel's absolute weights to 8: a derivative
            # moves by less than 2e-6, the magnitude by less than 3e-6 -- 1e-4 leaves thirty times that
            assert canny_margin(log) > 1e-4, (shape, i, canny_margin(log))
            want = M.canny(log)
            assert 0 < want.mean() < 0.5
            for _ in range(8):
                moved = np.nextafter(log, np.where(rs.rand(*log.shape) < 0.5, np.float32(-np.inf), np.float32(np.inf)).astype(np.float32))
                moved[log == 0] = 0
                assert np.array_equal(M.canny(moved), want), (shape, i)


# ------------------------------------------------------------------------------------------------------------------ the classes
def test_dataset_classes_are_reexported_and_no_registry_entries():
    from patchrefinerv2_amd import datasets, tester
    from patchrefinerv2_amd.registry import DATASETS
    assert tester.KittiDataset is datasets.KittiDataset and tester.ScanNetDataset is datasets.ScanNetDataset
    assert tester.KittiDataset.dataset_name == "kitti" and tester.ScanNetDataset.dataset_name == "scannet"
    assert "KittiDataset" not in DATASETS and "ScanNetDataset" not in DATASETS
    assert "kitti" not in datasets.GT_FORMATS and datasets.KB_CROP == KB


def test_kitti_split_parsing(tmp_path):
    root = str(tmp_path)
    split, items = write_kitti_tree(root, shape=(8, 16))
    ds = _kitti(root, split, patch_raw_shape=[88, 152], pre_norm_bbox=False, do_kb_crop=False, pseudo_label_path="/nowhere")
    lines = open(split).read().splitlines()
    assert len(lines) == KITTI_FRAMES + 1 and " None " in lines[0] and lines[1].startswith(items[-1]["rel"])  # a None line; reverse order
    assert len(ds) == KITTI_FRAMES and [i["img_path"] for i in ds.data_infos] == sorted(it["img"] for it in items)
    for info, it in zip(ds.data_infos, items):
        assert info["img_path"] == os.path.join(root, "raw", it["rel"]) == it["img"]
        assert info["depth_map_path"] == os.path.join(root, "depth", it["rel_depth"]) == it["depth"] and info["filename"] == it["rel"]
        assert info["img_file_basename"] == os.path.splitext(it["rel"])[0].replace("/", "_")
    assert ds.data_infos[0]["img_file_basename"] == "2011_09_26_2011_09_26_drive_0002_sync_image_02_data_0000000000"
    assert (ds.patch_raw_shape, ds.pre_norm_bbox, ds.do_kb_crop, ds.min_depth, ds.max_depth, ds.mode) == ((88, 152), False, False, 1e-3, 80, "infer")
    assert _kitti(root, split).do_kb_crop is True and _kitti(root, split).patch_raw_shape == (176, 304)


def test_scannet_split_parsing_and_the_basename_hack(tmp_path):
    from patchrefinerv2_amd import tester
    split, items = write_scannet_tree(str(tmp_path))
    ds = _scannet(split, patch_raw_shape=[360, 480], pre_norm_bbox=False)
    assert open(split).read().splitlines()[0].startswith(items[-1]["img"])
    assert len(ds) == SCANNET_FRAMES and [i["img_path"] for i in ds.data_infos] == [it["img"] for it in items]
    assert [i["depth_map_path"] for i in ds.data_infos] == [it["depth"] for it in items]
    assert [i["img_file_basename"] for i in ds.data_infos] == [f"{SCANNET_SCENE}_000000", f"{SCANNET_SCENE}_000120"]
    # the reference's expressions on a literal path of its own split file (scannet_dataset.py:191-193)
    path = "/ibex/ai/home/liz0l/codes/datasets/scannet_pp_select_val_lr/data/7b6477cb95/iphone/rgb/frame_004560.jpg"
    base = os.path.splitext(path)[0].replace("/", "_")[1:]
    assert tester.ScanNetDataset.basename_of(path) == base[-34:-24] + "_" + base[-6:] == "7b6477cb95_004560"
    assert (ds.patch_raw_shape, ds.pre_norm_bbox) == ((360, 480), False) and _scannet(split).patch_raw_shape == (720, 960)


def test_unbuilt_modes_raise(tmp_path):
    root = str(tmp_path)
    ksplit, _ = write_kitti_tree(os.path.join(root, "k"), n=1, shape=(8, 16))
    ssplit, _ = write_scannet_tree(os.path.join(root, "s"), n=1)
    for make, cite in ((lambda **kw: _kitti(os.path.join(root, "k"), **dict(dict(split=ksplit), **kw)), "kitti_dataset.py"),
                       (lambda **kw: _scannet(**dict(dict(split=ssplit), **kw)), "scannet_dataset.py")):
        with pytest.raises(NotImplementedError, match=rf"train.*{cite}"):
            make(mode="train")
        with pytest.raises(NotImplementedError, match=rf"random_crop.*{cite}"):
            make(transform_cfg=dict(_tc(), random_crop=True, random_crop_size=[176, 304]))
        with pytest.raises(NotImplementedError, match=rf"with_pseudo_label.*{cite}"):
            make(with_pseudo_label=True, pseudo_label_path=root)
        with pytest.raises(NotImplementedError, match="bicubic"):
            make(resize_mode="bicubic")
        with pytest.raises(NotImplementedError):
            make(split=None)


def test_kitti_reader_fills_the_slot_and_names_malformed_files(tmp_path):
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    root = str(tmp_path)
    split, items = write_kitti_tree(root, n=2)
    ds = _kitti(root, split)
    slot = host_slot(KITTI_SHAPE)
    ds._read(1, slot)
    it = items[1]
    assert slot["shape"] == KITTI_SHAPE and slot["img_shape"] == KB
    assert np.array_equal(slot["depth"].numpy().view(np.uint16).reshape(KITTI_SHAPE), it["raw"])  # uncropped
    top, left = KITTI_SHAPE[0] - 352, (KITTI_SHAPE[1] - 1216) // 2
    assert np.array_equal(slot["img"].numpy()[:352 * 1216 * 3].reshape(KB + (3,)), it["pixels"][top:top + 352, left:left + 1216])
    plain = _kitti(root, split, do_kb_crop=False)
    plain._read(1, slot)
    assert slot["img_shape"] == KITTI_SHAPE and np.array_equal(slot["img"].numpy().reshape(KITTI_SHAPE + (3,)), it["pixels"])

    def fails(path, dataset=ds):
        with pytest.raises(ValueError, match=re.escape(path)):
            dataset._read(0, host_slot(KITTI_SHAPE))
    it = items[0]
    Image.fromarray((it["raw"] >> 8).astype(np.uint8)).save(it["depth"])  # an 8-bit depth file
    fails(it["depth"])
    with pytest.raises(ValueError, match="KITTI depth map is 16-bit greyscale"):
        ds._read(0, host_slot(KITTI_SHAPE))
    write_png16(it["depth"], it["raw"])
    ds._read(0, host_slot(KITTI_SHAPE))
    Image.fromarray(it["pixels"][:-1]).save(it["img"])  # an image of another size
    fails(it["img"])
    Image.fromarray(it["pixels"][:300]).save(it["img"])  # image and depth agree, and are smaller than the crop
    write_png16(it["depth"], it["raw"][:300])
    fails(it["depth"])
    with pytest.raises(ValueError, match="smaller than the kb-crop"):
        ds._read(0, host_slot(KITTI_SHAPE))
    plain._read(0, host_slot(KITTI_SHAPE))  # (without the crop every size will do)


def test_scannet_reader_fills_the_slot_and_names_malformed_files(tmp_path):
    from PIL import Image
    split, items = write_scannet_tree(str(tmp_path))
    ds = _scannet(split)
    slot = host_slot(SCANNET_DEPTH, SCANNET_IMG)
    ds._read(1, slot)
    it = items[1]
    assert slot["shape"] == SCANNET_DEPTH and slot["img_shape"] == SCANNET_IMG  # the samples at their own size
    assert np.array_equal(slot["depth"].numpy().view(np.uint16).reshape(SCANNET_DEPTH), it["raw"])
    assert np.array_equal(slot["img"].numpy().reshape(SCANNET_IMG + (3,)), it["pixels"])
    it = items[0]
    Image.fromarray((it["raw"] >> 4).astype(np.uint8)).save(it["depth"])
    with pytest.raises(ValueError, match=re.escape(it["depth"])):
        ds._read(0, host_slot(SCANNET_DEPTH, SCANNET_IMG))
    Image.fromarray(np.dstack([it["pixels"], np.full(SCANNET_IMG, 255, np.uint8)]), "RGBA").save(it["img"])  # convert("RGB") drops the alpha
    slot = host_slot(SCANNET_DEPTH, SCANNET_IMG)
    with pytest.raises(ValueError):
        ds._read(0, slot)
    assert np.array_equal(slot["img"].numpy().reshape(SCANNET_IMG + (3,)), it["pixels"])


def test_evaluate_is_the_nanmean(tmp_path):
    import warnings
    root = str(tmp_path)
    ksplit, _ = write_kitti_tree(os.path.join(root, "k"), n=1, shape=(8, 16))
    ssplit, _ = write_scannet_tree(os.path.join(root, "s"), n=1)
    nan = float("nan")
    for ds, keys in ((_kitti(os.path.join(root, "k"), ksplit), KEYS10), (_scannet(ssplit), KEYS30)):
        rows = [{k: 1.0 + i for i, k in enumerate(keys)}, {k: nan for k in keys}, {k: 4.0 + i for i, k in enumerate(keys)}]
        rows[1]["see"] = 0.0  # a frame with an empty Garg crop: NaN keys, see 0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ev = ds.evaluate(rows)
        assert tuple(ev) == keys and ev["a1"] == (rows[0]["a1"] + rows[2]["a1"]) / 2 and all(np.isfinite(v) for v in ev.values())
        for k in keys:
            assert ev[k] == float(np.nanmean([r[k] for r in rows]))
    sc = _scannet(ssplit)
    assert sc.evaluate_consistency([dict(consistency_error=0.25), dict(consistency_error=nan), dict(consistency_error=0.75)]) == dict(consistency_error=0.5)
    assert not hasattr(_kitti(os.path.join(root, "k"), ksplit), "evaluate_consistency")


def test_cli_test_types_build_the_datasets(tmp_path):
    from patchrefinerv2_amd import tester
    from patchrefinerv2_amd.registry import DATASETS, Config
    cli = cli_module()
    kroot = str(tmp_path / "kitti")
    ksplit, _ = write_kitti_tree(kroot, n=2, shape=(8, 16))
    ssplit, _ = write_scannet_tree(str(tmp_path / "scannet"))
    kcfg, scfg = tmp_path / "kitti.py", tmp_path / "scannet.py"
    kcfg.write_text(kitti_config_text(kroot, ksplit))
    scfg.write_text(scannet_config_text(ssplit))
    for cfg_path, kind, cls, other in ((kcfg, "kitti", tester.KittiDataset, scfg), (scfg, "scannet", tester.ScanNetDataset, kcfg)):
        cfg = Config.fromfile(str(cfg_path))
        ns = dict(config=str(cfg_path), image_raw_shape=[8, 16], edge_metrics=True, ssi_metrics=True)
        d = cli.dataset_config(cfg, argparse.Namespace(test_type=kind, **ns))
        assert d["type"] == cls.__name__ and d["ssi_metrics"] is True
        assert "image_resolution" not in d and "image_raw_shape" not in d and "edge_metrics" not in d  # only --ssi-metrics goes in
        ds = cli_dataset(cfg_path, kind, ssi_metrics=True)
        assert type(ds) is cls and len(ds) == 2 and ds.ssi_metrics and ds.max_depth == 80 and ds.mode == "infer"
        assert not cli_dataset(cfg_path, kind).ssi_metrics
        assert cls.__name__ not in DATASETS  # built by its constructor
        # another dataset under this test type is refused; --test-type normal still reports the type as not built, with a hint
        with pytest.raises(SystemExit, match=rf"--test-type {kind} needs val_dataloader.dataset.type = '{cls.__name__}'"):
            cli.dataset_config(Config.fromfile(str(other)), argparse.Namespace(test_type=kind, **ns))
        with pytest.raises(SystemExit, match=rf"{cls.__name__} is not built .*cityscapes, kitti, scannet and eth.*--test-type {kind}"):
            cli.dataset_config(cfg, argparse.Namespace(test_type="normal", **ns))
        assert f"--test-type {kind}" in cli.__doc__
    u4k = Config.fromfile(os.path.join(ROOT, "configs", "v2_dav2_mobile_u4k.py"))
    with pytest.raises(SystemExit, match="needs val_dataloader.dataset.type = 'KittiDataset'"):
        cli.dataset_config(u4k, argparse.Namespace(test_type="kitti", config="u4k", image_raw_shape=[8, 16], edge_metrics=False))
    assert cli_dataset(kcfg, "kitti").do_kb_crop is True and cli_dataset(kcfg, "kitti").data_root == kroot


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_is_declared_bound_and_exported():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    s = "prv2_depth16_gt"
    assert s in L.SIGNATURES and re.search(rf"\bint {s}\(", hdr) and hasattr(raw, s)
    args = re.search(rf"\bint {s}\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(args.split(",")) == len(L.SIGNATURES[s][1]) == 13
    for cite in ("kitti_dataset.py:123-131", "scannet_dataset.py:112-118"):
        assert cite in hdr  # the entry cites its reference lines
    assert L.ABI_VERSION == 20 and L.load().prv2_abi_version() == L.ABI_VERSION and "#define PRV2_ABI_VERSION 20" in hdr
    t = torch_ops.load()
    assert "depth16_gt" in torch_ops.OPS and hasattr(t, "depth16_gt") and hasattr(ops, "depth16_gt")
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.depth16_gt(torch.zeros(4, 4, dtype=torch.uint16), 4, 4, 256.0, 0, 0, False, 1.0)
    with pytest.raises(ValueError, match="GPU"):
        ops.depth16_gt(torch.zeros(4, 4, dtype=torch.uint16), (4, 4), 256.0)


def test_entry_point_rejects_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null, aligned address that is never dereferenced: every call below fails its checks first

    def err(code):
        assert code != 0
        return lib.prv2_last_error()

    def call(src=P, sh=9, sw=14, grid=0, top=4, left=3, H=5, W=7, divisor=256.0, depth=P, boundary=P):
        return lib.prv2_depth16_gt(src, sh, sw, grid, top, left, H, W, divisor, 1.0, depth, boundary, None)
    assert b"null" in err(call(src=None)) and b"null" in err(call(depth=None)) and b"null" in err(call(boundary=None))
    assert b"source shape" in err(call(sh=0)) and b"source shape" in err(call(sw=-1))
    assert b"output shape" in err(call(H=0)) and b"output shape" in err(call(W=-3))
    assert b"2^31" in err(call(sh=65536, sw=32768)) and b"2^31" in err(call(grid=1, top=0, left=0, H=65536, W=32768))
    assert b"unknown grid" in err(call(grid=2))
    for kw in (dict(top=5), dict(left=8), dict(top=-1), dict(left=-1), dict(H=6), dict(W=12), dict(top=2147483647), dict(left=2147483647)):
        assert b"outside" in err(call(**kw)), kw
    assert b"no window offset" in err(call(grid=1, top=1, left=0)) and b"no window offset" in err(call(grid=1, top=0, left=2))
    assert b"not positive" in err(call(divisor=0.0)) and b"not positive" in err(call(divisor=-256.0)) and b"not positive" in err(call(divisor=float("nan")))
    assert b"depth16_gt" in lib.prv2_last_error()
