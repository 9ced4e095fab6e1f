"""CPU: CityScapesDataset without a GPU -- the specification of its device work and the host half of the class.

``decode_spec_cs`` restates cityscapes_dataset.py:153-174 and :300 in numpy with the reference's own slices.  The specification of the
segmentation-edge detector is metrics.seg_canny (kornia is not installed: its parity is unpinned, the restatement is the
specification); its two rules that replace library calls are checked here against what they replace -- the axis rule against
round(atan2 * 4 / pi) in float64, the connected-component hysteresis against an explicit iteration of kornia's loop.  The generators
of the synthetic tree (``write_cityscapes_tree``) and of the test scenes are shared with tests/test_cityscapes_gpu.py."""
import argparse
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from test_eth_dataset_host import gradient_sum
from test_general_gt_host import boundaries_spec, decode_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prv2_cityscapes_gt", "prv2_seg_canny", "prv2_cityscapes_masks")
NEW_OPS = ("cityscapes_gt", "seg_canny", "cityscapes_masks")
KEYS17 = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see",
          "EdgeAcc", "EdgeComp", "precision", "recall", "f1_score", "hamming", "acc")  # cityscapes_dataset.py:422-440
SKY, BUILDING, ROAD, PERSON, CAR, POLE = (70, 130, 180), (70, 70, 70), (128, 64, 128), (220, 20, 60), (0, 0, 142), (153, 153, 153)
CS_SHAPE, CS_FRAMES, CS_SEED = (64, 128), 2, 4  # the synthetic tree of the dataset / CLI tests on the GPU
CS_BASELINE, CS_FX = 0.209313, 2262.52          # a Cityscapes camera; frame i has fx + 10 i


# ------------------------------------------------------------------------------------------------------------------ scenes
def seg_scene(h, w, seed=0):
    """a colour segmentation map, uint8 [h, w, 3], piecewise constant: a vertical boundary (road | building: R == 70, G != 130) and a
    horizontal one (sky above road) that both reach the frame's border, a diagonal one (person), a curved one (car), a one-pixel-wide
    pole, and a region of the sky colour"""
    y, x = np.mgrid[0:h, 0:w]
    s = np.empty((h, w, 3), np.uint8)
    s[:] = ROAD
    o = seed % 5
    s[(y < 0.3 * h) & (x < 0.55 * w + o)] = SKY
    s[x >= 0.55 * w + o] = BUILDING
    s[(y >= 0.3 * h) & (x * h + y * w < 0.45 * h * w + o * h)] = PERSON
    s[np.hypot(y - 0.62 * h, x - 0.36 * w - o) < 0.17 * min(h, w)] = CAR
    s[h // 5:(4 * h) // 5, min(int(0.8 * w) + o, w - 1)] = POLE
    return s


def disp_scene(seg, seed=0):
    """uint16 disparity samples of a segmentation scene: one disparity per class (sky: none) and a few zeros (invalid samples)"""
    h, w = seg.shape[:2]
    d = np.full((h, w), 12.0)
    for colour, v in ((SKY, 0.0), (BUILDING, 7.0), (PERSON, 55.0), (CAR, 31.0), (POLE, 20.0)):
        d[(seg == np.array(colour, np.uint8)).all(-1)] = v
    raw = np.where(d > 0, np.round(d * 256) + 1, 0).astype(np.uint16)
    rs = np.random.RandomState(100 + seed)
    raw.reshape(-1)[rs.permutation(h * w)[:max(1, h * w // 200)]] = 0
    return raw


def image_scene(h, w, seed=0):
    """a photograph, uint8 [h, w, 3]: flat colour blocks of another layout than the segmentation map and a faint ramp"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.full((h, w, 3), 90, np.int32) + (x * 12 // max(w, 1))[..., None]
    img[(x > 0.3 * w + seed) & (y > 0.55 * h)] += np.array([60, 40, 10])
    img[np.hypot(y - 0.3 * h, x - 0.7 * w) < 0.2 * min(h, w)] += np.array([20, 80, 50])
    return img.astype(np.uint8)


def decode_spec_cs(disp_u16, seg_u8, factor):
    """cityscapes_dataset.py:153-174, :300 -> (depth float32, boundary uint8, seg float32 [3, h, w] or None); the band slices are
    the reference's own expressions"""
    depth, _ = decode_spec("cityscapes", disp_u16, factor=factor)
    depth = depth.copy()
    h, w = depth.shape
    depth[-h // 4:, :] = -1.
    depth[:, :w // 16] = -1.
    depth[:, -w // 16:] = -1.
    seg = None
    if seg_u8 is not None:
        depth[np.logical_and(seg_u8[:, :, 0] == 70, seg_u8[:, :, 1] == 130)] = 0
        seg = np.ascontiguousarray((seg_u8.astype(np.float32) / 1.0).transpose(2, 0, 1))
    return depth, boundaries_spec(depth, 1.0), seg


def seg_canny_spec(seg):
    from patchrefinerv2_amd import metrics as M
    return M.seg_canny(seg)


def masks_spec(seg_edges, gt_edges, hr_region):
    from patchrefinerv2_amd import metrics as M
    return M.cityscapes_masks(seg_edges, gt_edges, hr_region)


def cs_factor(i):
    return float(np.float32(CS_BASELINE * (CS_FX + 10 * i)))


def write_cityscapes_tree(root, n, shape, seed=CS_SEED, with_seg=True):
    """a synthetic Cityscapes tree under ``root``: leftImg8bit / disparity / gtFine / camera folders of one city, a split file of
    'img disp' lines relative to the root written in REVERSE order (the dataset sorts by image path) -> (split path, [dict(img, disp,
    seg, camera: absolute paths; rel: the split's image name; pixels, raw, seg_u8: the arrays; factor)] sorted by image path)"""
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    items = []
    for kind in ("leftImg8bit", "disparity", "gtFine", "camera"):
        os.makedirs(os.path.join(root, kind, "val", "ulm"), exist_ok=True)
    for i in range(n):
        stem = f"val/ulm/ulm_{i:06d}_000019"
        rel_img, rel_disp = f"leftImg8bit/{stem}_leftImg8bit.png", f"disparity/{stem}_disparity.png"
        it = dict(rel=rel_img, rel_disp=rel_disp, img=os.path.join(root, rel_img), disp=os.path.join(root, rel_disp),
                  seg=os.path.join(root, f"gtFine/{stem}_gtFine_color.png"), camera=os.path.join(root, f"camera/{stem}_camera.json"))
        it["seg_u8"] = seg_scene(*shape, seed=seed + i)
        it["raw"], it["pixels"], it["factor"] = disp_scene(it["seg_u8"], seed + i), image_scene(*shape, seed=seed + i), cs_factor(i)
        Image.fromarray(it["pixels"]).save(it["img"])
        write_png16(it["disp"], it["raw"])
        if with_seg:  # (the dataset's colour maps are RGBA files)
            Image.fromarray(np.dstack([it["seg_u8"], np.full(shape, 255, np.uint8)]), "RGBA").save(it["seg"])
        with open(it["camera"], "w") as f:
            json.dump(dict(extrinsic=dict(baseline=CS_BASELINE, pitch=0.03, x=1.7), intrinsic=dict(fx=CS_FX + 10 * i, fy=2265.3, u0=1096.9)), f)
        items.append(it)
    split = os.path.join(root, "val.txt")
    with open(split, "w") as f:
        for it in reversed(items):
            f.write(f"{it['rel']} {it['rel_disp']}\n")
    return split, sorted(items, key=lambda it: it["img"])


def cityscapes_config_text(root, split, extra=""):
    """the project's small config with a CityScapesDataset as its val_dataloader (the keys of configs/_base_/datasets/cityscapes.py)"""
    return (f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n{extra}"
            f"val_dataloader = dict(_delete_=True, batch_size=1, num_workers=1, dataset=dict(type='CityScapesDataset', mode='infer', "
            f"with_seg_map=True, data_root={root!r}, split={split!r}, min_depth=1e-3, max_depth=250, resize_mode='depth-anything', "
            f"transform_cfg=dict(degree=1.0, network_process_size=[384, 512])))\n")


def cli_module():
    spec = importlib.util.spec_from_file_location("prv2_tools_test_cityscapes", os.path.join(ROOT, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def cli_dataset(cfg_path, **ns):
    """the dataset ``tools/test.py CONFIG --test-type cityscapes`` builds"""
    from patchrefinerv2_amd.registry import Config
    cli = cli_module()
    args = argparse.Namespace(**dict(dict(test_type="cityscapes", config=str(cfg_path), image_raw_shape=[8, 16], edge_metrics=False), **ns))
    return cli.build_dataset(cli.dataset_config(Config.fromfile(str(cfg_path)), args))


def _dataset(root, split, **kw):
    """the dataset with the keys of configs/_base_/datasets/cityscapes.py's val_dataloader (built by its class: it is no registry entry)"""
    from patchrefinerv2_amd import tester
    cfg = dict(mode="infer", split=split, data_root=root, with_seg_map=True, min_depth=1e-3, max_depth=250,
               transform_cfg=dict(degree=1.0, network_process_size=[384, 512]))
    cfg.update(kw)
    return tester.CityScapesDataset(**cfg)


def host_slot(shape, with_seg=True):
    """a staging slot in plain host memory (the dataset's own are pinned, which needs a GPU)"""
    px = shape[0] * shape[1]
    return dict(img=torch.empty(px * 3, dtype=torch.uint8), disp=torch.empty(px * 2, dtype=torch.uint8),
                seg=torch.empty(px * 3, dtype=torch.uint8) if with_seg else None, shape=None, factor=None)


# ------------------------------------------------------------------------------------------------------------------ the spec
def test_scenes_hold_what_the_detector_must_face():
    s = seg_scene(37, 53)
    colours = {tuple(c) for c in s.reshape(-1, 3)}
    assert colours == {SKY, BUILDING, ROAD, PERSON, CAR, POLE}
    assert ((s[:, :, 0] == 70) & (s[:, :, 1] == 130)).any() and ((s[:, :, 0] == 70) & (s[:, :, 1] != 130)).any()
    pole = (s == np.array(POLE, np.uint8)).all(-1)
    assert pole.any(1).sum() > 5 and pole.sum(1).max() == 1  # one pixel wide
    assert (s[0] != s[0, 0]).any() and (s[:, 0] != s[0, 0]).any()  # boundaries reach the border
    e = seg_canny_spec(s.transpose(2, 0, 1).astype(np.float32))
    assert e.dtype == bool and e.shape == (37, 53) and 0 < e.mean() < 0.5
    raw = disp_scene(s)
    assert raw.dtype == np.uint16 and (raw == 0).any() and (raw > 256).any()


@pytest.mark.parametrize("h,w", [(3, 9), (3, 3), (4, 16), (5, 17), (8, 16), (37, 53), (64, 128), (1024, 2048)])
def test_band_rule_is_pythons_floor_division(h, w):
    """-h // 4 = -ceil(h / 4), w // 16 and -w // 16 = -ceil(w / 16): w < 16 clears no left column and still the last one"""
    raw = np.full((h, w), 2561, np.uint16)
    depth, boundary, seg = decode_spec_cs(raw, None, 100.0)
    band = depth == -1
    rows, left, right = -(-h // 4), w // 16, -(-w // 16)
    want = np.zeros((h, w), bool)
    want[h - rows:] = True
    want[:, :left] = True
    want[:, w - right:] = True
    assert seg is None and np.array_equal(band, want) and rows >= 1 and right >= 1
    if w < 16:
        assert not band[0, 0] or h - rows == 0
        assert band[:, -1].all() and not band[:h - rows, :w - 1].any()
    assert (depth[~band] == np.float32(100.0) / np.float32(10)).all()
    assert np.array_equal(boundary, boundaries_spec(depth))


def test_sky_is_cleared_after_the_bands_and_building_is_kept():
    h, w = 37, 53
    s = seg_scene(h, w)
    s[-1, :5], s[-1, 5:9] = SKY, BUILDING  # inside the bottom band
    depth, boundary, seg = decode_spec_cs(disp_scene(s), s, cs_factor(0))
    sky, building = (s == np.array(SKY, np.uint8)).all(-1), (s == np.array(BUILDING, np.uint8)).all(-1)
    assert (depth[sky] == 0).all() and (depth[-1, :5] == 0).all() and (depth[-1, 5:9] == -1).all()
    assert (depth[building & (depth != -1)] >= 0).all() and (depth[building] > 0).any()
    assert seg.dtype == np.float32 and seg.shape == (3, h, w) and seg.max() == 220 and np.array_equal(seg[:, 0, 0], np.float32(SKY))
    assert boundary.dtype == np.uint8 and 0 < boundary.mean() < 0.5


def kornia_hysteresis_loop(weak, strong):
    """kornia.filters.canny's hysteresis, iterated as it is written there: edges = 0.5 weak + 0.5 strong; until nothing changes, a
    0.5 pixel with a 1 among its eight neighbours (zero padding) becomes 1; what is 1 at the end is the result"""
    edges = 0.5 * weak.astype(np.float32) + 0.5 * strong.astype(np.float32)
    old = -np.ones_like(edges)
    h, w = edges.shape
    rounds = 0
    while (old != edges).any():
        wk, st = edges == 0.5, edges == 1
        p = np.pad(st, 1)
        near = np.zeros((h, w), bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    near |= p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        hm = ((near & wk) | st).astype(np.float32)
        old = edges
        edges = hm + (hm == 0) * wk * np.float32(0.5)
        rounds += 1
    return hm == 1, rounds


def test_hysteresis_is_the_fixed_point_of_kornias_loop():
    from patchrefinerv2_amd import metrics as M
    mag = np.zeros((24, 40), np.float32)
    mag[2, 2:30] = 0.15                      # a weak-only ridge: dropped
    mag[6, 2:30], mag[6, 29] = 0.15, 0.5     # a weak ridge attached to one strong pixel at its end: kept, over 27 rounds
    mag[10:20, 35] = 0.15                    # a weak ridge touching a strong pixel diagonally
    mag[9, 36] = 0.3
    mag[22, 0], mag[23, 1] = 0.3, 0.15       # in the corner
    mag[14, 10] = 0.3                        # a strong pixel alone
    mag[16, 5:8] = 0.1                       # at the low threshold: not weak
    weak, strong = mag > np.float32(0.1), mag > np.float32(0.2)
    want, rounds = kornia_hysteresis_loop(weak, strong)
    got = M.seg_canny_hysteresis(weak, strong)
    assert np.array_equal(got, want) and rounds > 20
    assert not got[2].any() and got[6, 2:30].all() and got[10:20, 35].all() and got[23, 1] and got[14, 10] and not got[16, 5:8].any()
    rs = np.random.RandomState(3)
    for dens in (0.1, 0.3, 0.6):
        weak = rs.rand(33, 47) < dens
        strong = weak & (rs.rand(33, 47) < 0.1)
        assert np.array_equal(M.seg_canny_hysteresis(weak, strong), kornia_hysteresis_loop(weak, strong)[0]), dens
    assert not M.seg_canny_hysteresis(np.zeros((4, 5), bool), np.zeros((4, 5), bool)).any()


def test_axis_rule_equals_rounded_atan2():
    """kornia: round(atan2(gy, gx) * 4 / pi) mod 4 picks 0: (x + 1, y), 1: (x + 1, y + 1), 2: (x, y + 1), 3: (x - 1, y + 1) and the
    opposite neighbour -- the axes 0, 2, 1, 3 of metrics.seg_canny_axis"""
    from patchrefinerv2_amd import metrics as M
    rs = np.random.RandomState(0)
    gx = (rs.randn(200000) * 10.0 ** rs.randint(-3, 3, 200000)).astype(np.float32)
    gy = (rs.randn(200000) * 10.0 ** rs.randint(-3, 3, 200000)).astype(np.float32)
    ang = np.arctan2(gy.astype(np.float64), gx.astype(np.float64))
    dist = np.minimum((ang - np.pi / 8) % (np.pi / 4), np.pi / 4 - (ang - np.pi / 8) % (np.pi / 4))
    keep = dist > 1e-6
    assert keep.mean() > 0.99
    sector = np.round(ang * 4 / np.pi).astype(np.int64) % 4
    want = np.array([0, 2, 1, 3], np.uint8)[sector]
    got = M.seg_canny_axis(gx, gy)
    assert got.dtype == np.uint8 and np.array_equal(got[keep], want[keep])
    assert set(np.unique(got)) == {0, 1, 2, 3}
    f = np.float32
    cases = [(0, 0, 0), (3, 0, 0), (-3, 0, 0), (0, 2, 1), (0, -2, 1), (1, 1, 2), (-1, -1, 2), (1, -1, 3), (-1, 1, 3), (5, 2, 0), (2, 5, 1)]
    for x, y, k in cases:
        assert int(M.seg_canny_axis(np.array([f(x)]), np.array([f(y)]))[0]) == k, (x, y)
    assert M.SEG_CANNY_TAN_PI_8.dtype == np.float32 and float(M.SEG_CANNY_TAN_PI_8) == float(np.float32(0.414213568))  # the kernel's literal


def test_seg_canny_spec_properties():
    from patchrefinerv2_amd import metrics as M
    w5 = M.seg_canny_weights()
    assert w5.dtype == np.float32 and w5.shape == (5,) and np.array_equal(w5, w5[::-1]) and abs(float(w5.sum()) - 1) < 1e-6
    assert abs(float(w5[2]) - 0.40262) < 1e-5 and abs(float(w5[0]) - 0.054489) < 1e-5
    flat = np.full((3, 7, 9), 128, np.float32)
    assert not M.seg_canny(flat).any()  # mag = sqrt(1e-6) = 1e-3 everywhere: never a maximum
    for shape in ((2, 9), (9, 2)):
        with pytest.raises(ValueError, match="3 x 3"):
            M.seg_canny(np.zeros((3,) + shape, np.float32))
    s = seg_scene(37, 53).transpose(2, 0, 1).astype(np.float32)
    e = M.seg_canny(s)
    assert np.array_equal(e, M.seg_canny(torch.from_numpy(s)[None]))  # [1, 3, H, W] tensors too
    # the two pixels beside an axis-aligned step have mathematically equal magnitudes: the strict > keeps at most one of them (the
    # last bit decides which, and none where the two float32 values are equal)
    x0 = int(np.ceil(0.55 * 53))
    assert ((e[26:34, x0 - 1].astype(int) + e[26:34, x0].astype(int)) <= 1).all() and not e[26:34, x0 - 3].any() and not e[26:34, x0 + 2].any()
    mag, axis = M.seg_canny_magnitude(s)
    assert mag.dtype == np.float32 and axis.dtype == np.uint8 and float(mag.min()) == float(np.sqrt(np.float32(1e-6)))


def test_flatten_and_edge_mask_never_overlap():
    rs = np.random.RandomState(1)
    for shape in ((1, 1), (7, 9), (37, 53)):
        for dens in (0.02, 0.3):
            s, g, r = (rs.rand(*shape) < d for d in (dens, dens, 0.4))
            edge, flatten = masks_spec(s, g, r)
            assert edge.shape == flatten.shape == shape and edge.dtype == flatten.dtype == bool
            assert not (edge & flatten).any() and not (flatten & r).any() and not (edge & ~s).any()
            assert (edge | flatten | r).all()
    g = np.zeros((9, 12), bool)
    g[4, 5] = True
    edge, flatten = masks_spec(np.ones((9, 12), bool), g, np.zeros((9, 12), bool))
    want = np.zeros((9, 12), bool)
    want[1:8, 2:9] = True  # the 7 x 7 window
    assert np.array_equal(edge, want) and np.array_equal(flatten, ~want)
    g[:] = False
    g[0, 0] = True
    assert masks_spec(np.ones((9, 12), bool), g, g)[0].sum() == 16  # clipped at the frame


def test_no_dataset_image_has_a_pixel_near_the_threshold():
    """the condition under which the device's image-edge region (frac 0.05) equals the host's pixel for pixel"""
    for i in range(CS_FRAMES):
        img = torch.from_numpy(image_scene(*CS_SHAPE, seed=CS_SEED + i).astype(np.float32) / np.float32(255)).permute(2, 0, 1).contiguous()
        g64, g32 = gradient_sum(img, torch.float64), gradient_sum(img, torch.float32)
        mx = float(g64.max())
        assert not ((g64 - 0.05 * mx).abs() <= 1e-5 * mx).any()
        assert torch.equal(g32 >= g32.max() * 0.05, g64 >= g64.max() * 0.05)
        assert 0.02 < float((g64 >= 0.05 * mx).float().mean()) < 0.5


# ------------------------------------------------------------------------------------------------------------------ the class
def test_dataset_class_is_reexported():
    from patchrefinerv2_amd import datasets, tester
    assert tester.CityScapesDataset is datasets.CityScapesDataset
    assert tester.CityScapesDataset.dataset_name == "cityscapes" and datasets.CITYSCAPES_METRIC_KEYS == KEYS17


def test_split_parsing_sorting_and_the_three_path_rules(tmp_path):
    root = str(tmp_path)
    split, items = write_cityscapes_tree(root, 3, (8, 16))
    ds = _dataset(root, split, patch_raw_shape=[128, 256], filter_sky=False, pre_norm_bbox=False, base=2.0, filter_thr=0.3)
    assert len(ds) == 3 and [i["img_path"] for i in ds.data_infos] == sorted(it["img"] for it in items)
    assert open(split).read().splitlines()[0].startswith(items[-1]["rel"])  # the file itself is in reverse order
    for info, it in zip(ds.data_infos, items):
        assert info["img_path"] == it["img"] and info["depth_map_path"] == it["disp"] and info["filename"] == it["rel"]
        assert info["camera_info"] == it["camera"] and info["camera_info"].endswith("_camera.json") and os.path.exists(info["camera_info"])
        assert info["seg_map"] == it["seg"] and info["seg_map"].endswith("_gtFine_color.png") and os.path.exists(info["seg_map"])
        assert info["img_file_basename"] == os.path.splitext(it["rel"])[0].replace("/", "_") == "leftImg8bit_val_ulm_" + os.path.basename(it["rel"])[:-4]
    assert (ds.patch_raw_shape, ds.filter_sky, ds.pre_norm_bbox, ds.base, ds.filter_thr) == ((128, 256), False, False, 2.0, 0.3)
    assert (ds.min_depth, ds.max_depth, ds.mode, ds.with_seg_map, ds.data_root) == (1e-3, 250, "infer", True, root)
    plain = _dataset(root, split, with_seg_map=False)
    assert all("seg_map" not in i for i in plain.data_infos) and plain.filter_sky is True and plain.base == float(np.exp(1))


def test_unbuilt_modes_raise(tmp_path):
    root = str(tmp_path)
    split, _ = write_cityscapes_tree(root, 1, (8, 16))
    tc = dict(degree=1.0, network_process_size=[384, 512])
    with pytest.raises(NotImplementedError, match="train"):
        _dataset(root, split, mode="train")
    with pytest.raises(NotImplementedError, match="random_crop"):
        _dataset(root, split, transform_cfg=dict(tc, random_crop=True, random_crop_size=[256, 512]))
    with pytest.raises(NotImplementedError, match="input_size_shallow"):
        _dataset(root, split, transform_cfg=dict(tc, input_size_shallow=[512, 1024]))
    with pytest.raises(NotImplementedError, match="with_pseudo_label"):
        _dataset(root, split, with_pseudo_label=True, pseudo_label_path=root)
    with pytest.raises(NotImplementedError, match="with_uncert"):
        _dataset(root, split, with_uncert=True)
    with pytest.raises(NotImplementedError):
        _dataset(root, split, resize_mode="bicubic")
    with pytest.raises(NotImplementedError):
        _dataset(root, None)


def test_reader_fills_the_slot_and_names_malformed_files(tmp_path):
    from PIL import Image
    from patchrefinerv2_amd import datasets
    root = str(tmp_path)
    shape = (8, 16)
    split, items = write_cityscapes_tree(root, 2, shape)
    ds = _dataset(root, split)
    slot = host_slot(shape)
    ds._read(1, slot)
    it = items[1]
    assert slot["shape"] == shape and slot["factor"] == it["factor"] == float(np.float32(CS_BASELINE * (CS_FX + 10)))
    assert np.array_equal(slot["disp"].numpy().view(np.uint16).reshape(shape), it["raw"])
    assert np.array_equal(slot["img"].numpy().reshape(shape + (3,)), it["pixels"])
    assert np.array_equal(slot["seg"].numpy().reshape(shape + (3,)), it["seg_u8"])  # the RGBA file's RGB bytes
    assert datasets.read_cityscapes_camera(it["camera"]) == it["factor"]

    def fails(path):
        with pytest.raises(ValueError, match=re.escape(path)):
            ds._read(0, host_slot(shape))
    it = items[0]
    Image.fromarray((it["raw"] >> 8).astype(np.uint8)).save(it["disp"])  # an 8-bit disparity file
    fails(it["disp"])
    from patchrefinerv2_amd.output import write_png16
    write_png16(it["disp"], it["raw"])
    ds._read(0, host_slot(shape))
    Image.fromarray(it["seg_u8"][:, :-1]).save(it["seg"])  # a segmentation map of another size
    fails(it["seg"])
    Image.fromarray(it["seg_u8"]).save(it["seg"])
    Image.fromarray(it["pixels"][:-1]).save(it["img"])  # an image of another size
    fails(it["img"])
    Image.fromarray(it["pixels"]).save(it["img"])
    for cam in (dict(extrinsic=dict(pitch=0.0), intrinsic=dict(fx=2262.52)), dict(extrinsic=dict(baseline=0.2), intrinsic=dict(fy=1.0)), dict(), [1]):
        with open(it["camera"], "w") as f:
            json.dump(cam, f)
        fails(it["camera"])


def test_get_metrics_needs_the_segmentation_map_and_the_image(tmp_path):
    root = str(tmp_path)
    split, _ = write_cityscapes_tree(root, 1, (8, 16))
    ds = _dataset(root, split)
    z = torch.zeros(1, 1, 8, 16)
    with pytest.raises(ValueError, match="seg_image"):
        ds.get_metrics(z, z, torch.zeros(8, 16), image_hr=torch.zeros(3, 8, 16))
    with pytest.raises(ValueError, match="image_hr"):
        ds.get_metrics(z, z, torch.zeros(8, 16), seg_image=torch.zeros(3, 8, 16))


def test_evaluate_is_the_nanmean(tmp_path):
    root = str(tmp_path)
    split, _ = write_cityscapes_tree(root, 1, (8, 16))
    ds = _dataset(root, split)
    rows = [{k: 1.0 + i for i, k in enumerate(KEYS17)}, {k: 4.0 + i for i, k in enumerate(KEYS17)}]
    rows[1]["EdgeComp"] = float("nan")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev = ds.evaluate(rows)
    assert tuple(ev) == KEYS17 and ev["EdgeComp"] == rows[0]["EdgeComp"] and ev["a1"] == 2.5
    for k in KEYS17:
        assert ev[k] == float(np.nanmean([r[k] for r in rows]))


def test_cli_test_type_cityscapes_builds_the_dataset(tmp_path):
    from patchrefinerv2_amd import tester
    from patchrefinerv2_amd.registry import Config
    cli = cli_module()
    root = str(tmp_path / "data")
    split, _ = write_cityscapes_tree(root, 2, (8, 16))
    cfg_path = tmp_path / "cfg.py"
    cfg_path.write_text(cityscapes_config_text(root, split))
    cfg = Config.fromfile(str(cfg_path))
    ns = dict(config=str(cfg_path), image_raw_shape=[8, 16], edge_metrics=True, ssi_metrics=True)
    d = cli.dataset_config(cfg, argparse.Namespace(test_type="cityscapes", **ns))
    assert d["type"] == "CityScapesDataset" and "image_resolution" not in d and "image_raw_shape" not in d and "edge_metrics" not in d
    ds = cli_dataset(cfg_path, ssi_metrics=True)
    assert isinstance(ds, tester.CityScapesDataset) and len(ds) == 2 and ds.with_seg_map and ds.ssi_metrics
    assert ds.resize_mode == "depth-anything" and ds.max_depth == 250
    assert not cli_dataset(cfg_path).ssi_metrics
    # another dataset under --test-type cityscapes is refused; --test-type normal points at the route
    u4k = Config.fromfile(os.path.join(ROOT, "configs", "v2_dav2_mobile_u4k.py"))
    with pytest.raises(SystemExit, match="needs val_dataloader.dataset.type = 'CityScapesDataset'"):
        cli.dataset_config(u4k, argparse.Namespace(test_type="cityscapes", **ns))
    with pytest.raises(SystemExit, match="--test-type cityscapes"):
        cli.dataset_config(cfg, argparse.Namespace(test_type="normal", **ns))
    text = open(os.path.join(ROOT, "tools", "test.py")).read()
    assert "--test-type cityscapes" in cli.__doc__ and "cityscapes: " in text.split('"--test-type", default')[1][:900]


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_bound_and_exported():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and re.search(rf"\bint {s}\(", hdr) and hasattr(raw, s), s
        args = re.search(rf"\bint {s}\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[s][1]), s
    for cite in ("cityscapes_dataset.py:153-174", "cityscapes_dataset.py:333-334", "cityscapes_dataset.py:360-365"):
        assert cite in hdr  # each entry cites its reference lines
    assert L.load().prv2_abi_version() == L.ABI_VERSION
    t = torch_ops.load()
    for o in NEW_OPS:
        assert o in torch_ops.OPS and hasattr(t, o) and hasattr(ops, o)
    calls = (lambda: t.cityscapes_gt(torch.zeros(4, 4, dtype=torch.uint16), None, 1.0), lambda: t.seg_canny(torch.zeros(3, 4, 4), [0.2] * 5, 0.1, 0.2),
             lambda: t.cityscapes_masks(torch.zeros(4, 4, dtype=torch.bool), torch.zeros(4, 4, dtype=torch.bool), torch.zeros(4, 4, dtype=torch.uint8)))
    for call in calls:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
    with pytest.raises(ValueError, match="GPU"):
        ops.cityscapes_gt(torch.zeros(4, 4, dtype=torch.uint16), None, 1.0)
    with pytest.raises(ValueError, match="GPU"):
        ops.seg_canny(torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="GPU"):
        ops.cityscapes_masks(torch.zeros(4, 4, dtype=torch.bool), torch.zeros(4, 4, dtype=torch.bool), torch.zeros(4, 4, dtype=torch.uint8))


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null, aligned address that is never dereferenced: every call below fails its checks first

    def err(code):
        assert code != 0
        return lib.prv2_last_error()

    def gt(disp=P, seg=P, h=4, w=4, depth=P, boundary=P, seg_out=P):
        return lib.prv2_cityscapes_gt(disp, seg, h, w, 1.0, depth, boundary, seg_out, None)
    assert b"null" in err(gt(disp=None)) and b"null" in err(gt(depth=None)) and b"null" in err(gt(boundary=None))
    assert b"together" in err(gt(seg=None)) and b"together" in err(gt(seg_out=None))
    assert b"shape" in err(gt(h=0)) and b"shape" in err(gt(w=-1)) and b"2^31" in err(gt(h=32768, w=32768))
    assert b"cityscapes_gt" in lib.prv2_last_error()

    ws = lib.prv2_edges_workspace_bytes(1, 5, 7)
    w5 = (ctypes.c_float * 5)(0.1, 0.2, 0.4, 0.2, 0.1)

    def sc(seg=P, h=5, w=7, gw=ctypes.addressof(w5), edges=P, wsp=P, wsb=ws):
        return lib.prv2_seg_canny(seg, h, w, gw, 0.1, 0.2, edges, wsp, wsb, None)
    assert b"null" in err(sc(seg=None)) and b"null" in err(sc(gw=None)) and b"null" in err(sc(edges=None))
    assert b"3 x 3" in err(sc(h=2)) and b"3 x 3" in err(sc(w=2)) and b"shape" in err(sc(h=0))
    assert b"workspace" in err(sc(wsp=None)) and b"workspace" in err(sc(wsb=ws - 1))
    assert b"seg_canny" in lib.prv2_last_error()

    def mk(s=P, g=P, r=P, h=4, w=4, e=P, f=P):
        return lib.prv2_cityscapes_masks(s, g, r, h, w, e, f, None)
    for kw in (dict(s=None), dict(g=None), dict(r=None), dict(e=None), dict(f=None)):
        assert b"null" in err(mk(**kw))
    assert b"shape" in err(mk(h=0)) and b"2^31" in err(mk(h=65536, w=32768))
    assert b"cityscapes_masks" in lib.prv2_last_error()
