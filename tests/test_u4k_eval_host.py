"""CPU: the U4K dataset evaluation without a GPU -- the split / extrinsics parsing of UnrealStereo4kDataset, the modes that are not
built, the argument checks of the three csrc/evalgt.hip entry points through the C ABI, and tools/test.py --test-type."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prv2_u8_image", "prv2_disp_gt", "prv2_depth_metrics_workspace_bytes", "prv2_depth_metrics")
NEW_OPS = ("u8_image", "disp_gt", "depth_metrics")


def write_u4k_tree(root, frames, shape, seed=0):
    """a synthetic U4K tree: <root>/<scene>/Image0/<n>.raw (BGR bytes), Disp0/<n>.npy, Extrinsics0|1/<n>.txt and splits/val.txt;
    ``frames``: [(scene, number, focal, baseline)] -> the split path (lines in the order given)"""
    h, w = shape
    os.makedirs(os.path.join(root, "splits"), exist_ok=True)
    lines = []
    for k, (scene, num, focal, base) in enumerate(frames):
        rs = np.random.RandomState(seed + k)
        for sub in ("Image0", "Image1", "Disp0", "Disp1", "Extrinsics0", "Extrinsics1"):
            os.makedirs(os.path.join(root, scene, sub), exist_ok=True)
        rs.randint(0, 256, (h, w, 3)).astype(np.uint8).tofile(os.path.join(root, scene, "Image0", f"{num}.raw"))
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        disp = 20.0 + 30.0 * (x > w * 0.4 + 7 * k) + 12.0 * (np.hypot(x - w * 0.6, y - h * 0.5) < h * 0.25) + 0.2 * np.sin(y / 5.0)
        disp[:2] = 0.0  # depth inf: invalid rows
        np.save(os.path.join(root, scene, "Disp0", f"{num}.npy"), disp.astype(np.float32))
        for cam, tx in (("Extrinsics0", 0.25), ("Extrinsics1", 0.25 + base)):
            with open(os.path.join(root, scene, cam, f"{num}.txt"), "w") as f:
                f.write(f"{focal} 0.0 {w / 2} 0.0 {focal} {h / 2} 0.0 0.0 1.0\n1.0 0.0 0.0 {tx} 0.0 1.0 0.0 0.0 0.0 0.0 1.0 0.0\n")
        lines.append(f"{scene}/Image0/{num}.png {scene}/Image1/{num}.png {scene}/Disp0/{num}.npy {scene}/Disp1/{num}.npy")
    split = os.path.join(root, "splits", "val.txt")
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    return split


def _dataset(root, split, shape, **kw):
    from patchrefinerv2_amd.registry import DATASETS
    from patchrefinerv2_amd import tester  # noqa: F401  (registers the datasets)
    cfg = dict(type="UnrealStereo4kDataset", mode="infer", data_root=root, split=split, min_depth=1e-3, max_depth=80,
               transform_cfg=dict(network_process_size=[384, 512]), image_raw_shape=shape)
    cfg.update(kw)
    return DATASETS.build(cfg)


def test_load_data_list_paths_order_basenames_and_depth_factor(tmp_path):
    root = str(tmp_path / "u4k")
    frames = [("00008", "00003", 1200.0, 0.5), ("00001", "00010", 1000.0, 0.25), ("00001", "00002", 1100.5, 0.125)]
    split = write_u4k_tree(root, frames, (6, 8))
    ds = _dataset(root, split, (6, 8))
    assert len(ds) == 3 and ds.dataset_name == "u4k" and (ds.min_depth, ds.max_depth) == (1e-3, 80)
    assert ds.network_process_size == (384, 512)
    infos = ds.data_infos
    # sorted by image path: scene 00001 frame 00002, then 00010, then scene 00008; the basename drops its first character (:155-156)
    assert [i["filename"] for i in infos] == ["00001/Image0/00002.raw", "00001/Image0/00010.raw", "00008/Image0/00003.raw"]
    assert [i["img_file_basename"] for i in infos] == ["0001_Image0_00002", "0001_Image0_00010", "0008_Image0_00003"]
    for i in infos:
        assert i["img_path"] == os.path.join(root, i["filename"]) and i["img_path"].endswith(".raw")
        assert i["depth_map_path"] == os.path.join(root, i["filename"].replace("Image0", "Disp0").replace(".raw", ".npy"))
    want = {"00002": (1100.5, 0.125), "00010": (1000.0, 0.25), "00003": (1200.0, 0.5)}
    for i in infos:
        focal, base = want[i["filename"][-9:-4]]
        assert i["focal"] == focal
        assert i["depth_factor"] == abs(0.25 - (0.25 + base)) * focal  # the reference's own expression (u4k_dataset.py:107-110)


def test_modes_that_are_not_built_raise(tmp_path):
    root = str(tmp_path / "u4k")
    split = write_u4k_tree(root, [("00001", "00002", 1000.0, 0.5)], (4, 4))
    with pytest.raises(NotImplementedError, match="train"):
        _dataset(root, split, (4, 4), mode="train")
    with pytest.raises(NotImplementedError, match="consistency"):
        _dataset(root, split, (4, 4), consistency=True)
    with pytest.raises(NotImplementedError):
        _dataset(root, None, (4, 4))


def test_symbols_are_bound_and_ops_reject_cpu_tensors():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and f"{s}(" in hdr, s
    assert "evalgt.hip" in open(os.path.join(ROOT, "patchrefinerv2_amd", "csrc", "Makefile")).read()
    ops = torch_ops.load()
    for o in NEW_OPS:
        assert o in torch_ops.OPS and hasattr(ops, o)
    f, b = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    calls = [lambda: ops.u8_image(torch.zeros(8, 8, 3, dtype=torch.uint8), True), lambda: ops.disp_gt(f[0], 2.0, 1.0),
             lambda: ops.depth_metrics(f, f, b, None, 0.1, 10.0, 0, 8, 0, 8)]
    for c in calls:
        with pytest.raises((RuntimeError, NotImplementedError)):
            c()


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null address that is never dereferenced: every call below fails its checks first

    def err(code):
        assert code != 0
        return lib.prv2_last_error()
    assert b"null" in err(lib.prv2_u8_image(None, 4, 4, 1, P, None))
    assert b"null" in err(lib.prv2_u8_image(P, 4, 4, 1, None, None))
    assert b"shape" in err(lib.prv2_u8_image(P, 0, 4, 1, P, None))
    assert b"shape" in err(lib.prv2_u8_image(P, 4, -1, 0, P, None))
    assert b"null" in err(lib.prv2_disp_gt(None, 4, 4, 2.0, 1.0, P, P, None))
    assert b"null" in err(lib.prv2_disp_gt(P, 4, 4, 2.0, 1.0, None, P, None))
    assert b"null" in err(lib.prv2_disp_gt(P, 4, 4, 2.0, 1.0, P, None, None))
    assert b"shape" in err(lib.prv2_disp_gt(P, 4, 0, 2.0, 1.0, P, P, None))
    assert b"shape" in err(lib.prv2_disp_gt(P, -4, 4, 2.0, 1.0, P, P, None))
    ws = lib.prv2_depth_metrics_workspace_bytes(2, 16, 24)
    assert ws >= 2 * 3 * 12 * 8 and lib.prv2_depth_metrics_workspace_bytes(0, 16, 24) == -1
    assert lib.prv2_depth_metrics_workspace_bytes(1, 0, 24) == -1 and lib.prv2_depth_metrics_workspace_bytes(1, 16, -2) == -1

    def dm(gt=P, pred=P, n=2, h=16, w=24, crop=(0, 16, 0, 24), sums=P, wsp=P, wsb=ws):
        return lib.prv2_depth_metrics(gt, pred, None, None, n, h, w, 0.1, 10.0, *crop, sums, wsp, wsb, None)
    assert b"null" in err(dm(gt=None))
    assert b"null" in err(dm(pred=None))
    assert b"null" in err(dm(sums=None))
    assert b"workspace" in err(dm(wsp=None))
    assert b"workspace" in err(dm(wsb=ws - 1))
    assert b"frame count" in err(dm(n=0))
    assert b"shape" in err(dm(h=0))
    assert b"shape" in err(dm(w=-3))
    assert b"crop" in err(dm(crop=(0, 17, 0, 24)))
    assert b"crop" in err(dm(crop=(5, 4, 0, 24)))
    assert b"crop" in err(dm(crop=(0, 16, -1, 24)))


def test_crop_rectangles_equal_compute_metrics_masks():
    """metrics._eval_crop: the rectangle of compute_metrics' eval_mask (metric.py:108-120), clipped like numpy's slices"""
    from patchrefinerv2_amd.metrics import _eval_crop
    for h, w in ((48, 64), (480, 640), (375, 1242), (1, 1)):
        for garg, eigen, ds in ((False, False, ""), (True, False, "kitti"), (False, True, "kitti"), (False, True, "nyu"), (True, True, "nyu")):
            m = np.zeros((h, w))
            if not (garg or eigen):
                m[:] = 1
            elif garg:
                m[int(0.40810811 * h):int(0.99189189 * h), int(0.03594771 * w):int(0.96405229 * w)] = 1
            elif ds == "kitti":
                m[int(0.3324324 * h):int(0.91351351 * h), int(0.0359477 * w):int(0.96405229 * w)] = 1
            else:
                m[45:471, 41:601] = 1
            y0, y1, x0, x1 = _eval_crop(h, w, garg, eigen, ds)
            assert 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
            r = np.zeros((h, w))
            r[y0:y1, x0:x1] = 1
            assert np.array_equal(r, m), (h, w, garg, eigen, ds)


def test_metrics_from_sums_empty_and_plain():
    from patchrefinerv2_amd.metrics import metrics_from_sums
    e = metrics_from_sums([0.0] * 12, True)
    assert e["see"] == 0.0 and all(np.isnan(v) for k, v in e.items() if k != "see")
    assert "see" not in metrics_from_sums([0.0] * 12, False)
    m = metrics_from_sums([4, 4, 4, 4, 2.0, 16.0, 1.0, 8.0, 4.0, 6.0, 2, 3.0], True)
    assert m["a1"] == 1.0 and m["abs_rel"] == 0.5 and m["rmse"] == 2.0 and m["log_10"] == 0.25 and m["sq_rel"] == 1.5 and m["see"] == 1.5
    assert m["rmse_log"] == np.sqrt(2.0) and m["silog"] == 100.0  # sqrt(8 / 4 - (4 / 4)^2) * 100


def _cli():
    spec = importlib.util.spec_from_file_location("prv2_tools_test", os.path.join(ROOT, "tools", "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_test_type_selects_the_dataloader_section(tmp_path):
    import argparse
    from patchrefinerv2_amd.registry import Config
    cli = _cli()
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "v2_dav2_mobile_u4k.py"))
    ns = lambda t: argparse.Namespace(test_type=t, config="cfg.py", image_raw_shape=[270, 480], edge_metrics=False)  # noqa: E731
    g = cli.dataset_config(cfg, ns("general"))
    assert g["type"] == "ImageDataset" and g["image_resolution"] == [270, 480] and "image_raw_shape" not in g  # as before
    for t, split in (("normal", "val.txt"), ("test_in", "test.txt"), ("test_out", "test_out.txt")):
        d = cli.dataset_config(cfg, ns(t))
        assert d["type"] == "UnrealStereo4kDataset" and d["mode"] == "infer" and d["split"] == "./data/u4k/splits/" + split
        assert d["image_raw_shape"] == [270, 480] and d["data_root"] == "./data/u4k" and (d["min_depth"], d["max_depth"]) == (1e-3, 80)
    assert cli.dataset_config(cfg, ns("normal"))["resize_mode"] == "depth-anything"
    with pytest.raises(SystemExit, match="one of general"):
        cli.dataset_config(cfg, ns("bogus"))
    for kind in ("CityScapesDataset", "KittiDataset", "ScanNetDataset", "ETH3DDataset"):
        cfg.merge_from_dict({"val_dataloader.dataset.type": kind})
        with pytest.raises(SystemExit, match=rf"{kind} is not built .*cityscapes, kitti, scannet and eth"):
            cli.dataset_config(cfg, ns("normal"))


def test_cli_without_val_dataloader_exits_with_a_clear_message(tmp_path):
    cfg = tmp_path / "cfg.py"
    cfg.write_text("model = dict(type='PatchRefinerPlus', config=dict())\n"
                   "general_dataloader = dict(dataset=dict(type='ImageDataset', rgb_image_dir=''))\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), str(cfg), "--synthetic-weights", "--test-type", "normal"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert re.search(r"--test-type normal needs val_dataloader\.dataset in the config", r.stderr), r.stderr[-1500:]
    assert "Traceback" not in r.stderr
