#!/usr/bin/env python
"""Pin the general dataset's ground-truth decoders to the reference: writes tests/golden/general_gt.npz.

BUILD BOX ONLY (needs the reference checkout, oracle.refharness.REF; leaves oracle/ untouched).  Imports the reference's own
estimator/datasets/general_dataset.py under oracle.refharness.install() -- as tools/make_edge_golden.py imports its metric.py --
and runs its ``DepthMap`` class (:75-158) on small synthetic files of every format this project decodes:

  u4k         val_gt/<n>.npy (float32 and float64 disparity) with val_factor/<n>.txt
  mid         gts/<n>.pfm in both byte orders with calibs/<n>.txt
  cityscapes  16-bit greyscale PNG
  eth3d       raw float32; the reference hard-codes 4032 x 6048, so that case runs at full size and only SHA-256 digests of ``gt`` and
              ``edge`` and their 16 x 16 corner are recorded (the input is ``eth3d_input()``, a formula the test repeats)

Stubs (modules that are absent, none of them arithmetic under test):
  cv2.imread(path, IMREAD_UNCHANGED)   -> PIL (a 16-bit PNG's uint16 samples, which is what OpenCV returns for it)
  imageio                              -> an empty module (only the 'gta' branch uses it)
  estimator.utils.metric               -> as tools/make_edge_golden.py loads it (get_boundaries touches none of its stubs)
  estimator.registry.DATASETS          -> the harness's registry stand-in
  estimator.datasets.{transformers, u4k_dataset}, zoedepth / depth_anything Resize -> empty stand-ins: DepthMap uses none of them
  estimator.datasets.utils             -> the reference's file; its readPFM reads ``sys.version`` without importing sys, so the
                                          module is handed ``sys``
For every case the arrays the files were written from, the reference's ``gt`` and ``edge``, and the parsed numbers are stored.

    python tools/make_general_gt_golden.py
"""
from __future__ import annotations

import hashlib
import importlib
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "general_gt.npz")
ETH_SHAPE = (4032, 6048)


def load_reference_dataset():
    from oracle import refharness
    refharness.install()
    from PIL import Image
    cv2 = sys.modules["cv2"]
    cv2.IMREAD_UNCHANGED = -1
    cv2.imread = lambda path, flag=1: np.asarray(Image.open(path)).copy()
    import make_edge_golden  # (tools/: the reference's metric.py with its absent dependencies stubbed; get_boundaries uses none)
    metric = make_edge_golden.load_reference_metric()
    u = sys.modules["estimator.utils"]
    u.get_boundaries, u.compute_metrics = metric.get_boundaries, metric.compute_metrics
    sys.modules["estimator.registry"].DATASETS = refharness.install.MODELS  # (the harness's registry stand-in: a decorator that records)
    d = types.ModuleType("estimator.datasets")
    d.__path__ = [os.path.join(refharness.REF, "estimator/datasets")]
    sys.modules["estimator.datasets"] = d
    tr = types.ModuleType("estimator.datasets.transformers")
    tr.aug_color = tr.aug_flip = tr.to_tensor = tr.random_crop = tr.aug_rotate = None
    u4k = types.ModuleType("estimator.datasets.u4k_dataset")
    u4k.UnrealStereo4kDataset = object
    sys.modules.update({"estimator.datasets.transformers": tr, "estimator.datasets.u4k_dataset": u4k})
    for name in ("zoedepth.models.base_models.midas", "depth_anything.transform"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                m.Resize = object
                sys.modules[name] = m
    utils = importlib.import_module("estimator.datasets.utils")
    utils.sys = sys
    return importlib.import_module("estimator.datasets.general_dataset")


def eth3d_input(shape=ETH_SHAPE) -> np.ndarray:
    """a deterministic full-size ETH3D map (integer arithmetic only, then one float32 scale): planes with steps of several
    metres, fine texture below the edge threshold, and inf / -inf / NaN holes as the dataset's raw files have them"""
    h, w = shape
    y, x = np.arange(h, dtype=np.uint32)[:, None], np.arange(w, dtype=np.uint32)[None, :]
    t = ((x * np.uint32(2654435761) + y * np.uint32(40503)) >> np.uint32(7)) & np.uint32(1023)      # texture 0 .. 1023
    steps = (x // np.uint32(577) + y // np.uint32(811)) % np.uint32(5)                                # planes 0 .. 4
    d = (t.astype(np.float32) * np.float32(1.0 / 2048.0) + steps.astype(np.float32) * np.float32(2.5) + np.float32(1.0)).astype(np.float32)
    k = (x * np.uint32(7919) + y * np.uint32(104729)) % np.uint32(9973)
    d[k == 0] = np.inf
    d[k == 1] = -np.inf
    d[k == 2] = np.nan
    d[(x % np.uint32(1511) < 3) & (y % np.uint32(997) < 2)] = np.inf  # small blocks of missing depth
    return d


def small_disparity(h, w, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = (20.0 + 30.0 * (x > w * 0.4) + 12.0 * (np.hypot(x - w * 0.6, y - h * 0.5) < h * 0.3) + 0.2 * rs.rand(h, w)).astype(np.float32)
    d[0, ::2] += 3.0   # steps on the frame borders and in the corners
    d[-1, 1::2] += 3.0
    d[::2, 0] += 3.0
    d[1::2, -1] += 3.0
    d[h // 2, 1] = d[h // 2, 0] + np.float32(1.0)                        # a step of exactly th
    d[h // 2 + 2, 1] = np.nextafter(d[h // 2 + 2, 0] + np.float32(1.0), np.float32(np.inf))  # and one just above it
    return d


def write_pfm(path, disp, little):
    """a one-channel PFM: rows bottom-to-top, negative scale = little-endian"""
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n%s\n" % (disp.shape[1], disp.shape[0], b"-1.0" if little else b"1.0"))
        f.write(np.flipud(disp).astype("<f4" if little else ">f4").tobytes())


def main():
    from patchrefinerv2_amd.tester import write_png16
    gd = load_reference_dataset()
    rec, names = {}, []

    def run(name, root, files, kind, **inputs):
        with np.errstate(divide="ignore", invalid="ignore"):
            m = gd.DepthMap(root, files, 0, kind)
        names.append(name)
        rec[f"{name}/kind"] = np.array(kind)
        for k, v in inputs.items():
            rec[f"{name}/{k}"] = v
        rec[f"{name}/gt"], rec[f"{name}/edge"] = np.asarray(m.gt), np.asarray(m.edge)
        rec[f"{name}/name"] = np.array(m.name)
        print(f"  {name}: gt {m.gt.dtype} {m.gt.shape}, {int(np.asarray(m.edge).sum())} edge pixels, name {m.name!r}")
        return m

    with tempfile.TemporaryDirectory() as tmp:
        # u4k: disparity .npy + factor file
        gt_dir, fac_dir = os.path.join(tmp, "u4k", "val_gt"), os.path.join(tmp, "u4k", "val_factor")
        os.makedirs(gt_dir), os.makedirs(fac_dir)
        for n, dtype in (("a32", np.float32), ("b64", np.float64)):
            d = small_disparity(21, 30, 1).astype(dtype)
            d[3, 4], d[5, 6] = 0.0, np.nan
            np.save(os.path.join(gt_dir, f"{n}.npy"), d)
            with open(os.path.join(fac_dir, f"{n}.txt"), "w") as f:
                f.write("1234.5678\n")
            run(f"u4k_{n}", gt_dir, [f"{n}.npy"], "u4k", input=d, factor=np.float64(1234.5678))
        # mid: PFM in both byte orders + calibration file
        gt_dir, cal_dir = os.path.join(tmp, "mid", "gts"), os.path.join(tmp, "mid", "calibs")
        os.makedirs(gt_dir), os.makedirs(cal_dir)
        calib = "cam0=[3997.684 0 1176.728; 0 3997.684 1011.728; 0 0 1]\ncam1=[3997.684 0 1307.839; 0 3997.684 1011.728; 0 0 1]\n" \
                "doffs=131.111\nbaseline=193.001\nwidth=2964\nheight=1988\nndisp=280\n"
        for n, little in (("le", True), ("be", False)):
            d = small_disparity(17, 23, 2) * np.float32(4.0)
            d[2, 3] = d[2, 4] = d[9, 0] = d[16, 22] = np.inf   # the invalid pixels of the dataset
            d[4, 5], d[6, 7], d[8, 9] = -np.inf, np.nan, np.float32(-131.111)  # (doffs cancels: a division by zero)
            write_pfm(os.path.join(gt_dir, f"{n}.pfm"), d, little)
            with open(os.path.join(cal_dir, f"{n}.txt"), "w") as f:
                f.write(calib)
            run(f"mid_{n}", gt_dir, [f"{n}.pfm"], "mid", input=d, little=np.array(little), factor=np.float64(193.001 * 3997.684),
                doffs=np.float64(131.111), calib=np.array(calib))
        # cityscapes: 16-bit disparity PNG
        gt_dir = os.path.join(tmp, "cs")
        os.makedirs(gt_dir)
        rs = np.random.RandomState(3)
        v = (2000 + 6000 * (np.mgrid[0:19, 0:26][1] > 11) + rs.randint(0, 40, (19, 26))).astype(np.uint16)
        v[0, :4] = (0, 1, 2, 65535)
        v[5, 5:9], v[18, 25], v[18, 0], v[0, 25] = 0, 0, 1, 65535
        v[7:9, 13:17] = rs.randint(1, 300, (2, 4))  # near range: large depth steps
        write_png16(os.path.join(gt_dir, "c.png"), v)
        run("cityscapes", gt_dir, ["c.png"], "cityscapes", input=v)
        # eth3d: full size (the shape is a literal in the reference): digests + a corner
        gt_dir = os.path.join(tmp, "eth")
        os.makedirs(gt_dir)
        eth3d_input().tofile(os.path.join(gt_dir, "e.raw"))
        with np.errstate(invalid="ignore"):
            m = gd.DepthMap(gt_dir, ["e.raw"], 0, "eth3d")
        gt, edge = np.ascontiguousarray(m.gt), np.ascontiguousarray(m.edge)
        assert gt.shape == ETH_SHAPE and gt.dtype == np.float32 and edge.dtype == np.float32
        rec["eth3d/shape"] = np.array(ETH_SHAPE)
        rec["eth3d/gt_sha256"], rec["eth3d/edge_sha256"] = np.array(hashlib.sha256(gt.tobytes()).hexdigest()), np.array(hashlib.sha256(edge.tobytes()).hexdigest())
        rec["eth3d/gt_corner"], rec["eth3d/edge_corner"] = gt[:16, :16].copy(), edge[:16, :16].copy()
        rec["eth3d/edge_count"], rec["eth3d/zero_count"] = np.array(int(edge.sum())), np.array(int((gt == 0).sum()))
        print(f"  eth3d: {int(edge.sum())} edge pixels, {int((gt == 0).sum())} zeros, gt {rec['eth3d/gt_sha256']}")
    rec["cases"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
