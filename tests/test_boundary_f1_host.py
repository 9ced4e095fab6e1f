"""CPU: the scale-invariant boundary F1 without a GPU -- metrics.compute_boundary_f1 (the numpy specification) against the hand case of
its definition and against a plain-Python restatement with scalar loops, its properties, the flag's way from tools/test.py into the
dataset classes, and the new entry points' declaration, binding and argument checks through the C ABI."""
import argparse
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_eth_dataset_host import eth_config_text, write_eth_tree
from test_u4k_eval_host import _cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prv2_boundary_f1_workspace_bytes", "prv2_boundary_f1")
BOUNDARY_KEYS = ("si_boundary_f1", "si_boundary_p", "si_boundary_r")
MN, MX = 0.1, 10.0
PLAIN = dict(garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=MN, max_depth_eval=MX)


def spec(gt, pred, thresholds=None, **kw):
    """(dict with curves, counts row) of the specification"""
    from patchrefinerv2_amd import metrics as M
    return M.compute_boundary_f1(gt, pred, thresholds=thresholds, curves=True, return_counts=True, **dict(PLAIN, **kw))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def f32(x):
    return float(np.float32(x))


def restate(gt, pred, thresholds, mn=MN, mx=MX, crop=None):
    """the definition pair by pair, in scalar Python on fp32 values: -> the row n_h, n_v, then [T][L, T, R, B][tp, np, ng]"""
    h, w = len(gt), len(gt[0])
    y0, y1, x0, x1 = crop or (0, h, 0, w)
    mn, mx = f32(mn), f32(mx)

    def valid(y, x):
        g = f32(gt[y][x])
        return y0 <= y < y1 and x0 <= x < x1 and g > mn and g < mx  # (a NaN compares false)

    def clean(v):
        v = f32(v)
        if math.isnan(v):
            return mn
        return min(max(v, mn), mx)

    def over(a, t, b):  # a > t * b with the product rounded to fp32
        return a > f32(np.float32(t) * np.float32(b))
    nh = nv = 0
    counts = [[[0, 0, 0] for _ in range(4)] for _ in thresholds]
    for y in range(h):
        for x in range(w):
            for d_fwd, d_bwd, yy, xx in ((0, 2, y, x + 1), (1, 3, y + 1, x)):  # horizontal: L / R; vertical: T / B
                if yy >= h or xx >= w or not (valid(y, x) and valid(yy, xx)):
                    continue
                if d_fwd == 0:
                    nh += 1
                else:
                    nv += 1
                ga, gb, pa, pb = f32(gt[y][x]), f32(gt[yy][xx]), clean(pred[y][x]), clean(pred[yy][xx])
                for i, t in enumerate(thresholds):
                    for d, (fp, fg) in ((d_fwd, (over(pa, t, pb), over(ga, t, gb))), (d_bwd, (over(pb, t, pa), over(gb, t, ga)))):
                        counts[i][d][0] += int(fp and fg)
                        counts[i][d][1] += int(fp)
                        counts[i][d][2] += int(fg)
    return [float(nh), float(nv)] + [float(v) for per_t in counts for per_d in per_t for v in per_d]


def frame(shape, seed, hard=True):
    """ground truth with depth steps, and with ``hard`` holes (0), a NaN and a too-far pixel; a prediction with its own steps, and with
    ``hard`` NaN / inf / negative / out-of-range values inside the mask"""
    h, w = shape
    rs = np.random.RandomState(seed)
    gt = (1.0 + 0.2 * rs.rand(h, w)).astype(np.float32)
    gt[rs.rand(h, w) < 0.3] *= np.float32(1.5)
    gt[rs.rand(h, w) < 0.1] *= np.float32(2.5)
    pred = (gt * (0.9 + 0.25 * rs.rand(h, w))).astype(np.float32)
    pred[rs.rand(h, w) < 0.2] *= np.float32(1.3)
    if hard and h * w >= 7:
        flat_g, flat_p = gt.reshape(-1), pred.reshape(-1)
        idx = rs.permutation(h * w)
        holes = max(1, h * w // 9)
        flat_g[idx[:holes]] = 0.0
        flat_g[idx[holes]] = np.nan
        flat_g[idx[holes + 1]] = 11.0
        inside = [i for i in idx[holes + 2:] if MN < flat_g[i] < MX]
        for i, v in zip(inside, (np.nan, np.inf, -np.inf, -1.0, 0.01, 50.0)):
            flat_p[i] = v
    return gt, pred


SHAPES = [(1, 1), (1, 7), (7, 1), (5, 9), (37, 53)]


# ------------------------------------------------------------------------------------------------------------------ the hand case
def test_the_hand_case_of_the_definition():
    g = np.array([[1, 2, 2], [1, 1, 4]], np.float32)
    p = np.array([[1, 1.2, 2.4], [1, 1, 1]], np.float32)
    out, row = spec(g, p, thresholds=(1.1, 1.5))
    assert row.tolist() == [4, 3] + [0, 0, 0, 1, 2, 1, 1, 2, 2, 0, 0, 1] + [0, 0, 0, 0, 1, 1, 0, 1, 2, 0, 0, 1]
    assert out["boundary_p"] == [0.25, 0.0] and out["boundary_r"] == [0.375, 0.0]
    assert out["boundary_f1"][0] == pytest.approx(0.3, abs=1e-15) and out["boundary_f1"][1] == 0.0
    assert out["boundary_thresholds"] == [f32(1.1), f32(1.5)]
    w0 = float(np.float32(1.1)) / (float(np.float32(1.1)) + float(np.float32(1.5)))
    assert out["si_boundary_p"] == w0 * 0.25 and out["si_boundary_r"] == w0 * 0.375
    assert out["si_boundary_f1"] == pytest.approx(w0 * 0.3, abs=1e-15)
    g2 = g.copy()
    g2[0, 2] = 0.0  # pixel (row 0, column 2) invalid
    _, row = spec(g2, p, thresholds=(1.1, 1.5))
    assert row.tolist() == [3, 2] + [0, 0, 0, 1, 1, 1, 1, 1, 2, 0, 0, 0] + [0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 0, 0]
    assert restate(g.tolist(), p.tolist(), (1.1, 1.5)) == spec(g, p, thresholds=(1.1, 1.5))[1].tolist()


# ------------------------------------------------------------------------------------------------------------------ per-pair restatement
@pytest.mark.parametrize("shape", SHAPES)
def test_specification_against_the_per_pair_restatement(shape):
    from patchrefinerv2_amd import metrics as M
    gt, pred = frame(shape, 100 + shape[0] * 7 + shape[1])
    th = M.boundary_thresholds()
    out, row = spec(gt, pred)
    assert row.dtype == np.float64 and row.shape == (122,)
    assert row.tolist() == restate(gt.tolist(), pred.tolist(), th.tolist())
    if shape == (37, 53):
        assert np.isnan(gt).any() and (gt == 0).any() and row[0] > 0 and row[1] > 0 and row[2:].reshape(10, 4, 3)[..., 0].min() > 0
        for crop_kw, crop in ((dict(garg_crop=True), (15, 36, 1, 51)),):  # a crop whose border cuts pairs
            assert M._eval_crop(37, 53, True, False, "") == crop
            _, cropped = spec(gt, pred, **crop_kw)
            assert cropped.tolist() == restate(gt.tolist(), pred.tolist(), th.tolist(), crop=crop) and cropped[0] < row[0]
    if shape == (1, 1):
        assert row.tolist() == [0.0] * 122
    if shape == (1, 7):
        assert row[1] == 0 and row[0] > 0
    if shape == (7, 1):
        assert row[0] == 0 and row[1] > 0


def test_other_threshold_counts_and_orders_against_the_restatement():
    gt, pred = frame((5, 9), 3)
    for th in ((1.3,), (1.25, 1.05, 1.5), tuple(np.linspace(1.02, 2.0, 16))):
        th32 = [f32(t) for t in th]
        assert spec(gt, pred, thresholds=th)[1].tolist() == restate(gt.tolist(), pred.tolist(), th32)


# ------------------------------------------------------------------------------------------------------------------ properties
def test_prediction_equal_to_the_ground_truth_scores_one():
    gt, _ = frame((37, 53), 5, hard=False)
    out, row = spec(gt, gt.copy())
    c = row[2:].reshape(10, 4, 3)
    assert c[..., 2].min() > 0 and (c[..., 0] == c[..., 1]).all() and (c[..., 0] == c[..., 2]).all()
    assert out["si_boundary_f1"] == 1.0 and out["si_boundary_p"] == 1.0 and out["si_boundary_r"] == 1.0
    assert out["boundary_f1"] == [1.0] * 10


@pytest.mark.parametrize("scale", [2.0, 0.5])
def test_counts_do_not_depend_on_the_predictions_scale(scale):
    gt, pred = frame((37, 53), 6, hard=False)
    mx = 40.0  # neither map touches the clamp; a power of two scales fp32 values exactly, so every test keeps its outcome
    assert pred.min() * 0.5 > MN and pred.max() * 2.0 < mx and gt.min() > MN and gt.max() < mx
    scaled = (pred * np.float32(scale)).astype(np.float32)
    assert spec(gt, pred, max_depth_eval=mx)[1].tolist() == spec(gt, scaled, max_depth_eval=mx)[1].tolist()


def test_a_constant_prediction_has_no_boundary():
    gt, _ = frame((37, 53), 7, hard=False)
    out, row = spec(gt, np.full_like(gt, 2.0))
    c = row[2:].reshape(10, 4, 3)
    assert (c[..., 1] == 0).all() and (c[..., 0] == 0).all() and c[..., 2].max() > 0
    assert out["si_boundary_f1"] == 0.0 and out["si_boundary_p"] == 0.0 and out["si_boundary_r"] == 0.0


def test_no_valid_pair_gives_nan_and_evaluate_skips_the_frame():
    from patchrefinerv2_amd import metrics as M
    gt, pred = frame((5, 9), 8, hard=False)
    alone = np.zeros_like(gt)
    alone[::2, ::2] = 2.0  # valid pixels, none next to another
    for g in (np.zeros_like(gt), alone, gt[:1, :1]):
        out, row = spec(g, pred[:g.shape[0], :g.shape[1]])
        assert row[0] == 0 and row[1] == 0 and (row == 0).all()
        assert all(np.isnan(out[k]) for k in BOUNDARY_KEYS) and all(np.isnan(v) for v in out["boundary_f1"])
    scored = M.compute_boundary_f1(gt, pred, **PLAIN)
    assert tuple(scored) == BOUNDARY_KEYS and np.isfinite(list(scored.values())).all()
    nan = M.compute_boundary_f1(alone, pred, **PLAIN)
    ev = M.evaluate([dict(a1=0.5, **scored), dict(a1=0.7, **nan)])
    assert ev["a1"] == 0.6 and all(ev[k] == scored[k] for k in BOUNDARY_KEYS)
    assert all(np.isnan(v) for k, v in M.evaluate([dict(nan)]).items())


def test_a_pair_with_one_invalid_pixel_is_not_counted():
    g = np.array([[1, 4, 1, 4]], np.float32)
    p = np.array([[4, 1, 4, 1]], np.float32)
    _, row = spec(g, p, thresholds=(1.5,))
    assert row.tolist() == [3, 0, 0, 2, 1, 0, 0, 0, 0, 1, 2, 0, 0, 0]
    g[0, 1] = 0.0  # takes the pairs (0, 1) and (1, 2) away, whatever the prediction holds there
    for bad in (1.0, np.nan, np.inf):
        p[0, 1] = bad
        assert spec(g, p, thresholds=(1.5,))[1].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]


def test_threshold_counts_and_values():
    from patchrefinerv2_amd import metrics as M
    gt, pred = frame((5, 9), 9)
    assert M.boundary_thresholds().dtype == np.float32 and M.boundary_thresholds().tolist() == [f32(v) for v in np.linspace(1.05, 1.25, 10)]
    for T in (1, 16):
        th = M.boundary_thresholds(T)
        out, row = spec(gt, pred, thresholds=th)
        assert th.shape == (T,) and row.shape == (2 + 12 * T,) and len(out["boundary_f1"]) == T
    for T in (0, 17):
        with pytest.raises(ValueError):
            M.boundary_thresholds(T)
        with pytest.raises(ValueError):
            spec(gt, pred, thresholds=[1.1] * T)
    for bad in (1.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            spec(gt, pred, thresholds=(1.1, bad))
    with pytest.raises(ValueError):
        M.boundary_from_values(np.zeros(13), (1.1,))


def test_resize_of_a_smaller_prediction_is_compute_metrics_own():
    gt, pred = frame((37, 53), 10)
    small = torch.from_numpy(np.nan_to_num(pred, nan=1.0, posinf=9.0, neginf=0.2))[None, None, ::2, ::2].contiguous()
    up = F.interpolate(small, (37, 53), mode="bilinear", align_corners=False)
    a, b = spec(gt, small), spec(gt, up)
    assert a[1].tolist() == b[1].tolist() and a[0] == b[0] and a[1][0] > 0


# ------------------------------------------------------------------------------------------------------------------ the flag
def test_boundary_f1_flag_reaches_every_dataset_constructor(tmp_path):
    from patchrefinerv2_amd import tester  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS, Config
    cli = _cli()
    base = os.path.join(ROOT, "configs", "v2_dav2_mobile_u4k.py")

    def ns(t, **kw):
        return argparse.Namespace(test_type=t, config="cfg.py", image_raw_shape=[6, 8], edge_metrics=False, **kw)
    cfg = Config.fromfile(base)
    for t, kind in (("general", "ImageDataset"), ("normal", "UnrealStereo4kDataset"), ("test_in", "UnrealStereo4kDataset"),
                    ("test_out", "UnrealStereo4kDataset")):
        before = cli.dataset_config(cfg, ns(t))                       # a namespace without the attribute: as today
        assert before["type"] == kind and "boundary_f1" not in before
        assert cli.dataset_config(cfg, ns(t, boundary_f1=False)) == before
        assert cli.dataset_config(cfg, ns(t, boundary_f1=True)) == dict(before, boundary_f1=True)
        assert cli.dataset_config(cfg, ns(t, boundary_f1=True, ssi_metrics=True)) == dict(before, ssi_metrics=True, boundary_f1=True)
    split, _ = write_eth_tree(str(tmp_path / "data"), 1, (12, 20), (7, 11))
    (tmp_path / "eth.py").write_text(eth_config_text(split, (7, 11), (24, 40)))
    ecfg = Config.fromfile(str(tmp_path / "eth.py"))
    before = cli.dataset_config(ecfg, ns("normal"))
    on = cli.dataset_config(ecfg, ns("normal", boundary_f1=True))
    assert before["type"] == "ETHDataset" and "boundary_f1" not in before and on == dict(before, boundary_f1=True)
    assert DATASETS.build(on).boundary_f1 is True and DATASETS.build(before).boundary_f1 is False
    (tmp_path / "rgb").mkdir()
    assert DATASETS.build(dict(type="ImageDataset", rgb_image_dir=str(tmp_path / "rgb"), boundary_f1=True)).boundary_f1 is True
    for cls in (tester.ImageDataset, tester.UnrealStereo4kDataset, tester.ETHDataset, tester.CityScapesDataset, tester.KittiDataset,
                tester.ScanNetDataset):
        assert inspect.signature(cls.__init__).parameters["boundary_f1"].default is False, cls.__name__
    src = open(os.path.join(ROOT, "tools", "test.py")).read()
    assert '"--boundary-f1"' in src and src.count('getattr(args, "boundary_f1", False)') == 2  # the constructed branch and the registry's


def test_image_dataset_host_route_adds_the_keys_only_with_the_flag(tmp_path):
    """a CPU ``result`` is scored by the host specification; without the flag get_metrics returns today's dict"""
    from patchrefinerv2_amd import metrics as M
    from patchrefinerv2_amd.tester import ImageDataset
    (tmp_path / "rgb").mkdir()
    g, p = frame((37, 53), 11)
    gt, pred = torch.from_numpy(np.nan_to_num(g))[None, None], torch.from_numpy(np.nan_to_num(p, nan=2.0, posinf=9.0, neginf=0.2))[None, None]
    edges = torch.from_numpy(M.get_boundaries(np.nan_to_num(g), th=1, dilation=0))

    def metrics(**kw):
        return ImageDataset(str(tmp_path / "rgb"), min_depth=MN, max_depth=MX, **kw).get_metrics(gt, pred, edges)
    plain = metrics()
    assert tuple(plain) == ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")
    on = metrics(boundary_f1=True)
    assert tuple(on) == tuple(plain) + BOUNDARY_KEYS and all(on[k] == plain[k] for k in plain)
    want = M.compute_boundary_f1(gt, pred, **PLAIN)
    assert {k: on[k] for k in BOUNDARY_KEYS} == want and 0 < want["si_boundary_f1"] < 1
    ssi = metrics(ssi_metrics=True)
    both = metrics(ssi_metrics=True, boundary_f1=True)
    assert tuple(both) == tuple(ssi) + BOUNDARY_KEYS and tuple(ssi) == tuple(plain) + M.SSI_KEYS  # ssi before boundary
    assert all(both[k] == ssi[k] for k in ssi) and all(both[k] == on[k] for k in BOUNDARY_KEYS)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_bound_and_exported_on_abi_20():
    from patchrefinerv2_amd import lib as L, metrics as M, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for s, n_args in zip(NEW_SYMBOLS, (3, 19)):
        assert s in L.SIGNATURES and re.search(rf"\bint(?:64_t)? {s}\(", hdr) and hasattr(raw, s), s
        args = re.search(rf"\bint(?:64_t)? {s}\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[s][1]) == n_args, s
    assert "Boundary F1 evaluation" in hdr and "compare-after-multiply" in hdr and "(L, T, R, B)" in hdr
    assert int(re.search(r"#define PRV2_BOUNDARY_MAX_THRESHOLDS (\d+)", hdr).group(1)) == L.BOUNDARY_MAX_THRESHOLDS == ops.BOUNDARY_MAX_THRESHOLDS == 16
    assert re.search(r"#define PRV2_BOUNDARY_VALUES\(T\) \(2 \+ 12 \* \(T\)\)", hdr) and L.boundary_values(10) == 122
    assert L.load().prv2_abi_version() == 20
    t = torch_ops.load()
    assert "boundary_f1" in torch_ops.OPS and hasattr(t, "boundary_f1") and hasattr(ops, "boundary_f1")
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.boundary_f1(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), 0.1, 10.0, 0, 4, 0, 4, [1.1])
    for f in (M.boundary_thresholds, M.compute_boundary_f1, M.compute_boundary_f1_fused, M.boundary_from_values):
        assert callable(f)
    assert M.BOUNDARY_KEYS == BOUNDARY_KEYS
    mk = open(os.path.join(ROOT, "patchrefinerv2_amd", "csrc", "Makefile")).read()
    assert "boundary_eval.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1) and "-ffp-contract=off" in mk


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
    wsb = lib.prv2_boundary_f1_workspace_bytes
    assert wsb(0, 16, 24) == -1 and wsb(1, 0, 24) == -1 and wsb(1, 16, -2) == -1 and wsb(65536, 16, 24) == -1
    one = wsb(1, 270, 480)
    assert one > 0 and wsb(3, 270, 480) == 3 * one  # per frame: a frame's blocks do not depend on the frame count
    good = (ctypes.c_float * 2)(1.1, 1.5)

    def call(gt=P, pred=P, n=1, h=16, w=24, ph=16, pw=24, crop=(0, 16, 0, 24), th=good, nt=2, out=P, ws=P, wsbytes=None):
        if isinstance(th, (list, tuple)):
            th = (ctypes.c_float * len(th))(*th)
        code = lib.prv2_boundary_f1(gt, pred, n, h, w, ph, pw, 0.1, 10.0, *crop, th, nt, out, ws,
                                    wsb(1, 16, 24) * max(n, 1) if wsbytes is None else wsbytes, None)
        assert code != 0
        return lib.prv2_last_error()
    assert b"null" in call(gt=None) and b"null" in call(pred=None) and b"null" in call(out=None) and b"null" in call(th=None)
    assert b"workspace" in call(ws=None)
    assert b"frame count" in call(n=0)
    assert b"shape" in call(h=0) and b"prediction shape" in call(ph=0) and b"prediction shape" in call(pw=-1)
    assert b"2^31" in call(h=65536, w=32768, crop=(0, 1, 0, 1))
    for crop in ((-1, 16, 0, 24), (0, 17, 0, 24), (5, 4, 0, 24), (0, 16, 0, 25), (0, 16, 9, 8)):
        assert b"crop" in call(crop=crop)
    assert b"thresholds" in call(nt=0) and b"thresholds" in call(nt=17) and b"thresholds" in call(nt=-1)
    for bad in (1.0, 0.9, float("nan"), float("inf")):
        assert b"threshold 1" in call(th=[1.1, bad])
    assert b"workspace" in call(wsbytes=8)
    assert b"boundary_f1" in lib.prv2_last_error()
