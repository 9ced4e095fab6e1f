"""CPU: the scale-and-shift-invariant evaluation without a GPU -- metrics.compute_scale_and_shift / compute_ssi_metrics against the
reference's recorded float64 outputs (tests/golden/ssi_eval.npz, tools/make_ssi_golden.py), the flag's way from tools/test.py into the
three dataset classes, and the new entry points' declaration, binding and argument checks through the C ABI."""
import argparse
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_eth_dataset_host import eth_config_text, write_eth_tree
from test_u4k_eval_host import _cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prv2_ssi_metrics_workspace_bytes", "prv2_ssi_metrics")
SSI_KEYS = ("ssi_scale", "ssi_shift", "ssi_l1", "ssi_gm", "gm", "ssi_gm_inv", "ssi_a1", "ssi_a2", "ssi_a3", "ssi_abs_rel", "ssi_rmse",
            "ssi_log_10", "ssi_rmse_log", "ssi_silog", "ssi_sq_rel")
RTOL = 1e-12  # float64 against float64, the same formulas


def load_cases():
    """tests/golden/ssi_eval.npz -> (min_depth, max_depth, {name: dict(gt, pred fp32; mask bool; crop; n; and for n > 1 the reference's
    float64 results: want = the fifteen keys in SSI_KEYS' order)})"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ssi_eval.npz"))
    out = {}
    for name in z["cases"]:
        gt, pred = z[f"{name}/gt"].astype(np.float32), z[f"{name}/pred"].astype(np.float32)  # (the large case is stored as fp16, exactly)
        mask = z[f"{name}/mask"]
        if mask.dtype != bool:
            mask = np.unpackbits(mask)[:gt.size].reshape(gt.shape).astype(bool)
        c = dict(gt=gt, pred=pred, mask=mask, crop=tuple(int(v) for v in z[f"{name}/crop"]), n=float(z[f"{name}/n"]))
        if c["n"] > 1:
            c["want"] = dict(zip(SSI_KEYS, list(z[f"{name}/scale_shift"]) + list(z[f"{name}/loss_f64"]) + list(z[f"{name}/errors"])))
        out[str(name)] = c
    return float(z["min_depth"]), float(z["max_depth"]), out


MN, MX, CASES = load_cases()
SCORED = [k for k, c in CASES.items() if c["n"] > 1]


def crop_args(name):
    """the compute_metrics arguments that give the case's crop"""
    return dict(garg_crop=name.startswith("garg"), eigen_crop=False, dataset="", min_depth_eval=MN, max_depth_eval=MX)


def test_fixture_holds_the_cases_the_kernels_can_go_wrong_on():
    assert {"t2x7", "t5x7", "holes37x53", "garg37x53", "big270x480", "constpred8x16", "single5x7"} <= set(CASES)
    h = CASES["holes37x53"]
    assert np.isnan(h["gt"]).any() and (h["gt"] == 0).any() and (h["gt"] > MX).any() and np.isnan(h["pred"][~h["mask"]]).any()
    assert CASES["single5x7"]["n"] == 1 and CASES["constpred8x16"]["n"] == 128
    assert CASES["garg37x53"]["crop"] != (0, 37, 0, 53) and CASES["garg37x53"]["n"] < h["n"]


@pytest.mark.parametrize("name", SCORED)
def test_compute_scale_and_shift_against_the_reference(name):
    from patchrefinerv2_amd import metrics as M
    c = CASES[name]
    s, t = M.compute_scale_and_shift(c["pred"], c["gt"], c["mask"])
    np.testing.assert_allclose([s, t], [c["want"]["ssi_scale"], c["want"]["ssi_shift"]], rtol=RTOL, atol=0)
    sb, tb = M.compute_scale_and_shift(np.stack([c["pred"]] * 2), np.stack([c["gt"]] * 2), np.stack([c["mask"]] * 2))  # [B, H, W]
    assert sb.shape == (2,) and sb[0] == sb[1] == s and tb[0] == tb[1] == t


def test_constant_prediction_has_a_zero_determinant_and_no_fit():
    from patchrefinerv2_amd import metrics as M
    c = CASES["constpred8x16"]
    assert (c["pred"] == 2.0).all() and c["mask"].all()
    assert M.compute_scale_and_shift(c["pred"], c["gt"], c["mask"]) == (0.0, 0.0)
    assert (c["want"]["ssi_scale"], c["want"]["ssi_shift"]) == (0.0, 0.0)
    m = M.compute_ssi_metrics(c["gt"], c["pred"], **crop_args("constpred8x16"))
    assert m["ssi_scale"] == 0.0 and m["ssi_shift"] == 0.0 and m["ssi_gm"] == m["gm"] == m["ssi_gm_inv"]  # the gradients of gt alone
    np.testing.assert_allclose(m["ssi_l1"], np.abs(c["gt"].astype(np.float64)).mean(), rtol=RTOL)


@pytest.mark.parametrize("name", SCORED)
def test_compute_ssi_metrics_against_the_reference(name):
    from patchrefinerv2_amd import metrics as M
    c = CASES[name]
    m = M.compute_ssi_metrics(torch.from_numpy(c["gt"])[None, None], torch.from_numpy(c["pred"])[None, None], **crop_args(name))
    assert tuple(m) == SSI_KEYS
    for k in SSI_KEYS:
        np.testing.assert_allclose(m[k], c["want"][k], rtol=RTOL, atol=0, err_msg=f"{name} {k}")


def test_one_valid_pixel_or_none_gives_nan_everywhere():
    from patchrefinerv2_amd import metrics as M
    c = CASES["single5x7"]
    for gt in (c["gt"], np.zeros_like(c["gt"])):
        m = M.compute_ssi_metrics(gt, c["pred"], **crop_args("single5x7"))
        assert tuple(m) == SSI_KEYS and all(np.isnan(v) for v in m.values())
    assert all(np.isnan(v) for v in M.ssi_from_values([1.0] * 6 + [1.0] + [2.0] * 34).values())


@pytest.mark.parametrize("name", ["holes37x53", "garg37x53", "t5x7"])
def test_aligned_error_keys_are_compute_metrics_of_the_aligned_prediction(name):
    """ssi_a1 ... ssi_sq_rel == metrics.compute_metrics(gt, (s * p + t).astype(float32)), exactly.  The maps go in as float64 tensors
    holding those fp32 values, the depth range as its fp32 values (what an fp32 map is clamped to): compute_errors then works in
    float64 as the device sums do (from fp32 pixels) on the decisions fp32 arrays give; as fp32 arrays its own arithmetic would be
    fp32 and the device could only follow it to 1e-7."""
    from patchrefinerv2_amd import metrics as M
    c = CASES[name]
    m = M.compute_ssi_metrics(c["gt"], c["pred"], **crop_args(name))
    aligned = (m["ssi_scale"] * c["pred"].astype(np.float64) + m["ssi_shift"]).astype(np.float32)
    gt = np.where(np.isnan(c["gt"]), np.float32(0), c["gt"])
    kw = dict(crop_args(name), min_depth_eval=float(np.float32(MN)), max_depth_eval=float(np.float32(MX)))
    assert (aligned[c["mask"]] < np.float32(MN)).any() or name != "t5x7"  # t5x7 holds a pixel the clamp moves
    want = M.compute_metrics(torch.from_numpy(gt).double(), torch.from_numpy(aligned).double(), interpolate=False, **kw)
    assert {k: m["ssi_" + k] for k in want} == {k: float(v) for k, v in want.items()}


def test_resize_of_a_smaller_prediction_is_compute_metrics_own():
    from patchrefinerv2_amd import metrics as M
    import torch.nn.functional as F
    c = CASES["holes37x53"]
    small = torch.from_numpy(np.nan_to_num(c["pred"], nan=1.0))[None, None, ::2, ::2].contiguous()
    up = F.interpolate(small, (37, 53), mode="bilinear", align_corners=False)
    assert M.compute_ssi_metrics(c["gt"], small, **crop_args("holes37x53")) == M.compute_ssi_metrics(c["gt"], up, **crop_args("holes37x53"))


# ------------------------------------------------------------------------------------------------------------------ the flag
def test_ssi_metrics_flag_reaches_all_three_dataset_constructors(tmp_path):
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
        assert before["type"] == kind and "ssi_metrics" not in before
        assert cli.dataset_config(cfg, ns(t, ssi_metrics=False)) == before
        on = cli.dataset_config(cfg, ns(t, ssi_metrics=True))
        assert on == dict(before, ssi_metrics=True)
    split, _ = write_eth_tree(str(tmp_path / "data"), 1, (12, 20), (7, 11))
    (tmp_path / "eth.py").write_text(eth_config_text(split, (7, 11), (24, 40)))
    ecfg = Config.fromfile(str(tmp_path / "eth.py"))
    before = cli.dataset_config(ecfg, ns("normal"))
    on = cli.dataset_config(ecfg, ns("normal", ssi_metrics=True))
    assert before["type"] == "ETHDataset" and "ssi_metrics" not in before and on == dict(before, ssi_metrics=True)
    assert DATASETS.build(on).ssi_metrics is True and DATASETS.build(before).ssi_metrics is False
    (tmp_path / "rgb").mkdir()
    assert DATASETS.build(dict(type="ImageDataset", rgb_image_dir=str(tmp_path / "rgb"), ssi_metrics=True)).ssi_metrics is True
    for cls in (tester.ImageDataset, tester.UnrealStereo4kDataset, tester.ETHDataset):
        assert inspect.signature(cls.__init__).parameters["ssi_metrics"].default is False
    src = open(os.path.join(ROOT, "tools", "test.py")).read()
    assert '"--ssi-metrics"' in src and 'getattr(args, "ssi_metrics", False)' in src


def test_image_dataset_host_route_adds_the_keys_only_with_the_flag(tmp_path):
    """a CPU ``result`` is scored by the host restatement; without the flag get_metrics returns today's dict"""
    from patchrefinerv2_amd import metrics as M
    from patchrefinerv2_amd.tester import ImageDataset
    (tmp_path / "rgb").mkdir()
    c = CASES["holes37x53"]
    gt, pred = torch.from_numpy(np.nan_to_num(c["gt"]))[None, None], torch.from_numpy(np.nan_to_num(c["pred"], nan=2.0))[None, None]
    edges = torch.from_numpy(M.get_boundaries(np.nan_to_num(c["gt"]), th=1, dilation=0))
    plain = ImageDataset(str(tmp_path / "rgb"), min_depth=MN, max_depth=MX).get_metrics(gt, pred, edges)
    assert tuple(plain) == ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")
    both = ImageDataset(str(tmp_path / "rgb"), min_depth=MN, max_depth=MX, ssi_metrics=True).get_metrics(gt, pred, edges)
    assert tuple(both) == tuple(plain) + SSI_KEYS
    assert all(both[k] == plain[k] for k in plain)
    want = M.compute_ssi_metrics(gt, pred, garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=MN, max_depth_eval=MX)
    assert {k: both[k] for k in SSI_KEYS} == want
    assert M.evaluate([both, both])["ssi_l1"] == both["ssi_l1"]


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_bound_and_exported_on_abi_20():
    from patchrefinerv2_amd import lib as L, metrics as M, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and re.search(rf"\bint(?:64_t)? {s}\(", hdr) and hasattr(raw, s), s
        args = re.search(rf"\bint(?:64_t)? {s}\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[s][1]), s
    assert "losses.py:523-544" in hdr and "losses.py:600-700" in hdr  # the entry cites its reference lines
    assert int(re.search(r"#define PRV2_SSI_VALUES (\d+)", hdr).group(1)) == L.SSI_VALUES == ops.SSI_VALUES == 41
    assert L.load().prv2_abi_version() == 20
    t = torch_ops.load()
    assert "ssi_metrics" in torch_ops.OPS and hasattr(t, "ssi_metrics") and hasattr(ops, "ssi_metrics")
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.ssi_metrics(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), 0.1, 10.0, 0, 4, 0, 4)
    for f in (M.compute_scale_and_shift, M.compute_ssi_metrics, M.compute_ssi_metrics_fused, M.ssi_from_values):
        assert callable(f)
    assert M.SSI_KEYS == SSI_KEYS
    mk = open(os.path.join(ROOT, "patchrefinerv2_amd", "csrc", "Makefile")).read()
    assert "ssi_eval.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1) and "-ffp-contract=off" in mk


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
    wsb = lib.prv2_ssi_metrics_workspace_bytes
    assert wsb(0, 16, 24) == -1 and wsb(1, 0, 24) == -1 and wsb(1, 16, -2) == -1 and wsb(65536, 16, 24) == -1
    one = wsb(1, 270, 480)
    assert one > 0 and wsb(3, 270, 480) == 3 * one  # per frame: a frame's blocks do not depend on the frame count

    def call(gt=P, pred=P, n=1, h=16, w=24, ph=16, pw=24, crop=(0, 16, 0, 24), out=P, ws=P, wsbytes=None):
        code = lib.prv2_ssi_metrics(gt, pred, n, h, w, ph, pw, 0.1, 10.0, *crop, out, ws, wsb(1, 16, 24) * max(n, 1) if wsbytes is None else wsbytes, None)
        assert code != 0
        return lib.prv2_last_error()
    assert b"null" in call(gt=None) and b"null" in call(pred=None) and b"null" in call(out=None) and b"workspace" in call(ws=None)
    assert b"frame count" in call(n=0)
    assert b"shape" in call(h=0) and b"prediction shape" in call(ph=0) and b"prediction shape" in call(pw=-1)
    assert b"2^31" in call(h=65536, w=32768, crop=(0, 1, 0, 1))
    for crop in ((-1, 16, 0, 24), (0, 17, 0, 24), (5, 4, 0, 24), (0, 16, 0, 25), (0, 16, 9, 8)):
        assert b"crop" in call(crop=crop)
    assert b"workspace" in call(wsbytes=8)
    assert b"ssi_metrics" in lib.prv2_last_error()
