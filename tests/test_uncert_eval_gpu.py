"""GPU: the sparsification scores (AUSE / AURG) -- csrc/sparsify.hip on both dispatch routes against the host specification
metrics.compute_uncertainty_metrics (thresholds and kept counts bit for bit, curves and scores within RTOL), its bit-exactness
(call to call, torch op or C ABI), and Tester.generate_pl(uncert_metrics=True) / tools/test.py --uncert-metrics over a two-frame
synthetic U4K tree.

RTOL: both sides add the same fp32 terms in float64, only the order differs.  A curve value is compared relative to itself; a score is a
mean of differences of curve values (it may cancel to nothing), so it is compared relative to the largest value of its sparsification
curve in the specification.  The largest deviation measured over every case below on one MI355X is MEASURED; the tests assert four
times that (the project's habit, tests/test_eth_dataset_gpu.py), which is far inside 1e-9, the bound --ssi-metrics uses for float64
sums."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_u4k_eval_gpu import FRAMES, RAW, SPLIT, _write_cfg, route  # noqa: E402,F401
from test_u4k_eval_host import write_u4k_tree  # noqa: E402
from test_uncert_eval_host import CURVES, KEYS, MN, MX, frame  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
MEASURED = 3.683e-16  # one MI355X, [1, 384, 512] gated, both routes (the sums are in a fixed order: the figure repeats from run to run)
RTOL = 4 * MEASURED
assert RTOL <= 1e-9
LEVELS = 20
torch.set_grad_enabled(False)

# [1, 5, 7]: n < L, less than one wave; [2, 37, 53]: two frames with different valid counts, ragged against every tile; [1, 64, 257]: a
# row length that is no multiple of 4; [1, 384, 512]: 48 blocks of the sums pass and the final reduction over them
SHAPES = [(1, 5, 7), (2, 37, 53), (1, 64, 257), (1, 384, 512)]
CONTENTS = ["continuous", "quantised", "gated", "empty_frame", "dirty_pred"]


@functools.lru_cache(maxsize=None)
def case(shape, content):
    """-> (gt, pred, uncert, count or None, min_count, [the specification's dict per frame]); built and scored once per session"""
    from patchrefinerv2_amd import metrics as M
    b, h, w = shape
    maps = []
    for f in range(b):
        gt, pred, uncert, count = frame((h, w), 100 * h + 10 * f + CONTENTS.index(content), hard=content == "dirty_pred")
        if h * w < 64:  # n < L: eleven valid pixels
            keep = np.zeros(h * w, bool)
            keep[[0, 3, 4, 9, 13, 17, 18, 22, 29, 30, 34]] = True
            gt = np.where(keep.reshape(h, w), gt, np.float32(0))
        if f == 1:  # another valid count than frame 0
            gt[: h // 3] = 0.0
            gt[:, w // 2:w // 2 + 5] = 20.0
        if content == "quantised":  # four values: massive ties
            uncert = (np.floor(uncert * 4 / float(uncert.max())).clip(0, 3) / 4).astype(np.float32)
        if content == "gated":  # a third of the pixels under min_count
            count = (np.arange(h * w).reshape(h, w) % 3 + 1).astype(np.float32) * 4
        maps.append((gt, pred, uncert, count))
    if content == "empty_frame":  # a frame without a valid pixel in front of the valid ones
        gt, pred, uncert, count = maps[0]
        maps.insert(0, (np.zeros_like(gt), pred, uncert, count))
    gt, pred, uncert, count = (np.stack([m[k] for m in maps]) for k in range(4))
    min_count = 6.0 if content == "gated" else 0.0
    cnt = count if content == "gated" else None
    want = [M.compute_uncertainty_metrics(gt[f], pred[f], uncert[f], None if cnt is None else cnt[f], min_count, MN, MX, LEVELS, curves=True)
            for f in range(gt.shape[0])]
    return gt, pred, uncert, cnt, min_count, want


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(ops, c):
    gt, pred, uncert, cnt, min_count, _ = c
    return ops.sparsify(dev(gt), dev(pred), dev(uncert), dev(cnt), min_count, MN, MX, LEVELS)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def f32_bits_equal(a, b):
    """bit for bit, every NaN one value"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def deviation(got, want, what):
    """the largest relative deviation of the curves and scores; asserts RTOL after printing every figure"""
    worst = 0.0
    for k in CURVES:
        d = float(np.max(np.abs(got[k] - want[k]) / np.abs(want[k]))) if np.all(want[k] != 0) else float(np.max(np.abs(got[k] - want[k])))
        print(f"{what} {k}: rel {d:.3e}")
        worst = max(worst, d)
    for k in KEYS:
        scale = float(np.max(np.abs(want["spars_" + k.split("_", 1)[1]])))
        d = abs(got[k] - want[k]) / scale if scale else abs(got[k] - want[k])
        print(f"{what} {k}: got {got[k]!r} want {want[k]!r} rel-to-curve {d:.3e}")
        worst = max(worst, d)
    print(f"{what}: largest relative deviation {worst:.3e}")
    assert worst <= RTOL, (what, worst)
    return worst


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_op_against_the_host_specification(route, shape, content):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    c = case(shape, content)
    want = c[5]
    out = run(route, c)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(want), 1 + 10 * LEVELS) and out.is_cuda
    assert same_bits(run(route, c), out)  # the same bits on every call
    rows = out.cpu().numpy()
    counts = {w["n"] for w in want}
    assert len(counts) == len(want)  # the frames of a batch differ in their valid count
    for f, (row, w) in enumerate(zip(rows, want)):
        what = f"{route.DISPATCH} {shape} {content} frame {f}"
        got = M.uncertainty_from_values(row, LEVELS, curves=True)
        assert got["n"] == w["n"] == row[0], what
        if w["n"] == 0:
            assert np.isnan(row[1:1 + 3 * LEVELS]).all() and (row[1 + 3 * LEVELS:] == 0).all(), what
            assert all(np.isnan(got[k]) for k in KEYS)
            continue
        assert f32_bits_equal(got["thresholds"], w["thresholds"]), what
        assert np.array_equal(got["kept_count"], w["kept_count"]) and np.array_equal(row[1 + 3 * LEVELS:1 + 4 * LEVELS], w["kept_count"]), what
        deviation(got, w, what)
    if content == "gated" and shape[1] * shape[2] >= 64:  # the gated third ties at +inf: kept whole until n_k drops under the other two thirds
        assert np.isinf(want[0]["thresholds"][0, 0]) and want[0]["kept_count"][7] < want[0]["n"] * 0.67
    if content == "quantised":
        assert len(set(want[0]["kept_count"])) <= 4
    if shape == (1, 5, 7):
        assert 1 <= want[-1]["n"] <= 11 < LEVELS


@pytest.mark.parametrize("shape,content", [((2, 37, 53), "gated"), ((1, 384, 512), "dirty_pred"), ((1, 64, 257), "empty_frame")])
def test_fused_route_returns_the_specifications_dicts(route, shape, content):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    gt, pred, uncert, cnt, min_count, want = case(shape, content)
    got = M.compute_uncertainty_metrics_fused(dev(gt), dev(pred), dev(uncert), dev(cnt), min_count, MN, MX, LEVELS, curves=True)
    assert isinstance(got, list) and len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert tuple(g)[:4] == KEYS
        if w["n"]:
            deviation(g, w, f"fused {route.DISPATCH} {shape} {content} frame {f}")
        else:
            assert all(np.isnan(g[k]) for k in KEYS)
    one = M.compute_uncertainty_metrics_fused(dev(gt[-1]), dev(pred[-1]), dev(uncert[-1]), None if cnt is None else dev(cnt[-1]), min_count, MN,
                                              MX, LEVELS)  # [H, W]: a dict, and a frame alone has the bits it has in a batch
    assert one == {k: got[-1][k] for k in KEYS}
    with pytest.raises(ValueError, match="resize"):
        M.compute_uncertainty_metrics_fused(dev(gt), dev(pred[:, :-1]), dev(uncert))


def test_uncertainty_equal_to_the_error_is_the_oracle_on_the_device(route):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    gt, pred, _, _, _, _ = case((1, 64, 257), "continuous")
    g, p = gt[0], np.clip(pred[0], np.float32(MN), np.float32(MX))
    r = M.compute_uncertainty_metrics_fused(dev(gt[0]), dev(pred[0]), dev(np.abs(g - p) / g), None, 0, MN, MX, LEVELS, curves=True)
    assert r["ause_abs_rel"] == 0.0 and np.array_equal(r["spars_abs_rel"], r["oracle_abs_rel"])  # the same buckets, the same order of sums
    flat = M.compute_uncertainty_metrics_fused(dev(gt[0]), dev(pred[0]), dev(np.full_like(g, 0.5)), None, 0, MN, MX, LEVELS)
    assert flat["aurg_abs_rel"] == 0.0 and flat["aurg_rmse"] == 0.0


def test_torch_op_and_c_abi_agree_bitwise(monkeypatch):
    from patchrefinerv2_amd import ops
    got = {}
    for r in ("ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", r)
        got[r] = [run(ops, case(s, c)) for s, c in (((2, 37, 53), "gated"), ((1, 384, 512), "continuous"), ((1, 5, 7), "empty_frame"))]
    for a, b in zip(got["ctypes"], got["torch"]):
        assert same_bits(a, b)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def pl_run(tmp_path_factory):
    """a two-frame synthetic U4K tree, the model the CLI would build for it (synthetic weights), and Tester.generate_pl in an r-mode
    with and without the flag, same seed; ``scored`` holds host copies of the device maps the scoring was handed"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS, Config, build_model
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    tmp = tmp_path_factory.mktemp("uncert")
    root = str(tmp / "data")
    write_u4k_tree(root, FRAMES, RAW, seed=5)
    cfg_path = _write_cfg(tmp, root)
    cfg = Config.fromfile(cfg_path)
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)  # tools/test.py's defaults
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    ds = DATASETS.build(dict(cfg.val_dataloader.dataset.to_dict(), image_raw_shape=list(RAW)))
    kw = dict(cai_mode="r4", image_raw_shape=RAW, patch_split_num=SPLIT, count_thr=0.2, seed=621)
    off = Tester(None, RunnerInfo(rank=0, world_size=1, save=True, work_dir=str(tmp / "off")), ds, model)
    res_off = off.generate_pl(**kw)
    on = Tester(None, RunnerInfo(rank=0, world_size=1, save=True, work_dir=str(tmp / "on")), ds, model)
    scored = []
    inner = on._uncert_metrics

    def recording(item, depth, uncertainty, count_map, min_count, cai_mode):
        assert depth.is_cuda and uncertainty.is_cuda and count_map.is_cuda and item["depth_gt"].is_cuda  # nothing extra crosses PCIe
        out = inner(item, depth, uncertainty, count_map, min_count, cai_mode)  # (raises for a result of another shape)
        scored.append(tuple(t.cpu().numpy().reshape(RAW) for t in (item["depth_gt"], depth, uncertainty, count_map)) + (min_count,))
        return out
    on._uncert_metrics = recording
    res_on = on.generate_pl(uncert_metrics=True, **kw)
    last_eval = dict(on.last_eval)
    with pytest.raises(ValueError, match=r"r-modes return the raw shape") as err:
        on.generate_pl(uncert_metrics=True, **dict(kw, cai_mode="m1"))
    ds.close()
    return dict(tmp=tmp, cfg=cfg_path, ds=ds, off=res_off, on=res_on, scored=scored[:2], last_eval=last_eval, off_tester=off, err=str(err.value))


def test_generate_pl_scores_equal_the_specification_on_the_models_maps(pl_run):
    from patchrefinerv2_amd import metrics as M
    assert len(pl_run["scored"]) == 2 and [r["name"] for r in pl_run["on"]] == ["0001_Image0_00002", "0001_Image0_00004"]
    for r, (gt, depth, unc, count, min_count) in zip(pl_run["on"], pl_run["scored"]):
        assert r["shape"] == (1, 1) + RAW and tuple(r["uncert_metrics"]) == KEYS
        assert min_count == 0.2 * r["n_tiles"] and (count < min_count).any() and (count >= min_count).any()
        want = M.compute_uncertainty_metrics(gt, depth, unc, count, min_count, 1e-3, 80, LEVELS, curves=True)
        assert want["n"] > 1000 and all(np.isfinite(r["uncert_metrics"][k]) for k in KEYS)
        # the model's maps are not among the cases MEASURED covers, so the bound here is the worst case of the arithmetic: a float64 sum
        # of n non-negative terms is within (n - 1) 2^-53 of the exact sum in any order, two orders are within twice that
        rtol = min(1e-9, 2 * want["n"] * 2.0 ** -53)
        for k in KEYS:
            scale = float(np.max(np.abs(want["spars_" + k.split("_", 1)[1]])))
            d = abs(r["uncert_metrics"][k] - want[k]) / scale
            print(f"{r['name']} {k}: got {r['uncert_metrics'][k]!r} want {want[k]!r} rel-to-curve {d:.3e}")
            assert d <= rtol, (r["name"], k, d, rtol)
    assert pl_run["on"][0]["uncert_metrics"] != pl_run["on"][1]["uncert_metrics"]


def test_last_eval_is_the_nanmean(pl_run):
    rows = [r["uncert_metrics"] for r in pl_run["on"]]
    assert pl_run["last_eval"] == {k: float(np.nanmean([m[k] for m in rows])) for k in KEYS}


def test_without_the_flag_nothing_changes(pl_run):
    assert all("uncert_metrics" not in r for r in pl_run["off"]) and not hasattr(pl_run["off_tester"], "last_eval")
    assert pl_run["off"] == [{k: v for k, v in r.items() if k != "uncert_metrics"} for r in pl_run["on"]]
    off, on = pl_run["tmp"] / "off", pl_run["tmp"] / "on"
    names = sorted(os.listdir(off))
    assert names == sorted(os.listdir(on)) and len(names) == 10
    for name in names:
        assert (off / name).read_bytes() == (on / name).read_bytes(), name


def test_m_mode_with_the_flag_names_the_shapes(pl_run):
    assert "(224, 448)" in pl_run["err"] and str(RAW) in pl_run["err"] and "m1" in pl_run["err"]


def test_cli_prints_the_four_keys(pl_run):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), pl_run["cfg"], "--synthetic-weights", "--cai-mode", "r4",
                        "--test-type", "normal", "--image-raw-shape", str(RAW[0]), str(RAW[1]), "--patch-split-num", "2", "2", "--generate-pl",
                        "--count-thr", "0.2", "--uncert-metrics"], capture_output=True, text=True, timeout=600, cwd=str(pl_run["tmp"]))
    assert r.returncode == 0, r.stderr[-2000:]
    for res in pl_run["on"]:
        line = re.search(rf"{res['name']}: (ause_abs_rel .*)", r.stdout)
        assert line, r.stdout[-2000:]
        printed = {k: float(v) for k, v in (kv.split(" ") for kv in line.group(1).split(", "))}
        assert tuple(printed) == KEYS
        for k, v in printed.items():
            assert abs(v - res["uncert_metrics"][k]) <= 1e-6 * max(1.0, abs(res["uncert_metrics"][k])), (k, v, res["uncert_metrics"][k])
    summary = [ln for ln in r.stdout.splitlines() if "ause_abs_rel" in ln and "aurg_rmse" in ln and "Image0" not in ln]
    assert summary, r.stdout[-2000:]
