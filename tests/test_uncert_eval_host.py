"""CPU: the sparsification scores (AUSE / AURG) of a per-pixel uncertainty without a GPU -- metrics.compute_uncertainty_metrics against a
literal stable-argsort implementation written here, its properties, Tester.generate_pl(uncert_metrics=True) over a stub model, and the
new entry points' declaration, binding and argument checks.  The scores are not in the reference: there is no golden file."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prv2_sparsify_workspace_bytes", "prv2_sparsify")
KEYS = ("ause_abs_rel", "aurg_abs_rel", "ause_rmse", "aurg_rmse")
CURVES = ("spars_abs_rel", "spars_rmse", "oracle_abs_rel", "oracle_rmse", "kept")
MN, MX = 0.1, 10.0


def frame(shape, seed, hard=True):
    """gt / pred / uncert / count fp32 of ``shape``: gt partly outside (MN, MX) and NaN, pred with NaN, inf and values outside the
    range, the uncertainty loosely following the error"""
    rs = np.random.RandomState(seed)
    h, w = shape
    gt = (0.3 + 9.0 * rs.rand(h, w)).astype(np.float32)
    pred = (gt * (1.0 + 0.2 * rs.randn(h, w))).astype(np.float32)
    uncert = (np.abs(gt - pred) * (0.5 + rs.rand(h, w))).astype(np.float32)
    count = rs.randint(1, 9, (h, w)).astype(np.float32)
    if hard and h * w >= 20:
        flat = rs.permutation(h * w)
        gt.flat[flat[0:3]] = (0.0, 11.0, np.nan)       # invalid pixels
        gt.flat[flat[3]] = np.inf
        pred.flat[flat[4:9]] = (np.nan, np.inf, -np.inf, 0.01, 25.0)  # cleaned: min, max, min, min, max
        pred.flat[flat[0]] = np.nan                     # outside the valid set: never looked at
    return gt, pred, uncert, count


def literal(gt, pred, uncert, count=None, min_count=0, mn=MN, mx=MX, levels=20):
    """the definition by a stable argsort: keep the first n_k of the order, then add the ties of the last kept key"""
    mn32, mx32 = np.float32(mn), np.float32(mx)
    with np.errstate(invalid="ignore"):
        valid = (gt > mn32) & (gt < mx32)
    p = pred.copy()
    for i in range(p.size):
        v = p.flat[i]
        if np.isnan(v):
            v = mn32
        elif v < mn32:
            v = mn32
        elif v > mx32:
            v = mx32
        p.flat[i] = v
    key = uncert.copy()
    if count is not None:
        key[count.astype(np.float64) < min_count] = np.inf
    g, p, key = gt[valid], p[valid], key[valid]
    n = g.size
    e_rel = (np.abs(g - p) / g).astype(np.float32)
    e_sq = ((g - p) * (g - p)).astype(np.float32)

    def sets(K):
        order = np.argsort(K, kind="stable")  # NaN last
        for k in range(levels):
            nk = n - (n * k) // levels
            keep = np.zeros(n, bool)
            keep[order[:nk]] = True
            last = K[order[nk - 1]]
            for i in order[nk:]:  # the ties of the last kept key (a NaN ties with every NaN)
                if K[i] == last or (np.isnan(K[i]) and np.isnan(last)):
                    keep[i] = True
                else:
                    break
            yield last, keep
    out = {c: np.zeros(levels) for c in CURVES}
    thr = np.zeros((3, levels), np.float32)
    for k, (t, keep) in enumerate(sets(key)):
        thr[0, k] = t
        out["kept"][k] = keep.sum() / n
        out["spars_abs_rel"][k] = e_rel[keep].astype(np.float64).sum() / keep.sum()
        out["spars_rmse"][k] = np.sqrt(e_sq[keep].astype(np.float64).sum() / keep.sum())
    for k, (t, keep) in enumerate(sets(e_rel)):
        thr[1, k] = t
        out["oracle_abs_rel"][k] = e_rel[keep].astype(np.float64).sum() / keep.sum()
    for k, (t, keep) in enumerate(sets(e_sq)):
        thr[2, k] = t
        out["oracle_rmse"][k] = np.sqrt(e_sq[keep].astype(np.float64).sum() / keep.sum())
    out["thresholds"] = thr
    for x in ("abs_rel", "rmse"):
        out["ause_" + x] = float(np.mean(out["spars_" + x] - out["oracle_" + x]))
        out["aurg_" + x] = float(np.mean(out["spars_" + x][0] - out["spars_" + x]))
    return out


def spec(*a, **kw):
    from patchrefinerv2_amd import metrics as M
    kw.setdefault("min_depth_eval", MN)
    kw.setdefault("max_depth_eval", MX)
    return M.compute_uncertainty_metrics(*a, **kw)


# ------------------------------------------------------------------------------------------------------------------ the specification
@pytest.mark.parametrize("shape,levels,quant,gate", [((13, 17), 20, False, False), ((13, 17), 20, True, False), ((9, 31), 7, False, True),
                                                    ((20, 20), 64, True, True), ((5, 7), 20, False, False), ((3, 3), 1, False, False)])
def test_specification_against_a_literal_argsort(shape, levels, quant, gate):
    gt, pred, uncert, count = frame(shape, 7 * shape[0] + levels)
    if quant:
        uncert = (np.floor(uncert * 4 / max(float(uncert.max()), 1e-6)).clip(0, 3) / 4).astype(np.float32)  # four values: massive ties
    kw = dict(count=count, min_count=3.5) if gate else {}
    got = spec(gt, pred, uncert, levels=levels, curves=True, **kw)
    want = literal(gt, pred, uncert, levels=levels, **kw)
    assert tuple(got)[:4] == KEYS and all(k in got for k in CURVES)
    assert np.array_equal(got["thresholds"], want["thresholds"], equal_nan=True)
    for k in CURVES:
        assert got[k].shape == (levels,)
        np.testing.assert_allclose(got[k], want[k], rtol=1e-13, atol=0, err_msg=k)  # the same fp32 terms, float64 sums in another order
    for k in KEYS:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-13 * max(1.0, float(np.abs(want["spars_rmse"]).max())), err_msg=k)
    assert set(spec(gt, pred, uncert, levels=levels, **kw)) == set(KEYS)
    assert got["kept"][0] == 1.0 and (np.diff(got["kept"]) <= 0).all() and got["n"] == int(got["kept_count"][0])
    # torch tensors and [1, 1, H, W] are the same frame
    t = lambda a: torch.from_numpy(a)[None, None]  # noqa: E731
    assert spec(t(gt), t(pred), t(uncert), levels=levels, **{k: (t(v) if k == "count" else v) for k, v in kw.items()}) == {k: got[k] for k in KEYS}


def test_terms_are_fp32_and_the_prediction_is_cleaned():
    gt = np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]], np.float32)
    pred = np.array([[np.nan, np.inf, -np.inf, 0.01, 25.0, 6.5]], np.float32)
    r = spec(gt, pred, np.zeros_like(gt), levels=1, curves=True)
    clean = np.array([MN, MX, MN, MN, MX, 6.5], np.float32)
    e_rel = np.abs(gt[0] - clean) / gt[0]
    assert e_rel.dtype == np.float32
    assert r["spars_abs_rel"][0] == e_rel.astype(np.float64).sum() / 6 and r["thresholds"][1, 0] == e_rel.max()
    assert r["thresholds"][2, 0] == ((gt[0] - clean) * (gt[0] - clean)).max()


def test_uncertainty_equal_to_the_error_is_the_oracle():
    gt, pred, _, _ = frame((13, 17), 3, hard=False)
    g, p = gt, np.clip(pred, np.float32(MN), np.float32(MX))
    r = spec(gt, pred, np.abs(g - p) / g, curves=True)
    assert r["ause_abs_rel"] == 0.0 and np.array_equal(r["spars_abs_rel"], r["oracle_abs_rel"])
    assert r["aurg_abs_rel"] > 0 and r["ause_rmse"] >= 0
    r = spec(gt, pred, (g - p) * (g - p))
    assert r["ause_rmse"] == 0.0


def test_constant_uncertainty_gives_a_flat_curve():
    gt, pred, _, _ = frame((13, 17), 4)
    r = spec(gt, pred, np.full_like(gt, 0.25), curves=True)
    assert r["aurg_abs_rel"] == 0.0 and r["aurg_rmse"] == 0.0 and (r["kept"] == 1.0).all()
    assert (r["spars_abs_rel"] == r["spars_abs_rel"][0]).all() and r["ause_abs_rel"] > 0


def test_inverted_uncertainty_gains_nothing():
    gt, pred, _, _ = frame((13, 17), 5, hard=False)
    g, p = gt, np.clip(pred, np.float32(MN), np.float32(MX))
    r = spec(gt, pred, -(np.abs(g - p) / g))
    assert r["aurg_abs_rel"] <= 0 and r["ause_abs_rel"] > 0


def test_no_valid_pixel_gives_nan_and_fewer_pixels_than_levels_work():
    gt, pred, uncert, _ = frame((5, 7), 6)
    r = spec(np.zeros_like(gt), pred, uncert, curves=True)
    assert all(np.isnan(r[k]) for k in KEYS) and all(np.isnan(r[k]).all() for k in CURVES) and r["n"] == 0
    g7 = np.zeros_like(gt)
    g7.flat[[1, 5, 9, 13, 20, 27, 33]] = gt.flat[[1, 5, 9, 13, 20, 27, 33]]
    g7[g7 == 0] = 0.0
    r = spec(g7, np.nan_to_num(pred, nan=1.0, posinf=1.0, neginf=1.0), uncert, levels=20, curves=True)
    assert r["n"] == 7 and all(np.isfinite(r[k]) for k in KEYS)
    want = literal(g7, np.nan_to_num(pred, nan=1.0, posinf=1.0, neginf=1.0), uncert, levels=20)
    assert np.array_equal(r["kept"], want["kept"]) and sorted(set(r["kept_count"])) == list(range(1, 8))  # n_k = 7 - floor(7 k / 20)


def test_nan_and_inf_uncertainty_order_last():
    gt, pred, uncert, _ = frame((10, 10), 8, hard=False)  # 100 valid pixels
    u = uncert.copy()
    u.flat[[3, 40]] = np.nan
    u.flat[[7, 8, 77]] = np.inf
    r = spec(gt, pred, u, levels=50, curves=True)  # n_k = 100 - 2 k: 95 finite keys, then three +inf, then two NaN
    assert np.isnan(r["thresholds"][0, 0]) and r["kept_count"][0] == 100  # level 0: the NaN threshold keeps everything
    assert r["thresholds"][0, 1] == np.inf and r["kept_count"][1] == 98   # level 1 (98 wanted): the NaN are gone first
    assert r["thresholds"][0, 2] == np.inf and r["kept_count"][2] == 98   # level 2 (96 wanted): the three +inf tie and stay
    assert np.isfinite(r["thresholds"][0, 3]) and r["kept_count"][3] == 94


def test_count_override_removes_exactly_the_low_count_pixels_at_level_one():
    gt, pred, uncert, _ = frame((10, 10), 9, hard=False)
    count = np.full_like(gt, 8.0)
    low = [2, 50, 51, 99]  # 4 pixels < n / L = 5
    count.flat[low] = 1.0
    r = spec(gt, pred, uncert, count=count, min_count=0.05 * 40, levels=20, curves=True)
    assert r["thresholds"][0, 0] == np.inf and r["kept_count"][0] == 100
    assert r["kept_count"][1] == 95 and np.isfinite(r["thresholds"][0, 1])
    keep = np.ones(100, bool)
    keep[low] = False
    d = gt.ravel() - np.clip(pred.ravel(), np.float32(MN), np.float32(MX))
    e = (np.abs(d) / gt.ravel())
    # the 95 wanted at level 1 are the 96 gated-in pixels minus the most uncertain one
    rest = np.where(keep)[0]
    rest = rest[np.argsort(uncert.ravel()[rest], kind="stable")][:95]
    np.testing.assert_allclose(r["spars_abs_rel"][1], e[rest].astype(np.float64).sum() / 95, rtol=1e-14)
    assert spec(gt, pred, uncert, count=count, min_count=0.5) == spec(gt, pred, uncert)  # nothing under the threshold: no override


def test_pixels_outside_the_depth_range_never_contribute():
    gt, pred, uncert, count = frame((13, 17), 10)
    a = spec(gt, pred, uncert, curves=True)
    with np.errstate(invalid="ignore"):
        out = ~((gt > np.float32(MN)) & (gt < np.float32(MX)))
    assert out.sum() >= 4
    p2, u2 = pred.copy(), uncert.copy()
    p2[out], u2[out] = 1e6, np.nan
    b = spec(gt, p2, u2, curves=True)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    sub = spec(gt[~out][None], pred[~out][None], uncert[~out][None], curves=True)  # the valid pixels alone, as one row
    assert sub["n"] == a["n"] and np.array_equal(sub["thresholds"], a["thresholds"]) and np.array_equal(sub["kept_count"], a["kept_count"])


def test_shapes_and_levels_are_checked():
    from patchrefinerv2_amd import metrics as M
    gt, pred, uncert, count = frame((5, 7), 11)
    with pytest.raises(ValueError, match="resize"):
        spec(gt, pred[:4], uncert)
    with pytest.raises(ValueError, match="resize"):
        spec(gt, pred, uncert, count=count[:, :6])
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="levels"):
            spec(gt, pred, uncert, levels=bad)
        with pytest.raises(ValueError, match="levels"):
            M.uncertainty_from_values(np.zeros(11), bad)
    assert M.UNCERT_KEYS == KEYS and M.UNCERT_CURVES == CURVES


def test_values_row_to_scores():
    """uncertainty_from_values on a hand-made row of prv2_sparsify: n, 3 L thresholds, seven rows of L suffix sums"""
    from patchrefinerv2_amd import metrics as M
    L = 2
    row = np.array([4.0] + [9, 1, 8, 2, 7, 3] + [4, 2, 2.0, 0.5, 8.0, 0.5, 4, 2, 2.0, 0.25, 4, 3, 8.0, 0.75])
    r = M.uncertainty_from_values(row, L, curves=True)
    assert np.array_equal(r["kept"], [1.0, 0.5]) and np.array_equal(r["spars_abs_rel"], [0.5, 0.25]) and np.array_equal(r["spars_rmse"], [np.sqrt(2), 0.5])
    assert np.array_equal(r["oracle_abs_rel"], [0.5, 0.125]) and np.array_equal(r["oracle_rmse"], [np.sqrt(2), 0.5])
    assert r["ause_abs_rel"] == 0.0625 and r["aurg_abs_rel"] == 0.125 and r["ause_rmse"] == 0.0
    assert np.array_equal(r["thresholds"], np.array([[9, 1], [8, 2], [7, 3]], np.float32))
    empty = M.uncertainty_from_values(np.r_[0.0, np.full(6, np.nan), np.zeros(14)], L)
    assert tuple(empty) == KEYS and all(np.isnan(v) for v in empty.values())


# ------------------------------------------------------------------------------------------------------------------ the tester's flag
H, W, N_TILES = 12, 20, 40


class StubModel:
    """what generate_pl needs of a model (as tests/test_uncertainty_host.py's): host maps, no return_device"""
    device = torch.device("cpu")
    needs_coarse = False

    def __init__(self, out_shape=(H, W)):
        self.out_shape, self.kw = out_shape, []

    def resizer(self, hr):
        return hr[:, :, ::2, ::2]

    def __call__(self, mode=None, image_hr=None, return_uncertainty=False, **kw):
        self.kw.append(kw)
        b = image_hr.shape[0]
        g = torch.Generator().manual_seed(3)
        t = lambda: torch.rand(b, 1, *self.out_shape, generator=g) * 3 + 0.5  # noqa: E731
        self.last_plan = [dict(kind="init", raw=[(0, 0)] * N_TILES)]
        return t(), dict(uncertainty=t(), count_map=torch.floor(t() * 4))


class StubDataset:
    min_depth, max_depth = MN, MX

    def __init__(self, n, gt_every=0):
        self.n, self.gt_every = n, gt_every

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        item = dict(image_hr=torch.zeros(3, H, W), img_file_basename=f"img{i}")
        if self.gt_every and i % self.gt_every == 0:
            item["depth_gt"] = torch.full((1, 1, H, W), 2.0)
        return item


def _tester(ds, model, tmp_path, save=True):
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    return Tester(None, RunnerInfo(rank=0, world_size=1, save=save, work_dir=str(tmp_path)), ds, model)


def test_generate_pl_without_the_flag_is_unchanged_and_items_without_gt_are_skipped(tmp_path):
    import inspect
    from patchrefinerv2_amd.tester import Tester
    assert inspect.signature(Tester.generate_pl).parameters["uncert_metrics"].default is False
    a = _tester(StubDataset(2, gt_every=1), StubModel(), tmp_path / "a")
    res_a = a.generate_pl(image_raw_shape=(H, W), patch_split_num=(2, 2))  # ground truth present, flag off: nothing is scored
    assert all(set(r) == {"name", "shape", "mean", "n_tiles"} for r in res_a) and not hasattr(a, "last_eval")
    model = StubModel()
    b = _tester(StubDataset(2), model, tmp_path / "b")
    res_b = b.generate_pl(image_raw_shape=(H, W), patch_split_num=(2, 2), uncert_metrics=True)  # flag on, no ground truth: skipped
    assert res_b == res_a and b.last_eval == {}
    assert all("return_device" not in kw for kw in model.kw)
    for name in sorted(os.listdir(tmp_path / "a")):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    assert len(os.listdir(tmp_path / "b")) == 10


def test_generate_pl_flag_with_a_result_of_another_shape_names_the_shapes(tmp_path):
    t = _tester(StubDataset(1, gt_every=1), StubModel(out_shape=(8, 16)), tmp_path, save=False)
    with pytest.raises(ValueError, match=r"\(8, 16\).*\(12, 20\).*r-modes return the raw shape"):
        t.generate_pl(cai_mode="m1", image_raw_shape=(H, W), patch_split_num=(2, 2), uncert_metrics=True)


def test_cli_offers_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--uncert-metrics" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "cfg.py", "--uncert-metrics"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--uncert-metrics needs --generate-pl" in r.stderr


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
    assert "n_k = n - floor(n k / L)" in hdr and "ties are kept" in hdr  # the header states the definition
    assert int(re.search(r"#define PRV2_SPARSIFY_MAX_LEVELS (\d+)", hdr).group(1)) == L.SPARSIFY_MAX_LEVELS == ops.SPARSIFY_MAX_LEVELS == 64
    assert re.search(r"#define PRV2_SPARSIFY_VALUES\(L\) \(1 \+ 10 \* \(L\)\)", hdr) and L.sparsify_values(20) == 201
    assert L.load().prv2_abi_version() == 20
    t = torch_ops.load()
    assert "sparsify" in torch_ops.OPS and hasattr(t, "sparsify") and hasattr(ops, "sparsify")
    with pytest.raises((RuntimeError, NotImplementedError)):
        t.sparsify(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), None, 0.0, 0.1, 10.0, 20)
    for f in (M.compute_uncertainty_metrics, M.compute_uncertainty_metrics_fused, M.uncertainty_from_values):
        assert callable(f)
    mk = open(os.path.join(ROOT, "patchrefinerv2_amd", "csrc", "Makefile")).read()
    assert "sparsify.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1) and "-ffp-contract=off" in mk


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first
    wsb = lib.prv2_sparsify_workspace_bytes
    assert wsb(0, 16, 24, 20) == -1 and wsb(1, 0, 24, 20) == -1 and wsb(1, 16, -2, 20) == -1 and wsb(65536, 16, 24, 20) == -1
    assert wsb(1, 16, 24, 0) == -1 and wsb(1, 16, 24, 65) == -1 and wsb(1, 32768, 32768, 20) == -1
    one = wsb(1, 270, 480, 20)
    assert one >= 13 * 270 * 480 and wsb(1, 270, 480, 64) > one

    def call(gt=P, pred=P, uncert=P, count=None, n=1, h=16, w=24, levels=20, out=P, ws=P, wsbytes=None):
        nbytes = wsb(max(n, 1), 16, 24, 20) if wsbytes is None else wsbytes
        code = lib.prv2_sparsify(gt, pred, uncert, count, 0.0, n, h, w, 0.1, 10.0, levels, out, ws, nbytes, None)
        assert code != 0
        return lib.prv2_last_error()
    assert b"null" in call(gt=None) and b"null" in call(pred=None) and b"null" in call(uncert=None) and b"null" in call(out=None)
    assert b"workspace" in call(ws=None) and b"misaligned" in call(ws=P + 4)
    assert b"frame count" in call(n=0) and b"shape" in call(h=0) and b"shape" in call(w=-1)
    assert b"2^29" in call(h=32768, w=32768)
    assert b"levels" in call(levels=0) and b"levels" in call(levels=65)
    assert b"workspace" in call(wsbytes=wsb(1, 16, 24, 20) - 1)
    assert b"sparsify" in lib.prv2_last_error()


def test_wrappers_reject_wrong_inputs_without_gpu():
    """every check comes before the first launch; the last one is the device"""
    from patchrefinerv2_amd import metrics as M, ops
    z = torch.zeros(2, 5, 7)
    ok = dict(gt=z, pred=z, uncert=z)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.sparsify(**ok)  # host tensors
    with pytest.raises(ValueError, match="dtype"):
        ops.sparsify(**dict(ok, pred=z.double()))
    with pytest.raises(ValueError, match="dtype"):
        ops.sparsify(**ok, count=z.int())
    with pytest.raises(ValueError, match=r"expected \[H, W\] or \[B, H, W\]"):
        ops.sparsify(**dict(ok, uncert=z[None]))
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.sparsify(**dict(ok, gt=np.zeros((5, 7), np.float32)))
    with pytest.raises(ValueError, match="does not match gt"):
        ops.sparsify(**dict(ok, pred=z[:, :4]))
    with pytest.raises(ValueError, match="does not match gt"):
        ops.sparsify(**ok, count=z[:1])
    for bad in (0, 65):
        with pytest.raises(ValueError, match="levels"):
            ops.sparsify(**ok, levels=bad)
        with pytest.raises(ValueError, match="levels"):
            M.compute_uncertainty_metrics_fused(z, z, z, levels=bad)
    with pytest.raises(ValueError, match="GPU tensor"):
        M.compute_uncertainty_metrics_fused(z, z, z)
