"""GPU: edge-aware evaluation (csrc/edges.hip).  The device Canny equals metrics.canny bit for bit on the same fp32 input, the
exact distance transform equals scipy's, the boundary statistics equal the host version, everything is deterministic and B frames
equal B single calls; the Tester scores frames with edge metrics on the device as the host route does."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)


def _dev_canny(img):
    from patchrefinerv2_amd import ops
    return ops.canny(torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(DEV))[0].cpu().numpy()


def _check_canny(img, what=""):
    from patchrefinerv2_amd import metrics as M
    ref = M.canny(img)
    got = _dev_canny(img)
    assert np.array_equal(got, ref), (what, img.shape, int((got != ref).sum()), int(ref.sum()))
    return ref


def _smooth(rng, shape, s, amp=1.0):
    return (ndi.gaussian_filter(rng.standard_normal(shape), s) * amp).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ Canny
@pytest.mark.parametrize("shape", [(3, 3), (5, 7), (37, 53), (1080, 1920), (2160, 3840)])
def test_canny_bit_identical_smooth_fields(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for k, (s, amp) in enumerate([(2.0, 30.0), (0.7, 3.0)] if min(shape) > 100 else [(1.0, 20.0), (0.5, 2.0), (3.0, 80.0)]):
        _check_canny(_smooth(rng, shape, s, amp), f"smooth {k}")


def test_canny_steps_and_ramps_eight_orientations():
    y, x = np.mgrid[0:61, 0:83].astype(np.float64)
    for k in range(8):
        a = k * np.pi / 8
        u = np.cos(a) * (x - 41) + np.sin(a) * (y - 30)
        _check_canny((u > 0.3).astype(np.float32) * 1.5, f"step {k}")
        _check_canny((0.2 * u + 2.0 * (u > 5)).astype(np.float32), f"ramp+step {k}")
        _check_canny(np.clip(u, -4, 4).astype(np.float32) * 0.4, f"ramp {k}")


def test_canny_gradient_ties_zeros_and_plateaus():
    y, x = np.mgrid[0:48, 0:64].astype(np.float32)
    _check_canny(((x + y) > 50).astype(np.float32), "diagonal step |gx| == |gy|")
    _check_canny(((x - y) > 10).astype(np.float32) * 3, "anti-diagonal step")
    _check_canny(np.zeros((48, 64), np.float32), "zero")
    _check_canny(np.full((48, 64), 5.0, np.float32), "constant")
    p = np.zeros((48, 64), np.float32)
    p[10:30, 10:30], p[20:40, 30:50] = 2.0, 2.0  # plateaus meeting at corners
    p[5:8, 55:60] = 1.0
    _check_canny(p, "plateaus")
    c = ((x // 4 + y // 4) % 2).astype(np.float32)  # checkerboard: every sector and many exact ties
    _check_canny(c, "checker")


def test_canny_nan_and_inf():
    rng = np.random.default_rng(5)
    img = _smooth(rng, (64, 96), 1.5, 20.0)
    img[10, 10], img[40, 70], img[0, 5] = np.nan, np.inf, -np.inf
    img[30, 30:33] = np.inf
    with np.errstate(invalid="ignore"):
        _check_canny(img, "nan/inf")


def _serpentine(h, w, pitch=8):
    """a comb-shaped band whose boundary is one long 1-pixel contour across the whole frame"""
    m = np.zeros((h, w), bool)
    rows = list(range(4, h - 8, pitch))
    for i, r in enumerate(rows):
        m[r:r + pitch // 2, 4:w - 4] = True
        if i + 1 < len(rows):
            c = slice(w - 4 - pitch // 2, w - 4) if i % 2 == 0 else slice(4, 4 + pitch // 2)
            m[r:rows[i + 1] + 1, c] = True
    return m


def test_hysteresis_serpentine_and_spiral_stress():
    """a weak contour winding through every tile of a 4K frame is kept whole through one strong end; without it, all of it goes"""
    from patchrefinerv2_amd import metrics as M
    h, w = 2160, 3840
    band = _serpentine(h, w)
    weak = band.astype(np.float32) * 0.06  # gradient magnitude between the low (0.1) and high (0.2) thresholds
    mag_peak = float(ndi.sobel(ndi.gaussian_filter(weak, 1.0), 0).max())
    assert 0.1 < mag_peak < 0.2, mag_peak
    y0 = list(range(4, h - 8, 8))[-1]  # the last stripe: its step rises smoothly to 3x (magnitude > high)
    strong = (weak * (1 + 2.0 * np.clip((np.arange(h)[:, None] - (y0 - 8)) / 8.0, 0, 1))).astype(np.float32)
    kept = _check_canny(strong, "serpentine with strong end")
    assert kept.sum() > (h * w) / 8 and np.array_equal(kept, M.canny(strong, high_threshold=0.1))  # every low pixel is kept
    assert ndi.label(kept, np.ones((3, 3)))[1] == 1
    gone = _dev_canny(weak)
    assert not gone.any() and not M.canny(weak).any()
    # spiral + thousands of small components
    y, x = np.mgrid[0:1024, 0:1024].astype(np.float64)
    r, t = np.hypot(x - 512, y - 512), np.arctan2(y - 512, x - 512)
    spiral = (np.mod(r - 6 * t, 24) < 8) & (r < 500)
    rng = np.random.default_rng(9)
    dots = np.zeros_like(spiral)
    ys, xs = rng.integers(2, 1020, 6000), rng.integers(2, 1020, 6000)
    dots[ys, xs] = True
    img = spiral * 0.06 + ndi.binary_dilation(dots) * rng.choice([0.06, 1.0], size=spiral.shape)
    _check_canny(img.astype(np.float32), "spiral + dots")


# ------------------------------------------------------------------------------------------------------------------ distance transform
def _check_edt(mask):
    from patchrefinerv2_amd import ops
    d2 = ops.edt_sq(torch.from_numpy(mask).to(DEV))[0].cpu().numpy()
    ref = ndi.distance_transform_edt(~mask)
    got = np.sqrt(d2.astype(np.float64))
    assert np.array_equal(got, ref), (mask.shape, int((got != ref).sum()))


def test_edt_exact():
    rng = np.random.default_rng(3)
    for shape, p in (((37, 53), 0.01), ((64, 64), 0.001), ((300, 500), 0.0005), ((3, 3), 0.3)):
        m = rng.random(shape) < p
        m[shape[0] // 2, shape[1] // 2] = True
        _check_edt(m)
    for corner in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        m = np.zeros((45, 70), bool)
        m[corner] = True
        _check_edt(m)
    m = np.zeros((45, 70), bool)
    m[17, :] = True
    _check_edt(m)
    m = np.zeros((45, 70), bool)
    m[:, 33] = True
    _check_edt(m)
    m = rng.random((2160, 3840)) < 0.0002
    _check_edt(m)


def test_edt_empty_frame_is_int32_max():
    from patchrefinerv2_amd import ops
    d2 = ops.edt_sq(torch.zeros(2, 9, 11, dtype=torch.bool, device=DEV))
    assert (d2 == 2 ** 31 - 1).all()


# ------------------------------------------------------------------------------------------------------------------ preprocessing
def _ulps(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


@pytest.mark.parametrize("mode", ["log", "inv", "none"])
def test_preprocess_within_one_ulp(mode):
    from patchrefinerv2_amd import metrics as M, ops
    rng = np.random.default_rng(11)
    d = (rng.random((3, 120, 170)) * 20).astype(np.float32)
    d[0, :5, :5], d[1, 7, 9], d[2, 3, :4] = 0.0, -1.0, 1e-9
    for f in range(3):
        got = ops.depth_preprocess(torch.from_numpy(d).to(DEV), mode)[f].cpu().numpy()
        ref = M.preprocess_depth(d[f], mode)
        same_class = (np.isnan(got) == np.isnan(ref)) & (np.isinf(got) == np.isinf(ref))
        assert same_class.all()
        fin = np.isfinite(ref)
        assert (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all()
        if mode != "none":
            assert _ulps(got[fin], ref[fin]).max() <= 1, (mode, f)
        else:
            # log(x) / log(1.5): torch's vectorised fp32 log (<= 1 ulp) is divided by 0.405, which scales its error up to ~2.5 ulp
            # of the quotient -- so the quotient is held to 1 ulp of the same expression with a correctly rounded log, and to 4 of torch
            x = np.where(d[f] > 0, np.maximum(d[f], np.float32(np.finfo(np.float32).eps)), np.float32(0))
            with np.errstate(divide="ignore"):
                exact = np.float32(np.log(x.astype(np.float64))) / np.float32(M.LOG_1_5_F32)
            assert _ulps(got[fin], exact[fin]).max() <= 1 and _ulps(got[fin], ref[fin]).max() <= 4, (mode, f)


def test_preprocess_nan_propagates_like_torch():
    from patchrefinerv2_amd import metrics as M, ops
    d = np.full((8, 8), 2.0, np.float32)
    d[3, 3] = np.nan
    for mode in ("log", "inv", "none"):
        got = ops.depth_preprocess(torch.from_numpy(d).to(DEV), mode)[0].cpu().numpy()
        ref = M.preprocess_depth(d, mode)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), mode


def test_extract_edges_device_4k_close_to_host():
    from patchrefinerv2_amd import metrics as M
    rng = np.random.default_rng(2)
    y, x = np.mgrid[0:2160, 0:3840].astype(np.float32)
    depth = (3.0 + 2.0 * (x > 1700) + 1.5 * (np.hypot(x - 900, y - 1000) < 500) + np.exp(_smooth(rng, (2160, 3840), 20.0, 30.0))).astype(np.float32)
    got = M.extract_edges_device(torch.from_numpy(depth).to(DEV), "log").cpu().numpy()
    ref = M.extract_edges(depth, "log")
    assert ref.sum() > 1000 and (got != ref).mean() <= 1e-5, int((got != ref).sum())


# ------------------------------------------------------------------------------------------------------------------ boundary metrics
def _metric_pairs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "edge_metrics.npz"))
    out = [(z[f"{c}/gt_edges_log"], z[f"{c}/pred_edges_log"], z[f"{c}/valid"]) for c in z["cases"]]
    rng = np.random.default_rng(4)
    g = rng.random((540, 960)) < 0.01
    p = ndi.binary_dilation(g) & (rng.random(g.shape) < 0.3) | (rng.random(g.shape) < 0.002)
    v = rng.random(g.shape) < 0.9
    out += [(g, p, v), (np.zeros_like(g), p, v), (g, np.zeros_like(p), v), (g, p, np.zeros_like(v))]
    return out


def _close(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if np.isnan(b[k]):
            assert np.isnan(a[k]), (what, k)
        elif k in ("EdgeAcc", "EdgeComp"):
            assert abs(a[k] - b[k]) <= 1e-12 * abs(b[k]), (what, k, a[k], b[k])
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def test_boundary_metrics_device_equals_host():
    from patchrefinerv2_amd import metrics as M, ops
    for i, (g, p, v) in enumerate(_metric_pairs()):
        with np.errstate(invalid="ignore"):
            ref = M.compute_boundary_metrics(g, p, v)
        got = M.compute_boundary_metrics_device(*(torch.from_numpy(a).to(DEV) for a in (g, p, v)))
        _close(got, ref, i)
        gd, pd, vd = (torch.from_numpy(a).to(DEV) for a in (g, p, v))
        s = ops.boundary_stats(gd, pd, vd, ops.edt_sq(gd), ops.edt_sq(pd), ops.binary_dilate(gd, 5), ops.binary_dilate(pd, 5), 10.0)[0].cpu()
        ge, pe = M.binary_dilate(g, 5)[v], M.binary_dilate(p, 5)[v]
        assert s[:4].tolist() == [float((pe & ge).sum()), float((pe & ~ge).sum()), float((~pe & ge).sum()), float((~pe & ~ge).sum())]
        assert s[5].item() == float((g & v).sum())


@pytest.mark.parametrize("k", [3, 5, 7])
def test_dilate_equals_host(k):
    from patchrefinerv2_amd import metrics as M, ops
    rng = np.random.default_rng(k)
    m = rng.random((3, 50, 77)) < 0.02
    got = ops.binary_dilate(torch.from_numpy(m).to(DEV), k).cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f], M.binary_dilate(m[f], k))


# ------------------------------------------------------------------------------------------------------------------ determinism, frames
def test_deterministic_and_three_frames_equal_single_calls():
    from patchrefinerv2_amd import metrics as M, ops
    rng = np.random.default_rng(8)
    depth = torch.from_numpy(np.exp(np.stack([_smooth(rng, (540, 960), 6.0, 40.0) for _ in range(3)]))).to(DEV)
    e3 = M.extract_edges_device(depth, "inv")
    assert e3.shape == (3, 540, 960) and torch.equal(e3, M.extract_edges_device(depth, "inv"))
    for f in range(3):
        assert torch.equal(e3[f], M.extract_edges_device(depth[f], "inv"))
    g, p = e3, torch.roll(e3, 2, dims=2)
    v = depth > 1.0
    st = ops.boundary_stats(g, p, v, ops.edt_sq(g), ops.edt_sq(p), ops.binary_dilate(g, 5), ops.binary_dilate(p, 5), 10.0)
    st2 = ops.boundary_stats(g, p, v, ops.edt_sq(g), ops.edt_sq(p), ops.binary_dilate(g, 5), ops.binary_dilate(p, 5), 10.0)
    assert torch.equal(st, st2)
    for f in range(3):
        gf, pf, vf = g[f:f + 1], p[f:f + 1], v[f:f + 1]
        s1 = ops.boundary_stats(gf, pf, vf, ops.edt_sq(gf), ops.edt_sq(pf), ops.binary_dilate(gf, 5), ops.binary_dilate(pf, 5), 10.0)
        assert torch.equal(s1[0], st[f]) and torch.equal(ops.edt_sq(gf)[0], ops.edt_sq(g)[f])
    rows = M.compute_boundary_metrics_device(g, p, v)
    assert isinstance(rows, list) and len(rows) == 3 and rows[1] == M.compute_boundary_metrics_device(g[1], p[1], v[1])


def test_ctypes_route_in_child_process():
    """every GPU test above again with PRV2_DISPATCH=ctypes (the C ABI straight from ctypes)"""
    env = dict(os.environ, PRV2_DISPATCH="ctypes")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "not child_process and not tester and not 4k and not 2160 and not serpentine"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ Tester
def _tester_run(tmp_path, frame_batch, device_route=True):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    name = "v1_dav2s_1080p_m1"
    w = WORKLOADS[name]
    if not (tmp_path / "imgs").exists():
        (tmp_path / "imgs").mkdir()
        (tmp_path / "gt").mkdir()
        y, x = np.mgrid[0:540, 0:960].astype(np.float32)
        for i in range(3):
            rs = np.random.RandomState(40 + i)
            np.save(str(tmp_path / "imgs" / f"f{i}.npy"), rs.rand(90, 160, 3).astype(np.float32))
            gt = 2.0 + 3.0 * (x > 300 + 50 * i) + 1.5 * (np.hypot(x - 600, y - 270) < 120) + 0.1 * np.sin(y / 17.0)
            gt[:20] = 0.0  # invalid rows
            np.save(str(tmp_path / "gt" / f"f{i}.npy"), gt.astype(np.float32))
    m = build_model(model_config(name, prec="bf16x3", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    m.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    if not device_route:
        m.supports_return_device = False
    ds = ImageDataset(str(tmp_path / "imgs"), gt_dir=str(tmp_path / "gt"), min_depth=1e-3, max_depth=80, image_resolution=w["raw"],
                      edge_metrics=True)
    t = Tester(None, RunnerInfo(), ds, m)
    res = t.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621, frame_batch=frame_batch)
    return [r["metrics"] for r in res]


def test_tester_edge_metrics_device_equals_host_and_frame_batch(tmp_path):
    dev1 = _tester_run(tmp_path, 1)
    keys = ("EdgeAcc", "EdgeComp", "precision", "recall", "f1_score", "hamming", "acc", "edge_abs_rel", "noedge_abs_rel", "edge_a1",
            "noedge_rmse", "abs_rel")
    for m in dev1:
        for k in keys:
            assert k in m, k
    host = _tester_run(tmp_path, 1, device_route=False)
    # the boundary metrics score the PREDICTION's log-depth Canny edges: torch's CPU log and resize may differ from the device's in
    # the last ulp, which can move a handful of edge pixels (test_extract_edges_device_4k_close_to_host bounds that at 1e-5 of a
    # map) and each moves these means by ~1e-4; everything derived from the GT edges and the depth agrees to 1e-6 -- but SILog, whose
    # host route sums float32 (sqrt(E[e^2] - E[e]^2) cancels), and which already differs at ~5e-6 without edge metrics
    boundary = {"EdgeAcc", "EdgeComp", "precision", "recall", "f1_score", "hamming", "acc"}
    bad = []
    for a, b in zip(dev1, host):
        assert set(a) == set(b)
        for k in a:
            tol = (2e-3 if k in boundary else 2e-5 if k.endswith("silog") else 1e-6) * max(1.0, abs(float(b[k])))
            if not abs(float(a[k]) - float(b[k])) <= tol:
                bad.append((k, float(a[k]), float(b[k])))
    assert not bad, bad
    dev2 = _tester_run(tmp_path, 2)
    assert dev2 == dev1
