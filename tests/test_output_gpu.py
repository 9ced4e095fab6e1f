"""GPU: the output stage (csrc/output.hip, patchrefinerv2_amd/output.py).  Order statistics equal np.sort(valid)[k], the colour /
16-bit / pseudo-label scanlines equal what metrics.colorize, Tester._emit and Tester._write_pl build on the host from the same maps,
and Tester.run(save=True) / generate_pl(save=True) write the host route's files through the device route.

Two comparisons are made against the host function applied to the DEVICE's intermediate (not host route files): <name>_coarse.png
(CPU and device bilinear may differ in the last ulp) and <name>_edge.png (CPU and device log likewise); everything else is
byte-identical to the host route.  Order statistics are compared with ==, which takes -0.0 and +0.0 as equal: np.sort leaves their
mutual order unspecified (they compare equal), the device puts -0.0 first."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)
CMAPS = ("Spectral", "magma_r", "gray_r", "jet", "turbo_r")


@pytest.fixture(params=["torch"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    if os.environ.get("PRV2_DISPATCH") != "ctypes":
        monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _check_stats(ops, a, mask=None, invalid_val=-99.0, ranks=None):
    """a: numpy [B, H, W]; every requested rank of every frame against np.sort of the valid values"""
    B = a.shape[0]
    t = torch.from_numpy(a).to(DEV)
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    ranks = ranks or [0, 1, -1, -2, 3, 10 ** 9, -10 ** 9, a[0].size // 2]
    counts, out = ops.order_stats(t, ranks, mask=m, invalid_val=invalid_val)
    counts, out = counts.cpu().numpy(), out.cpu().numpy()
    for f in range(B):
        valid = a[f][mask[f]] if mask is not None else a[f][a[f] != np.float32(invalid_val)]
        n = valid.size
        assert counts[f] == n, (f, counts[f], n)
        if n == 0:
            assert np.isnan(out[f]).all()
            continue
        s = np.sort(valid)
        want = [s[min(max(k if k >= 0 else n + k, 0), n - 1)] for k in ranks]
        assert _same(out[f], want), (f, out[f], want)
    return counts, out


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (1080, 1920), (2160, 3840)])
def test_order_stats_equal_sort(ops, shape):
    rs = np.random.RandomState(shape[1])
    a = (rs.randn(1, *shape) * 20 + 30).astype(np.float32)
    _check_stats(ops, a)
    a.reshape(-1)[::5] = -99.0  # invalid_val pixels
    _check_stats(ops, a)
    _check_stats(ops, a, mask=rs.rand(1, *shape) > 0.4)
    _check_stats(ops, a, mask=np.zeros((1, *shape), dtype=bool))  # nothing valid


def test_order_stats_ties_signs_denormals_nan_inf(ops):
    rs = np.random.RandomState(11)
    h, w = 97, 131
    const = np.full((1, h, w), 2.5, dtype=np.float32)
    ties = rs.randint(0, 4, (1, h, w)).astype(np.float32)
    signs = (rs.randn(1, h, w) * 1e3).astype(np.float32)
    signs.reshape(-1)[:40] = np.tile(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 3e-38, -3e-38], dtype=np.float32), 5)
    zeros = np.where(rs.rand(1, h, w) > 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    nan = signs.copy()
    nan.reshape(-1)[[5, 77, 900]] = np.nan
    nan.reshape(-1)[901] = -np.nan
    inf = signs.copy()
    inf.reshape(-1)[[3, 99]] = np.inf
    inf.reshape(-1)[[4, 100]] = -np.inf
    for a in (const, ties, signs, zeros, nan, inf):
        _check_stats(ops, a, ranks=[0, 1, 2, 20, 21, -1, -2, -5])
    # the device's own order of the zeros: -0.0 first
    _, out = ops.order_stats(torch.from_numpy(zeros).to(DEV), [0, -1])
    assert np.signbit(out.cpu().numpy()[0, 0]) and not np.signbit(out.cpu().numpy()[0, 1])


def test_order_stats_frames_equal_single_calls_and_repeat(ops):
    rs = np.random.RandomState(2)
    a = (rs.rand(3, 211, 307) * 80).astype(np.float32)
    a[1] = np.round(a[1])
    mask = rs.rand(3, 211, 307) > 0.3
    ranks = [0, 5, 1000, -1, -7, 30000]
    c3, o3 = _check_stats(ops, a, mask=mask, ranks=ranks)
    t, m = torch.from_numpy(a).to(DEV), torch.from_numpy(mask).to(DEV)
    again = ops.order_stats(t, ranks, mask=m)
    assert np.array_equal(again[0].cpu().numpy(), c3) and np.array_equal(again[1].cpu().numpy().view(np.uint32), o3.view(np.uint32))
    for f in range(3):
        c1, o1 = ops.order_stats(t[f], ranks, mask=m[f])
        assert int(c1[0]) == c3[f] and np.array_equal(o1.cpu().numpy()[0].view(np.uint32), o3[f].view(np.uint32))
    # the gate of the pseudo-label route: valid needs not (gate < thr)
    gate = rs.randint(0, 5, a.shape).astype(np.float32)
    c, o = ops.order_stats(t, [0, -1], invalid_val=float("nan"), gate=torch.from_numpy(gate).to(DEV), gate_thr=1.5)
    for f in range(3):
        v = a[f][~(gate[f].astype(np.float64) < 1.5)]
        assert int(c[f]) == v.size and _same(o[f].cpu().numpy(), [v.min(), v.max()])


def test_percentile_device_equals_numpy(ops):
    from patchrefinerv2_amd.output import percentile_device
    rs = np.random.RandomState(4)
    a = (rs.randn(301, 517) * 9 + 20).astype(np.float32)
    t = torch.from_numpy(a).to(DEV)
    qs = [0, 2, 5, 33.3, 50, 95, 99.5, 100]
    got = percentile_device(t, qs, invalid_val=-99)
    assert _same(got, [np.percentile(a, p) for p in qs])
    mask = rs.rand(*a.shape) > 0.5
    assert _same(percentile_device(t, [2, 95], mask=torch.from_numpy(mask).to(DEV)), [np.percentile(a[mask], p) for p in (2, 95)])
    assert percentile_device(t, 100) == a.max() and percentile_device(t, 0) == a.min()
    with np.errstate(invalid="ignore"):
        for special in (np.nan, np.inf):  # one NaN map, one inf map: whatever np.percentile over value[mask] gives
            b = a.copy()
            b[7, 9] = special
            for q in ([0, 100], [2, 95]):
                assert _same(percentile_device(torch.from_numpy(b).to(DEV), q), [np.percentile(b, p) for p in q]), (special, q)


def _host_rgb(value, **kw):
    from patchrefinerv2_amd.metrics import colorize
    return np.ascontiguousarray(colorize(value, **kw)[..., :3])


@pytest.mark.parametrize("w", [1, 3, 961, 3840])
def test_colorize_device_equals_host(ops, w):
    from patchrefinerv2_amd.output import colorize_device
    h = {1: 37, 3: 29, 961: 23, 3840: 11}[w]
    rs = np.random.RandomState(w)
    a = (rs.rand(h, w) * 70 + 0.5).astype(np.float32)
    t = torch.from_numpy(a).to(DEV)
    for cmap in CMAPS:
        for lo, hi in ((0, 100), (2, 95)):
            img, rows = colorize_device(t, cmap=cmap, vminp=lo, vmaxp=hi)
            want = _host_rgb(a.copy(), cmap=cmap, vminp=lo, vmaxp=hi).reshape(h, w, 3)
            assert np.array_equal(img.cpu().numpy(), want), (cmap, lo, hi)
            raw = rows.cpu().numpy()[0, :h * (1 + 3 * w)].reshape(h, 1 + 3 * w)
            assert not raw[:, 0].any() and not rows.cpu().numpy()[0, h * (1 + 3 * w):].any()  # filter bytes, zero tail


def test_colorize_device_invalid_flat_nan_inf(ops):
    from patchrefinerv2_amd.output import colorize_device
    rs = np.random.RandomState(9)
    h, w = 41, 59
    a = (rs.rand(h, w) * 10 + 1).astype(np.float32)
    a[::7, ::3] = -99.0  # invalid_val pixels: background colour, out of the percentiles
    t = torch.from_numpy(a).to(DEV)
    assert np.array_equal(colorize_device(t, cmap="Spectral")[0].cpu().numpy(), _host_rgb(a.copy(), cmap="Spectral"))
    inv = rs.rand(h, w) > 0.8
    got = colorize_device(t, cmap="jet", invalid_mask=torch.from_numpy(inv), vminp=0, vmaxp=100, background_color=(1, 2, 3, 255))[0]
    assert np.array_equal(got.cpu().numpy(), _host_rgb(a.copy(), cmap="jet", invalid_mask=inv, vminp=0, vmaxp=100, background_color=(1, 2, 3, 255)))
    flat = np.full((h, w), 3.25, dtype=np.float32)
    assert np.array_equal(colorize_device(torch.from_numpy(flat).to(DEV), cmap="magma_r")[0].cpu().numpy(), _host_rgb(flat.copy(), cmap="magma_r"))
    # explicit float32 vmin / vmax, values below / above / exactly on them
    b = np.linspace(-1, 3, h * w).astype(np.float32).reshape(h, w)
    b[0, :3] = [0.5, 2.0, 1.0]
    got = colorize_device(torch.from_numpy(b).to(DEV), vmin=np.float32(0.5), vmax=np.float32(2.0), cmap="turbo_r")[0]
    assert np.array_equal(got.cpu().numpy(), _host_rgb(b.copy(), vmin=np.float32(0.5), vmax=np.float32(2.0), cmap="turbo_r"))
    with np.errstate(invalid="ignore"):
        for special in (np.nan, np.inf):
            c = a.copy()
            c[3, 4] = special
            got = colorize_device(torch.from_numpy(c).to(DEV), cmap="Spectral", vminp=0, vmaxp=100)[0]
            assert np.array_equal(got.cpu().numpy(), _host_rgb(c.copy(), cmap="Spectral", vminp=0, vmaxp=100)), special


def _rows16(arr_u16):
    h, w = arr_u16.shape
    raw = np.zeros((h, 1 + 2 * w), dtype=np.uint8)
    raw[:, 1:] = arr_u16.astype(">u2").view(np.uint8).reshape(h, 2 * w)
    return raw


def test_quantize16_mask_rows_equal_host(ops):
    rs = np.random.RandomState(6)
    for h, w in ((1, 1), (5, 3), (67, 1021)):
        a = (rs.rand(2, h, w) * 255.9).astype(np.float32)
        a.reshape(-1)[::11] = 0.0
        rows = ops.quantize16_rows(torch.from_numpy(a).to(DEV), 256.0).cpu().numpy()
        m = rs.rand(2, h, w) > 0.6
        mrows = ops.mask_rows(torch.from_numpy(m).to(DEV)).cpu().numpy()
        for f in range(2):
            want = _rows16((a[f] * 256).astype("uint16"))  # Tester._emit
            assert np.array_equal(rows[f, :want.size].reshape(want.shape), want) and not rows[f, want.size:].any()
            wm = np.zeros((h, 1 + w), dtype=np.uint8)
            wm[:, 1:] = m[f].astype(np.uint8) * 255
            assert np.array_equal(mrows[f, :wm.size].reshape(wm.shape), wm)


@pytest.mark.parametrize("case", ["spread", "flat", "all_low_count", "no_low_count"])
def test_pseudo_label_scanlines_equal_host(ops, tmp_path, case):
    """the five files of Tester._write_pl from the same maps, host route against OutputStage.submit_pseudo_label"""
    from patchrefinerv2_amd.output import OutputStage
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    rs = np.random.RandomState(8)
    h, w = 83, 127
    depth = (rs.rand(1, 1, h, w) * 60 + 1).astype(np.float32)
    unc = (rs.rand(1, 1, h, w) ** 2 * 0.7).astype(np.float32)
    cnt = rs.randint(1, 9, (1, 1, h, w)).astype(np.float32)
    n_tiles, thr = 40, 0.05  # count < 2 masked
    if case == "flat":
        unc[:] = 0.25
    if case == "all_low_count":
        cnt[:] = 1.0
    if case == "no_low_count":
        cnt[:] = 5.0
    (tmp_path / "host").mkdir()
    t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / "host")), None, None)
    t._write_pl("f", torch.from_numpy(depth), torch.from_numpy(unc), torch.from_numpy(cnt), n_tiles, thr)
    st = OutputStage(str(tmp_path / "dev"), workers=4)
    st.submit_pseudo_label(str(tmp_path / "dev" / "f"), *(torch.from_numpy(x).to(DEV) for x in (depth, unc, cnt)), n_tiles, thr)
    st.close()
    names = sorted(os.listdir(tmp_path / "host"))
    assert len(names) == 5 and names == sorted(os.listdir(tmp_path / "dev"))
    for n in names:
        assert (tmp_path / "dev" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), (case, n)


def test_upsample_bilinear_map_close_to_torch_cpu(ops):
    """within 2 ulp of CPU F.interpolate(bilinear, align_corners=False) on a positive random coarse map: the bound is on the
    evaluation order of one fp32 formula (three two-tap sums of positive terms, each rounding at most half an ulp; CPU torch's
    vectorised kernel contracts them to fused multiply-adds, which the device kernel follows: a float32 restatement of that
    order gave 0 ulp against CPU torch on this case, the uncontracted order 3 ulp in the sums and ~1e3 ulp when the source
    coordinate is rounded twice), not on the feature"""
    rs = np.random.RandomState(12)
    x = (rs.rand(2, 1, 384, 512) * 79 + 0.5).astype(np.float32)
    want = F.interpolate(torch.from_numpy(x), (2160, 3840), mode="bilinear", align_corners=False)[:, 0].numpy()
    got = ops.upsample_bilinear_map(torch.from_numpy(x[:, 0]).to(DEV), 2160, 3840).cpu().numpy()
    ulp = np.spacing(np.abs(want))
    worst = float((np.abs(got.astype(np.float64) - want) / ulp).max())
    print(f"upsample_bilinear_map: worst deviation from CPU torch {worst:.3f} ulp")
    assert worst <= 2.0, worst
    same = ops.upsample_bilinear_map(torch.from_numpy(x[:, 0]).to(DEV), 384, 512).cpu().numpy()
    assert np.array_equal(same, x[:, 0])


def test_ctypes_route_in_child_process():
    """every kernel test above again with PRV2_DISPATCH=ctypes (the C ABI straight from ctypes)"""
    env = dict(os.environ, PRV2_DISPATCH="ctypes")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "not child_process and not tester and not 2160"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ Tester
def _tester(tmp_path, work, device_output, gray=False):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    name = "v1_dav2s_1080p_m1"
    w = WORKLOADS[name]
    if not (tmp_path / "imgs").exists():
        (tmp_path / "imgs").mkdir()
        for i in range(3):
            np.save(str(tmp_path / "imgs" / f"f{i}.npy"), np.random.RandomState(60 + i).rand(90, 160, 3).astype(np.float32))
    m = build_model(model_config(name, prec="bf16x3", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    m.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    ds = ImageDataset(str(tmp_path / "imgs"), min_depth=1e-3, max_depth=80, image_resolution=w["raw"])
    info = RunnerInfo(save=True, work_dir=str(tmp_path / work), device_output=device_output, output_workers=4, gray_scale=gray)
    return Tester(None, info, ds, m), w, m


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _decode(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def test_tester_run_device_route_writes_the_host_routes_files(tmp_path):
    import random
    from patchrefinerv2_amd import metrics as M, ops
    th, w, m = _tester(tmp_path, "host", False)
    # the premise: two runs with one seed give bit-equal maps, and return_device=True returns the values the host map holds
    item = th.dataloader[0]
    hr = item["image_hr"][None].cuda()
    call = dict(mode="infer", cai_mode=w["mode"], process_num=4, tile_cfg=dict(image_raw_shape=w["raw"], patch_split_num=w["split"]),
                image_lr=m.resizer(hr), image_hr=hr)
    random.seed(621)
    d_host, log_h = m(**call)
    random.seed(621)
    d_dev, log_d = m(**call, return_device=True)
    assert d_dev.is_cuda and torch.equal(d_dev.cpu(), d_host), "premise: return_device=True must return the host map's values"
    res_h = th.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
    host = _files(tmp_path / "host")
    for work, fb in (("dev1", 1), ("dev2", 2)):
        td, _, _ = _tester(tmp_path, work, True)
        res_d = td.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621, frame_batch=fb)
        dev = _files(tmp_path / work)
        assert sorted(dev) == sorted(host) and len(dev) == 3 * 4
        for a, b in zip(res_h, res_d):  # entries unchanged (the mean: float32 sum on the host, float64 sum on the device)
            assert a["name"] == b["name"] and a["shape"] == b["shape"] and abs(a["mean"] - b["mean"]) <= 1e-5 * abs(a["mean"])
        for i in range(3):
            for s in (".png", "_uint16.png"):
                assert dev[f"f{i}{s}"] == host[f"f{i}{s}"], (work, i, s)
        if fb == 2:
            assert dev == _files(tmp_path / "dev1")
            continue
        # _edge.png: the host Canny on the DEVICE's log depth, dilated; _coarse.png: host colorize of the DEVICE-upsampled map
        d16 = _decode(host["f0_uint16.png"])
        assert d16.dtype == np.uint16 and np.array_equal(d16, (d_host.squeeze().numpy() * 256).astype("uint16"))
        logd = ops.depth_preprocess(d_dev.reshape(1, *d_dev.shape[-2:]), "log")[0].cpu().numpy()
        want_edge = M.binary_dilate(M.canny(logd, sigma=1.0), 3).astype(np.uint8) * 255
        assert np.array_equal(_decode(dev["f0_edge.png"]), want_edge) and want_edge.any()
        coarse = log_d["coarse_prediction"]
        up = ops.upsample_bilinear_map(coarse.reshape(1, *coarse.shape[-2:]).float(), *w["raw"])
        want_coarse = np.ascontiguousarray(M.colorize(up.cpu(), cmap="Spectral", vminp=0, vmaxp=100)[:, :, :3])
        assert np.array_equal(_decode(dev["f0_coarse.png"]), want_coarse)


def test_tester_generate_pl_and_gray_scale_device_route(tmp_path):
    kw = dict(cai_mode="r4", seed=621, count_thr=0.2)
    th, w, _ = _tester(tmp_path, "host", False)
    res_h = th.generate_pl(image_raw_shape=w["raw"], patch_split_num=w["split"], **kw)
    host = _files(tmp_path / "host")
    assert len(host) == 3 * 5
    for work, fb in (("dev1", 1), ("dev2", 2)):
        td, _, _ = _tester(tmp_path, work, True)
        res_d = td.generate_pl(image_raw_shape=w["raw"], patch_split_num=w["split"], frame_batch=fb, **kw)
        assert _files(tmp_path / work) == host, work
        for a, b in zip(res_h, res_d):
            assert set(a) == set(b) and a["n_tiles"] == b["n_tiles"] and abs(a["mean"] - b["mean"]) <= 1e-5 * abs(a["mean"])
    # gray_scale: run's colour map at percentiles (2, 95), generate_pl's gray_r
    tg, _, _ = _tester(tmp_path, "gray_host", False, gray=True)
    tg.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
    tg, _, _ = _tester(tmp_path, "gray_dev", True, gray=True)
    tg.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
    gh, gd = _files(tmp_path / "gray_host"), _files(tmp_path / "gray_dev")
    for i in range(3):
        assert gd[f"f{i}.png"] == gh[f"f{i}.png"]
