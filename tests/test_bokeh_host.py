"""No GPU: the depth-of-field export's host specification (patchrefinerv2_amd/output.py: bokeh_render_host / bokeh_image_host), its
options, the host route of the files, the CLI flags and the C ABI's argument checks.  The kernel (csrc/bokeh.hip) is compared with this
specification bit for bit in tests/test_bokeh_gpu.py; here the specification itself is pinned: by properties that hold exactly, and by a
per-pixel float64 restatement that shares nothing with the vectorised loop but the per-pixel zk, r and m maps."""
import ctypes
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
INVALID = np.array([np.nan, np.inf, -np.inf, 0.0, -1.5, 0.2, 9.0], dtype=F32)  # the seven kinds of tests/test_stereo_gpu.py, range (0.5, 7)
K = (40.0, 40.0, 16.0, 12.0)  # fx, fy, cx, cy (fx is used)
LENS = dict(aperture=0.4, max_radius=3.5, depth_range=(0.5, 7.0))


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _image(h, w, seed=1):
    return np.random.RandomState(100 + seed).rand(3, h, w).astype(F32)


def _bytes(img):
    from patchrefinerv2_amd.output import color_bytes
    return np.moveaxis(color_bytes(np.asarray(img, dtype=F32) * F32(255)), 0, -1)


def _random_scene(h=24, w=32, seed=7):
    """random depth in [1, 6) with a constant block at 2 m and a tenth of the pixels invalid, one kind after the other"""
    rs = np.random.RandomState(seed)
    d = (1.0 + 5.0 * rs.rand(h, w)).astype(F32)
    d[5:15, 8:20] = F32(2.0)
    idx = rs.choice(h * w, size=h * w // 10, replace=False)
    d.reshape(-1)[idx] = np.resize(INVALID, idx.size)
    return d, rs.rand(3, h, w).astype(F32)


def _bar_scene(h=24, w=32):
    """a bar at 2 m (columns 12 .. 17) in front of a wall at 6 m"""
    d = np.full((h, w), 6.0, dtype=F32)
    d[:, 12:18] = F32(2.0)
    return d


# ------------------------------------------------------------------------------------------------------------------ (a) - (d)
def test_constant_depth_in_focus_is_the_image_exactly():
    from patchrefinerv2_amd.output import bokeh_render_host
    img = _image(24, 32)
    out, zf = bokeh_render_host(np.full((24, 32), 2.0, F32), img, K, focus=2.0, **LENS)
    assert out.dtype == np.float32 and out.shape == (3, 24, 32) and zf == F32(2.0)
    assert np.array_equal(out, img)  # m = 0.5 everywhere: one tap of weight ia = 4, a power of two
    out, zf = bokeh_render_host(np.full((24, 32), 2.0, F32), img, K, **LENS)  # the focus point finds the same distance
    assert np.array_equal(out, img) and zf == F32(2.0)


def test_a_sharp_bar_keeps_the_defocused_wall_off():
    from patchrefinerv2_amd.output import bokeh_render_host
    d, img = _bar_scene(), _image(24, 32)
    out, _ = bokeh_render_host(d, img, K, focus=2.0, **LENS)
    assert np.array_equal(out[:, :, 12:18], img[:, :, 12:18])  # inside the bar: the wall behind it has the larger disc and takes the bar's
    assert not np.array_equal(_bytes(out[:, :, :12]), _bytes(img[:, :, :12])) and not np.array_equal(_bytes(out[:, :, 18:]), _bytes(img[:, :, 18:]))


def test_a_defocused_bar_spreads_over_the_sharp_wall_within_its_reach():
    from patchrefinerv2_amd.output import bokeh_discs_host, bokeh_render_host
    d, img = _bar_scene(), _image(24, 32)
    out, _ = bokeh_render_host(d, img, K, focus=6.0, **LENS)
    r = bokeh_discs_host(d, K[0], 0.4, F32(6.0), 3.5, (0.5, 7.0))[1]
    reach = int(math.ceil(float(r[0, 12]) + 0.5)) - 1  # the columns the bar's disc covers beside it
    assert r[0, 0] == 0 and 2 <= reach <= 3
    assert not np.array_equal(out[:, :, 12 - reach:12], img[:, :, 12 - reach:12]) and not np.array_equal(out[:, :, 18:18 + reach], img[:, :, 18:18 + reach])
    assert np.array_equal(out[:, :, :12 - reach], img[:, :, :12 - reach]) and np.array_equal(out[:, :, 18 + reach:], img[:, :, 18 + reach:])
    assert not np.array_equal(out[:, :, 12:18], img[:, :, 12:18])  # the bar itself is blurred


def test_a_constant_colour_stays_constant():
    from patchrefinerv2_amd.output import bokeh_image_host
    d, _ = _random_scene()
    got = bokeh_image_host(d, np.full((3, 24, 32), 0.25, F32), K, focus=2.0, **LENS)
    assert got.dtype == np.uint8 and got.shape == (24, 32, 3) and (got == 64).all()


# ------------------------------------------------------------------------------------------------------------------ (e)
def _float64_restatement(d, img, fx, aperture, zf, rm, depth_range):
    """per output pixel, a double loop over its window in float64: only the per-pixel zk, r, m maps are the specification's"""
    from patchrefinerv2_amd.output import bokeh_discs_host
    zk, r, m, _ = (a.astype(np.float64) for a in bokeh_discs_host(d, fx, aperture, F32(zf), rm, depth_range))
    h, w = d.shape
    R = int(math.ceil(rm))
    c = np.where(np.isfinite(img), img, 0).astype(np.float64)
    out = np.zeros((3, h, w))
    for y in range(h):
        for x in range(w):
            sw, sc = 0.0, np.zeros(3)
            for yy in range(max(0, y - R), min(h, y + R + 1)):
                for xx in range(max(0, x - R), min(w, x + R + 1)):
                    me = m[yy, xx] if (zk[yy, xx] <= zk[y, x] or r[yy, xx] <= r[y, x]) else m[y, x]
                    wgt = min(1.0, max(0.0, me + 0.5 - math.hypot(yy - y, xx - x))) / (me * me)
                    if wgt > 0:
                        sw += wgt
                        sc += wgt * c[:, yy, xx]
            out[:, y, x] = sc / sw
    return out


def test_specification_equals_a_float64_restatement():
    """bytes equal wherever 255 v64 is farther than 5e-3 from a half-integer; at most 3 % of the values may be that close (this scene:
    1.3 %, no unequal byte anywhere, largest relative fp32 - fp64 difference 3.5e-7)"""
    from patchrefinerv2_amd.output import bokeh_image_host, bokeh_render_host
    d, img = _random_scene()
    assert all(np.isnan(d).any() if np.isnan(v) else (d == v).any() for v in INVALID)
    want = _float64_restatement(d, img, K[0], 0.4, 2.0, 3.5, (0.5, 7.0))
    out, _ = bokeh_render_host(d, img, K, focus=2.0, **LENS)
    v = 255.0 * want
    near_tie = np.abs((v - np.floor(v)) - 0.5) <= 5e-3
    share = float(near_tie.mean())
    rel = float(np.max(np.abs(out - want) / np.maximum(want, 1e-9)))
    print(f"near a half-integer: {share:.4f} of the values; largest relative fp32 - fp64 difference {rel:.3g}")
    assert share <= 0.03
    got = np.moveaxis(bokeh_image_host(d, img, K, focus=2.0, **LENS), -1, 0)
    ref = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    assert np.array_equal(got[~near_tie], ref[~near_tie]), int((got != ref)[~near_tie].sum())
    # sums of at most 81 non-negative terms: each of sw and sc carries at most (taps + 2) roundings of 2^-24, the quotient one more
    assert rel < (2 * (81 + 2) + 1) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ (f), (g)
def test_focus_distance_given_or_read_at_the_focus_point():
    from patchrefinerv2_amd.output import bokeh_focus_host, bokeh_render_host
    d, img = _random_scene()
    d[9, 20] = F32(3.25)  # the pixel of (u, v) = (0.64, 0.4): floor(0.4 * 24) = 9, floor(0.64 * 32) = 20
    a, za = bokeh_render_host(d, img, K, focus=3.25, **LENS)
    b, zb = bokeh_render_host(d, img, K, focus_point=(0.64, 0.4), **LENS)
    assert za == zb == F32(3.25) and np.array_equal(a, b) and not np.array_equal(a, img)
    assert bokeh_focus_host(d, None, (1.0, 1.0)) == d[23, 31]  # u = v = 1 is the last pixel
    for bad in (np.nan, np.inf, 0.2, 9.0):  # an invalid focus pixel: the image itself and a NaN focus
        d[12, 16] = F32(bad)
        out, zf = bokeh_render_host(d, img, K, **LENS)
        assert np.isnan(zf) and np.array_equal(out, img)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="focus"):
            bokeh_render_host(d, img, K, focus=bad, **LENS)
    for bad in ((-0.1, 0.5), (0.5, 1.5), (np.nan, 0.5)):
        with pytest.raises(ValueError, match="focus point"):
            bokeh_render_host(d, img, K, focus_point=bad, **LENS)
    for bad in (dict(aperture=-1.0), dict(aperture=INF), dict(max_radius=-1.0), dict(max_radius=np.nan)):
        with pytest.raises(ValueError):
            bokeh_render_host(d, img, K, focus=2.0, **{**LENS, **bad})


def test_zero_radius_small_frames_and_an_image_of_another_size():
    from patchrefinerv2_amd.output import bokeh_image_host, bokeh_render_host, sample_indices
    d, img = _random_scene()
    out, _ = bokeh_render_host(d, img, K, focus=2.0, aperture=0.4, max_radius=0.0, depth_range=(0.5, 7.0))
    assert np.array_equal(out, img)
    small = (1.0 + np.arange(45, dtype=F32).reshape(5, 9) / 10)  # a frame smaller than the window of 17 x 17
    out, zf = bokeh_render_host(small, _image(5, 9), K, aperture=2.0, max_radius=8.0)
    assert out.shape == (3, 5, 9) and np.isfinite(out).all() and zf == small[2, 4] and not np.array_equal(out, _image(5, 9))
    one, _ = bokeh_render_host(np.ones((1, 1), F32), np.full((3, 1, 1), 0.5, F32), K, max_radius=8.0)
    assert one.reshape(-1).tolist() == [0.5, 0.5, 0.5]
    big = _image(48, 64, 5)  # twice the map's size: sampled with the cloud's nearest rule
    big[0, 3, 3] = np.nan  # (a sampled pixel: (2 * 1 + 1) * 48 // 48 = 3) counts as 0
    grid = big[:, sample_indices(24, 48)[:, None], sample_indices(32, 64)[None, :]]
    assert np.isnan(grid[0, 1, 1])
    a = bokeh_image_host(d, big, K, focus=2.0, **LENS)
    b = bokeh_image_host(d, np.where(np.isnan(grid), F32(0), grid), K, focus=2.0, **LENS)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ (h)
def test_options_reject_unknown_keys():
    from patchrefinerv2_amd.output import _bokeh_options
    assert _bokeh_options({}) == dict(aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0)
    assert _bokeh_options(dict(focus=3, focus_point=[0.25, 1], max_radius=4)) == dict(aperture=0.025, focus=3.0, focus_point=(0.25, 1.0), max_radius=4.0)
    with pytest.raises(ValueError, match="radius"):
        _bokeh_options(dict(radius=4.0))


def test_write_geometry_host_and_the_testers_host_route(tmp_path, capsys):
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    d, img = _random_scene()
    d = np.where(np.isfinite(d), d, F32(2.0)).clip(0.5, 10.0).astype(F32)  # (Tester._emit's colour map needs finite values)
    k = O.camera_intrinsics((24, 32), (24, 32), fov=70.0)

    def files(work):
        return {n: (tmp_path / work / n).read_bytes() for n in sorted(os.listdir(tmp_path / work))}

    opt = dict(aperture=0.5, focus=2.0, max_radius=3.5)
    for work, kw in (("g0", {}), ("g1", dict(bokeh=None)), ("g2", dict(bokeh=opt))):
        (tmp_path / work).mkdir()
        O.write_geometry_host(str(tmp_path / work / "f"), d, img, k, **kw)
    assert set(files("g0")) == {"f.ply", "f_normal.png"} and files("g1") == files("g0")
    assert set(files("g2")) == set(files("g0")) | {"f_bokeh.png"} and {n: v for n, v in files("g2").items() if n != "f_bokeh.png"} == files("g0")
    want = O.bokeh_image_host(d, img, k, **opt)
    assert np.array_equal(_decode(files("g2")["f_bokeh.png"]), want) and not np.array_equal(want, _bytes(img))
    with pytest.raises(ValueError, match="bokeh"):
        O.write_geometry_host(str(tmp_path / "g0" / "x"), d, img, k, ply=False, normals=False, bokeh=dict(radius=1.0))
    capsys.readouterr()
    bad = d.copy()
    bad[12, 16] = np.nan
    O.write_geometry_host(str(tmp_path / "g0" / "y"), bad, img, k, ply=False, normals=False, bokeh=dict(max_radius=3.5))
    assert capsys.readouterr().out.count("warning") == 1 and np.array_equal(_decode((tmp_path / "g0" / "y_bokeh.png").read_bytes()), _bytes(img))

    dt, item = torch.from_numpy(d[None, None]), dict(img_file_basename="f", image_hr=torch.from_numpy(img)[None])

    def run(work, **flags):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), fov=70.0, ply_depth_range=(0.0, 9.0), **flags), None, None)
        t._emit([], item, dt, None, (24, 32))
        return files(work)

    assert Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_bokeh=False), None, None)._geometry(dt, (24, 32)) is None
    assert Tester(None, RunnerInfo(save=False, work_dir=str(tmp_path), save_bokeh=True), None, None)._geometry(dt, (24, 32)) is None
    geo = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_bokeh=True), None, None)._geometry(dt, (24, 32))
    assert geo["bokeh"] == dict(aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0) and not (geo["ply"] or geo["normals"] or geo["mesh"])
    assert "bokeh" not in Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_ply=True), None, None)._geometry(dt, (24, 32))
    plain = run("plain")
    assert set(plain) == {"f.png", "f_uint16.png", "f_edge.png"} and run("off", save_bokeh=False) == plain
    got = run("on", save_bokeh=True, bokeh_aperture=0.5, bokeh_focus_point=(0.25, 0.75), bokeh_max_radius=3.5)
    assert set(got) == set(plain) | {"f_bokeh.png"} and {n: v for n, v in got.items() if n != "f_bokeh.png"} == plain
    want = O.bokeh_image_host(d, img, k, aperture=0.5, focus_point=(0.25, 0.75), max_radius=3.5, depth_range=(0.0, 9.0))
    assert np.array_equal(_decode(got["f_bokeh.png"]), want)


@pytest.mark.parametrize("flags,message", [
    (["--save-bokeh"], "need --save"),
    (["--save", "--save-bokeh", "--bokeh-focus", "0"], "--bokeh-focus"),
    (["--save", "--save-bokeh", "--bokeh-focus-point", "0.5", "1.5"], "--bokeh-focus-point"),
    (["--save", "--save-bokeh", "--bokeh-max-radius", "33"], "--bokeh-max-radius"),
    (["--save", "--save-bokeh", "--bokeh-aperture", "-1"], "--bokeh-aperture"),
])
def test_cli_argument_errors(flags, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", *flags], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


def test_cli_flags_reach_runner_info():
    src = open(os.path.join(ROOT, "tools", "test.py")).read()
    for flag, key in (("--save-bokeh", "save_bokeh"), ("--bokeh-aperture", "bokeh_aperture"), ("--bokeh-focus", "bokeh_focus"),
                      ("--bokeh-focus-point", "bokeh_focus_point"), ("--bokeh-max-radius", "bokeh_max_radius")):
        assert f'"{flag}"' in src and re.search(rf"\b{key}=(tuple\()?args\.{key}\b", src), flag


# ------------------------------------------------------------------------------------------------------------------ (i)
SYMBOLS = ("prv2_bokeh_max_radius", "prv2_bokeh_tile_bound", "prv2_bokeh_render", "prv2_bokeh_rows")


def test_entry_points_declared_bound_exported_and_ops_registered():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert "Depth-of-field export" in hdr
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
    lib = L.load()
    assert lib.prv2_abi_version() == L.ABI_VERSION and 16 <= lib.prv2_bokeh_max_radius() <= 64
    assert lib.prv2_bokeh_tile_bound(-1) == 1  # the per-tile bound is on unless a measurement turns it off
    ops = torch_ops.load()
    for name in ("bokeh_render", "bokeh_rows"):
        assert name in torch_ops.OPS
        getattr(ops, name).default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.bokeh_render(torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), 5.0, 0.1, 0.0, 0.5, 0.5, 4.0, 0.0, INF)  # no CPU implementation to fall into


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)  # never dereferenced: every call fails its argument check before a launch
    cap = lib.prv2_bokeh_max_radius()
    nan = float("nan")

    def render(depth=p, image=p, n=1, h=4, w=4, ih=4, iw=4, fx=5.0, aperture=0.1, focus=0.0, u=0.5, v=0.5, rm=4.0, lo=0.0, hi=INF, out=p, used=p):
        return lib.prv2_bokeh_render(depth, image, n, h, w, ih, iw, fx, aperture, focus, u, v, rm, lo, hi, out, used, None)

    def rows(depth=p, image=p, n=1, h=4, w=4, ih=4, iw=4, fx=5.0, aperture=0.1, focus=0.0, u=0.5, v=0.5, rm=4.0, lo=0.0, hi=INF, buf=p, stride=64, used=p):
        return lib.prv2_bokeh_rows(depth, image, n, h, w, ih, iw, fx, aperture, focus, u, v, rm, lo, hi, buf, stride, used, None)
    for call in (render, rows):
        assert call(depth=None) != 0 and "null" in err()
        assert call(image=None) != 0 and "null" in err()
        assert call(used=None) != 0 and "null" in err()
        assert call(n=0) != 0 and "frame count" in err()
        assert call(h=0) != 0 and "shape" in err()
        assert call(w=-1) != 0 and "shape" in err()
        assert call(ih=0) != 0 and "image shape" in err()
        assert call(iw=0) != 0 and "image shape" in err()
        for bad in (0.0, -5.0, INF, nan):
            assert call(fx=bad) != 0 and "focal" in err()
        for bad in (-0.1, INF, nan):
            assert call(aperture=bad) != 0 and "aperture" in err()
        for bad in (nan, -1.0, cap + 0.5):
            assert call(rm=bad) != 0 and "max_radius" in err() and "prv2_bokeh_max_radius" in err()
        assert call(lo=nan) != 0 and "NaN" in err()
        assert call(hi=nan) != 0 and "NaN" in err()
        assert call(focus=INF) != 0 and "focus" in err()
        for bad in (dict(u=-0.1), dict(u=1.1), dict(v=-0.1), dict(v=1.5), dict(u=nan), dict(v=nan)):
            assert call(**bad) != 0 and "focus point" in err()
    assert render(out=None) != 0 and "null" in err()
    assert rows(buf=None) != 0 and "null" in err()
    assert rows(buf=odd) != 0 and "aligned" in err()
    assert rows(stride=48) != 0 and "stride" in err()  # 4 rows of 13 bytes need 64
    assert rows(stride=72) != 0 and "stride" in err()  # not a multiple of 16


def test_wrappers_validate_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.bokeh_render(torch.ones(4, 4), torch.ones(3, 4, 4), K)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.bokeh_rows(torch.ones(4, 4), torch.ones(3, 4, 4), K)
