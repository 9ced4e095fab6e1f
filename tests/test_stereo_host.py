"""CPU: the host half of the stereo export (patchrefinerv2_amd/output.py).  The host specification of the right-eye view on
hand-checkable rows and against a row-by-row restatement in plain Python, the three layouts, the C entry points (declared, bound,
exported, rejecting bad arguments without a GPU), the CLI's argument error and the tester's host route."""
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
SYMBOLS = ("prv2_stereo_max_width", "prv2_stereo_source", "prv2_stereo_rows")
F32 = np.float32
INF = float("inf")
K = np.array([50.0, 55.0, 19.5, 14.25], dtype=F32)  # fx, fy, cx, cy


def _image(h, w, seed=0):
    return np.random.RandomState(seed).rand(3, h, w).astype(F32)


def _bytes(img):
    """the left eye: the image's bytes on its own grid, [h, w, 3]"""
    from patchrefinerv2_amd.output import color_bytes
    return np.moveaxis(color_bytes(np.asarray(img, dtype=F32) * F32(255)), 0, -1)


def _source_by_row(depth, fx, baseline, convergence=INF, depth_range=(0.0, INF), edge_thr=0.05):
    """the rule of the issue, pixel by pixel in plain Python (float32 scalars) -> (src, filled)"""
    d = np.asarray(depth, dtype=F32)
    h, w = d.shape
    k = F32(F32(fx) * F32(baseline))
    c = F32(0) if math.isinf(convergence) else F32(k / F32(convergence))
    lo, hi, thr = F32(depth_range[0]), F32(depth_range[1]), F32(edge_thr)

    def valid(z):
        return bool(np.isfinite(z) and z > lo and z < hi)

    def target(x, z):
        with np.errstate(all="ignore"):
            tf = F32(F32(x) - np.rint(F32(F32(k / z) - c)))
        return -1 if np.isnan(tf) else int(min(max(tf, F32(-1)), F32(w)))

    src, filled = np.full((h, w), -1, dtype=np.int32), np.full((h, w), -1, dtype=np.int32)
    for y in range(h):
        best = {}
        for x in range(w):
            z = d[y, x]
            if not valid(z):
                continue
            t = e = target(x, z)
            if x + 1 < w and valid(d[y, x + 1]):
                zn = d[y, x + 1]
                if not thr > 0 or not abs(F32(z - zn)) > F32(thr * min(z, zn)):
                    e = max(t, target(x + 1, zn) - 1)
            for q in range(max(t, 0), min(e, w - 1) + 1):
                if q not in best or (z, x) < (d[y, best[q]], best[q]):
                    best[q] = x
        for q, x in best.items():
            src[y, q] = x
        for q in range(w):
            if q in best:
                filled[y, q] = best[q]
                continue
            left = max((p for p in best if p < q), default=None)
            right = min((p for p in best if p > q), default=None)
            if left is not None and right is not None:
                filled[y, q] = best[right] if d[y, best[right]] > d[y, best[left]] else best[left]
            elif left is not None or right is not None:
                filled[y, q] = best[left if right is None else right]
    return src, filled


def _scene(h, w, seed):
    """step blocks over a slanted background, noise, and every kind of invalid value"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (3.0 + 0.04 * x + 0.01 * y + 0.02 * rs.rand(h, w)).astype(F32)
    d[:, w // 5:w // 3] = 1.5
    d[h // 2:, w // 2:2 * w // 3] = 2.0
    idx = rs.choice(h * w, size=max(5, h * w // 10), replace=False)
    d.reshape(-1)[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=F32), idx.size)
    return d


def test_a_plane_shifts_by_its_disparity():
    from patchrefinerv2_amd.output import stereo_image_host, stereo_source_host
    h, w = 3, 16
    d = np.full((h, w), 2.5, dtype=F32)
    img = _image(h, w, 1)
    for fx, baseline in ((50.0, 0.3), (50.0, 0.125), (37.0, 0.1)):  # 6, 2.5 (a tie: to even, 2) and 1.48
        shift = int(np.rint(F32(F32(fx) * F32(baseline)) / F32(2.5)))
        assert shift == {0.3: 6, 0.125: 2, 0.1: 1}[baseline]
        src, filled = stereo_source_host(d, (fx, 1, 0, 0), baseline)
        want = np.arange(w) + shift
        assert np.array_equal(src, np.tile(np.where(want < w, want, -1), (h, 1)))
        assert np.array_equal(filled, np.tile(np.minimum(want, w - 1), (h, 1)))  # the right border: from the left neighbour
        view = stereo_image_host(d, img, (fx, 1, 0, 0), baseline)
        assert np.array_equal(view, _bytes(img)[:, np.minimum(want, w - 1)])


def test_zero_baseline_and_convergence_at_the_plane_give_the_left_image():
    from patchrefinerv2_amd.output import stereo_image_host, stereo_source_host
    h, w = 4, 13
    img = _image(h, w, 2)
    rough = (2.0 + np.random.RandomState(0).rand(h, w)).astype(F32)
    assert np.array_equal(stereo_image_host(rough, img, K, 0.0), _bytes(img))
    ident = np.tile(np.arange(w, dtype=np.int32), (h, 1))
    for got in stereo_source_host(rough, K, 0.0):
        assert np.array_equal(got, ident)
    plane = np.full((h, w), 4.0, dtype=F32)
    assert not np.array_equal(stereo_image_host(plane, img, K, 0.5), _bytes(img))
    assert np.array_equal(stereo_image_host(plane, img, K, 0.5, convergence=4.0), _bytes(img))
    rough[2, 3] = np.nan  # identity on every valid row: the other rows stay what they were
    src, filled = stereo_source_host(rough, K, 0.0)
    assert np.array_equal(np.delete(src, 2, axis=0), np.delete(ident, 2, axis=0)) and src[2, 3] == -1 and filled[2, 3] in (2, 4)


def test_a_foreground_block_occludes_and_its_hole_fills_from_the_farther_side():
    from patchrefinerv2_amd.output import stereo_source_host
    d = np.full((1, 12), 2.0, dtype=F32)
    d[0, 4:7] = 1.0  # disparity 6 in front of 3
    src, filled = stereo_source_host(d, (10.0, 1, 0, 0), 0.6)
    # the block's last pixel and the background's x = 3 both land on column 0: the nearer one shows
    assert src.tolist() == [[6, -1, -1, -1, 7, 8, 9, 10, 11, -1, -1, -1]]
    # one hole run right of the block, filled from the background on its right, not from the block on its left
    assert filled.tolist() == [[6, 7, 7, 7, 7, 8, 9, 10, 11, 11, 11, 11]]
    # a hole between a far surface on the left and a near one on the right takes the left one
    # (an eye to the LEFT: s = -1 for the far four, -4 for the near eight)
    d = np.array([[4.0] * 4 + [1.0] * 8], dtype=F32)
    src, filled = stereo_source_host(d, (4.0, 1, 0, 0), -1.0)
    assert src.tolist() == [[-1, 0, 1, 2, 3, -1, -1, -1, 4, 5, 6, 7]] and filled.tolist() == [[0, 0, 1, 2, 3, 3, 3, 3, 4, 5, 6, 7]]


def test_equal_depths_keep_the_smaller_source_column():
    """the tie case of the issue: the first pixel's span reaches the third pixel's target, both have Z = 1"""
    from patchrefinerv2_amd.output import stereo_source_host
    z = np.array([[1.0, 1.04, 1.0]], dtype=F32)
    src, filled = stereo_source_host(z, (50.0, 1, 0, 0), 1.0, convergence=1.0, edge_thr=0.05)
    assert src.tolist() == [[0, 0, 0]] and filled.tolist() == [[0, 0, 0]]
    assert [a.tolist() for a in _source_by_row(z, 50.0, 1.0, 1.0)] == [[[0, 0, 0]], [[0, 0, 0]]]
    src, _ = stereo_source_host(z, (50.0, 1, 0, 0), 1.0, convergence=1.0, edge_thr=0.03)  # not joined: no span, no tie
    assert src.tolist() == [[0, -1, 2]]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 0.0, -1.5, 0.5, 9.0])
def test_invalid_pixels_make_holes_and_never_win(bad):
    from patchrefinerv2_amd.output import stereo_image_host, stereo_source_host
    d = np.full((2, 9), 2.0, dtype=F32)
    d[0, 4] = bad  # (0.5 and 9 are outside the range below; 0.5 would win every depth test it entered)
    src, filled = stereo_source_host(d, (10.0, 1, 0, 0), 0.2, depth_range=(1.0, 8.0))
    assert src.tolist() == [[1, 2, 3, -1, 5, 6, 7, 8, -1], [1, 2, 3, 4, 5, 6, 7, 8, -1]]
    assert filled[0].tolist() == [1, 2, 3, 3, 5, 6, 7, 8, 8] and not (src == 4)[0].any()
    for got, want in zip(stereo_source_host(d, (10.0, 1, 0, 0), 0.2, depth_range=(1.0, 8.0)), _source_by_row(d, 10.0, 0.2, depth_range=(1.0, 8.0))):
        assert np.array_equal(got, want)
    d[1] = bad  # a row of nothing but invalid pixels is black
    src, filled = stereo_source_host(d, (10.0, 1, 0, 0), 0.2, depth_range=(1.0, 8.0))
    assert (src[1] == -1).all() and (filled[1] == -1).all()
    view = stereo_image_host(d, _image(2, 9), (10.0, 1, 0, 0), 0.2, depth_range=(1.0, 8.0))
    assert not view[1].any() and view[0].any()


def test_targets_off_either_edge_are_dropped():
    from patchrefinerv2_amd.output import stereo_source_host
    d = np.full((1, 6), 1.0, dtype=F32)
    src, filled = stereo_source_host(d, (4.0, 1, 0, 0), 1.0)  # shift 4 to the left
    assert src.tolist() == [[4, 5, -1, -1, -1, -1]] and filled.tolist() == [[4, 5, 5, 5, 5, 5]]
    src, filled = stereo_source_host(d, (4.0, 1, 0, 0), -1.0)  # and to the right
    assert src.tolist() == [[-1, -1, -1, -1, 0, 1]] and filled.tolist() == [[0, 0, 0, 0, 0, 1]]
    src, _ = stereo_source_host(d, (4.0, 1, 0, 0), 100.0)  # everything off the frame
    assert (src == -1).all()
    tiny = np.full((1, 6), 1e-30, dtype=F32)  # k / Z overflows to inf: the target clips to -1
    assert (stereo_source_host(tiny, (4.0e20, 1, 0, 0), 1.0e20)[0] == -1).all()


def test_edge_thr_decides_which_neighbours_are_joined():
    from patchrefinerv2_amd.output import stereo_source_host
    d = np.array([[4.0, 2.0, 2.0, 2.0]], dtype=F32)  # negative disparities: s = 2 - 4 = -2 and 4 - 4 = 0
    cam = dict(intrinsics=(8.0, 1, 0, 0), baseline=1.0, convergence=2.0)
    src, _ = stereo_source_host(d, edge_thr=0.05, **cam)  # 4 | 2 is a depth edge: x = 0 covers its own target only
    assert src.tolist() == _source_by_row(d, 8.0, 1.0, 2.0, edge_thr=0.05)[0].tolist() == [[-1, 1, 2, 3]]
    far = np.array([[2.0, 4.0, 4.0, 9.0]], dtype=F32)  # t = 0, 3, 4 -> w, 6 -> w
    src, _ = stereo_source_host(far, edge_thr=0.05, **cam)
    assert src.tolist() == [[0, -1, -1, 1]]
    for thr in (0.0, -1.0):  # every valid pair is joined: x = 0 stretches up to the column before x = 1's target
        src, _ = stereo_source_host(far, edge_thr=thr, **cam)
        assert src.tolist() == [[0, 0, 0, 1]]
        assert src.tolist() == _source_by_row(far, 8.0, 1.0, 2.0, edge_thr=thr)[0].tolist()
    far[0, 1] = np.nan  # but never across an invalid pixel
    assert stereo_source_host(far, edge_thr=0.0, **cam)[0].tolist() == [[0, -1, -1, -1]]


@pytest.mark.parametrize("case", [dict(baseline=0.4), dict(baseline=0.4, convergence=2.5), dict(baseline=-0.3), dict(baseline=0.4, edge_thr=0.0),
                                  dict(baseline=0.4, depth_range=(1.6, 4.5)), dict(baseline=1.5, edge_thr=0.5)])
def test_specification_equals_the_row_by_row_restatement(case):
    from patchrefinerv2_amd.output import stereo_source_host
    d = _scene(7, 61, seed=3)
    got = stereo_source_host(d, K, **case)
    want = _source_by_row(d, K[0], **case)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] == -1).any() and (got[0] >= 0).any() and got[0].dtype == got[1].dtype == np.int32
    assert np.array_equal(got[1][got[0] >= 0], got[0][got[0] >= 0])  # the fill touches holes only


def test_layouts_shapes_and_channels():
    from patchrefinerv2_amd.output import sample_indices, stereo_image_host, stereo_source_host, stereo_view_host
    h, w = 6, 21
    d, img = _scene(h, w, seed=5), _image(9, 13, 4)  # an image of another size: nearest samples
    img[1, 2, 3], img[0, 0, 0], img[2, 1, 1] = np.nan, 1.7, -0.3
    cam = dict(intrinsics=K, baseline=0.3, convergence=6.0)
    left = _bytes(img)[sample_indices(h, 9)[:, None], sample_indices(w, 13)[None, :]]
    _, filled = stereo_source_host(d, **cam)
    right = np.where((filled >= 0)[..., None], left[np.arange(h)[:, None], np.maximum(filled, 0)], 0).astype(np.uint8)
    view = stereo_view_host(d, img, **cam)
    assert view.dtype == np.uint8 and view.shape == (h, w, 3) and np.array_equal(view, right)
    assert np.array_equal(stereo_image_host(d, img, layout="right", **cam), right)
    sbs = stereo_image_host(d, img, layout="sbs", **cam)
    assert sbs.shape == (h, 2 * w, 3) and np.array_equal(sbs[:, :w], left) and np.array_equal(sbs[:, w:], right)
    ana = stereo_image_host(d, img, layout="anaglyph", **cam)
    assert ana.shape == (h, w, 3) and np.array_equal(ana[..., 0], left[..., 0]) and np.array_equal(ana[..., 1:], right[..., 1:])
    assert not np.array_equal(left, right)
    with pytest.raises(ValueError, match="layout"):
        stereo_image_host(d, img, layout="left", **cam)
    with pytest.raises(ValueError, match="convergence"):
        stereo_source_host(d, K, 0.3, convergence=0.0)


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def test_write_geometry_host_and_the_testers_host_route(tmp_path):
    """without ``stereo`` write_geometry_host and Tester._emit write exactly the files they wrote before; with it one PNG more, the
    host specification's pixels at the result's grid; _geometry is None without any flag"""
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    d = torch.from_numpy(_scene(24, 40, seed=3)[None, None])
    d[d != d] = 2.0
    d = d.clamp(0.5, 10.0)  # (Tester._emit's colour map needs finite values)
    img = torch.from_numpy(_image(24, 40, 1))
    item = dict(img_file_basename="f", image_hr=img[None])
    k = O.camera_intrinsics((24, 40), (24, 40), fov=70.0)

    def files(work):
        return {n: (tmp_path / work / n).read_bytes() for n in sorted(os.listdir(tmp_path / work))}

    for work, kw in (("g0", {}), ("g1", dict(stereo=None)), ("g2", dict(stereo=dict(baseline=0.2, layout="anaglyph")))):
        (tmp_path / work).mkdir()
        O.write_geometry_host(str(tmp_path / work / "f"), d[0, 0].numpy(), img.numpy(), k, mesh=True, **kw)
    assert set(files("g0")) == {"f.ply", "f_normal.png", "f_mesh.ply"} and files("g1") == files("g0")
    assert set(files("g2")) == set(files("g0")) | {"f_anaglyph.png"} and {n: v for n, v in files("g2").items() if n != "f_anaglyph.png"} == files("g0")
    assert np.array_equal(_decode(files("g2")["f_anaglyph.png"]), O.stereo_image_host(d[0, 0].numpy(), img.numpy(), k, 0.2, layout="anaglyph"))
    with pytest.raises(ValueError, match="stereo"):
        O.write_geometry_host(str(tmp_path / "g0" / "x"), d[0, 0].numpy(), img.numpy(), k, ply=False, normals=False, stereo=dict(base=1.0))

    def run(work, **flags):
        info = RunnerInfo(save=True, work_dir=str(tmp_path / work), fov=70.0, ply_edge_thr=0.3, ply_depth_range=(0.0, 9.0), **flags)
        t = Tester(None, info, None, None)
        t._emit([], item, d, None, (24, 40))
        return files(work)

    for flags in (dict(), dict(save_stereo=False), dict(save_ply=False, save_normals=False, save_mesh=False, save_stereo=False)):
        assert Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), **flags), None, None)._geometry(d, (24, 40)) is None
    assert Tester(None, RunnerInfo(save=False, work_dir=str(tmp_path), save_stereo=True), None, None)._geometry(d, (24, 40)) is None
    geo = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_stereo=True), None, None)._geometry(d, (24, 40))
    assert geo["stereo"] == dict(baseline=0.065, convergence=INF, layout="right") and not (geo["ply"] or geo["normals"] or geo["mesh"])
    assert "stereo" not in Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_ply=True), None, None)._geometry(d, (24, 40))
    plain = run("plain")
    assert set(plain) == {"f.png", "f_uint16.png", "f_edge.png"} and run("off", save_stereo=False) == plain
    right = run("right", save_stereo=True, stereo_baseline=0.5)
    assert set(right) == set(plain) | {"f_right.png"} and {n: v for n, v in right.items() if n != "f_right.png"} == plain
    want = O.stereo_image_host(d[0, 0].numpy(), img.numpy(), k, 0.5, depth_range=(0.0, 9.0), edge_thr=0.3)
    assert np.array_equal(_decode(right["f_right.png"]), want) and not np.array_equal(want, _bytes(img.numpy()))
    sbs = run("sbs", save_stereo=True, save_ply=True, stereo_baseline=0.5, stereo_convergence=3.0, stereo_layout="sbs")
    assert set(sbs) == set(plain) | {"f_sbs.png", "f.ply"}
    want = O.stereo_image_host(d[0, 0].numpy(), img.numpy(), k, 0.5, 3.0, (0.0, 9.0), 0.3, "sbs")
    assert _decode(sbs["f_sbs.png"]).shape == (24, 80, 3) and np.array_equal(_decode(sbs["f_sbs.png"]), want)


@pytest.mark.parametrize("flags,message", [
    (["--save-stereo"], "need --save"),
    (["--save-stereo", "--stereo-layout", "sbs", "--stereo-baseline", "0.1"], "need --save"),
    (["--save", "--save-stereo", "--stereo-layout", "left"], "--stereo-layout"),
    (["--save", "--save-stereo", "--stereo-convergence", "0"], "--stereo-convergence"),
])
def test_cli_argument_errors(flags, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", *flags], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


def test_entry_points_declared_bound_exported_and_ops_registered():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20 and "Stereo export" in hdr
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
    lib = L.load()
    assert lib.prv2_abi_version() == 20 and lib.prv2_stereo_max_width() >= 8192
    ops = torch_ops.load()
    for name in ("stereo_rows", "stereo_source"):
        assert name in torch_ops.OPS
        getattr(ops, name).default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.stereo_source(torch.zeros(1, 4, 4), 5.0, 0.1, INF, 0.0, INF, 0.05)  # no CPU implementation to fall into


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)  # never dereferenced: every call fails its argument check before a launch
    limit = lib.prv2_stereo_max_width()

    def source(depth=p, n=1, h=4, w=4, fx=5.0, baseline=0.1, convergence=INF, lo=0.0, thr=0.05, src=p, filled=p):
        return lib.prv2_stereo_source(depth, n, h, w, fx, baseline, convergence, lo, INF, thr, src, filled, None)
    assert source(depth=None) != 0 and "null" in err()
    assert source(src=None) != 0 and "null" in err()
    assert source(filled=None) != 0 and "null" in err()
    assert source(n=0) != 0 and "frame count" in err()
    assert source(h=0) != 0 and "shape" in err()
    assert source(w=limit + 1) != 0 and str(limit) in err() and "prv2_stereo_max_width" in err()
    assert source(fx=0.0) != 0 and "focal" in err()
    assert source(baseline=INF) != 0 and "baseline" in err()
    assert source(convergence=0.0) != 0 and "convergence" in err()
    assert source(convergence=float("nan")) != 0 and "convergence" in err()
    assert source(lo=float("nan")) != 0 and "NaN" in err()
    assert source(thr=float("nan")) != 0 and "NaN" in err()

    rb, rb2 = lib.prv2_rows_bytes(4, 4, 3), lib.prv2_rows_bytes(4, 8, 3)

    def rows(image=p, ih=8, layout=0, out=p, fstride=rb, w=4):
        return lib.prv2_stereo_rows(p, image, 1, 4, w, ih, 8, 5.0, 0.1, INF, 0.0, INF, 0.05, layout, out, fstride, None)
    assert rows(image=None) != 0 and "null" in err()
    assert rows(ih=0) != 0 and "image shape" in err()
    assert rows(layout=3) != 0 and "layout" in err()
    assert rows(out=None) != 0 and "null" in err()
    assert rows(out=odd) != 0 and "aligned" in err()
    assert rows(fstride=rb - 16) != 0 and "stride" in err()
    assert rb2 > rb and rows(layout=1, fstride=rb) != 0 and "stride" in err()  # side by side: rows of 2 w pixels
    assert rows(w=limit + 1, fstride=1 << 30) != 0 and "prv2_stereo_max_width" in err()
    with pytest.raises(RuntimeError):
        L.check(rows(out=None), "stereo_rows")


def test_wrappers_validate_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    d = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="GPU"):
        ops.stereo_source(d, K, 0.1)  # a CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        ops.stereo_rows(d, torch.zeros(3, 4, 4), K, 0.1)
    with pytest.raises(ValueError, match="layout"):
        ops.stereo_rows(d, torch.zeros(3, 4, 4), K, 0.1, layout="left")
