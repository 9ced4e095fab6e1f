"""GPU: the depth-of-field export (csrc/bokeh.hip through ops.bokeh_render / ops.bokeh_rows, OutputStage.submit_geometry(bokeh=...)).
The oracle is the host specification of patchrefinerv2_amd/output.py (numpy float32): the fp32 planes, the focus distances and the
scanline bytes are compared for equality, on both dispatch routes.  A workgroup owns a tile of 64 x 16 outputs and streams the source
rows it reaches through LDS in bands of 16; the shapes are the smallest at which tiling, halo, bands and bounds can go wrong."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32 = np.float32
INF = float("inf")
INVALID = np.array([np.nan, np.inf, -np.inf, 0.0, -1.5, 0.2, 9.0], dtype=F32)
# (frames, rows, columns), max_radius, image size as a multiple of the map's (or its rows and columns)
CASES = [((1, 1, 1), 4.0, 1),      # the smallest frame
         ((1, 5, 9), 8.0, 1),      # a window larger than the frame
         ((1, 37, 53), 5.0, 1),    # ragged in both directions against the tile
         ((2, 64, 80), 8.0, 1),    # two frames, the second with another depth under the focus point; four tile rows, two tile columns
         ((1, 9, 300), None, 1),   # one tile row, the widest window (None: the cap)
         ((1, 130, 70), 2.5, 2)]   # a fractional radius, the image at twice the map's size
# the two branches of the image's nearest sampling (csrc/scene.h nearest) that CASES leaves out
SAMPLING = [((1, 37, 53), 5.0, (23, 91)),  # no multiple of the map's size: the division, with a remainder
            ((1, 1, 300), 8.0, 1)]         # the map's size on a ragged row: the shortcut
SCENES = ("bar_sharp", "bar_blur", "slant", "random", "invalid", "invalid_focus", "in_focus")
torch.set_grad_enabled(False)


@pytest.fixture(params=["torch", "ctypes"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _cap():
    from patchrefinerv2_amd import lib as L
    return float(L.load().prv2_bokeh_max_radius())


def _camera(h, w):
    from patchrefinerv2_amd.output import camera_intrinsics
    return camera_intrinsics((h, w), (h, w), fov=63.0) + F32(0.37)


def _image(hi, wi, seed):
    img = np.random.RandomState(100 + seed).rand(3, hi, wi).astype(F32) * F32(1.2) - F32(0.1)  # below 0 and above 1 clamp
    img.reshape(-1)[::31] = np.nan
    if img.size > 40:
        img.reshape(-1)[40] = np.inf
    return img


def _scene(name, B, h, w, rm):
    """-> depth [B, h, w], the keyword arguments of the call but the intrinsics.  The aperture makes a difference of 0.4 / m in inverse
    depth reach max_radius: the scenes hold radii from 0 to the cap"""
    rs = np.random.RandomState(B * 1000 + h * 31 + w)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    fx = float(_camera(h, w)[0])
    kw = dict(aperture=2.0 * rm / (fx * 0.4), max_radius=rm, depth_range=(0.0, INF))
    if name in ("bar_sharp", "bar_blur"):  # a bar at 2 m in front of a wall at 6 m, focused on the bar / on the wall
        d = np.full((h, w), 6.0, dtype=F32)
        d[:, w // 3:max(w // 2, w // 3 + 1)] = 2.0
        kw.update(focus=2.0 if name == "bar_sharp" else 6.0)
    elif name == "slant":  # a plane: every radius between 0 and the cap, the focus point's column sharp
        d = (1.0 + 4.0 * x / w + 0.05 * y).astype(F32)
    elif name == "random":  # random depth, 10 % invalid pixels of every kind, a valid pixel under the focus point
        d = (1.0 + 5.0 * rs.rand(h, w)).astype(F32)
        idx = rs.choice(h * w, size=(h * w + 9) // 10, replace=False)
        d.reshape(-1)[idx] = np.resize(INVALID, idx.size)
        kw.update(depth_range=(0.5, 7.0), focus_point=(0.25, 0.75))
    elif name in ("invalid", "invalid_focus"):  # no valid pixel: the image itself and a NaN focus / every pixel infinitely far
        d = np.resize(INVALID, (h, w)).astype(F32)
        kw.update(depth_range=(0.5, 7.0), **(dict(focus=2.0) if name == "invalid_focus" else {}))
    elif name == "in_focus":  # every radius 0: every tile leaves by the early exit
        d = np.full((h, w), 3.0, dtype=F32)
    else:
        raise KeyError(name)
    d = np.stack([d] + [np.roll(d, 3 * f, axis=1) + F32(0.25 * f) for f in range(1, B)])
    if name == "random":
        u, v = kw["focus_point"]
        d[:, min(h - 1, int(v * h)), min(w - 1, int(u * w))] = [2.5 + f for f in range(B)]
    return np.ascontiguousarray(d, dtype=F32), kw


_HOST = {}


def _host(name, case):
    """the specification's planes and focus distances of a scene, computed once and shared (never modified)"""
    from patchrefinerv2_amd.output import bokeh_render_host
    shape, rm, scale = case
    rm = _cap() if rm is None else rm
    key = (name, shape, rm, scale)
    if key not in _HOST:
        B, h, w = shape
        d, kw = _scene(name, B, h, w, rm)
        k = _camera(h, w)
        hi, wi = scale if isinstance(scale, tuple) else (h * scale, w * scale)
        img = np.stack([_image(hi, wi, f) for f in range(B)])
        res = [bokeh_render_host(d[f], img[f], k, **kw) for f in range(B)]
        _HOST[key] = (d, img, k, kw, np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=F32))
    return _HOST[key]


def _rows_to_image(rows, h, wout):
    """scanline buffer [B, bytes] (a device tensor) -> uint8 [B, h, wout, 3]; every filter byte and the tail are zero"""
    r = rows.cpu().numpy()
    body = r[:, :h * (1 + 3 * wout)].reshape(r.shape[0], h, 1 + 3 * wout)
    assert not body[:, :, 0].any() and not r[:, h * (1 + 3 * wout):].any()
    assert r.shape[1] == (h * (1 + 3 * wout) + 15) // 16 * 16
    return body[:, :, 1:].reshape(r.shape[0], h, wout, 3)


def _to_bytes(planes):
    from patchrefinerv2_amd.output import color_bytes
    with np.errstate(all="ignore"):
        return np.moveaxis(color_bytes(planes * F32(255)), -3, -1)


def _sampled(img, h, w):
    from patchrefinerv2_amd.output import sample_indices
    g = img[..., sample_indices(h, img.shape[-2])[:, None], sample_indices(w, img.shape[-1])[None, :]]
    return np.where(np.isfinite(g), g, F32(0)).astype(F32)


def _same_floats(got, want):
    """equal values, NaN at the same positions"""
    return got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_planes_focus_and_rows_equal_the_host_specification(ops, case, name):
    (B, h, w), _, _ = case
    d, img, k, kw, want, focus = _host(name, case)
    dd, di = torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV)
    out, used = ops.bokeh_render(dd, di, k, **kw)
    assert out.dtype == used.dtype == torch.float32 and tuple(out.shape) == (B, 3, h, w) and tuple(used.shape) == (B,)
    assert torch.equal(out.cpu(), torch.from_numpy(want)), int((out.cpu().numpy() != want).sum())
    assert _same_floats(used.cpu().numpy(), focus), (used.cpu().numpy(), focus)
    rows, used = ops.bokeh_rows(dd, di, k, **kw)
    got = _rows_to_image(rows, h, w)
    assert np.array_equal(got, _to_bytes(want)), int((got != _to_bytes(want)).sum())
    assert _same_floats(used.cpu().numpy(), focus)
    if name in ("invalid", "in_focus"):  # the image itself
        assert np.array_equal(want, _sampled(img, h, w)) and np.isnan(focus).all() == (name == "invalid")
    if name in ("bar_blur", "slant", "invalid_focus") and w > 1:
        assert not np.array_equal(want, _sampled(img, h, w))
    if name == "random" and B == 2:
        assert focus.tolist() == [2.5, 3.5]


@pytest.mark.parametrize("case", SAMPLING, ids=lambda c: "x".join(map(str, c[0])))
def test_image_sampling_branches_equal_the_host_specification(ops, case):
    (B, h, w), _, _ = case
    d, img, k, kw, want, focus = _host("random", case)
    assert (img.shape[2:] == (h, w)) == (case[2] == 1)
    dd, di = torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV)
    out, used = ops.bokeh_render(dd, di, k, **kw)
    assert torch.equal(out.cpu(), torch.from_numpy(want)), int((out.cpu().numpy() != want).sum())
    assert _same_floats(used.cpu().numpy(), focus), (used.cpu().numpy(), focus)
    rows, used = ops.bokeh_rows(dd, di, k, **kw)
    got = _rows_to_image(rows, h, w)
    assert np.array_equal(got, _to_bytes(want)), int((got != _to_bytes(want)).sum())
    assert _same_floats(used.cpu().numpy(), focus)


def test_a_batch_equals_its_frames_alone_and_a_second_call(ops):
    case = CASES[3]
    d, img, k, kw, want, focus = _host("random", case)
    dd, di = torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV)
    out, used = ops.bokeh_render(dd, di, k, **kw)
    rows, _ = ops.bokeh_rows(dd, di, k, **kw)
    for f in range(2):
        o1, u1 = ops.bokeh_render(dd[f], di[f], k, **kw)  # [h, w] and [3, hi, wi]
        r1, _ = ops.bokeh_rows(dd[f], di[f], k, **kw)
        assert torch.equal(o1[0], out[f]) and torch.equal(u1[0], used[f]) and torch.equal(r1[0], rows[f])
    again, used2 = ops.bokeh_render(dd, di, k, **kw)
    rows2, _ = ops.bokeh_rows(dd, di, k, **kw)
    assert torch.equal(again, out) and torch.equal(used2, used) and torch.equal(rows2, rows)


def test_the_per_tile_bound_changes_no_bit(ops):
    """the walk of a tile is bounded by the radii in its reach; with the bound off every tile walks the full window: the same bits"""
    lib = ops.L.load()
    case = CASES[2]
    for name in ("slant", "random", "in_focus"):
        d, img, k, kw, want, _ = _host(name, case)
        dd, di = torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV)
        assert lib.prv2_bokeh_tile_bound(0) == 1
        try:
            out, _ = ops.bokeh_render(dd, di, k, **kw)
            rows, _ = ops.bokeh_rows(dd, di, k, **kw)
        finally:
            assert lib.prv2_bokeh_tile_bound(1) == 0
        assert torch.equal(out.cpu(), torch.from_numpy(want)) and np.array_equal(_rows_to_image(rows, *case[0][1:]), _to_bytes(want))


def test_validation(ops):
    d, img, k, kw, _, _ = _host("random", CASES[1])
    dd, di = torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV)
    for call in (ops.bokeh_render, ops.bokeh_rows):
        with pytest.raises(ValueError):
            call(dd.cpu(), di, k)
        with pytest.raises(ValueError):
            call(dd, di.cpu(), k)
        with pytest.raises(ValueError):
            call(dd, torch.ones(2, 3, 4, 5, device=DEV), k)
        for bad in (dict(aperture=-1.0), dict(aperture=INF), dict(focus=0.0), dict(focus=float("nan")), dict(focus=INF), dict(focus_point=(0.5, 1.5)),
                    dict(max_radius=-1.0), dict(max_radius=_cap() + 1.0), dict(max_radius=float("nan")), dict(depth_range=(float("nan"), 1.0))):
            with pytest.raises(ValueError):
                call(dd, di, k, **bad)


# ------------------------------------------------------------------------------------------------------------------ OutputStage
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("device_deflate", [False, True])
def test_output_stage_writes_the_host_routes_file(tmp_path, device_deflate, capfd):
    from patchrefinerv2_amd.output import OutputStage, write_geometry_host
    case = CASES[2]
    (_, h, w), rm, _ = case
    d, _, k, kw, _, _ = _host("random", case)
    img = _image(30, 41, 11)
    geo = dict(depth_range=kw["depth_range"])
    bokeh = dict(aperture=kw["aperture"], focus_point=kw["focus_point"], max_radius=rm)
    (tmp_path / "host").mkdir()
    write_geometry_host(str(tmp_path / "host" / "f"), d[0], img, k, ply=False, normals=True, bokeh=bokeh, **geo)
    host = _files(tmp_path / "host")
    assert set(host) == {"f_normal.png", "f_bokeh.png"}

    def run(work, depth=d[0], **more):
        stage = OutputStage(str(tmp_path / work), workers=2, device_deflate=device_deflate)
        stage.submit_geometry(os.path.join(str(tmp_path / work), "f"), torch.from_numpy(depth).to(DEV), torch.from_numpy(img), k, ply=False,
                              normals=True, **geo, **more)
        stage.close()
        return _files(tmp_path / work), stage

    capfd.readouterr()
    dev, stage = run("dev", bokeh=bokeh)
    assert "warning" not in capfd.readouterr().out
    assert set(dev) == set(host)
    for n in host:
        assert np.array_equal(_decode(dev[n]), _decode(host[n])), n
        assert device_deflate or dev[n] == host[n], n  # the same container and deflate: the same file
    off, stage_off = run("off")
    assert set(off) == {"f_normal.png"} and np.array_equal(_decode(off["f_normal.png"]), _decode(host["f_normal.png"]))
    assert stage.files - stage_off.files == 1
    if not device_deflate:
        assert stage.bytes_d2h - stage_off.bytes_d2h == (h * (1 + 3 * w) + 15) // 16 * 16 + 4  # the scanlines and the focus distance
    blind = d[0].copy()
    blind[int(0.75 * h), int(0.25 * w)] = np.nan  # no valid depth under the focus point: the image, and one warning line
    nofocus, _ = run("nofocus", depth=blind, bokeh=bokeh)
    assert capfd.readouterr().out.count("warning") == 1
    assert np.array_equal(_decode(nofocus["f_bokeh.png"]), _to_bytes(_sampled(img, h, w)))


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_save_bokeh(tmp_path):
    """tools/test.py --save --device-output --save-bokeh in a fresh process writes the specification's pixels: the same run on the host
    route (the same model, weights and frame: the same map) writes <name>_bokeh.png from bokeh_render_host itself
    (tests/test_bokeh_host.py pins that file to the specification)"""
    (tmp_path / "imgs").mkdir()
    np.save(str(tmp_path / "imgs" / "frame0.npy"), np.random.RandomState(20).rand(90, 160, 3).astype(np.float32))
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   "model = dict(config=dict(patch_process_shape=[112, 224], image_raw_shape=[256, 512], patch_split_num=[2, 2],\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")

    def run(work, *route):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), str(cfg), "--synthetic-weights", "--cai-mode", "r4",
                            "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(tmp_path / work),
                            "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", *route, "--save-bokeh", "--bokeh-aperture", "0.5",
                            "--bokeh-focus-point", "0.25", "0.5", "--bokeh-max-radius", "3"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return _decode((tmp_path / work / "frame0_bokeh.png").read_bytes())

    dev, host = run("dev", "--device-output"), run("host")
    assert dev.shape == (256, 512, 3) and np.array_equal(dev, host)
    sharp = _decode((tmp_path / "dev" / "frame0.png").read_bytes())
    assert sharp.shape == dev.shape and dev.any()
