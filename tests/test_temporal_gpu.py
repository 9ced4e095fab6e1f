"""GPU: temporal stabilisation (csrc/temporal.hip through ops.temporal_step and temporal.TemporalStabilizer).  The oracle is the numpy
specification temporal.temporal_step_host: the output maps, the state (its map and both luma buffers) and every word of the stats
rows are compared for EQUALITY, on both dispatch routes.  A block owns 8 rows x 1024 columns, a thread a quad of columns; rows of
w % 4 == 0 take the 16-byte accesses, the others the scalar path; an image of the map's size is read in quads, any other is gathered."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32 = np.float32
NAN, INF = float("nan"), float("inf")
torch.set_grad_enabled(False)

# (h, w), image (ih, iw) or None for the map's size: one pixel; smaller than a quad; exactly one block; one past the block both ways;
# w % 4 != 0 (the scalar path) at more than one block per row; images of another size (smaller, and twice the map)
CASES = [((1, 1), None), ((3, 5), None), ((8, 1024), None), ((9, 1025), None), ((37, 2051), None), ((9, 1028), None),
         ((9, 1025), (23, 31)), ((37, 2051), (74, 4102)), ((16, 1024), (23, 31))]


@pytest.fixture(params=["torch", "ctypes"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def sequence(h, w, ih, iw, frames=3, seed=0):
    """a jittering estimator over a static scene with every special pixel -> [(x fp32 [h, w], image fp32 [3, ih, iw])]: frame 1 is
    fitted against a clean frame 0, frame 2 against an output that carries frame 1's special pixels"""
    rng = np.random.default_rng(seed + 31 * h + w)
    n = h * w
    base = 1.5 + 4.0 * (np.arange(n, dtype=np.float64).reshape(h, w) / max(n - 1, 1)) + 0.3 * np.sin(np.arange(w) / 7.0)[None, :]
    tex = (rng.random((3, ih, iw)) * 0.6 + 0.2).astype(F32)
    seq = []
    for t in range(frames):
        s, b = 1.0 + rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03)
        x = (s * base + b + rng.normal(0.0, 0.002, size=base.shape)).astype(F32)
        img = np.clip(tex + rng.integers(-2, 3, size=(1, ih, iw)).astype(F32) / F32(255), 0, 1).astype(F32)
        if t and ih * iw > 40:  # a block that moves: not static
            c0 = (5 * t) % max(iw - 4, 1)
            img[:, ih // 3:ih // 3 + 3, c0:c0 + 4] = 1.0 - img[:, ih // 3:ih // 3 + 3, c0:c0 + 4]
        img.reshape(-1)[::53] = np.nan  # byte 0
        img.reshape(-1)[1::59] = 1.7     # clamps to 255
        if t and n > 80:
            flat = x.reshape(-1)
            vals = (NAN, INF, -INF, 0.0, -1.5, 1024.0, 5000.0, 3.0e38, 1e-4, 0.001, 1023.999)
            for i, v in enumerate(vals):
                flat[(7 + 13 * i + 101 * t) % n] = v
            flat[(n // 2 + t) % n] *= F32(0.4)  # outside the fit gate
        seq.append((x, img))
    return seq


_HOST = {}


def host_run(key, seq, **kw):
    """the specification over a sequence, computed once per case -> (outs [n, h, w], rows int64 [n, 12], state (y, L), previous luma)"""
    from patchrefinerv2_amd import temporal as T
    k = (key, tuple(sorted(kw.items())))
    if k not in _HOST:
        st, outs, rows, lumas = None, [], [], []
        for x, img in seq:
            out, st, row = T.temporal_step_host(x, img, st, **kw)
            outs.append(out), rows.append(row), lumas.append(st[1])
        _HOST[k] = (np.stack(outs), np.stack(rows), st, lumas[-2] if len(lumas) > 1 else None)
    return _HOST[k]


def device_run(ops, seq, groups, **kw):
    """the same through ops.temporal_step, the sequence cut into calls of ``groups`` frames"""
    h, w = seq[0][0].shape
    d = torch.from_numpy(np.stack([x for x, _ in seq])).to(DEV)
    img = torch.from_numpy(np.stack([i for _, i in seq])).to(DEV)
    state = torch.full((h, w), NAN, device=DEV)
    luma = torch.full((2, h, w), 77, dtype=torch.uint8, device=DEV)
    cur, present, k, outs, rows = 0, False, 0, [], []
    for n in groups:
        out, stats = ops.temporal_step(d[k:k + n], img[k:k + n], state, luma[cur], luma[1 - cur], present, **kw)
        assert out.shape == (n, h, w) and stats.shape == (n, 12) and stats.dtype == torch.int64 and stats.is_cuda
        outs.append(out), rows.append(stats)
        cur, present, k = cur ^ (n & 1), True, k + n
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy(), torch.cat(rows).cpu().numpy(), state.cpu().numpy(), luma[cur].cpu().numpy(), luma[1 - cur].cpu().numpy()


def assert_equal_bits(dev, host, what=""):
    outs, rows, state, L, Lprev = dev
    h_outs, h_rows, (h_y, h_L), h_Lprev = host
    assert outs.tobytes() == h_outs.tobytes(), f"{what}: out differs at {np.argwhere(outs.view(np.uint32) != h_outs.view(np.uint32))[:4]}"
    assert np.array_equal(rows, h_rows), f"{what}: stats\n{rows}\n{h_rows}"
    assert state.tobytes() == h_y.tobytes(), f"{what}: state map"
    assert np.array_equal(L, h_L), f"{what}: luma"
    if h_Lprev is not None:
        assert np.array_equal(Lprev, h_Lprev), f"{what}: the previous luma (the other buffer of the pair)"


@pytest.mark.parametrize("shape,ishape", CASES)
def test_bits_equal_the_specification(ops, shape, ishape):
    from patchrefinerv2_amd import temporal as T
    (h, w), (ih, iw) = shape, ishape or shape
    seq = sequence(h, w, ih, iw)
    host = host_run((shape, ishape), seq)
    stats = [T.stats_dict(r, h * w) for r in host[1]]
    assert stats[0]["reset"]
    if h * w >= 8192:  # the case does what it is there for: a fit, gated-out pixels, the special pixels in the output
        assert all(s["fitted"] and 0.5 * h * w < s["n"] < s["n_gate"] < h * w for s in stats[1:])
        assert np.isnan(host[0][1:]).any() and np.isinf(host[0][1:]).any() and (host[0][1:] <= 0).any()
    else:
        assert all(s["reset"] for s in stats) == (h * w < 64)
    assert_equal_bits(device_run(ops, seq, (1, 1, 1)), host, "one frame per call")
    assert_equal_bits(device_run(ops, seq, (3,)), host, "one call")


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(anchor=0.0), dict(anchor=1.0, alpha=0.9, rho=0.01), dict(tau=0), dict(tau=255, rho=3.0)])
def test_parameters(ops, kw):
    seq = sequence(9, 1025, 9, 1025)
    assert_equal_bits(device_run(ops, seq, (2, 1), **kw), host_run(("params", (9, 1025)), seq, **kw), str(kw))


def test_identity_and_scene_cut_branches(ops):
    """a constant map (det = 0: identity, blended) and a cut (fewer static pixels than the minimum count: reset) on the device"""
    from patchrefinerv2_amd import temporal as T
    h, w = 12, 260
    img = np.full((3, h, w), 0.5, F32)
    cut = img.copy()
    cut[:, :, 20:] = 0.9
    seq = [(np.full((h, w), 2.0, F32), img), (np.full((h, w), 2.5, F32), img), (np.full((h, w), 2.25, F32), cut), (np.full((h, w), 2.0, F32), cut)]
    host = host_run("branches", seq, rho=0.25)
    st = [T.stats_dict(r, h * w) for r in host[1]]
    assert [s["reset"] for s in st] == [True, False, False, False] and not any(s["fitted"] for s in st) and st[2]["n_gate"] == 12 * 20
    seq[2] = (seq[2][0], np.where(np.arange(w)[None, None, :] >= 5, F32(0.9), F32(0.5)) * np.ones((3, h, 1), F32))
    host = host_run("branches2", seq, rho=0.25)
    st = [T.stats_dict(r, h * w) for r in host[1]]
    assert [s["reset"] for s in st] == [True, False, True, False] and st[2]["n_gate"] == 60 < 64
    for groups in ((4,), (1, 3), (2, 2)):
        assert_equal_bits(device_run(ops, seq, groups, rho=0.25), host, str(groups))
    # a fitted scale of 3 (inside the fit gate, outside [0.5, 2]): identity
    x = np.rint((1.0 + 0.2 * np.arange(h * w, dtype=np.float64).reshape(h, w) / (h * w - 1)) * 256).astype(F32) / F32(256)
    seq = [(F32(3) * x - F32(2), img), (x, img)]
    host = host_run("slope3", seq, anchor=1.0)
    s = T.stats_dict(host[1][1], h * w)
    assert not s["reset"] and not s["fitted"] and s["n"] == h * w and s["scale"] == 1.0
    assert_equal_bits(device_run(ops, seq, (2,), anchor=1.0), host, "slope 3")


def test_grouping_and_repeats_give_identical_bits():
    """five frames stepped as 5 x 1, 2 + 3 and 1 x 5 frames per call, and twice: the same bits; and the specification's"""
    from patchrefinerv2_amd import temporal as T
    seq = sequence(37, 2051, 40, 999, frames=5, seed=3)
    d = torch.from_numpy(np.stack([x for x, _ in seq])).to(DEV)[:, None]
    img = torch.from_numpy(np.stack([i for _, i in seq])).to(DEV)
    runs = []
    for groups in ((1, 1, 1, 1, 1), (2, 3), (5,), (5,)):
        stab, outs, stats, k = T.TemporalStabilizer(), [], [], 0
        for n in groups:
            o, s = stab.step(d[k:k + n], img[k:k + n])
            assert o.is_cuda and o.shape == (n, 1, 37, 2051)
            outs.append(o), stats.extend(s)
            k += n
        runs.append((torch.cat(outs).cpu().numpy().tobytes(), stats, tuple(a.tobytes() for a in stab.state_host())))
    assert all(r == runs[0] for r in runs[1:])
    h_outs, h_rows, (h_y, h_L), _ = host_run("grouping", seq)
    assert runs[0][0] == h_outs.tobytes() and runs[0][1] == [T.stats_dict(r, 37 * 2051) for r in h_rows]
    assert runs[0][2] == (h_y.tobytes(), h_L.tobytes())
    assert [s["reset"] for s in runs[0][1]] == [True, False, False, False, False]
    # a frame of another shape starts a new sequence; reset() forgets it
    stab = T.TemporalStabilizer()
    stab.step(d[:2], img[:2])
    assert stab.step(d[2:3, :, :30, :40].contiguous(), img[2:3])[1][0]["reset"]
    assert not stab.step(d[3:4, :, :30, :40].contiguous(), img[3:4])[1][0]["reset"]
    stab.reset()
    assert stab.step(d[4:5, :, :30, :40].contiguous(), img[4:5])[1][0]["reset"]


def test_sums_at_the_overflow_bound():
    """one 4032 x 6048 frame whose halves sit at q = 2^18 - 1 and q = 2^17, stepped against itself (the state is uploaded): the five
    sums equal their closed forms -- sum qx^2 is 8.4e17, beyond float64's integers and what an int32 or a float sum would hold"""
    from patchrefinerv2_amd import ops, temporal as T
    h, w = 4032, 6048
    x = torch.empty((1, h, w), device=DEV)
    x[:, :h // 2] = (2 ** 18 - 1) / 256.0
    x[:, h // 2:] = 2 ** 17 / 256.0
    img = torch.full((1, 3, 1, 1), 0.5, device=DEV)  # luma 128 everywhere
    state = x[0].clone()
    luma = torch.full((2, h, w), 128, dtype=torch.uint8, device=DEV)
    luma[1] = 0
    out, stats = ops.temporal_step(x, img, state, luma[0], luma[1], True, anchor=1.0)
    s = T.stats_dict(stats.cpu().numpy()[0], h * w)
    half, a, b = h // 2 * w, 2 ** 18 - 1, 2 ** 17
    assert not s["reset"] and s["n"] == s["n_gate"] == h * w
    assert s["sums"] == (half * (a + b), half * (a * a + b * b), half * (a * a + b * b), half * (a + b))
    assert s["sums"][1] > 2 ** 59 and s["change_before_sum"] == 0
    assert bool((luma[1] == 128).all())
    if s["fitted"]:  # the fit of a frame against itself: the identity within float64's rounding of the sums
        assert abs(s["scale"] - 1.0) < 1e-9 and abs(s["shift"]) < 1e-6
    assert torch.allclose(out, x, rtol=1e-6, atol=0) and torch.equal(out[0], state)


def test_arguments_are_checked_before_anything_is_launched():
    from patchrefinerv2_amd import ops
    h, w = 6, 10
    d, img = torch.rand(2, h, w, device=DEV) + 1, torch.rand(2, 3, h, w, device=DEV)
    state, luma = torch.full((h, w), 5.0, device=DEV), torch.full((2, h, w), 9, dtype=torch.uint8, device=DEV)
    bad = [
        (dict(depth=d.cpu()), "GPU"), (dict(depth=d.double()), "float32"), (dict(depth=d[:, :, ::2]), "contiguous"), (dict(depth=d[0]), "n, H, W"),
        (dict(image=img[:1]), "image"), (dict(image=img[:, :2]), "image"), (dict(state_depth=state[:3]), "state_depth"),
        (dict(luma_prev=luma[0].float()), "luma_prev"), (dict(luma_next=luma[0]), "differ"), (dict(luma_next=luma[1, :3]), "luma_next"),
        (dict(alpha=1.0), "alpha"), (dict(tau=256), "tau"), (dict(rho=0.0), "rho"), (dict(anchor=2.0), "anchor"),
    ]
    for dispatch in ("torch", "ctypes"):
        ops.DISPATCH, before = dispatch, ops.DISPATCH
        try:
            for kw, msg in bad:
                args = dict(depth=d, image=img, state_depth=state, luma_prev=luma[0], luma_next=luma[1], state_present=False)
                args.update(kw)
                with pytest.raises(ValueError, match=msg):
                    ops.temporal_step(**args)
        finally:
            ops.DISPATCH = before
    torch.cuda.synchronize()
    assert bool((state == 5.0).all()) and bool((luma == 9).all())  # nothing ran
    # the torch op's own checks, and the library's through it
    t = ops._tops()
    with pytest.raises(RuntimeError, match="luma"):
        t.temporal_step_(d, img, 0.5, 6, 0.05, 0.9, state, luma[0], luma[1, :3], False)
    with pytest.raises(RuntimeError, match="alpha"):
        t.temporal_step_(d, img, 1.5, 6, 0.05, 0.9, state, luma[0], luma[1], False)
    with pytest.raises(RuntimeError, match="tau"):
        t.temporal_step_(d, img, 0.5, 999, 0.05, 0.9, state, luma[0], luma[1], False)
    torch.cuda.synchronize()
    assert bool((state == 5.0).all()) and bool((luma == 9).all())


# ------------------------------------------------------------------------------------------------------------------ Tester
RAW, SPLIT, PPS = (256, 512), (2, 2), (112, 224)  # oracle.cases.E2E_V2: the smallest V2 case the end-to-end GPU tests use


def _write_cfg(tmp_path):
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(RAW)}, patch_split_num={list(SPLIT)},\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")
    return str(cfg)


def _write_video(folder, frames=4):
    """a nearly static clip: one texture, per-frame noise of a grey level or two and a small block that moves"""
    os.makedirs(folder)
    rng = np.random.RandomState(11)
    tex = rng.rand(RAW[0], RAW[1], 3).astype(F32) * F32(0.6) + F32(0.2)
    for k in range(frames):
        im = np.clip(tex + rng.randint(-1, 2, size=(RAW[0], RAW[1], 1)).astype(F32) / F32(255), 0, 1)
        im[100:120, 40 + 30 * k:70 + 30 * k] = 0.95
        np.save(os.path.join(folder, f"frame{k}.npy"), im.astype(F32))


def _files(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def test_tester_run_writes_the_same_files_on_both_routes(tmp_path, monkeypatch):
    """Tester.run --save --temporal-stabilize with the device output stage against the host writer, one and two frames per call: the
    same files; what the stabiliser was handed, replayed through the specification, gives the entries' ``temporal`` and the maps"""
    from patchrefinerv2_amd import models, temporal as T, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import Config, build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    cfg = Config.fromfile(_write_cfg(tmp_path))
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)  # tools/test.py's defaults
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    _write_video(str(tmp_path / "imgs"))
    ds = ImageDataset(str(tmp_path / "imgs"), min_depth=1e-3, max_depth=80, image_resolution=RAW)
    seen = []
    step = T.TemporalStabilizer.step

    def recording(self, depth, image_hr):
        out, stats = step(self, depth, image_hr)
        seen.append((depth.cpu().numpy(), image_hr.cpu().numpy(), out.cpu().numpy(), depth.is_cuda))
        return out, stats
    monkeypatch.setattr(T.TemporalStabilizer, "step", recording)
    flags = dict(temporal_stabilize=True, temporal_anchor=1.0, save_ply=True, save_stereo=True, fov=70.0)

    def run(work, fb, **info):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), output_workers=4, **info), ds, model)
        res = t.run(cai_mode="r4", image_raw_shape=RAW, patch_split_num=SPLIT, seed=621, frame_batch=fb)
        return _files(tmp_path / work), res, dict(getattr(t, "last_eval", None) or {})

    host, res_h, eval_h = run("host", 1, **flags)
    n_host = len(seen)
    dev1, res_1, eval_1 = run("dev1", 1, device_output=True, **flags)
    dev2, res_2, eval_2 = run("dev2", 2, device_output=True, **flags)
    off, res_off, _ = run("off", 2, device_output=True, **{k: v for k, v in flags.items() if not k.startswith("temporal")})
    assert set(host) == set(dev1) == set(dev2) == set(off) and {f"frame{k}{e}" for k in range(4) for e in (".png", "_uint16.png", ".ply", "_right.png")} <= set(host)
    assert dev1 == host and dev2 == host
    slim = lambda res: [(r["name"], r["shape"], r["temporal"]) for r in res]  # noqa: E731  (``mean`` is a host or a device sum)
    assert slim(res_1) == slim(res_h) == slim(res_2) and eval_1 == eval_h == eval_2
    assert [r["name"] for r in res_h] == [f"frame{k}" for k in range(4)] and all("temporal" not in r for r in res_off)
    # the first frame leaves as it came; the later ones are stabilised, so their files differ from the plain run's
    assert {n: v for n, v in off.items() if n.startswith("frame0")} == {n: v for n, v in host.items() if n.startswith("frame0")}
    assert all(off[f"frame{k}_uint16.png"] != host[f"frame{k}_uint16.png"] for k in (1, 2, 3))
    assert all(d for *_, d in seen)  # the model's device maps went in
    assert [s[0].shape[0] for s in seen] == [1] * 4 + [1] * 4 + [2, 2] and n_host == 4
    # replay: the specification on the maps the model returned
    st, k = None, 0
    for depth, image, out, _ in seen[:4]:
        want, st, row = T.temporal_step_host(depth[0, 0], image[0], st, anchor=1.0)
        s = T.stats_dict(row, RAW[0] * RAW[1])
        assert out[0, 0].tobytes() == want.tobytes()
        assert res_h[k]["temporal"] == {key: s[key] for key in Tester.TEMPORAL_KEYS} and s["reset"] == (k == 0)
        assert k == 0 or (not s["reset"] and s["static_fraction"] > 0.5)
        k += 1
    assert set(eval_h) == {"temporal_change_before", "temporal_change_after"} and eval_h["temporal_change_after"] <= eval_h["temporal_change_before"]
    for a, b in zip(seen[:4], [(s[0][f:f + 1], s[1][f:f + 1], s[2][f:f + 1]) for s in seen[8:] for f in range(2)]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b))  # two frames per call: the same maps in, the same out


def test_cli_temporal_stabilize(tmp_path):
    _write_video(str(tmp_path / "imgs"), frames=2)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), _write_cfg(tmp_path), "--synthetic-weights", "--cai-mode", "r4",
                        "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(out),
                        "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", "--device-output", "--frame-batch", "2",
                        "--temporal-stabilize", "--temporal-anchor", "1.0", "--temporal-tau", "8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame0: temporal reset" in r.stdout and "frame1: temporal scale" in r.stdout and "temporal_change_after" in r.stdout, r.stdout
    assert {"frame0_uint16.png", "frame1_uint16.png"} <= set(os.listdir(out))
