"""GPU: the motion stage of the temporal stabiliser (csrc/motion.hip through ops.temporal_motion_step and
temporal.TemporalStabilizer(motion=True)).  The oracle is the numpy specification (temporal.temporal_step_host(motion_range=R),
temporal_motion_host): the output maps, the state (its map and both luma buffers), every word of both stats blocks and the blocks'
vectors are compared for EQUALITY, on both dispatch routes.  A block is 16 x 16 pixels; the coarse search's workgroup owns 2 x 2 blocks,
the refinement's four consecutive blocks; rows of w % 4 == 0 on aligned buffers take the 16-byte accesses, the others the scalar path."""
import ctypes
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
NAN, INF = float("nan"), float("inf")
torch.set_grad_enabled(False)

# (h, w), image (ih, iw) or None for the map's size: one pixel; one partial block; exactly one block; a one-row, one-column remainder;
# a resampled luma with w % 4 != 0 (the element-wise path); the vector path; several workgroup tiles in x; tall and thin
SHAPES = [((1, 1), None), ((7, 9), None), ((16, 16), None), ((17, 33), None), ((53, 37), (31, 45)), ((64, 128), None), ((100, 260), None),
          ((144, 16), None)]
CONTENTS = [("translate", 1), ("translate", 8), ("translate", 16), ("split", 8), ("random", 8)]


@pytest.fixture(params=["torch", "ctypes"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def texture(rng, h, w):
    """uint8 noise smoothed by a 3 x 3 box"""
    a = rng.integers(0, 256, size=(h + 2, w + 2)).astype(np.int32)
    return (sum(a[i:i + h, j:j + w] for i in range(3) for j in range(3)) // 9).astype(np.uint8)


def grey(tex):
    """the fp32 [3, h, w] image whose luma is ``tex``"""
    return np.repeat((tex.astype(F32) / F32(255))[None], 3, axis=0)


def sequence(h, w, ih, iw, content, R, frames=3, seed=0):
    """[(x fp32 [h, w], image fp32 [3, ih, iw])]: a jittering estimator over a scene that moves as ``content`` says; the later frames
    carry every kind of invalid depth, which the state then carries too"""
    rng = np.random.default_rng(seed + 31 * h + w + 7 * R)
    reach = 4 * R + 1
    big = texture(rng, ih + 2 * frames * reach, iw + 2 * frames * reach)
    c0 = frames * reach
    n = h * w
    base = 1.5 + 4.0 * (np.arange(n, dtype=np.float64).reshape(h, w) / max(n - 1, 1)) + 0.3 * np.sin(np.arange(w) / 7.0)[None, :]
    seq = []
    for t in range(frames):
        sgn = 1 if t % 2 == 0 else -1  # (4R, -(4R + 1)) then (-4R, 4R + 1) between consecutive frames
        oy, ox = (c0 + 4 * R, c0 - reach) if sgn > 0 else (c0, c0)
        if content == "translate":
            tex = big[oy:oy + ih, ox:ox + iw]
        elif content == "split":  # left of a column inside a block: (3 t, -5 t); right of it: (-6 t, 2 t)
            tex = big[c0 + 3 * t:c0 + 3 * t + ih, c0 - 5 * t:c0 - 5 * t + iw].copy()
            cut = min(iw - 1, 16 * (iw // 32) + 7)
            tex[:, cut:] = big[c0 - 6 * t:c0 - 6 * t + ih, c0 + 2 * t + cut:c0 + 2 * t + iw]
        else:
            tex = rng.integers(0, 256, size=(ih, iw)).astype(np.uint8)
        s, b = 1.0 + rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03)
        x = (s * base + b + rng.normal(0.0, 0.002, size=base.shape)).astype(F32)
        if t and n > 80:
            flat = x.reshape(-1)
            for i, v in enumerate((NAN, INF, -INF, 0.0, -1.5, 1024.0, 5000.0, 3.0e38, 1e-4)):
                flat[(7 + 13 * i + 101 * t) % n] = v
        seq.append((x, grey(tex)))
    return seq


_HOST = {}


def host_run(key, seq, R, **kw):
    """the specification over a sequence, once per case -> (outs, rows [n, 12], motion rows [n, 8], vectors [n, nby, nbx, 2], state
    (y, L), previous luma)"""
    from patchrefinerv2_amd import temporal as T
    k = (key, R, tuple(sorted(kw.items())))
    if k not in _HOST:
        st, outs, rows, mrows, vecs, lumas = None, [], [], [], [], []
        for x, img in seq:
            h, w = x.shape
            L = T.luma_host(img, h, w)
            vecs.append(np.zeros(T.motion_blocks(h, w) + (2,), np.int16) if st is None else T.temporal_motion_host(L, st[1], R)[0])
            out, st, row, mrow = T.temporal_step_host(x, img, st, motion_range=R, **kw)
            outs.append(out), rows.append(row), mrows.append(mrow), lumas.append(st[1])
        _HOST[k] = (np.stack(outs), np.stack(rows), np.stack(mrows), np.stack(vecs), st, lumas[-2] if len(lumas) > 1 else None)
    return _HOST[k]


def device_run(ops, seq, groups, R, offset=0, **kw):
    """the same through ops.temporal_motion_step, the sequence cut into calls of ``groups`` frames; ``offset``: every buffer starts that
    many elements into its allocation (unaligned base pointers)"""
    h, w = seq[0][0].shape

    def dev(a, fill=None):  # a tensor of a's shape and dtype, ``offset`` elements into a larger one
        a = torch.as_tensor(a)
        big = torch.empty(a.numel() + offset, dtype=a.dtype, device=DEV)
        t = big[offset:].view(a.shape)
        t.copy_(a) if fill is None else t.fill_(fill)
        return t
    d, img = dev(np.stack([x for x, _ in seq])), dev(np.stack([i for _, i in seq]))
    state = dev(torch.empty((h, w)), NAN)
    luma = [dev(torch.empty((h, w), dtype=torch.uint8), 77), dev(torch.empty((h, w), dtype=torch.uint8), 77)]
    cur, present, k, outs, rows, mrows, vecs = 0, False, 0, [], [], [], []
    for n in groups:
        out, stats, mstats, vec = ops.temporal_motion_step(d[k:k + n], img[k:k + n], state, luma[cur], luma[1 - cur], present, motion_range=R, **kw)
        assert out.shape == (n, h, w) and stats.shape == (n, 12) and mstats.shape == (n, 8) and mstats.dtype == torch.int64 and mstats.is_cuda
        assert vec.shape == (n, -(-h // 16), -(-w // 16), 2) and vec.dtype == torch.int16
        outs.append(out), rows.append(stats), mrows.append(mstats), vecs.append(vec)
        cur, present, k = cur ^ (n & 1), True, k + n
    torch.cuda.synchronize()
    cat = lambda ts: torch.cat(ts).cpu().numpy()  # noqa: E731
    return cat(outs), cat(rows), cat(mrows), cat(vecs), state.cpu().numpy(), luma[cur].cpu().numpy(), luma[1 - cur].cpu().numpy()


def assert_equal_bits(dev, host, what=""):
    outs, rows, mrows, vecs, state, L, Lprev = dev
    h_outs, h_rows, h_mrows, h_vecs, (h_y, h_L), h_Lprev = host
    assert np.array_equal(vecs, h_vecs), f"{what}: vectors differ at {np.argwhere(vecs != h_vecs)[:4]}\n{vecs[vecs != h_vecs][:8]}\n{h_vecs[vecs != h_vecs][:8]}"
    assert np.array_equal(mrows, h_mrows), f"{what}: motion stats\n{mrows}\n{h_mrows}"
    assert outs.tobytes() == h_outs.tobytes(), f"{what}: out differs at {np.argwhere(outs.view(np.uint32) != h_outs.view(np.uint32))[:4]}"
    assert np.array_equal(rows, h_rows), f"{what}: stats\n{rows}\n{h_rows}"
    assert state.tobytes() == h_y.tobytes(), f"{what}: state map"
    assert np.array_equal(L, h_L), f"{what}: luma"
    if h_Lprev is not None:
        assert np.array_equal(Lprev, h_Lprev), f"{what}: the previous luma (the other buffer of the pair)"


@pytest.mark.parametrize("content,R", CONTENTS)
@pytest.mark.parametrize("shape,ishape", SHAPES)
def test_bits_equal_the_specification(ops, shape, ishape, content, R):
    (h, w), (ih, iw) = shape, ishape or shape
    seq = sequence(h, w, ih, iw, content, R)
    host = host_run((shape, ishape, content), seq, R)
    assert (host[2][0] == 0).all() and host[2][1, 0] == host[3].shape[1] * host[3].shape[2]  # no stage without a state; every block after
    if content != "translate" and h * w >= 4096:  # the case does what it is there for: blocks move, the state carries invalid depths
        assert host[2][1:, 1].min() > 0 and not np.isfinite(host[0][1:]).all()
    assert_equal_bits(device_run(ops, seq, (1, 1, 1), R), host, "one frame per call")
    assert_equal_bits(device_run(ops, seq, (3,), R), host, "one call")


def test_translation_is_found_on_the_device(ops):
    """the translated texture at the reach of R = 8: the interior blocks report exactly the shift, as the specification does"""
    seq = sequence(160, 176, 160, 176, "translate", 8, frames=2)
    host = host_run("reach", seq, 8)
    assert (host[3][1, 4:6, 4:7] == (-32, 33)).all()
    assert_equal_bits(device_run(ops, seq, (2,), 8), host, "reach")


def test_zero_motion_equals_the_plain_step(ops):
    """a static camera: every vector is zero, and the frame's bits and stats equal ops.temporal_step's"""
    rng = np.random.default_rng(5)
    tex = texture(rng, 48, 80)
    seq = []
    for t in range(3):
        x = ((1.0 + 0.03 * (t - 1)) * (2.0 + np.arange(48 * 80, dtype=np.float64).reshape(48, 80) / 4000.0)).astype(F32)
        seq.append((x, grey(np.clip(tex.astype(np.int32) + rng.integers(-1, 2, size=tex.shape), 0, 255).astype(np.uint8))))
    outs, rows, mrows, vecs, state, L, Lp = device_run(ops, seq, (3,), 8)
    assert not vecs.any() and (mrows[1:, 0] == 15).all() and not mrows[:, 1:6].any() and (mrows[1:, 6] == mrows[1:, 7]).all()
    d = torch.from_numpy(np.stack([x for x, _ in seq])).to(DEV)
    img = torch.from_numpy(np.stack([i for _, i in seq])).to(DEV)
    st, lu = torch.full((48, 80), NAN, device=DEV), torch.full((2, 48, 80), 77, dtype=torch.uint8, device=DEV)
    p_out, p_rows = ops.temporal_step(d, img, st, lu[0], lu[1], False)
    assert p_out.cpu().numpy().tobytes() == outs.tobytes() and np.array_equal(p_rows.cpu().numpy(), rows)
    assert st.cpu().numpy().tobytes() == state.tobytes() and np.array_equal(lu[1].cpu().numpy(), L) and not p_rows[1:, 0].any().item()


def test_grouping_and_repeats_give_identical_bits():
    """five panning frames stepped as 5 x 1, 2 + 3 and 1 x 5 frames per call, and twice: the same bits, and the specification's"""
    from patchrefinerv2_amd import temporal as T
    h, w = 80, 112
    rng = np.random.default_rng(9)
    big = texture(rng, h + 80, w + 80)
    seq = []
    for t in range(5):
        x = ((1.0 + 0.04 * (-1) ** t) * (2.0 + np.arange(h * w, dtype=np.float64).reshape(h, w) / 5000.0)).astype(F32)
        seq.append((x, grey(big[40 + 3 * t:40 + 3 * t + h, 40 - 7 * t:40 - 7 * t + w])))
    d = torch.from_numpy(np.stack([x for x, _ in seq])).to(DEV)[:, None]
    img = torch.from_numpy(np.stack([i for _, i in seq])).to(DEV)
    runs = []
    for groups in ((1, 1, 1, 1, 1), (2, 3), (5,), (5,)):
        stab, outs, stats, k = T.TemporalStabilizer(motion=True), [], [], 0
        for n in groups:
            o, s = stab.step(d[k:k + n], img[k:k + n])
            assert o.is_cuda and o.shape == (n, 1, h, w)
            outs.append(o), stats.extend(s)
            k += n
        runs.append((torch.cat(outs).cpu().numpy().tobytes(), stats, tuple(a.tobytes() for a in stab.state_host())))
    assert all(r == runs[0] for r in runs[1:])
    h_outs, h_rows, h_mrows, _, (h_y, h_L), _ = host_run("grouping", seq, 8)
    assert runs[0][0] == h_outs.tobytes() and runs[0][1] == [T.stats_dict(r, h * w, m) for r, m in zip(h_rows, h_mrows)]
    assert runs[0][2] == (h_y.tobytes(), h_L.tobytes())
    st = runs[0][1]
    assert st[0]["motion"]["blocks"] == 0 and all(s["motion"]["moving_fraction"] > 0.5 and s["static_fraction"] > 0.6 for s in st[1:])
    assert T.TemporalStabilizer().step(d[:1], img[:1])[1][0]["motion"] is None


def test_unaligned_base_pointers(ops):
    """every map and luma buffer one element into its allocation: w % 4 == 0, yet the element-wise path"""
    seq = sequence(64, 128, 64, 128, "split", 8)
    assert_equal_bits(device_run(ops, seq, (2, 1), 8, offset=1), host_run(((64, 128), None, "split"), seq, 8), "offset 1")


def test_parameters_reach_the_step(ops):
    seq = sequence(53, 37, 31, 45, "split", 4)
    kw = dict(alpha=0.9, tau=20, rho=0.5, anchor=1.0)
    assert_equal_bits(device_run(ops, seq, (3,), 4, **kw), host_run("params", seq, 4, **kw), str(kw))


def test_arguments_are_checked_before_anything_is_launched():
    from patchrefinerv2_amd import lib, ops
    h, w, n = 20, 36, 2
    d, img = torch.rand(n, h, w, device=DEV) + 1, torch.rand(n, 3, h, w, device=DEV)
    state, luma = torch.full((h, w), 5.0, device=DEV), torch.full((2, h, w), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((n, h, w), -3.0, device=DEV)
    stats, mstats = torch.full((n, 12), -1, dtype=torch.int64, device=DEV), torch.full((n, 8), -1, dtype=torch.int64, device=DEV)
    vec = torch.full((n, 2, 3, 2), -1, dtype=torch.int16, device=DEV)
    L = lib.load()
    wsb = L.prv2_temporal_motion_workspace_bytes(h, w)
    assert wsb > L.prv2_temporal_workspace_bytes(h, w) + 5 * h * w
    assert L.prv2_temporal_motion_workspace_bytes(0, 4) == -1 and L.prv2_temporal_motion_workspace_bytes(8192, 4097) == -1
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    good = dict(depth=d.data_ptr(), image=img.data_ptr(), n=n, h=h, w=w, ih=h, iw=w, alpha=0.5, tau=6, rho=0.05, anchor=0.9, R=8,
                state=state.data_ptr(), l0=luma[0].data_ptr(), l1=luma[1].data_ptr(), present=1, out=out.data_ptr(), stats=stats.data_ptr(),
                mstats=mstats.data_ptr(), vec=vec.data_ptr(), ws=ws.data_ptr(), wsb=wsb, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [dict(R=0), dict(R=17), dict(R=-1), dict(wsb=wsb - 1), dict(depth=0), dict(mstats=0), dict(ws=0), dict(l1=luma[0].data_ptr()),
           dict(out=d.data_ptr()), dict(n=0), dict(h=8192, w=4097), dict(tau=256), dict(present=2)]
    for kw in bad:
        assert L.prv2_temporal_motion_step(*{**good, **kw}.values()) != 0, kw
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((state == 5.0).all()) and bool((luma == 9).all()) and bool((mstats == -1).all()) and bool((vec == -1).all())
    # the wrappers' own checks, on both routes, and the torch op's
    args = dict(depth=d, image=img, state_depth=state, luma_prev=luma[0], luma_next=luma[1], state_present=True)
    for dispatch in ("torch", "ctypes"):
        ops.DISPATCH, before = dispatch, ops.DISPATCH
        try:
            for kw, msg in [(dict(motion_range=0), "motion_range"), (dict(motion_range=17), "motion_range"), (dict(motion_range=2.5), "motion_range"),
                            (dict(luma_next=luma[0]), "differ"), (dict(depth=d.cpu()), "GPU"), (dict(tau=256), "tau")]:
                with pytest.raises(ValueError, match=msg):
                    ops.temporal_motion_step(**{**args, **kw})
        finally:
            ops.DISPATCH = before
    with pytest.raises(RuntimeError, match="motion_range"):
        ops._tops().temporal_motion_step_(d, img, 0.5, 6, 0.05, 0.9, 99, state, luma[0], luma[1], True)
    torch.cuda.synchronize()
    assert bool((state == 5.0).all()) and bool((luma == 9).all())
    # and the good call runs
    assert L.prv2_temporal_motion_step(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((mstats[:, 0] == 6).all()) and bool((out > 0).all())


# ------------------------------------------------------------------------------------------------------------------ Tester
RAW, SPLIT, PPS = (256, 512), (2, 2), (112, 224)  # oracle.cases.E2E_V2: the smallest V2 case the end-to-end GPU tests use
PAN = (3, -7)  # pixels per frame


def _write_cfg(tmp_path):
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(RAW)}, patch_split_num={list(SPLIT)},\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")
    return str(cfg)


def _write_video(folder, frames=3):
    """a panning clip: one large smoothed texture seen through a window that moves by PAN per frame"""
    os.makedirs(folder)
    big = texture(np.random.default_rng(11), RAW[0] + 64, RAW[1] + 64)
    for k in range(frames):
        y, x = 32 + PAN[0] * k, 32 + PAN[1] * k
        np.save(os.path.join(folder, f"frame{k}.npy"), np.repeat(big[y:y + RAW[0], x:x + RAW[1], None].astype(F32) / F32(255), 3, axis=2))


def _files(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


def test_tester_run_writes_the_same_files_on_both_routes(tmp_path, monkeypatch):
    """Tester.run --save --temporal-stabilize --temporal-motion with the device output stage against the host writer, one and three
    frames per call: the same files and entries; what the stabiliser was handed, replayed through its host route (the specification),
    gives the same maps and the same ``temporal`` entries; the pan is found and most of the frame is static again"""
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
        seen.append((depth.cpu(), image_hr.cpu(), out.cpu().numpy(), depth.is_cuda))
        return out, stats
    monkeypatch.setattr(T.TemporalStabilizer, "step", recording)
    flags = dict(temporal_stabilize=True, temporal_motion=True, temporal_motion_range=4)

    def run(work, fb, **info):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), output_workers=4, **info), ds, model)
        res = t.run(cai_mode="r4", image_raw_shape=RAW, patch_split_num=SPLIT, seed=621, frame_batch=fb)
        return _files(tmp_path / work), res, dict(getattr(t, "last_eval", None) or {})

    host, res_h, eval_h = run("host", 1, **flags)
    dev1, res_1, eval_1 = run("dev1", 1, device_output=True, **flags)
    dev3, res_3, eval_3 = run("dev3", 3, device_output=True, **flags)
    plain, res_p, eval_p = run("plain", 3, device_output=True, temporal_stabilize=True)
    assert {f"frame{k}{e}" for k in range(3) for e in (".png", "_uint16.png")} <= set(host)
    assert dev1 == host and dev3 == host
    slim = lambda res: [(r["name"], r["shape"], r["temporal"]) for r in res]  # noqa: E731
    assert slim(res_1) == slim(res_h) == slim(res_3) and eval_1 == eval_h == eval_3
    assert set(eval_h) == {"temporal_change_before", "temporal_change_after", "temporal_moving_fraction"} and eval_h["temporal_moving_fraction"] > 0.8
    assert all(d for *_, d in seen) and [s[0].shape[0] for s in seen] == [1] * 6 + [3, 3]
    # the pan is found; with it most of the frame is static, without it little is
    assert "motion" not in res_p[1]["temporal"] and res_h[0]["temporal"]["motion"]["blocks"] == 0
    for k in (1, 2):
        m = res_h[k]["temporal"]["motion"]
        assert m["blocks"] == 16 * 32 and abs(m["mean_dy"] - PAN[0]) < 0.3 and abs(m["mean_dx"] - PAN[1]) < 0.7 and m["sad"] < m["sad_zero"] / 4
        assert res_h[k]["temporal"]["static_fraction"] > 0.8 > 0.3 > res_p[k]["temporal"]["static_fraction"]
    assert all(plain[f"frame{k}_uint16.png"] != host[f"frame{k}_uint16.png"] for k in (1, 2))
    # replay: the stabiliser's host route on the maps the model returned
    stab, k = T.TemporalStabilizer(motion=True, motion_range=4), 0
    for depth, image, out, _ in seen[:3]:
        want, stats = step(stab, depth, image)
        assert want.numpy().tobytes() == out.tobytes() and res_h[k]["temporal"] == Tester._temporal_entry(stats[0])
        k += 1
    with pytest.raises(ValueError, match="temporal_motion without temporal_stabilize"):
        Tester(None, RunnerInfo(temporal_motion=True), ds, model).run(cai_mode="r4", image_raw_shape=RAW, patch_split_num=SPLIT)


def test_cli_temporal_motion(tmp_path):
    _write_video(str(tmp_path / "imgs"), frames=2)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "test.py"), _write_cfg(tmp_path), "--synthetic-weights", "--cai-mode", "r4",
           "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(out),
           "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", "--device-output", "--frame-batch", "2"]
    r = subprocess.run(cmd + ["--temporal-stabilize", "--temporal-motion", "--temporal-motion-range", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame1: temporal scale" in r.stdout and "frame1: motion (dy, dx) mean (" in r.stdout and "temporal_moving_fraction" in r.stdout, r.stdout
    assert "frame0: motion" not in r.stdout and {"frame0_uint16.png", "frame1_uint16.png"} <= set(os.listdir(out))
    r = subprocess.run(cmd + ["--temporal-motion"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "ValueError: temporal_motion without temporal_stabilize" in r.stderr, r.stderr[-2000:]
