"""GPU: B frames per forward call.  Every batched op equals the single-frame op applied per frame (both dispatch routes), and a
B-frame model call equals B sequential calls bit for bit -- depth and coarse prediction -- for every tiling model, cai-mode and
arithmetic, with launch batches that span frames, several streams, a captured hipGraph and the next batch announced."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops as o_ops  # noqa: E402
from oracle.cases import E2E_V1, E2E_V2, e2e_v1_sd, e2e_v2_sd, rand_image  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)


@pytest.fixture(params=["ctypes", "torch"])
def route(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


# tiles of three frames, interleaved in one list
FRAMES_OF = [2, 0, 1, 2, 1, 0, 0, 2]


def test_crop_resize_frames_equals_per_frame(route):
    ops = route
    B, H, W, ch, cw, oh, ow = 3, 96, 128, 48, 64, 30, 42
    img = torch.rand(B, 3, H, W, generator=_g(1)).to(DEV)
    hw = [(0, 0), (48, 64), (17, 33), (48, 0), (0, 64), (31, 7), (5, 60), (40, 50)]
    tiles = torch.tensor([(f, h, w) for f, (h, w) in zip(FRAMES_OF, hw)], dtype=torch.int32, device=DEV)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    out = ops.Feat.alloc(len(hw), oh, ow, 4, DEV)
    ops.crop_resize(img, tiles, ch, cw, oh, ow, mean, std, out)
    for i, (f, (h, w)) in enumerate(zip(FRAMES_OF, hw)):
        one = ops.Feat.alloc(1, oh, ow, 4, DEV)
        ops.crop_resize(img[f].contiguous(), torch.tensor([[h, w]], dtype=torch.int32, device=DEV), ch, cw, oh, ow, mean, std, one)
        assert torch.equal(out.view()[i, ..., :3], one.view()[0, ..., :3]), i


@pytest.mark.parametrize("c,oh", [(32, 24), (32, 8), (3, 12)])  # rows kernel, per-pixel kernel, scalar channels
def test_roi_align_frames_equals_per_frame_and_torchvision(route, c, oh):
    ops = route
    B, h, w = 3, 24, 32
    feat = torch.randn(B, h, w, c, generator=_g(2)).to(DEV)
    x1 = torch.rand(len(FRAMES_OF), generator=_g(3)) * 20
    y1 = torch.rand(len(FRAMES_OF), generator=_g(4)) * 14
    b4 = torch.stack([x1, y1, x1 + 8 + 4 * torch.rand(len(FRAMES_OF), generator=_g(5)), y1 + 6 + 4 * torch.rand(len(FRAMES_OF), generator=_g(6))], 1)
    b5 = torch.cat([torch.tensor(FRAMES_OF, dtype=torch.float32)[:, None], b4], 1)
    scale, ow = 0.75, oh + 4
    got = ops.roi_align(ops.Feat(feat), b5.to(DEV), scale, oh, ow)
    for i, f in enumerate(FRAMES_OF):
        one = ops.roi_align(ops.Feat(feat[f:f + 1].contiguous()), b4[i:i + 1].contiguous().to(DEV), scale, oh, ow)
        assert torch.equal(got.view()[i], one.view()[0]), i
    ref = o_ops.roi_align(feat.permute(0, 3, 1, 2).cpu(), b5, (oh, ow), scale, aligned=True)
    err = float((got.to_nchw().cpu() - ref).abs().max())
    assert err <= 2e-6 * max(1.0, float(ref.abs().max())), err


def test_roi_align_x2_frames_equals_per_frame(route):
    """the pre-split output format (a GatedConvUnit's coarse half) through the B-frame entry point"""
    ops = route
    B, h, w, c, oh, ow = 3, 16, 20, 16, 16, 20
    feat = torch.randn(B, h, w, c, generator=_g(7)).to(DEV)
    x1 = torch.rand(len(FRAMES_OF), generator=_g(8)) * 10
    b4 = torch.stack([x1, x1 * 0.5, x1 + 9, x1 * 0.5 + 7], 1)
    b5 = torch.cat([torch.tensor(FRAMES_OF, dtype=torch.float32)[:, None], b4], 1).to(DEV)
    got = ops.Feat(torch.zeros((len(FRAMES_OF), oh, ow, c), device=DEV), x2=True)
    ops.roi_align(ops.Feat(feat), b5, 1.0, oh, ow, out=got)
    for i, f in enumerate(FRAMES_OF):
        one = ops.Feat(torch.zeros((1, oh, ow, c), device=DEV), x2=True)
        ops.roi_align(ops.Feat(feat[f:f + 1].contiguous()), b4[i:i + 1].contiguous().to(DEV), 1.0, oh, ow, out=one)
        assert torch.equal(got.buf[i], one.buf[0]), i


def test_coarse_taps_frames_equal_per_frame(route):
    """knot tables of B frames in one launch; the gather reads each tile's own frame (boxes of split-4 tiles: bin == knot spacing)"""
    ops = route
    B, h, w, cout, ph, pw, H, W = 3, 12, 16, 8, 48, 64, 96, 128
    g = ops.Feat(torch.randn(B, h, w, 9 * cout, generator=_g(9)).to(DEV))
    kb = (0.25, 0.25)
    taps = ops.CoarseTaps(g, cout, kb)
    singles = [ops.CoarseTaps(ops.Feat(g.buf[f:f + 1].contiguous()), cout, kb) for f in range(B)]
    for f in range(B):
        assert torch.equal(taps.v.view()[f], singles[f].v.view()[0]), f
    hw = [(0, 0), (24, 32), (72, 96), (48, 0), (12, 16), (60, 80), (36, 48), (0, 96)]
    b4 = torch.tensor([[w0 / W * pw, h0 / H * ph, (w0 + 32) / W * pw, (h0 + 24) / H * ph] for h0, w0 in hw], dtype=torch.float32)
    b5 = torch.cat([torch.tensor(FRAMES_OF, dtype=torch.float32)[:, None], b4], 1).to(DEV)
    got = taps.gather(b5, h / ph, h, w)
    for i, f in enumerate(FRAMES_OF):
        one = singles[f].gather(b4[i:i + 1].contiguous().to(DEV), h / ph, h, w)
        assert torch.equal(got.view()[i], one.view()[0]), i


def test_blend_frames_equal_per_frame(route):
    """paste + update + resize of B maps, frame f's tiles a contiguous group of a frame-major list (predictions at a frame stride)"""
    ops = route
    B, n, ph, pw, H, W = 3, 6, 12, 16, 24, 32
    mask = torch.rand(ph, pw, generator=_g(10)).to(DEV)
    mask[:2] = 0
    preds = (torch.rand(B * n, ph, pw, generator=_g(11)) * 10).to(DEV)
    gen = np.random.RandomState(12)
    proc = torch.tensor([[(0, 0), (0, 16), (12, 0), (12, 16)] + [tuple(gen.randint(0, 13, 2)) for _ in range(2)] for _ in range(B)],
                        dtype=torch.int32).to(DEV)  # [B, n, 2]
    avg, cnt = torch.zeros(B, H, W, device=DEV), torch.zeros(B, H, W, device=DEV)
    pv = preds.view(B, n, ph, pw)
    ops.blend_paste_frames(avg, cnt, pv[:, :4], mask, proc[:, :4], ph, pw)
    ops.blend_update_frames(avg, cnt, pv[:, 4:], mask, proc[:, 4:], ph, pw)
    a2, c2 = ops.blend_resize(avg, cnt, 36, 48)
    for f in range(B):
        sa, sc = torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)
        ops.blend_paste(sa, sc, preds[f * n:f * n + 4], mask, proc[f, :4].contiguous(), ph, pw)
        ops.blend_update(sa, sc, preds[f * n + 4:f * n + n], mask, proc[f, 4:].contiguous(), ph, pw)
        assert torch.equal(avg[f], sa) and torch.equal(cnt[f], sc), f
        ra, rc = ops.blend_resize(sa, sc, 36, 48)
        assert torch.equal(a2[f], ra) and torch.equal(c2[f], rc), f


# ------------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------------
def _build(kind, c, sd, **extra):
    from patchrefinerv2_amd import models  # noqa: F401
    from patchrefinerv2_amd.registry import build_model
    cfg = dict(c["ref_config"])
    cfg["coarse_branch"] = dict(type="DA2", pretrained=None, model_cfg={**c["da2_cfg"]})
    if kind == "PatchRefiner":
        cfg["refiner"] = dict(cfg["refiner"])
        cfg["refiner"]["fine_branch"] = dict(type="DA2", pretrained=None, model_cfg={**c["da2_cfg"]})
    cfg.update(extra)
    m = build_model(dict(type=kind, config=cfg))
    m.load_state_dict(sd, strict=True)
    return m


def _frames(m, c, seeds):
    hr = torch.cat([rand_image(s, 1, *c["raw"]) for s in seeds]).to(DEV)
    return hr, m.resizer(hr)


def _check(m, c, mode, hr, lr, frame_seeds=None, base_seed=621, **kw):
    """one B-frame call against B sequential calls (``random`` seeded once, or per frame with ``frame_seeds``)"""
    tc = dict(image_raw_shape=c["raw"], patch_split_num=c["split"])
    B = hr.shape[0]
    random.seed(base_seed)
    seq = []
    for f in range(B):
        if frame_seeds is not None:
            random.seed(frame_seeds[f])
        d, log = m(mode="infer", cai_mode=mode, process_num=4, tile_cfg=tc, image_lr=lr[f:f + 1], image_hr=hr[f:f + 1])
        seq.append((d, log["coarse_prediction"].clone() if log.get("coarse_prediction") is not None else None))
    after_seq = random.random()
    random.seed(base_seed)
    d, log = m(mode="infer", cai_mode=mode, process_num=4, tile_cfg=tc, image_lr=lr, image_hr=hr, frame_seeds=frame_seeds, **kw)
    assert random.random() == after_seq  # ``random`` consumed exactly as by the B sequential calls
    assert tuple(d.shape) == (B,) + tuple(seq[0][0].shape[1:])
    assert torch.equal(d.cpu(), torch.cat([s[0].cpu() for s in seq])), mode
    if seq[0][1] is not None:
        cp = log["coarse_prediction"]
        assert tuple(cp.shape) == (B,) + tuple(seq[0][1].shape[1:])
        assert torch.equal(cp, torch.cat([s[1] for s in seq])), mode
    return d


@pytest.mark.parametrize("prec", ["bf16x3", "f32", "f16f6"])
def test_v2_frames_equal_sequential(prec):
    """V2 (bf16x3: the per-frame coarse-tap tables; f32: the plain ROI path; f16f6: the fp16 + fp6 layers and their range guard) over
    m1 / m2 / r8, launch batches below and above one frame's tile count, 3 streams"""
    from patchrefinerv2_amd import ops
    c = E2E_V2
    modes = ["m1", "m2", "r8"] if prec == "bf16x3" else ["r8"] if prec == "f32" else ["m2", "r8"]
    for mb in ((3, 64) if prec == "bf16x3" else (5,)):
        m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec=prec, max_batch=mb, n_streams=3)
        hr, lr = _frames(m, c, (0, 3, 5))
        for mode in modes:
            _check(m, c, mode, hr, lr)
        _check(m, c, "r8", hr, lr, frame_seeds=[11, 621, 11])
        if prec == "f16f6":
            assert ops.F6Range.active(DEV) and getattr(m, "f6_guarded_frames", 0) > 0 and getattr(m, "f6_recalibrations", 0) == 0


def test_v2_frames_without_coarse_taps_equal_sequential(monkeypatch):
    """the plain ROI path of the bf16 modes (tap tables switched off)"""
    from patchrefinerv2_amd import ops
    monkeypatch.setattr(ops, "COARSE_TAPS", False)
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="bf16x3", max_batch=3, n_streams=3)
    hr, lr = _frames(m, c, (1, 2, 4))
    _check(m, c, "m2", hr, lr)


def test_v1_frames_equal_sequential():
    c = E2E_V1
    for mb in (3, 64):
        m = _build("PatchRefiner", c, e2e_v1_sd(), prec="bf16x3", max_batch=mb, n_streams=3)
        hr, lr = _frames(m, c, (0, 1, 2))
        for mode in ("m1", "m2", "r8"):
            _check(m, c, mode, hr, lr)
    m = _build("PatchRefiner", c, e2e_v1_sd(), prec="f32", max_batch=5, n_streams=3)
    hr, lr = _frames(m, c, (0, 1, 2))
    _check(m, c, "r8", hr, lr)


def test_frames_with_hip_graph_and_next_batch_announced():
    c = E2E_V2
    sd = e2e_v2_sd()
    g = _build("PatchRefinerPlus", c, sd, prec="bf16x3", max_batch=3, n_streams=3, hip_graph=True)
    hr, lr = _frames(g, c, (0, 3, 5))
    for it in range(3):  # eager first call, captured second, replayed third (other random tiles)
        _check(g, c, "r8", hr, lr, base_seed=621 + it)
    assert any(isinstance(v, dict) for v in g._graphs.values())
    # next_image_lr: the next batch's coarse forward beside this batch's tiles
    m = _build("PatchRefinerPlus", c, sd, prec="bf16x3", max_batch=3, n_streams=2)
    hr2, lr2 = _frames(m, c, (7, 8, 9))
    tc = dict(image_raw_shape=c["raw"], patch_split_num=c["split"])
    refs = []
    for h_, l_ in ((hr, lr), (hr2, lr2)):
        random.seed(5)
        d, log = m(mode="infer", cai_mode="r8", process_num=4, tile_cfg=tc, image_lr=l_, image_hr=h_)
        refs.append((d, log["coarse_prediction"].clone()))
    random.seed(5)
    d1, log1 = m(mode="infer", cai_mode="r8", process_num=4, tile_cfg=tc, image_lr=lr, image_hr=hr, next_image_lr=lr2)
    c1 = log1["coarse_prediction"].clone()
    assert "_coarse_prefetched" in m.__dict__
    random.seed(5)
    d2, log2 = m(mode="infer", cai_mode="r8", process_num=4, tile_cfg=tc, image_lr=lr2, image_hr=hr2)
    assert "_coarse_prefetched" not in m.__dict__  # consumed
    assert torch.equal(d1, refs[0][0]) and torch.equal(c1, refs[0][1])
    assert torch.equal(d2, refs[1][0]) and torch.equal(log2["coarse_prediction"], refs[1][1])
    _check(m, c, "r8", hr2, lr2, base_seed=5)


def test_baseline_pretrain_frames_equal_sequential():
    from oracle.cases import BASELINE, baseline_kwargs, baseline_sd
    from patchrefinerv2_amd import models  # noqa: F401
    from patchrefinerv2_amd.registry import build_model
    c = BASELINE
    for target, modes in (("fine", ("m2", "r2")), ("coarse", ("m1",))):
        m = build_model(dict(type="BaselinePretrain", **baseline_kwargs(target), max_batch=3, n_streams=3))
        m.load_dict(baseline_sd())
        hr, lr = _frames(m, c, (0, 1, 2))
        for mode in modes:
            _check(m, c, mode, hr, lr)


def test_semi_delegates_frames():
    from patchrefinerv2_amd import models
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="bf16x3", max_batch=4)
    semi = object.__new__(models.PatchRefinerSemi)
    semi.__dict__["student_model"] = m
    hr, lr = _frames(m, c, (0, 3))
    _check(semi, c, "r8", hr, lr, frame_seeds=[1, 2])


def test_rejected_frame_inputs():
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="bf16x3")
    hr, lr = _frames(m, c, (0, 1))
    tc = dict(image_raw_shape=c["raw"], patch_split_num=c["split"])
    with pytest.raises(ValueError, match="patch-sharded"):
        m(mode="infer", cai_mode="m1", tile_cfg=tc, image_lr=lr, image_hr=hr, shard=(0, 2))
    with pytest.raises(ValueError, match="frames"):
        m(mode="infer", cai_mode="m1", tile_cfg=tc, image_lr=lr[:1], image_hr=hr)
    with pytest.raises(ValueError, match="frame_seeds"):
        m(mode="infer", cai_mode="m1", tile_cfg=tc, image_lr=lr, image_hr=hr, frame_seeds=[1, 2, 3])


# ------------------------------------------------------------------------------------------------------------------------------
# full size (synthetic weights)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,prec", [("v1_dav2s_1080p_m1", 4, "bf16x3"), ("v2_zoe_4k_r32", 2, "f16f6")])
def test_full_size_workload_frames_equal_sequential(name, B, prec):
    from patchrefinerv2_amd import ops, weights as W
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    w = WORKLOADS[name]
    m = build_model(model_config(name, prec=prec, max_batch=int(w.get("max_batch", 41)), n_streams=3))
    m.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    hr = torch.cat([torch.rand(1, 3, *w["raw"], generator=_g(100 + f)) for f in range(B)]).to(DEV)
    lr = m.resizer(hr)
    tc = dict(image_raw_shape=w["raw"], patch_split_num=w["split"])
    seeds = [621 + f for f in range(B)]
    seq = []
    for f in range(B):
        random.seed(seeds[f])
        d, log = m(mode="infer", cai_mode=w["mode"], process_num=4, tile_cfg=tc, image_lr=lr[f:f + 1], image_hr=hr[f:f + 1], return_device=True)
        seq.append((d.clone(), log["coarse_prediction"].clone()))
    d, log = m(mode="infer", cai_mode=w["mode"], process_num=4, tile_cfg=tc, image_lr=lr, image_hr=hr, frame_seeds=seeds, return_device=True)
    assert torch.equal(d, torch.cat([s[0] for s in seq])) and torch.equal(log["coarse_prediction"], torch.cat([s[1] for s in seq]))
    if prec == "f16f6":
        assert getattr(m, "f6_recalibrations", 0) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------------------------------------
def test_cli_frame_batch_writes_identical_pngs(tmp_path):
    (tmp_path / "imgs").mkdir()
    for i in range(3):
        np.save(str(tmp_path / "imgs" / f"frame{i}.npy"), np.random.RandomState(10 + i).rand(90, 160, 3).astype(np.float32))
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   "model = dict(config=dict(patch_process_shape=[112, 224], image_raw_shape=[256, 512], patch_split_num=[2, 2],\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")
    outs = {}
    for fb in (1, 2):
        out = tmp_path / f"out{fb}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), str(cfg), "--synthetic-weights", "--cai-mode", "r4",
                            "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(out),
                            "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", "--frame-batch", str(fb)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ": depth " in ln]
        assert [ln.split(":")[0].split()[-1] for ln in lines] == ["frame0", "frame1", "frame2"], r.stdout
        outs[fb] = (out, lines)
    names = sorted(os.listdir(outs[1][0]))
    assert len(names) == 12 and names == sorted(os.listdir(outs[2][0]))
    for n in names:
        assert (outs[1][0] / n).read_bytes() == (outs[2][0] / n).read_bytes(), n
    assert outs[1][1] == outs[2][1]
