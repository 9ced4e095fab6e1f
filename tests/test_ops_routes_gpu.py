"""The two routes of the host mirror (ops.DISPATCH: torch.ops.prv2.* / ctypes on the C ABI) are one wrapper each: every wrapper that reports to
ops.PROFILER must leave the SAME records -- kernel tag with shape string, executed FLOPs (or bytes, in the tag), reference-graph FLOPs -- and
the same output bits on both.  bench.py's roofline is computed from those records.  Shapes: the smallest case of each op in
tests/test_hip_ops.py / tests/test_frame_batch_gpu.py / tests/test_upconv5.py (host code is under test, not the kernels)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def feat(P, seed, n, c, h, w):
    return P.Feat.from_nchw(rnd(seed, n, c, h, w).to(DEV))


def conv_w(P, seed, cout, cin, k, prec, bias=True, **kw):
    return P.pack_conv((rnd(seed, cout, cin, k, k) / np.sqrt(cin * k * k)).to(DEV), rnd(seed + 1, cout).to(DEV) if bias else None, prec=prec, **kw)


# ---- one function per case: builds its inputs from seeds, calls the wrappers, returns their outputs ------------------------------------
def conv2d(P):
    return [P.conv2d(feat(P, 1, 1, 34, 17, 23), conv_w(P, 2, 32, 34, 3, P.PREC_F32, bias=False))]


def conv2d_f32_strip(P):
    """3x3 stride 1, w = 72 = 2 * 32 + 8 in f32 mode: with the profiler on, tiles and remainder strip are two launches and two records"""
    return [P.conv2d(feat(P, 1, 1, 34, 4, 72), conv_w(P, 2, 40, 34, 3, P.PREC_F32), act=P.ACT_GELU)]


def conv2d_ups(P):
    n, (h, w), (H, W), c1, cin, cout = 1, (6, 9), (29, 70), 32, 66, 130
    u = feat(P, 1, n, c1, h, w)
    x = P.Feat.alloc(n, H, W, cin, DEV)
    x.buf[..., c1:cin] = rnd(2, n, H, W, cin - c1).to(DEV)
    cw = conv_w(P, 3, cout, cin, 3, P.L.PREC_BF16X3, pad=1)
    assert P.conv2d_ups_supported(x, u, cw)
    return [P.conv2d_ups(x, u, cw, act=P.ACT_GELU, res=feat(P, 5, n, cout, H, W))]


def upconv3x3(P):
    u, cw = feat(P, 1, 1, 32, 6, 8), conv_w(P, 2, 64, 32, 3, P.L.PREC_BF16X3, pad=1)
    assert P.upconv3x3_supported(u, 24, 32, cw)
    return [P.upconv3x3(u, 24, 32, cw)]


def upconv5x5(P):
    ci, m, (H, W) = 32, 16, (14, 24)
    w1, b1, tb = rnd(2, m, ci, 3, 3) / (3 * ci ** 0.5), rnd(3, m) * 0.2, rnd(4, 9, m) * 0.1
    w2, b2 = rnd(5, 32, m, 3, 3) / (3 * m ** 0.5), rnd(6, 32) * 0.2
    cw5 = P.compose_upconv5x5(w1, b1, tb, w2, b2, DEV, P.L.PREC_BF16X3)
    u = feat(P, 1, 1, ci, 7, 9)
    assert P.upconv5x5_supported(u, H, W, cw5)
    return [P.upconv5x5(u, H, W, cw5, act=P.ACT_RELU)]


def conv2d_cout1(P):
    x = feat(P, 1, 2, 32, 20, 24)
    return [P.conv2d_cout1(x, (rnd(2, 1, 32, 3, 3) / 17).to(DEV), None, 3, res=(rnd(3, 2, 1, 20, 24) + 1).to(DEV), clamp0=True)]


def dwconv2d(P):
    x, k = feat(P, 1, 2, 32, 20, 24), 3
    wt = (rnd(6, 32, 1, k, k) / k).view(32, k * k).t().contiguous().to(DEV)
    return [P.dwconv2d(x, wt, rnd(7, 32).to(DEV), k, 2, True), P.dwconv2d(x, wt, None, k, 1, False)]


def squeeze_excite(P):
    n, c, cse = 1, 8, 1
    x = feat(P, 21, n, c, 1, 1)
    mean = P.global_avgpool(x)
    gate = P.se_gate(mean, (rnd(23, cse, c) / np.sqrt(c)).to(DEV), rnd(24, cse).to(DEV), rnd(25, c, cse).t().contiguous().to(DEV), rnd(26, c).to(DEV))
    return [mean, gate, P.channel_scale_(x, gate)]


def layernorm_feat(P):
    x = P.Feat.from_nchw((rnd(1, 3, 32, 7, 5) * 3 + 1).to(DEV))
    return [P.layernorm_feat(x, rnd(2, 32).to(DEV), rnd(3, 32).to(DEV), 1e-6, P.ACT_GELU)]


def gemm_ss(P):
    M, K, N = 100, 64, 128
    g = torch.Generator().manual_seed(M + K)
    xs = P.split_ss(torch.randn(M, K, generator=g).to(DEV))
    cw = P.pack_conv((torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), (torch.randn(N, generator=g) * 0.1).to(DEV), prec=P.L.PREC_BF16X3)
    return [P.gemm_ss(xs, cw, act=P.ACT_GELU), P.gemm_ss(xs, cw, out_ss=True)]


def vit_attention(P):
    """gemm_ss_qkv -> attention_qkv_ss, and attention on the fp32 rows of the same Linear (f32, bf16x3, bf16x3 with split-swizzled output)"""
    B, N, H = 5, 37, 3
    g = torch.Generator().manual_seed(B * N + H)
    D = H * 64
    xs = P.split_ss(torch.randn(B * N, D, generator=g).to(DEV))
    cw = P.pack_conv((torch.randn(3 * D, D, generator=g) / D ** 0.5).to(DEV), (torch.randn(3 * D, generator=g) * 0.1).to(DEV), prec=P.L.PREC_BF16X3)
    qkv, qkv_ss = P.gemm_ss(xs, cw), P.gemm_ss_qkv(xs, cw, H)
    return [qkv_ss, P.attention_qkv_ss(qkv_ss, B, N, H), P.attention_qkv_ss(qkv_ss, B, N, H, out_ss=False), P.attention(qkv, B, N, H, P.PREC_F32),
            P.attention(qkv, B, N, H, P.L.PREC_BF16X3), P.attention(qkv, B, N, H, P.L.PREC_BF16X3, out_ss=True)]


FRAMES_OF = [1, 0, 1, 0]  # tiles of two frames, interleaved in one list


def _boxes(seed, k):
    g = torch.Generator().manual_seed(seed)
    x1, y1 = torch.rand(k, generator=g) * 20, torch.rand(k, generator=g) * 14
    b4 = torch.stack([x1, y1, x1 + 8 + 4 * torch.rand(k, generator=g), y1 + 6 + 4 * torch.rand(k, generator=g)], 1)
    return b4, torch.cat([torch.tensor(FRAMES_OF[:k], dtype=torch.float32)[:, None], b4], 1)


def roi_align(P):
    """one map with boxes [k, 4], B = 2 maps with boxes [k, 5]; fp32 and pre-split (X2) outputs"""
    maps = rnd(2, 2, 24, 32, 3).to(DEV)
    b4, b5 = _boxes(3, 4)
    outs = [P.roi_align(P.Feat(maps[:1].contiguous()), b4.to(DEV), 0.75, 12, 16), P.roi_align(P.Feat(maps), b5.to(DEV), 0.75, 12, 16)]
    maps, b4 = rnd(7, 2, 16, 20, 16).to(DEV), b4 * 0.5
    for feat_, boxes in ((P.Feat(maps[:1].contiguous()), b4), (P.Feat(maps), torch.cat([b5[:, :1], b4], 1))):
        outs.append(P.roi_align(feat_, boxes.to(DEV), 1.0, 16, 20, out=P.Feat(torch.zeros((4, 16, 20, 16), device=DEV), x2=True)))
    return outs


def crop_resize(P):
    """(not profiled: the records are empty on both routes) one frame with tiles [k, 2], B = 2 frames with tiles [k, 3]"""
    img = torch.rand(2, 3, 96, 128, generator=torch.Generator().manual_seed(1)).to(DEV)
    hw = [(0, 0), (48, 64), (17, 33), (31, 7)]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    one, two = P.Feat.alloc(4, 30, 42, 4, DEV), P.Feat.alloc(4, 30, 42, 4, DEV)
    P.crop_resize(img[0].contiguous(), torch.tensor(hw, dtype=torch.int32, device=DEV), 48, 64, 30, 42, mean, std, one)
    P.crop_resize(img, torch.tensor([(f, h, w) for f, (h, w) in zip(FRAMES_OF, hw)], dtype=torch.int32, device=DEV), 48, 64, 30, 42, None, None, two)
    return [one.view()[..., :3], two.view()[..., :3]]  # (crop_resize writes the three image channels)


def coarse_taps(P):
    """knot table + gather of one frame and of B = 2 frames (boxes of split-4 tiles: bin == knot spacing)"""
    h, w, cout, ph, pw, H, W = 12, 16, 8, 48, 64, 96, 128
    g = P.Feat(rnd(9, 2, h, w, 9 * cout).to(DEV))
    hw = [(0, 0), (24, 32), (72, 96), (48, 0)]
    b4 = torch.tensor([[w0 / W * pw, h0 / H * ph, (w0 + 32) / W * pw, (h0 + 24) / H * ph] for h0, w0 in hw], dtype=torch.float32)
    b5 = torch.cat([torch.tensor(FRAMES_OF, dtype=torch.float32)[:, None], b4], 1)
    one, two = P.CoarseTaps(P.Feat(g.buf[:1].contiguous()), cout, (0.25, 0.25)), P.CoarseTaps(g, cout, (0.25, 0.25))
    return [one.v, two.v, one.gather(b4.to(DEV), h / ph, h, w), two.gather(b5.to(DEV), h / ph, h, w)]


def upsample_bilinear(P):
    return [P.upsample_bilinear(feat(P, 1, 1, 98, 7, 11), 14, 21)]


def conv_border_bias(P):
    y = feat(P, 1, 2, 32, 6, 10)
    P.conv_border_bias(y, rnd(2, 9, 32).to(DEV))
    return [y]


def depth_pair_fill(P):
    n, h, w, oh, ow, c0 = 1, 12, 16, 3, 5, 0
    f1, f2 = (P.Feat(rnd(s, n, h, w, 1).to(DEV)) for s in (3, 4))
    got = P.Feat.alloc_raw(n, oh, ow, c0 + 2, DEV)
    P.depth_pair_fill(f1, f2, got, c0)
    return [got.buf]


# case -> number of profiler records it must leave (by_shape: the memory-bound kernels are itemised too)
CASES = [(conv2d, 1), (conv2d_f32_strip, 2), (conv2d_ups, 1), (upconv3x3, 1), (upconv5x5, 2), (conv2d_cout1, 1), (dwconv2d, 2), (squeeze_excite, 3),
         (layernorm_feat, 1), (gemm_ss, 2), (vit_attention, 7), (roi_align, 4), (crop_resize, 0), (coarse_taps, 4), (upsample_bilinear, 1),
         (conv_border_bias, 1), (depth_pair_fill, 1)]


def _bits(o):
    """an output as a tensor: a Feat's channels (its whole buffer when it is in the pre-split format)"""
    if isinstance(o, torch.Tensor):
        return o
    return o.buf if o.x2 else o.view()


def _run(P, monkeypatch, route, case):
    monkeypatch.setattr(P, "DISPATCH", route)
    P.PROFILER.start(timed=False, by_shape=True)
    try:
        outs = case(P)
    finally:
        records = P.PROFILER.stop()
    return [(tag, flops, algo) for tag, flops, _, _, algo in records], [_bits(o) for o in outs]


@pytest.mark.parametrize("case,n_records", CASES, ids=[c.__name__ for c, _ in CASES])
def test_both_routes_leave_the_same_records_and_bits(P, monkeypatch, case, n_records):
    rec_t, out_t = _run(P, monkeypatch, "torch", case)
    rec_c, out_c = _run(P, monkeypatch, "ctypes", case)
    assert rec_t == rec_c
    assert len(rec_t) == n_records, rec_t
    assert all(isinstance(tag, str) and tag for tag, _, _ in rec_t), rec_t
    assert len(out_t) == len(out_c)
    for i, (a, b) in enumerate(zip(out_t, out_c)):
        assert a.shape == b.shape and torch.equal(a, b), (case.__name__, i)
    if case is conv2d_f32_strip:
        (tag0, fl0, _), (tag1, fl1, _) = rec_t
        assert tag1.endswith(" strip8") and not tag0.endswith(" strip8"), rec_t
        full = 2.0 * 4 * 72 * 40 * 34 * 9
        assert fl0 == full * 64 / 72 and fl1 == full * 8 / 72, rec_t


@pytest.mark.parametrize("route", ["torch", "ctypes"])
def test_wrong_shapes_raise_the_same_text_on_both_routes(P, monkeypatch, route):
    monkeypatch.setattr(P, "DISPATCH", route)
    img = torch.zeros(2, 3, 16, 16, device=DEV)
    out = P.Feat.alloc(1, 8, 8, 4, DEV)
    with pytest.raises(AssertionError, match=r"crop_resize of B frames takes tiles \(frame, h, w\)"):
        P.crop_resize(img, torch.zeros((1, 2), dtype=torch.int32, device=DEV), 8, 8, 8, 8, None, None, out)
    with pytest.raises(ValueError, match=r"prv2 ops need float32 tensors on the GPU \(no CPU fallback exists\)"):
        P.crop_resize(torch.zeros(3, 16, 16), torch.zeros((1, 2), dtype=torch.int32, device=DEV), 8, 8, 8, 8, None, None, out)
    with pytest.raises(ValueError, match=r"bicubic_resize needs a uint8 or float32 image on the GPU"):
        P.bicubic_resize(torch.zeros(4, 4, 3), 8, 8)
