"""GPU: which kernel each rung of prv2_conv2d's ladder hands a layer to -- one explicit table of the smallest layer that takes the rung,
the literal prv2_last_kernel() string, and a float64 anchor of the result (tests/test_hip_ops.py's ``close`` and its tolerances for the
same comparison: 2e-5 in f32 mode, 3e-5 in bf16x3)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"f32": 2e-5, "bf16x3": 3e-5}


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def close(got, ref, tol, what=""):
    got = got.detach().cpu()
    err = float((got - ref).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    assert err <= tol * scale, f"{what}: max|d|={err:.3e} (scale {scale:.2f})"


# id, entry point, (n, h, w, cin, cout, k, stride), precision, options, kernel of the (last) launch
ROUTES = [
    ("c256", "conv2d", (1, 4, 16, 32, 256, 3, 1), "bf16x3", {}, "conv3x3_c256_kernel<256,bf16x3>"),
    ("c256-gamma-leaves", "conv2d", (1, 4, 24, 32, 256, 3, 1), "bf16x3", dict(gamma=True), "conv3x3_halo16_kernel<128,bf16x3>"),
    ("halo16-32", "conv2d", (1, 4, 24, 32, 32, 3, 1), "bf16x3", {}, "conv3x3_halo16_kernel<32,bf16x3>"),
    ("halo16-64", "conv2d", (1, 4, 24, 32, 64, 3, 1), "bf16x3", {}, "conv3x3_halo16_kernel<64,bf16x3>"),
    ("halo16-128", "conv2d", (1, 4, 24, 32, 130, 3, 1), "bf16x3", {}, "conv3x3_halo16_kernel<128,bf16x3>"),
    ("halo-f32", "conv2d", (1, 4, 24, 32, 32, 3, 1), "f32", {}, "conv3x3_halo_kernel<32,f32>"),
    ("strip-merged", "conv2d", (1, 4, 70, 32, 32, 3, 1), "bf16x3", {}, "conv3x3_halo16_kernel<32,bf16x3>"),
    ("strip-second-launch", "conv2d", (1, 4, 70, 32, 32, 3, 1), "f32", {}, "igemm_kernel<64,f32>"),
    ("no-halo-width-16", "conv2d", (1, 4, 16, 32, 32, 3, 1), "bf16x3", {}, "igemm_kernel<64,bf16x3>"),
    ("few-in", "conv2d", (1, 128, 128, 4, 32, 3, 2), "f32", {}, "conv_few_in_kernel<64,f32>"),
    ("1x1-small", "conv2d", (1, 64, 64, 80, 4, 1, 1), "f32", {}, "conv1x1_small_kernel<64,f32>"),
    ("1x1-gemm16", "conv2d", (1, 20, 28, 96, 256, 1, 1), "bf16x3", {}, "gemm16_kernel<64,bf16x3>"),  # (its own 64-column rule: 5 x 2 tiles)
    ("1x1-igemm-64-column-rule", "conv2d", (1, 20, 28, 96, 256, 1, 1), "f32", {}, "igemm_kernel<64,f32>"),
    ("convt-k2", "conv2d", (1, 8, 8, 32, 32, 2, 2), "f32", dict(convt=True), "igemm_kernel<64,f32>"),
    ("same-k3-s2", "conv2d", (1, 9, 9, 32, 32, 3, 2), "f32", dict(same=True), "igemm_kernel<64,f32>"),
    ("pre", "pre", (1, 4, 24, 32, 32, 3, 1), "bf16x3", {}, "conv3x3_halo16_kernel<32,bf16x3>"),
    ("pre-ln-256", "pre", (1, 4, 24, 32, 256, 3, 1), "bf16x3", dict(ln=True), "conv3x3_c256_kernel<256,bf16x3>"),
    ("tail", "tail", (1, 4, 24, 32, 32, 3, 1), "bf16x3", {}, "conv3x3_halo16_kernel<32,bf16x3>"),
]


def same_pads(size, k, s):
    total = max((-(-size // s) - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def conv64(x, wt, b, k, s, o):
    x, wt, b = x.double(), wt.double(), b.double()
    if o.get("convt"):
        return F.conv_transpose2d(x, wt, b, stride=k)
    if o.get("same"):
        (ly, hy), (lx, hx) = same_pads(x.shape[2], k, s), same_pads(x.shape[3], k, s)
        return F.conv2d(F.pad(x, (lx, hx, ly, hy)), wt, b, stride=s)
    return F.conv2d(x, wt, b, stride=s, padding=k // 2)


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_layer_takes_its_rung(P, route):
    name, entry, (n, h, w, cin, cout, k, s), prec, o, kernel = route
    PR = P.L.PREC_NAMES[prec]
    x = rnd(1, n, cin, h, w)
    wt = (rnd(2, cin, cout, k, k) if o.get("convt") else rnd(2, cout, cin, k, k)) / np.sqrt(cin * k * k)
    b = rnd(3, cout) * 0.1
    ref = conv64(x, wt, b, k, s, o)
    cw = P.pack_conv(wt.to(DEV), b.to(DEV), stride=s, convt_k=k if o.get("convt") else 0, prec=PR, same_pad=bool(o.get("same")))
    xf = P.Feat.from_nchw(x.to(DEV))
    if entry == "conv2d":
        gamma = 1 + 0.2 * rnd(4, cout) if o.get("gamma") else None
        if gamma is not None:
            ref = ref * gamma.double().view(1, -1, 1, 1)
        got = P.conv2d(xf, cw, gamma=gamma.to(DEV) if gamma is not None else None).to_nchw()
    elif entry == "pre":
        pre = rnd(5, n, cout, h, w)
        ref = ref + pre.double()
        ln = (1 + 0.2 * rnd(6, cout), 0.1 * rnd(7, cout)) if o.get("ln") else None
        if ln is not None:
            mu = ref.mean(1, keepdim=True)
            ref = (ref - mu) / torch.sqrt(((ref - mu) ** 2).mean(1, keepdim=True) + 1e-6) * ln[0].double().view(1, -1, 1, 1) + ln[1].double().view(1, -1, 1, 1)
        assert P.conv2d_pre_supported(h, w, cw, ln is not None)
        got = P.conv2d_pre(xf, cw, P.Feat.from_nchw(pre.to(DEV)), ln=(ln[0].to(DEV), ln[1].to(DEV)) if ln is not None else None).to_nchw()
    else:
        ph, pw = 3, 5
        p1, p2 = rnd(8, n, ph, pw, 1).abs(), rnd(9, n, ph, pw, 1).abs()
        buf = P.Feat.alloc_raw(n, h, w, cout + 2, DEV)
        buf.buf.fill_(float("nan"))
        dst = buf.slice(0, cout)
        assert P.conv2d_tail_supported(xf, cw, dst)
        P.conv2d_tail(xf, cw, dst, P.Feat(p1.to(DEV)), P.Feat(p2.to(DEV)))
        pair = torch.cat([F.interpolate(t.double().permute(0, 3, 1, 2), (h, w), mode="bilinear", align_corners=True) for t in (p1, p2)], 1)
        ref = torch.cat([ref, pair, torch.zeros(n, 2, h, w, dtype=torch.float64)], 1)
        got = buf.buf.permute(0, 3, 1, 2)
    got_kernel = P.L.load().prv2_last_kernel().decode()
    print(f"route {name}: {got_kernel}")
    assert got_kernel == kernel
    close(got, ref.float(), TOL[prec], f"{name} on {got_kernel}")
