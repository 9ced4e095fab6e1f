"""Batch independence of every size-dependent kernel choice ("Host-side choices that depend on the batch").

frame.py's drivers rest on one invariant: a patch's result does not depend on the batch it was computed in.  Several host-side choices
nevertheless depend on n or on M = n h w: tile widths picked by the size of the grid, persistent workgroups that walk several tiles once
there are more tiles than workgroups, block-id decodes that are functions of the grid size.  Each of them is crossed here BY SHAPE.

One method throughout: the big batch is drawn on the device from a seeded generator; the small batch is a contiguous copy of its first,
middle and last image (per-image side inputs -- res, mul, res2, pre, p1 / p2, boxes -- sliced the same way); the op runs on both and the
shared images must be ``torch.equal``.  After each call ``prv2_last_kernel()`` must name the kernel and tile width expected on that side,
so that a later change of a threshold fails the test instead of quietly no longer crossing it.  Each case is anchored ONCE against
float64, on the small batch only, with the tolerance the op has in its own test (test_hip_ops.py, test_chain32.py, test_conv3x3_f6.py,
test_upconv5.py); every other assertion is bit equality.

The thresholds are mirrored from the code.  The persistent grids of conv3x3_c256_f6_kernel and chain32_kernel are the literal 256 of
csrc/conv3x3_f6.hip / csrc/chain32.hip (A/B switches PRV2_F6_WGS / PRV2_CHAIN32_WGS, read once per process), not the device's CU count;
the tests take max(256, multi_processor_count) so that the big side walks several tiles per workgroup on either reading.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def _ops():
    from patchrefinerv2_amd import ops
    return ops


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def last_kernel():
    return _ops().L.load().prv2_last_kernel().decode()


def persistent_workgroups():
    """what the persistent kernels launch at most (the code's literal 256), and at least the device's CUs"""
    return max(256, torch.cuda.get_device_properties(0).multi_processor_count)


def picks(n):
    """the images of a batch of n that the small batch copies: first, middle (n > 2), last"""
    return sorted({0, n // 2, n - 1})


def sub(v, idx):
    """a contiguous copy of the images ``idx`` of a batch-leading tensor / Feat (None stays None)"""
    if v is None:
        return None
    P = _ops()
    i = torch.tensor(idx, device=DEV)
    if isinstance(v, P.Feat):
        return P.Feat(v.buf[i].contiguous(), v.c, v.c0, v.x2)
    return v[i].contiguous()


def head(v, n):
    """the first n images of a batch-leading tensor / Feat, in place (a prefix of a contiguous buffer is contiguous)"""
    if v is None:
        return None
    P = _ops()
    if isinstance(v, P.Feat):
        return P.Feat(v.buf[:n], v.c, v.c0, v.x2)
    return v[:n]


def raw(v):
    P = _ops()
    return v.buf[..., v.c0:v.c0 + v.c] if isinstance(v, P.Feat) else v


def bits(big, small, idx, what):
    """images ``idx`` of the big batch's output == the small batch's output, bit for bit"""
    a, b = raw(big)[torch.tensor(idx, device=DEV)], raw(small)
    if a.dtype.is_floating_point:   # (compare the bytes: NaN-proof, and X2 buffers are float32 containers)
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    diff = a != b
    assert a.shape == b.shape and not bool(diff.any()), \
        f"{what}: {int(diff.sum())} of {a.numel()} elements differ between an image in the batch and the same image in the small batch, " \
        f"max |d| = {float((a.view(torch.float32) - b.view(torch.float32)).abs().max()):.3e}, first at {diff.nonzero()[:4].tolist()}"


def close(got, ref, tol, what=""):
    """the criterion of test_hip_ops.close / test_chain32.close: max |d| <= tol max(1, max |ref|)"""
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    err = float((got - ref).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    assert got.shape == ref.shape and err <= tol * scale, f"{what}: max|d|={err:.3e} (scale {scale:.2f}, tol {tol:g})"


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / ref.norm())


# ---- float64 references (CPU, channels-last in and out) ---------------------------------------------------------------------------
def d64(t):
    return None if t is None else raw(t).detach().double().cpu()


def conv64(x, w, b=None, relu_in=False, pad=None):
    x = torch.relu(x) if relu_in else x
    pad = w.shape[-1] // 2 if pad is None else pad
    return F.conv2d(x.permute(0, 3, 1, 2), w.double().cpu(), b.double().cpu() if b is not None else None, padding=pad).permute(0, 2, 3, 1)


def ln64(t, lnw, lnb, eps=1e-6):
    mu = t.mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(((t - mu) ** 2).mean(-1, keepdim=True) + eps) * lnw.double().cpu() + lnb.double().cpu()


def x2_value(v):
    """what an X2 element stands for: bf16 hi (RNE) + bf16 lo (RNE of the remainder)"""
    hi = v.to(torch.bfloat16).float()
    return hi + (v - hi).to(torch.bfloat16).float()


def to_x2(P, f32):
    """the fp32 Feat [n, h, w, 256] as its producer writes it pre-split: an identity conv through the 256-column kernel's X2 writer"""
    out = P.Feat(torch.empty_like(f32.buf), x2=True)
    ident = torch.zeros(256, 256, 3, 3, device=DEV)
    ident[torch.arange(256), torch.arange(256), 1, 1] = 1.0
    P.conv2d(f32, P.pack_conv(ident, None, pad=1, prec=P.L.PREC_BF16X3), out)
    return out


ACT64 = {"none": lambda v: v, "gelu": F.gelu, "relu": torch.relu, "sigmoid": torch.sigmoid}


def act_id(P, name):
    return {"none": P.ACT_NONE, "gelu": P.ACT_GELU, "relu": P.ACT_RELU, "sigmoid": P.ACT_SIGMOID}[name]


# ---- a. igemm_kernel<64> <-> <128> ------------------------------------------------------------------------------------------------
def igemm_width(rows, cout):
    """csrc/igemm.hip: 64-column tiles while the 128-column grid has at most 128 workgroups (BM = 128 rows)"""
    return 64 if cout > 64 and cdiv(rows, 128) * cdiv(cout, 128) <= 128 else (128 if cout > 64 else 64)


IGEMM_CASES = [
    # prec, k, cin, cout, h, w, rows of the igemm launch per image, n of the big batch, tolerance of the op's own test
    ("f32", 3, 64, 128, 16, 16, 256, 65, 2e-5),      # width < 24: no halo kernel; 2 row tiles per image
    ("bf16x3", 3, 64, 128, 16, 16, 256, 65, 3e-5),
    ("f32", 1, 96, 256, 20, 28, 560, 15, 2e-5),      # 1x1: the rows of all images are one matrix, images start inside a tile
    ("f32", 3, 32, 128, 64, 72, 64 * 8, 33, 2e-5),   # the f32 remainder strip (width 64 + 8): M re-derived for the strip's launch
]


@pytest.mark.parametrize("case", IGEMM_CASES, ids=lambda c: f"{c[0]}-k{c[1]}-{c[2]}to{c[3]}-{c[4]}x{c[5]}")
def test_igemm_tile_width_does_not_change_the_bits(P, case):
    prec, k, cin, cout, h, w, rows, nb, tol = case
    g = gen(k * 1000 + cin + h)
    x = P.Feat(torch.randn(nb, h, w, cin, device=DEV, generator=g))
    res = P.Feat(torch.randn(nb, h, w, cout, device=DEV, generator=g))
    wt = torch.randn(cout, cin, k, k, device=DEV, generator=g) / (k * cin ** 0.5)
    b = torch.randn(cout, device=DEV, generator=g) * 0.1
    cw = P.pack_conv(wt, b, prec=P.L.PREC_NAMES[prec])
    idx = picks(nb)
    assert igemm_width(len(idx) * rows, cout) == 64 and igemm_width(nb * rows, cout) == 128
    big = P.conv2d(x, cw, act=P.ACT_GELU, res=res)
    assert last_kernel() == f"igemm_kernel<128,{prec}>", last_kernel()
    xs, rs = sub(x, idx), sub(res, idx)
    small = P.conv2d(xs, cw, act=P.ACT_GELU, res=rs)
    assert last_kernel() == f"igemm_kernel<64,{prec}>", last_kernel()
    bits(big, small, idx, f"igemm <128> vs <64> {case}")
    close(small.buf, F.gelu(conv64(d64(xs), wt, b)) + d64(rs), tol, f"igemm {case}")


# ---- b. gemm16_kernel<64> / <128> / <256> -----------------------------------------------------------------------------------------
ROWS = 300
EPILOGUES = {
    "none": dict(), "gelu": dict(act="gelu"), "gamma_res": dict(gamma=True, res=True), "gelu_gamma_res": dict(act="gelu", gamma=True, res=True),
    "sigmoid_mul_res": dict(act="sigmoid", mul=True, res=True), "ln_gelu": dict(act="gelu", ln=True),
}
GEMM16_CASES = {
    # K, N, {M: tile width csrc/gemm_m16.hip::launch_gemm16 picks}: 64 columns while cdiv(M, 128) cdiv(N, 128) <= 160, 256 rows once K >= 2048 and
    # cdiv(M, 256) cdiv(N, 128) >= 256
    "k128": (128, 256, {ROWS: 64, 10300: 128}),                      # 3 x 2 tiles; 81 x 2 = 162 tiles
    "k2048": (2048, 1024, {ROWS: 64, 2700: 128, 8000: 256}),         # 24; 22 x 8 = 176 tiles, 11 x 8 < 256; 32 x 8 = 256
    "ln": (256, 128, {ROWS: 128, 1000: 128}),                        # fused LayerNorm: no narrow tile; position inside the tile only
}


@functools.lru_cache(maxsize=None)
def _linear_operands(name):
    K, N, widths = GEMM16_CASES[name]
    M = max(widths)
    g = gen(K + N)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    return dict(x=r(M, K), w=r(N, K) / K ** 0.5, b=r(N) * 0.1, gamma=1 + 0.1 * r(N), res=r(M, N), mul=r(M, N), lnw=1 + 0.2 * r(N), lnb=0.1 * r(N))


@functools.lru_cache(maxsize=None)
def _linear_ref64(name, epi):
    """float64 of the first ROWS rows (shared by the arithmetic modes; never written again)"""
    o, e = _linear_operands(name), EPILOGUES[epi]
    t = d64(o["x"][:ROWS]) @ d64(o["w"]).t() + d64(o["b"])
    if e.get("ln"):
        t = ln64(t, o["lnw"], o["lnb"])
    t = ACT64[e.get("act", "none")](t)
    if e.get("gamma"):
        t = t * d64(o["gamma"])
    if e.get("mul"):
        t = d64(o["mul"][:ROWS]) * t
    if e.get("res"):
        t = t + d64(o["res"][:ROWS])
    return t


@pytest.mark.parametrize("prec,tol", [("bf16x3", 3e-5), ("bf16", 2e-2)])
@pytest.mark.parametrize("name,epi", [(n_, e_) for n_ in ("k128", "k2048") for e_ in EPILOGUES if e_ != "ln_gelu"] + [("ln", "ln_gelu")])
def test_gemm16_tile_shape_and_row_position_do_not_change_the_bits(P, name, epi, prec, tol):
    """ops.linear on M rows == ops.linear on 300 of those rows alone -- the first 300 and the last 300, which sit at another offset inside their
    tile -- across gemm16_kernel's 64-column, 128-row and 256-row variants, for the lean store loop (none, GELU, sigmoid x mul + res) and the
    general epilogue (gamma, fused LayerNorm)."""
    K, N, widths = GEMM16_CASES[name]
    o, e = _linear_operands(name), EPILOGUES[epi]
    cw = P.pack_conv(o["w"], o["b"], prec=P.L.PREC_NAMES[prec])

    def run(r0, r1):
        kw = dict(act=act_id(P, e.get("act", "none")), gamma=o["gamma"] if e.get("gamma") else None, ln=(o["lnw"], o["lnb"]) if e.get("ln") else None)
        for side in ("mul", "res"):
            if e.get(side):
                kw[side] = o[side][r0:r1].contiguous()
        y = P.linear(o["x"][r0:r1].contiguous(), cw, **kw)
        assert last_kernel() == f"gemm16_kernel<{widths[r1 - r0]},{prec}>", (r1 - r0, last_kernel())
        return y

    first = run(0, ROWS)
    for M in sorted(widths)[1:]:
        whole = run(0, M)
        for r0 in (0, M - ROWS):
            alone = first if r0 == 0 else run(r0, M)
            d = whole[r0:r0 + ROWS] != alone
            assert not bool(d.any()), (f"{name} {epi} {prec}: rows [{r0}, {r0 + ROWS}) of M = {M} (gemm16_kernel<{widths[M]}>) vs alone (<{widths[ROWS]}>): "
                                       f"{int(d.sum())} elements differ, max |d| = {float((whole[r0:r0 + ROWS] - alone).abs().max()):.3e}")
    close(first, _linear_ref64(name, epi), tol, f"linear {name} {epi} {prec}")


# ---- c. conv3x3_c256_f6_kernel: persistent workgroups walking several tiles ------------------------------------------------------
@pytest.mark.parametrize("x2_out", [False, True], ids=["fp32", "x2"])
@pytest.mark.parametrize("relu_in,with_res,with_bias", [(True, True, True), (False, False, False)], ids=["relu_res_bias", "bare"])
@pytest.mark.parametrize("h,w,nb", [(24, 32, 48), (19, 37, 30)])
def test_conv3x3_f6_persistent_tile_walk_does_not_change_the_bits(P, h, w, nb, relu_in, with_res, with_bias, x2_out):
    """8 x 16 tiles: 48 images of 24 x 32 are 288 tiles, 30 ragged images of 19 x 37 are 270 -- more than the persistent workgroups, which
    then walk two tiles with the next halo prefetched under the current tile -- against 3 images (one tile per workgroup).  ``cw.x_scale``
    stays at its default on both sides."""
    cin = 256
    g = gen(h * 100 + w)
    x = P.Feat(torch.randn(nb, h, w, cin, device=DEV, generator=g))
    res = P.Feat(torch.randn(nb, h, w, 256, device=DEV, generator=g)) if with_res else None
    wt = torch.randn(256, cin, 3, 3, device=DEV, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(256, device=DEV, generator=g) if with_bias else None
    assert P.conv3x3_f6_supported(x, 256, cin)
    cw = P.pack_conv3x3_f6(wt, b)
    idx = picks(nb)
    per_image = cdiv(h, 8) * cdiv(w, 16)
    assert len(idx) * per_image <= 256 and nb * per_image > persistent_workgroups()

    def run(xf, rf):
        out = P.Feat(torch.empty(xf.n, h, w, 256, device=DEV), x2=True) if x2_out else None
        y = P.conv3x3_f6(xf, cw, out, relu_in=relu_in, res=rf)
        assert last_kernel() == "conv3x3_c256_f6_kernel<256,f16f6>", last_kernel()
        return y

    big = run(x, res)
    xs, rs = sub(x, idx), sub(res, idx)
    small = run(xs, rs)
    assert cw.x_scale == 1.0
    bits(big, small, idx, f"conv3x3_f6 {nb}x{h}x{w} ({nb * per_image} tiles) vs {len(idx)} images")
    ref = conv64(d64(xs), wt, b, relu_in) + (d64(rs) if with_res else 0)
    if not x2_out:
        err = rel_l2(small.buf, ref)
        assert err < 4e-5, err                                     # (test_conv3x3_f6_vs_fp64)
    else:                                                          # (test_conv3x3_f6_x2_output: hi + lo of the fp32 result, 16 mantissa bits)
        o32 = P.conv3x3_f6(xs, cw, relu_in=relu_in, res=rs)
        assert rel_l2(o32.buf, ref) < 4e-5
        assert float((small.x2_to_float().buf.double() - o32.buf.double()).abs().max()) <= 2.0 ** -16 * float(o32.buf.abs().max())


# ---- d. chain32_c2f / chain32_enc: persistent workgroups walking several tiles ---------------------------------------------------
def _chain_weights(kind, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if kind == "c2f":
        return dict(w1=r(32, 32, 3, 3) / 17, b1=r(32) * 0.1, w2=r(32, 32, 3, 3) / 17, b2=r(32) * 0.1, lnw=1 + 0.2 * r(32), lnb=0.1 * r(32), wg=r(32, 32) / 5.6,
                    wo=r(32, 32) / 5.6, bo=r(32) * 0.1, w3=1 + 0.3 * r(32), b3=0.25)
    return dict(w1=r(32, 32, 3, 3) / 17, b1=r(32) * 0.1, ln1w=1 + 0.2 * r(32), ln1b=0.1 * r(32), w2=r(32, 34, 3, 3) / 17.5, b2=r(32) * 0.1, ln2w=1 + 0.2 * r(32),
                ln2b=0.1 * r(32))


@pytest.mark.parametrize("h,w,nb", [(24, 32, 48), (17, 29, 45)])
def test_chain32_c2f_persistent_tile_walk_does_not_change_the_bits(P, h, w, nb):
    """8 x 16 tiles: 288 / 270 tiles in the batch against 18 in the small one; with the coarse half ``pre``"""
    W = _chain_weights("c2f", 3)
    cw = dict(w1=P.pack_chain32(W["w1"], 0, DEV), w2=P.pack_chain32(W["w2"], 1, DEV), wg=P.pack_chain32(W["wg"], 1, DEV), wo=P.pack_chain32(W["wo"], 1, DEV),
              consts=P.chain32_consts(DEV, b1=W["b1"], ln1w=W["lnw"], ln1b=W["lnb"], b2=W["b2"], bo=W["bo"], w3=W["w3"]), b3=W["b3"])
    g = gen(h + w)
    x = P.Feat(torch.randn(nb, h, w, 32, device=DEV, generator=g))
    pre = P.Feat(torch.randn(nb, h, w, 32, device=DEV, generator=g) * 0.5)
    idx = picks(nb)
    per_image = cdiv(h, 8) * cdiv(w, 16)
    assert len(idx) * per_image <= 256 and nb * per_image > persistent_workgroups()
    last, depth = P.chain32_c2f(x, cw, pre)
    assert last_kernel() == "chain32_c2f_kernel<32,bf16x3>", last_kernel()
    xs, ps = sub(x, idx), sub(pre, idx)
    last_s, depth_s = P.chain32_c2f(xs, cw, ps)
    bits(last, last_s, idx, f"chain32_c2f last {nb}x{h}x{w}")
    bits(depth, depth_s, idx, f"chain32_c2f depth {nb}x{h}x{w}")
    xv = d64(xs)                                                    # (test_chain32.c2f_reference, channels-last)
    o = conv64(torch.relu(xv), W["w1"], W["b1"]) + xv
    f = torch.relu(ln64(conv64(o, W["w2"], W["b2"]) + d64(ps), W["lnw"], W["lnb"]))
    y = o * torch.sigmoid(f @ W["wg"].double().t())
    ref_last = y @ W["wo"].double().t() + W["bo"].double()
    ref_depth = (ref_last @ W["w3"].double().view(32, 1) + W["b3"]).permute(0, 3, 1, 2)
    close(last_s.buf, ref_last, 3e-5, "chain32_c2f last")
    close(depth_s, ref_depth, 3e-5, "chain32_c2f depth")


@pytest.mark.parametrize("h,w,nb", [(24, 32, 48), (17, 29, 45)])
def test_chain32_enc_persistent_tile_walk_does_not_change_the_bits(P, h, w, nb):
    """as above for the encoder chain, writing channels [64, 96) of the decoder's 100-channel concat buffer (test_chain32_enc_vs_fp64)"""
    W = _chain_weights("enc", 5)
    cw = dict(w1=P.pack_chain32(W["w1"], 0, DEV), w2=P.pack_chain32(W["w2"], 1, DEV), wt=P.pack_chain32(W["w2"], 2, DEV),
              consts=P.chain32_consts(DEV, b1=W["b1"], ln1w=W["ln1w"], ln1b=W["ln1b"], b2=W["b2"], ln2w=W["ln2w"], ln2b=W["ln2b"]))
    g = gen(2 * h + w)
    x = P.Feat(torch.randn(nb, h, w, 32, device=DEV, generator=g))
    pre = P.Feat(torch.randn(nb, h, w, 32, device=DEV, generator=g) * 0.5)
    p1, p2 = (torch.randn(nb, 1, h, w, device=DEV, generator=g).abs() * 3 for _ in range(2))
    idx = picks(nb)
    per_image = cdiv(h, 8) * cdiv(w, 16)
    assert len(idx) * per_image <= 256 and nb * per_image > persistent_workgroups()

    def run(xf, pf, a, b):
        buf = P.Feat(torch.zeros((xf.n, h, w, 100), device=DEV))
        out = P.chain32_enc(xf, cw, pf, a, b, out=buf.slice(64, 32))
        assert last_kernel() == "chain32_enc_kernel<32,bf16x3>", last_kernel()
        assert float(buf.buf[..., :64].abs().max()) == 0.0 and float(buf.buf[..., 96:].abs().max()) == 0.0
        return out

    big = run(x, pre, p1, p2)
    xs, ps, p1s, p2s = sub(x, idx), sub(pre, idx), sub(p1, idx), sub(p2, idx)
    small = run(xs, ps, p1s, p2s)
    bits(big, small, idx, f"chain32_enc {nb}x{h}x{w}")
    f = F.gelu(ln64(conv64(d64(xs), W["w1"], W["b1"]) + d64(ps), W["ln1w"], W["ln1b"]))
    f = torch.cat([f, d64(p1s).permute(0, 2, 3, 1), d64(p2s).permute(0, 2, 3, 1)], -1)
    close(raw(small), F.gelu(ln64(conv64(f, W["w2"], W["b2"]), W["ln2w"], W["ln2b"])), 3e-5, "chain32_enc")


# ---- e. kernels whose only dependence on n is the block-id decode ----------------------------------------------------------------
N_GRID = (3, 5, 8)   # batches: with B workgroups per image (B % 8 != 0, asserted per case) the grid size mod 8 is non-zero, non-zero, zero


def halo16_blocks(h, w, cout):
    """workgroups per image of the 16x16x32 halo kernels (csrc/conv3x3_m16.hip): 8 x 32-pixel tiles x column tiles + 32 x 8 strip tiles"""
    rem = w % 32
    strip = rem != 0 and rem <= 8 and w >= 64
    tiles_n = cdiv(cout, 128) if cout > 64 else 1
    return (cdiv(h, 8) * (w // 32 if strip else cdiv(w, 32)) + (cdiv(h, 32) if strip else 0)) * tiles_n


def c256_blocks(h, w):
    return cdiv(h, 8) * cdiv(w, 16)


def decode_sweep(make, run, per_image, what):
    """``make(n)`` -> the inputs of a batch of n (a dict of batch-leading tensors / Feats / None); ``run(inputs)`` -> a tuple of batch-leading
    outputs.  For every n of N_GRID: the batch == its picked images alone.  Returns (inputs, outputs) of the first small batch for the anchor."""
    assert per_image % 8 != 0 and sorted((n * per_image) % 8 == 0 for n in N_GRID) == [False, False, True], per_image
    master = make(max(N_GRID))
    anchor = None
    for n in N_GRID:
        inp = {k: head(v, n) for k, v in master.items()}
        big = run(inp)
        idx = picks(n)
        sm_in = {k: sub(v, idx) for k, v in inp.items()}
        small = run(sm_in)
        for j, (a, b) in enumerate(zip(big, small)):
            bits(a, b, idx, f"{what}: output {j}, n = {n} (grid {n * per_image}) vs {len(idx)} images")
        anchor = anchor or (sm_in, small)
    return anchor


HALO16_CASES = [
    # h, w, cin, cout, column tile, options -- shapes of test_hip_ops.GATE_CASES / STRIP_CASES / CONV_CASES
    (13, 24, 64, 32, 32, dict(bias=True, act="gelu")),
    (33, 40, 98, 64, 64, dict(bias=True, relu_in=True, res=True)),                   # tail tile (cin = 96 + 2)
    (13, 24, 64, 128, 128, dict(bias=True, act="gelu", res=True)),
    (11, 70, 66, 130, 128, dict(bias=True, res=True, res2=True, gamma=True)),        # tail tile, two column tiles, strip of 6 columns
    (19, 72, 64, 40, 64, dict(bias=True, ln=True, act="gelu")),                      # strip of 8 columns, fused LayerNorm
]


@pytest.mark.parametrize("case", HALO16_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}to{c[3]}")
def test_halo16_block_decode_is_batch_independent(P, case):
    h, w, cin, cout, bn, o = case
    g = gen(h * w + cout)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt, b = r(cout, cin, 3, 3) / (3 * cin ** 0.5), r(cout) * 0.1
    gamma, lnw, lnb = 1 + 0.1 * r(cout), r(cout).abs() + 0.5, r(cout) * 0.1
    cw = P.pack_conv(wt, b if o.get("bias") else None, pad=1, prec=P.L.PREC_BF16X3)

    def make(n):
        f = lambda c: P.Feat.from_nchw(r(n, c, h, w))  # noqa: E731  (from_nchw: pad channels behind an odd count are zeroed)
        return dict(x=f(cin), res=f(cout) if o.get("res") else None, res2=f(cout) if o.get("res2") else None)

    def run(i):
        y = P.conv2d(i["x"], cw, relu_in=bool(o.get("relu_in")), act=act_id(P, o.get("act", "none")), gamma=gamma if o.get("gamma") else None,
                     res=i["res"], res2=i["res2"], ln=(lnw, lnb) if o.get("ln") else None)
        assert last_kernel() == f"conv3x3_halo16_kernel<{bn},bf16x3>", last_kernel()
        return (y,)

    i, (y,) = decode_sweep(make, run, halo16_blocks(h, w, cout), f"halo16 {case}")
    t = conv64(d64(i["x"]), wt, b if o.get("bias") else None, bool(o.get("relu_in")))
    if o.get("ln"):
        t = ln64(t, lnw, lnb)
    t = ACT64[o.get("act", "none")](t)
    if o.get("gamma"):
        t = t * d64(gamma)
    for side in ("res", "res2"):
        if o.get(side):
            t = t + d64(i[side])
    close(raw(y), t, 3e-5, f"halo16 {case}")                         # (test_conv3x3_remainder_strip, bf16x3)


def test_halo16_ups_block_decode_is_batch_independent(P):
    """conv2d_ups: [up(x1) 64 | x2 32 | pred1 | pred2] -> 98 at 40 x 66 from 20 x 33 (test_hip_ops.UPS_CASES): tail tile + a 2-column strip"""
    (h, w), (H, W), c1, cin, cout = (20, 33), (40, 66), 64, 98, 98
    g = gen(77)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt, b = r(cout, cin, 3, 3) / (3 * cin ** 0.5), r(cout)
    cw = P.pack_conv(wt, b, pad=1, prec=P.L.PREC_BF16X3)

    def make(n):
        x = P.Feat.alloc(n, H, W, cin, DEV)
        x.buf[..., :c1] = float("nan")                                # never read
        x.buf[..., c1:cin] = r(n, H, W, cin - c1)
        return dict(x=x, u=P.Feat(r(n, h, w, c1)), res=P.Feat.from_nchw(r(n, cout, H, W)))

    def run(i):
        assert P.conv2d_ups_supported(i["x"], i["u"], cw)
        y = P.conv2d_ups(i["x"], i["u"], cw, act=P.ACT_GELU, res=i["res"])
        assert last_kernel() == "conv3x3_halo16_ups_kernel<128,bf16x3>", last_kernel()
        return (y,)

    i, (y,) = decode_sweep(make, run, halo16_blocks(H, W, cout), "conv2d_ups")
    up = F.interpolate(d64(i["u"]).permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    ref = F.gelu(conv64(torch.cat([up, d64(i["x"])[..., c1:]], -1), wt, b)) + d64(i["res"])
    close(raw(y), ref, 3e-5, "conv2d_ups")


def test_conv3x3_c256_block_decode_is_batch_independent(P):
    """the 256-column kernel in bf16x3 at the ragged 9 x 37 (6 tiles of 8 x 16), fused LayerNorm + GELU"""
    h, w, cin = 9, 37, 64
    g = gen(9 * 37)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt, b, lnw, lnb = r(256, cin, 3, 3) / (3 * cin ** 0.5), r(256) * 0.1, 1 + 0.2 * r(256), 0.1 * r(256)
    cw = P.pack_conv(wt, b, pad=1, prec=P.L.PREC_BF16X3)

    def run(i):
        y = P.conv2d(i["x"], cw, act=P.ACT_GELU, ln=(lnw, lnb))
        assert last_kernel() == "conv3x3_c256_kernel<256,bf16x3>", last_kernel()
        return (y,)

    i, (y,) = decode_sweep(lambda n: dict(x=P.Feat(r(n, h, w, cin))), run, c256_blocks(h, w), "conv3x3_c256")
    close(y.buf, F.gelu(ln64(conv64(d64(i["x"]), wt, b), lnw, lnb)), 2e-5, "conv3x3_c256")   # (test_conv2d_256_channels_take_the_wide_tile_kernel)


TAPS_SHAPE = ((20, 48), (20, 24), (0.25, 0.5))   # test_taps_fold.SHAPES["ragged20x24"]: coarse map, tile, knot offsets
TAPS_SCALE = 0.25


@pytest.mark.parametrize("addend", ["pre", "taps"])
@pytest.mark.parametrize("x2", [False, True], ids=["fp32", "x2"])
@pytest.mark.parametrize("kernel", ["bf16x3", "f6"])
def test_gate256_block_decode_is_batch_independent(P, kernel, x2, addend):
    """the 256-column GatedConvUnit tail kernels (conv3x3_c256_gate fp32 / X2 input, ..._gate_f6) over the unit's ``out`` (x = mul) with a residual:
    with a gathered ``pre`` at 9 x 37, and through the folded-taps entry (``taps=``, ``boxes=``: the per-tile boxes are sliced with the images) at
    the ragged 20 x 24"""
    F_ = 256
    (H, W), (h, w), kb = TAPS_SHAPE if addend == "taps" else ((0, 0), (9, 37), None)
    g = gen(31 + h)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt, b, w3, gb = r(F_, F_, 3, 3) / 48, r(F_) * 0.1, r(F_, F_, 1, 1) / 16, r(F_) * 0.1
    ln = (torch.rand(F_, device=DEV, generator=g) + 0.5, r(F_) * 0.1)
    gw = P.pack_gate(w3)
    cw = P.pack_conv3x3_f6(wt, b) if kernel == "f6" else P.pack_conv(wt, b, pad=1, prec=P.L.PREC_BF16X3)
    taps = P.CoarseTaps(P.Feat(r(1, H, W, 9 * F_) * 0.2), F_, kb) if addend == "taps" else None

    def make(n):
        o32 = P.Feat(r(n, h, w, F_))
        d = dict(x=to_x2(P, o32) if x2 else o32, res=P.Feat(r(n, h, w, F_)))
        if addend == "taps":       # boxes whose ROI bin is exactly the knot spacing, at fractional offsets inside the frame
            bh, bw, fh, fw = kb[0] * h / TAPS_SCALE, kb[1] * w / TAPS_SCALE, H / TAPS_SCALE, W / TAPS_SCALE
            org = torch.rand(n, 2, device=DEV, generator=g) * torch.tensor([fw - bw, fh - bh], device=DEV)
            d["boxes"] = torch.cat([org, org + torch.tensor([bw, bh], device=DEV)], 1).contiguous()
        else:
            d["pre"] = P.Feat(r(n, h, w, F_) * 0.5)
        return d

    def run(i):
        kw = dict(act=P.ACT_RELU, mul=i["x"], res=i["res"], pre_cin=F_)
        kw.update(dict(taps=taps, boxes=i["boxes"], spatial_scale=TAPS_SCALE) if addend == "taps" else dict(pre=i["pre"]))
        if kernel == "f6":
            y = P.conv3x3_ln_gate_f6(i["x"], cw, ln, gw, gb, **kw)
        else:
            y = P.conv3x3_ln_gate(i["x"], cw, ln, gw, gb, **kw)
        want = {"f6": "conv3x3_c256_gate_f6_kernel<256,f16f6>", "bf16x3": "conv3x3_c256_gate_x2_kernel<256,bf16x3>" if x2 else "conv3x3_c256_gate_kernel<256,bf16x3>"}[kernel]
        assert last_kernel() == want, last_kernel()
        return (y,)

    i, (y,) = decode_sweep(make, run, c256_blocks(h, w), f"gate256 {kernel} x2={x2} {addend}")
    xv = d64(i["x"].x2_to_float()) if x2 else d64(i["x"])
    mv = xv if x2 else x2_value(i["x"].buf).double().cpu()          # (the kernels multiply by the bf16 pair hi + lo of ``mul`` in either format)
    pre = d64(taps.gather(i["boxes"], TAPS_SCALE, h, w)) if addend == "taps" else d64(i["pre"])
    t = torch.relu(ln64(conv64(xv, wt, b) + pre, ln[0], ln[1]))
    ref = mv * torch.sigmoid(t @ d64(w3[:, :, 0, 0]).t() + d64(gb)) + d64(i["res"])
    if kernel == "f6":
        assert rel_l2(y.buf, ref) < 2e-5, rel_l2(y.buf, ref)       # (test_gate_unit_tail_f6_vs_fp64_and_bf16x3)
    else:
        close(y.buf, ref, 2e-5, "gate256 bf16x3")                  # (test_conv3x3_ln_gate_fused_tail)


@pytest.mark.parametrize("h,w,cin,C_", [(33, 40, 32, 128), (9, 37, 32, 32)])
def test_halo16_gate_block_decode_is_batch_independent(P, h, w, cin, C_):
    """the 128- and 32-channel GatedConvUnit tail on the halo16 kernels (test_hip_ops.GATE_CASES)"""
    g = gen(h + C_)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    w0, b0, w3, b3 = r(C_, cin, 3, 3) / (3 * cin ** 0.5), r(C_) * 0.1, r(C_, C_, 1, 1) / C_ ** 0.5, r(C_) * 0.1
    ln = (1 + 0.2 * r(C_), 0.1 * r(C_))
    cw, gw = P.pack_conv(w0, b0, pad=1, prec=P.L.PREC_BF16X3), P.pack_gate(w3)

    def run(i):
        assert P.conv3x3_ln_gate_supported(i["x"], cw)
        y = P.conv3x3_ln_gate(i["x"], cw, ln, gw, b3, act=P.ACT_RELU, mul=i["mul"], res=i["res"])
        assert last_kernel() == f"conv3x3_halo16_gate_kernel<{C_},bf16x3>", last_kernel()
        return (y,)

    i, (y,) = decode_sweep(lambda n: dict(x=P.Feat(r(n, h, w, cin)), mul=P.Feat(r(n, h, w, C_)), res=P.Feat(r(n, h, w, C_))), run, halo16_blocks(h, w, 32),
                           f"halo16 gate {C_}")
    t = torch.relu(ln64(conv64(d64(i["x"]), w0, b0), ln[0], ln[1]))
    close(y.buf, d64(i["mul"]) * torch.sigmoid(t @ d64(w3[:, :, 0, 0]).t() + d64(b3)) + d64(i["res"]), 2e-5, f"halo16 gate {C_}")


def _upconv3x3_ref(u, wt, b, H, W, act):
    up = F.interpolate(d64(u).permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return ACT64[act](conv64(up, wt, b))


def test_upconv3x3_block_decode_is_batch_independent(P):
    """(9, 12) -> (17, 23), 64 -> 32 (test_hip_ops.UPCONV_CASES): two 16 x 28 tiles per image, one pass"""
    (h, w), (H, W), cin, cout = (9, 12), (17, 23), 64, 32
    g = gen(912)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt, b = r(cout, cin, 3, 3) / (3 * cin ** 0.5), r(cout)
    cw = P.pack_conv(wt, b, pad=1, prec=P.L.PREC_BF16X3)

    def run(i):
        assert P.upconv3x3_supported(i["u"], H, W, cw)
        y = P.upconv3x3(i["u"], H, W, cw, act=P.ACT_RELU)
        assert last_kernel() == "upconv3x3_kernel<32,bf16x3>", last_kernel()
        return (y,)

    i, (y,) = decode_sweep(lambda n: dict(u=P.Feat(r(n, h, w, cin))), run, cdiv(H, 16) * cdiv(W, 28), "upconv3x3")
    close(y.buf, _upconv3x3_ref(i["u"], wt, b, H, W, "relu"), 2e-5, "upconv3x3")             # (test_upconv3x3_vs_fp64_upsample_then_conv)


def test_upconv3x3_pass_groups_do_not_change_the_bits(P):
    """csrc/upconv.hip spreads the 32-channel passes of a tile over cdiv(512, tiles) workgroups (at most one per pass): (13, 21) -> (26, 42), 32 -> 98
    is 4 tiles of 4 passes per image -- 3 images: every pass its own workgroup; 128 images (512 tiles): one workgroup runs all four"""
    (h, w), (H, W), cin, cout, nb = (13, 21), (26, 42), 32, 98, 128
    g = gen(1321)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt = r(cout, cin, 3, 3) / (3 * cin ** 0.5)
    cw = P.pack_conv(wt, None, pad=1, prec=P.L.PREC_BF16X3)
    u = P.Feat(r(nb, h, w, cin))
    idx = picks(nb)
    tiles, npass = cdiv(H, 16) * cdiv(W, 28), cdiv(cout, 32)
    groups = lambda n: max(1, min(npass, cdiv(512, n * tiles)))  # noqa: E731
    assert groups(len(idx)) == npass == 4 and groups(nb) == 1
    big = P.upconv3x3(u, H, W, cw, act=P.ACT_GELU)
    us = sub(u, idx)
    small = P.upconv3x3(us, H, W, cw, act=P.ACT_GELU)
    assert last_kernel() == "upconv3x3_kernel<32,bf16x3>", last_kernel()
    bits(big, small, idx, "upconv3x3: one pass group (512 tiles) vs four (12 tiles)")
    assert float(small.buf[..., cout:].abs().max()) == 0.0          # (pad channels behind cout = 96 + 2)
    close(raw(small), _upconv3x3_ref(us, wt, None, H, W, "gelu"), 2e-5, "upconv3x3 pass groups")


def test_upconv5x5_block_decode_and_ring_gemm_are_batch_independent(P):
    """(15, 20) -> (29, 39), 64 -> (32) -> 32 (test_upconv5.CASES): six 14 x 24 tiles per image.  The border ring goes through a 1x1 conv over the
    70 edge-line pixels of every image (gemm16_kernel, 896 columns): 48 images also cross its 64- / 128-column choice."""
    n5, ci, m, (uh, uw), (H, W) = 48, 64, 32, (15, 20), (29, 39)
    g = torch.Generator().manual_seed(5)
    rc = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    w1, b1, tb, w2, b2 = rc(m, ci, 3, 3) / (3 * ci ** 0.5), rc(m) * 0.2, rc(9, m) * 0.1, rc(32, m, 3, 3) / (3 * m ** 0.5), rc(32) * 0.2
    cw5 = P.compose_upconv5x5(w1, b1, tb, w2, b2, DEV, P.L.PREC_BF16X3)
    gd = gen(1520)
    lines = 2 * uw + 2 * uh
    ring_width = lambda n: 64 if cdiv(n * lines, 128) * cdiv(28 * 32, 128) <= 160 else 128  # noqa: E731  (launch_gemm16)

    def run(i):
        assert P.upconv5x5_supported(i["u"], H, W, cw5)
        y = P.upconv5x5(i["u"], H, W, cw5, act=P.ACT_RELU)
        assert last_kernel() == f"gemm16_kernel<{ring_width(i['u'].n)},bf16x3>", last_kernel()   # (the ring's GEMM is the op's last matrix kernel)
        return (y,)

    make = lambda n: dict(u=P.Feat(torch.randn(n, uh, uw, ci, device=DEV, generator=gd)))  # noqa: E731
    i, (y,) = decode_sweep(make, run, cdiv(H, 14) * cdiv(W, 24), "upconv5x5")
    u48 = make(n5)
    assert ring_width(n5) == 128 and ring_width(3) == 64
    big, idx = run(u48)[0], picks(n5)
    bits(big, run({"u": sub(u48["u"], idx)})[0], idx, "upconv5x5: ring GEMM on 128-column tiles (48 images) vs 64-column tiles")
    U = F.interpolate(d64(i["u"]).permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True)      # (test_upconv5.reference)
    t = F.conv2d(U, w1.double(), b1.double(), padding=1) + F.conv2d(torch.ones(1, 1, H, W, dtype=torch.float64), tb.double().t().reshape(m, 1, 3, 3), padding=1)
    close(y.buf, torch.relu(F.conv2d(t, w2.double(), b2.double(), padding=1)).permute(0, 2, 3, 1), 3e-5, "upconv5x5")


def test_conv2d_tail_block_decode_is_batch_independent(P):
    """conv + LayerNorm + GELU that closes the row with [pred1 | pred2 | 0 | 0] (test_conv2d_tail_equals_conv_then_depth_pair_fill): 40 x 66, 64 -> 32,
    a 2-column strip; the whole row -- tail channels included -- must not depend on the batch"""
    H, W, cin, cout, ph, pw = 40, 66, 64, 32, 14, 18
    g = gen(4066)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt = r(cout, cin, 3, 3) / (3 * cin ** 0.5)
    cw = P.pack_conv(wt, None, pad=1, prec=P.L.PREC_BF16X3)
    ln = (torch.rand(cout, device=DEV, generator=g) + 0.5, r(cout) * 0.1)

    def run(i):
        buf = P.Feat.alloc_raw(i["x"].n, H, W, cout + 2, DEV)
        buf.buf.fill_(float("nan"))
        dst = buf.slice(0, cout)
        assert P.conv2d_tail_supported(i["x"], cw, dst)
        P.conv2d_tail(i["x"], cw, dst, i["p1"], i["p2"], act=P.ACT_GELU, ln=ln)
        assert last_kernel() == "conv3x3_halo16_kernel<32,bf16x3>", last_kernel()
        return (buf.buf,)

    make = lambda n: dict(x=P.Feat(r(n, H, W, cin)), p1=P.Feat(r(n, ph, pw, 1).abs()), p2=P.Feat(r(n, ph, pw, 1).abs()))  # noqa: E731
    i, (row,) = decode_sweep(make, run, halo16_blocks(H, W, cout), "conv2d_tail")
    assert bool(torch.isfinite(row).all())
    close(row[..., :cout], F.gelu(ln64(conv64(d64(i["x"]), wt), ln[0], ln[1])), 3e-5, "conv2d_tail")


def test_conv2d_pre_block_decode_is_batch_independent(P):
    """17 x 29, 256 -> 128 with the pre-LayerNorm addend (test_conv2d_pre_addend_in_front_of_the_epilogue): three tiles per image"""
    h, w, cin, cout = 17, 29, 256, 128
    g = gen(1729)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    wt, b = r(cout, cin, 3, 3) / (3 * cin ** 0.5), r(cout) * 0.1
    ln = (torch.rand(cout, device=DEV, generator=g) + 0.5, r(cout) * 0.1)
    cw = P.pack_conv(wt, b, pad=1, prec=P.L.PREC_BF16X3)
    assert P.conv2d_pre_supported(h, w, cw, True)

    def run(i):
        y = P.conv2d_pre(i["x"], cw, i["pre"], act=P.ACT_GELU, ln=ln)
        assert last_kernel() == "conv3x3_halo16_kernel<128,bf16x3>", last_kernel()
        return (y,)

    i, (y,) = decode_sweep(lambda n: dict(x=P.Feat(r(n, h, w, cin)), pre=P.Feat(r(n, h, w, cout))), run, halo16_blocks(h, w, cout), "conv2d_pre")
    close(y.buf, F.gelu(ln64(conv64(d64(i["x"]), wt, b) + d64(i["pre"]), ln[0], ln[1])), 3e-5, "conv2d_pre")


# ---- f. attention ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [37, 259])
@pytest.mark.parametrize("variant", ["f32", "f32-bias", "bf16x3", "bf16x3-image", "qkv_ss", "qkv_ss-image"])
def test_attention_is_batch_independent(P, variant, N):
    """B = 3 against every image alone, fp32 output rows.  An odd token count puts image 1 on an odd global row: the swizzle key of the
    split-swizzled OPERAND rows (qkv_ss) depends on that.  Split-swizzled OUTPUTS (out_ss=True) are left out: their bytes are a function of the
    global row by design, so a batch's rows are not the rows of its images alone.  The packed bias image exists for the bf16 modes only; the f32
    kernel takes the same bias as rows."""
    B, H = 3, 2
    D = H * 64
    g = gen(N)
    kind, _, with_bias = variant.partition("-")
    ld = cdiv(N, 64) * 64
    rows = torch.zeros(H, N, ld, device=DEV)
    rows[:, :, :N] = torch.randn(H, N, N, device=DEV, generator=g) * 2.0
    bias = None if not with_bias else (rows if kind == "f32" else P.pack_attention_bias(rows, N))
    if kind == "qkv_ss":
        x = torch.randn(B * N, D, device=DEV, generator=g)
        cw = P.pack_conv(torch.randn(3 * D, D, device=DEV, generator=g) / D ** 0.5, torch.randn(3 * D, device=DEV, generator=g) * 0.1, prec=P.L.PREC_BF16X3)
        qkv = P.gemm_ss(P.split_ss(x), cw)                           # fp32 rows of the same Linear: the float64 anchor's input
        run = lambda r0, r1: P.attention_qkv_ss(P.gemm_ss_qkv(P.split_ss(x[r0:r1].contiguous()), cw, H), (r1 - r0) // N, N, H, bias=bias, out_ss=False)  # noqa: E731
    else:
        qkv = torch.randn(B * N, 3 * D, device=DEV, generator=g)
        run = lambda r0, r1: P.attention(qkv[r0:r1].contiguous(), (r1 - r0) // N, N, H, P.L.PREC_NAMES[kind], bias=bias)  # noqa: E731
    whole = run(0, B * N)
    for i in range(B):
        alone = run(i * N, (i + 1) * N)
        d = whole[i * N:(i + 1) * N] != alone
        assert not bool(d.any()), f"attention {variant} N = {N}: image {i} of {B} vs alone: {int(d.sum())} elements differ, max |d| = {float((whole[i * N:(i + 1) * N] - alone).abs().max()):.3e}"
    q, k, v = (t.permute(0, 2, 1, 3) for t in d64(qkv[:N]).view(1, N, 3, H, 64).unbind(2))
    sc = q @ k.transpose(-1, -2) * 0.125 + (d64(rows)[None, :, :, :N] if with_bias else 0)
    want = (sc.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(N, D)
    got = run(0, N)
    if kind == "qkv_ss":  # (test_attention_on_split_swizzled_qkv_is_bit_equal_to_the_pre_pass_path)
        assert float((got.double().cpu() - want).abs().max()) < 2e-4 * max(1.0, float(want.abs().max()))
    else:                 # (test_attention_score_bias_rows_and_packed_image with a bias, test_attention without)
        close(got, want, {("f32", ""): 1e-5, ("bf16x3", ""): 4e-5, ("f32", "bias"): 2e-6, ("bf16x3", "image"): 2e-5}[(kind, with_bias)], f"attention {variant}")
