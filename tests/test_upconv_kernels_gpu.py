"""GPU parity of the kernels that compute a conv over a bilinear(align_corners=True) upsample without forming the upsampled tensor --
upconv3x3_kernel (csrc/upconv.hip), upconv5x5_kernel with its _lines / _ring helpers (csrc/upconv5.hip) and the UPS loader of
conv3x3_halo16_ups_kernel (csrc/conv3x3_m16.hip) -- against plain torch in float64 on the CPU, at the smallest shapes that reach the
edges of their tile geometry: the full 11 x 17 source footprint of an upconv3x3 tile on both tile shapes (the last MFMA run of the waves
with mslot == 3, the last G-tile row, the column walk's deepest column), the 11 x 16 footprint of upconv5x5, the mixed side of the
``wide`` predicate, sources of one row / column / pixel, cout below one pass, sliced operands, conv2d_ups at and above a source step
of 1 and with a fused LayerNorm.  The references share nothing with the kernels' tap arithmetic: F.interpolate and F.conv2d in float64,
LayerNorm / activation / addend / residual written out.  The tables and the reference side need no GPU and no library:
tests/test_upconv_kernels_host.py checks them (the footprint every row claims against a float32 restatement of ac_tap and of the tile
choice, the 11 x 17 bound itself over every admitted size pair, the shape contracts, the float32 oracle's share of every tolerance, the
error of the bf16 emulation, discrimination).

Inputs go into ``Feat`` buffers and results come out of ``feat.buf`` with plain torch indexing.  A destination the test hands to an op is
NaN where the op must write (the in-place addend rows: the addend) and holds a sentinel in every other channel; a source read as a
channel slice has NaN in every channel outside the slice.  Every comparison prints ``err / tol`` before it asserts; the criterion is the
project's ``close``: max|got - ref| <= tol * max(1, max|ref|).

bf16 mode of upconv3x3 has two bars.  Against float64: four times the error of the EMULATION -- the same float64 graph on
u.to(bfloat16) and w.to(bfloat16), round to nearest even, which is what the footprint loader keeps (the hi plane) and what
pack_weight_kernel stores -- and never above the 6e-3 the op already had (the emulation sits 0.9e-3 .. 2.5e-3 of the scale from float64 on
these rows, so the cap is the bar wherever that distance exceeds 1.5e-3).  Against the emulation itself: 2e-5, the bf16x3 bar, because the
kernel then differs from it only by fp32 accumulation and fp32 interpolation weights, both of which that bar already absorbs.  On the
device the kernel stays within a fifth of that bar (most at steps that float32 does not hold exactly), so the emulation is the rule it follows.

No row of this file found a kernel wrong.  What the tables did find is about the earlier shapes: at a source step of exactly 1/2 (every
2 h - 1 size, the pyramid's included) a whole 16 x 28 tile stages and reads footprint row 10 and column 16 with an interpolation weight of
0, so a wrong value there cannot show; the ``carried`` rows have steps just under 1/2, where those weigh 0.2.  With the loader changed to
hand the kernel row 9 for row 10, or column 15 for column 16, every earlier test of the op still passed; the carried rows do not."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -7.5                 # what every channel beside a destination slice holds before and after
PRECS = ["bf16x3", "bf16"]
LN_EPS = 1e-6


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def roundup(a, b):
    return (a + b - 1) // b * b


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))


def relerr(a, ref):
    """max|a - ref| in units of the reference's scale max(1, max|ref|)"""
    return float((a.double() - ref.double()).abs().max()) / scale_of(ref)


def close(got, ref, tol, what, mask=None):
    """max|got - ref| <= tol * max(1, max|ref|) (over ``mask``), the output finite; prints and returns the share of the tolerance used"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    d = (got - ref.double()).abs()
    err, lim = float((d if mask is None else d[mask]).max()), tol * scale_of(ref)
    print(f"[upconv] {what}: err {err:.3e} tol {lim:.3e} ratio {err / lim:.3f}")
    assert err <= lim, f"{what}: max|d| = {err:.3e} > {lim:.3e}"
    return err / lim


def src_feat(P, x, c0, ld, fill=NAN):
    """x [n, c, h, w] as the channels [c0, c0 + c) of a fresh ld-channel NHWC buffer that holds ``fill`` elsewhere"""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), fill)
    buf[..., c0:c0 + c] = x.permute(0, 2, 3, 1)
    return P.Feat(buf.to(DEV)).slice(c0, c)


def dst_feat(P, n, h, w, c, c0, ld, init=None):
    """a destination: NaN (or ``init`` [n, c, h, w], the in-place addend) in the channels [c0, c0 + c), SENT in every other one"""
    buf = torch.full((n, h, w, ld), SENT)
    buf[..., c0:c0 + c] = NAN if init is None else init.permute(0, 2, 3, 1)
    return P.Feat(buf.to(DEV)).slice(c0, c)


def read(feat):
    """-> the destination slice as [n, c, h, w] on the CPU; asserts that its neighbours still hold SENT"""
    got = feat.buf.cpu()
    rest = torch.cat([got[..., :feat.c0], got[..., feat.c0 + feat.c:]], -1)
    assert bool((rest == SENT).all()), "channels beside the destination slice were written"
    return got[..., feat.c0:feat.c0 + feat.c].permute(0, 3, 1, 2).contiguous()


def last_kernel(P):
    return P.L.load().prv2_last_kernel().decode()


def up64(u, size, align_corners=True):
    return F.interpolate(u, size, mode="bilinear", align_corners=align_corners)


def up_steps(u, size, sy, sx):
    """bilinear interpolation at the source positions (y sy, x sx), clamped at the last row / column: align_corners=True when (sy, sx) are
    the axes' own steps (h - 1) / (H - 1), (w - 1) / (W - 1) -- handed the two SWAPPED it is the deliberately wrong variant of the mixed-step rows"""
    def taps(n_out, s, n_in):
        src = torch.arange(n_out, dtype=u.dtype) * s
        i0 = src.floor().long().clamp(max=n_in - 1)
        return i0, (i0 + 1).clamp(max=n_in - 1), src - i0
    y0, y1, wy = taps(size[0], sy, u.shape[2])
    x0, x1, wx = taps(size[1], sx, u.shape[3])
    rows = u[:, :, y0] * (1 - wy).view(-1, 1) + u[:, :, y1] * wy.view(-1, 1)
    return rows[..., x0] * (1 - wx) + rows[..., x1] * wx


ACTS = dict(none=lambda v: v, relu=torch.relu, gelu=F.gelu)


def act_id(P, act):
    return dict(none=P.ACT_NONE, relu=P.ACT_RELU, gelu=P.ACT_GELU)[act]


# ---- a. upconv3x3 ------------------------------------------------------------------------------------------------------------------------
# prv2_upconv3x3: 16 x 28 output tiles when both source steps fl((h - 1) / (H - 1)), fl((w - 1) / (W - 1)) are <= 0.5f, else 14 x 24 (steps up
# to 0.6f); a tile stages LR x LC = 11 x 17 source pixels.  ``foot`` = the largest (rows, columns) any tile of the row needs, which the
# host file recomputes.  Layout keys: u_slice -- u is the channels [32, 32 + cin) of a buffer 64 channels wider; out_c0 -- the first
# channel of the destination in its buffer; add -- "sep": a separate addend, the channels [4, 4 + cout) of a wider buffer (ld_add > cout),
# "inplace": add is out, as fusion.py calls it (bias=False).  ``carried``: some output of the tile that has the full footprint gives its LAST
# source row and its last source column an interpolation weight of at least 0.15 (the host file computes the weights).  At a step of
# exactly 1/2 -- (18, 30) -> (35, 59), every 2 h - 1 level of the pyramid -- a whole 16 x 28 tile stages and reads footprint row 10 and
# column 16 with weight 0: such a row shows a NaN there, not a wrong value, which is why the table has "carried-16x28" beside them
def A(id, n, hw, HW, cin, cout, act, bias, tile, foot, u_slice=False, out_c0=0, add=None, carried=False):
    return dict(id=id, n=n, hw=hw, HW=HW, cin=cin, cout=cout, act=act, bias=bias, tile=tile, foot=foot, u_slice=u_slice, out_c0=out_c0, add=add,
                carried=carried)


T0, T1 = (16, 28), (14, 24)
UPC_ROWS = [
    # the full footprint, 11 x 17 in ONE tile (tile row 1, tile column 1), on the 16 x 28 tile: one slab, then three (the other stage parity)
    A("full-16x28-1slab", 1, (18, 30), (35, 59), 32, 64, "none", True, T0, (11, 17)),
    A("full-16x28-3slabs", 1, (18, 30), (35, 59), 96, 32, "gelu", False, T0, (11, 17)),
    # ... with steps just under 1/2 (29/60, 52/106): the last footprint row and column weigh 0.2 in tile (2, 2); two slabs
    A("carried-16x28", 1, (30, 53), (61, 107), 64, 32, "none", True, T0, (11, 17), carried=True),
    # ... on the 14 x 24 tile (steps 17/29, 29/49); cout 98 = three passes + a partial channel quad in the fourth
    A("full-14x24-cout98", 1, (18, 30), (30, 50), 64, 98, "gelu", True, T1, (11, 17), carried=True),
    # the pyramid level of the workload that reaches 11 x 17; two images, four passes
    A("pyramid-25x33", 2, (25, 33), (49, 65), 64, 128, "none", True, T0, (11, 17)),
    # one axis at a step <= 1/2 (9/19), the other above (29/49): the mixed side of ``wide`` -> the 14 x 24 tile
    A("mixed-rows-fine", 1, (10, 30), (20, 50), 32, 32, "relu", False, T1, (8, 17)),
    A("mixed-cols-fine", 1, (30, 10), (50, 20), 32, 32, "relu", False, T1, (11, 10)),
    # a source of one row, one column, one pixel: step 0, every tap has i1 == i0
    A("source-1x3", 1, (1, 3), (2, 6), 32, 32, "none", True, T0, (1, 3)),
    A("source-3x1", 1, (3, 1), (6, 2), 32, 32, "none", True, T0, (3, 1)),
    A("source-1x1", 2, (1, 1), (2, 2), 32, 32, "gelu", True, T0, (1, 1)),
    # cout below one pass: most channel quads of the single pass are invalid (nvalid == 0), cout 20 ends on a whole quad, 2 x 2 ragged tiles
    A("cout8", 1, (9, 15), (17, 29), 32, 8, "none", True, T0, (9, 15)),
    A("cout20", 1, (9, 15), (17, 29), 32, 20, "gelu", False, T0, (9, 15)),
    # layouts, on the full-footprint shape of either tile
    A("u-slice-16x28", 1, (18, 30), (35, 59), 64, 40, "none", True, T0, (11, 17), u_slice=True),
    A("out-slice-16x28", 1, (18, 30), (35, 59), 64, 40, "relu", True, T0, (11, 17), out_c0=8),
    A("add-slice-16x28", 1, (18, 30), (35, 59), 64, 40, "gelu", True, T0, (11, 17), add="sep"),
    A("add-inplace-16x28", 1, (18, 30), (35, 59), 64, 40, "gelu", False, T0, (11, 17), add="inplace"),
    A("u-slice-14x24", 1, (18, 30), (30, 50), 64, 40, "none", True, T1, (11, 17), u_slice=True, carried=True),
    A("out-slice-14x24", 1, (18, 30), (30, 50), 64, 40, "relu", True, T1, (11, 17), out_c0=8, carried=True),
    A("add-slice-14x24", 1, (18, 30), (30, 50), 64, 40, "gelu", True, T1, (11, 17), add="sep", carried=True),
    A("add-inplace-14x24", 1, (18, 30), (30, 50), 64, 40, "gelu", False, T1, (11, 17), add="inplace", carried=True),
]
UPC_BY_ID = {r["id"]: r for r in UPC_ROWS}
UPC_TOL_X3 = 2e-5           # the op's bf16x3 bar; in bf16 mode the bar against the emulation
UPC_TOL_BF16_CAP = 6e-3     # the op's bf16 bar against float64 before this file; the derived one never exceeds it


def upc_inputs(row):
    """-> (u [n, cin, h, w], w [cout, cin, 3, 3], bias [cout] or None, addend [n, cout, H, W] or None)"""
    i = UPC_ROWS.index(UPC_BY_ID[row["id"]])
    n, cin, cout = row["n"], row["cin"], row["cout"]
    return (rnd(1000 + i, n, cin, *row["hw"]), rnd(1100 + i, cout, cin, 3, 3) / (9 * cin) ** 0.5, rnd(1200 + i, cout) if row["bias"] else None,
            rnd(1300 + i, n, cout, *row["HW"]) if row["add"] else None)


def upc_graph(row, u, w, b, add, dtype=torch.float64, up=up64):
    """act(conv3x3(up(u); w) + b + add) in ``dtype``; u and w may arrive as bfloat16 (the emulation): their conversion is exact"""
    y = F.conv2d(up(u.to(dtype), row["HW"]), w.to(dtype), None if b is None else b.to(dtype), padding=1)
    return ACTS[row["act"]](y if add is None else y + add.to(dtype))


@functools.lru_cache(maxsize=None)
def _upc_ref(rid):
    row = UPC_BY_ID[rid]
    u, w, b, add = upc_inputs(row)
    ref = upc_graph(row, u, w, b, add)
    emu = upc_graph(row, u.bfloat16(), w.bfloat16(), b, add)
    return ref, emu, relerr(emu, ref)


def upc_ref(row):
    """-> (float64 reference, float64 emulation of bf16 mode, the emulation's error in units of the reference's scale); computed once"""
    return _upc_ref(row["id"])


def upc_tol_bf16(row):
    """bf16 mode against float64: four times the emulation's own distance from float64, capped at the op's earlier bar"""
    return min(4.0 * upc_ref(row)[2], UPC_TOL_BF16_CAP)


def upc_layout(row):
    """-> (c0 of u, ld of u, c0 of out, ld of out, c0 of the addend, ld of the addend): whole buffers are 4 channels wider than the
    padded channel count, so that something beside the destination holds the sentinel in every row"""
    cin, cout = row["cin"], row["cout"]
    c0u, ldu = (32, cin + 64) if row["u_slice"] else (0, cin)
    return c0u, ldu, row["out_c0"], row["out_c0"] + roundup(cout, 4) + (8 if row["out_c0"] else 4), 4, roundup(cout, 4) + 8


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("row", UPC_ROWS, ids=lambda r: r["id"])
def test_upconv3x3(P, row, prec):
    n, (H, W), cout = row["n"], row["HW"], row["cout"]
    u_t, w_t, b_t, add_t = upc_inputs(row)
    c0u, ldu, c0o, ldo, c0a, lda = upc_layout(row)
    cw = P.pack_conv(w_t.to(DEV), b_t.to(DEV) if b_t is not None else None, pad=1, prec=P.L.PREC_NAMES[prec])
    u = src_feat(P, u_t, c0u, ldu)
    out = dst_feat(P, n, H, W, cout, c0o, ldo, init=add_t if row["add"] == "inplace" else None)
    add = out if row["add"] == "inplace" else src_feat(P, add_t, c0a, lda) if row["add"] == "sep" else None
    assert P.upconv3x3_supported(u, H, W, cw)
    P.upconv3x3(u, H, W, cw, out=out, act=act_id(P, row["act"]), bias=row["bias"], add=add)
    assert last_kernel(P) == f"upconv3x3_kernel<32,{prec}>"
    got = read(out)
    ref, emu, emu_err = upc_ref(row)
    what = f"a upconv3x3 {row['id']} {prec}"
    if prec == "bf16x3":
        close(got, ref, UPC_TOL_X3, what)
    else:
        print(f"[upconv] {what}: emulation's own error {emu_err:.3e} of the scale")
        close(got, emu, UPC_TOL_X3, what + " vs emulation")
        close(got, ref, upc_tol_bf16(row), what + " vs float64")


# ---- b. upconv5x5 with _lines and _ring ------------------------------------------------------------------------------------------------------
# prv2_upconv5x5: 14 x 24 output tiles with a two-pixel halo, source steps <= 0.5f, h, w >= 5, u.h, u.w >= 2, cout <= 32 and % 4 == 0.
# (id, n, ci, m, co, (uh, uw), (H, W), foot, options): tap_bias / b2 False = None; u_slice / out_c0 / carried as in group a
def B(id, n, ci, m, co, uhw, HW, foot, tap_bias=True, b2=True, u_slice=False, out_c0=0, carried=False):
    return dict(id=id, n=n, ci=ci, m=m, co=co, uhw=uhw, HW=HW, foot=foot, tap_bias=tap_bias, b2=b2, u_slice=u_slice, out_c0=out_c0, carried=carried)


UP5_ROWS = [
    B("full-11x16", 1, 32, 32, 32, (16, 26), (32, 52), (11, 16)),       # 11 rows and 16 columns in one tile (the last ones weigh 0.03 and 0.02)
    B("carried-11x16", 1, 32, 32, 32, (25, 42), (50, 84), (11, 16), carried=True),      # ... weighing 0.2 (as ``carried`` of group a)
    B("min-2x2", 2, 32, 32, 32, (2, 2), (5, 5), (2, 2)),                # the contract's minimum: the ring is 16 of 25 pixels, all corners meet
    B("min-3x4", 1, 32, 32, 32, (3, 4), (5, 7), (3, 4)),
    B("x4", 1, 64, 32, 32, (5, 6), (20, 24), (5, 6)),                   # source step about 1/4
    B("not-x2", 1, 32, 32, 32, (9, 14), (19, 29), (8, 13)),
    B("cout4", 1, 32, 32, 4, (7, 13), (14, 26), (7, 13)),
    B("cout20", 1, 32, 32, 20, (7, 13), (14, 26), (7, 13)),
    B("cin96", 1, 96, 32, 32, (7, 13), (14, 26), (7, 13)),              # three slabs
    B("no-tap-bias", 1, 32, 32, 32, (7, 13), (14, 26), (7, 13), tap_bias=False),
    B("no-b2", 1, 32, 32, 32, (7, 13), (14, 26), (7, 13), b2=False),
    B("u-slice", 1, 32, 32, 32, (16, 26), (32, 52), (11, 16), u_slice=True),
    B("out-slice", 1, 32, 32, 20, (16, 26), (32, 52), (11, 16), out_c0=8),
]
UP5_BY_ID = {r["id"]: r for r in UP5_ROWS}
UP5_TOL = {"bf16x3": 3e-5, "bf16": 3e-2}     # the op's own bars (tests/test_upconv5.py)


def up5_inputs(row):
    """-> (u, w1 [m, ci, 3, 3], b1 [m], tap_bias [9, m] or None, w2 [co, m, 3, 3], b2 [co] or None), scaled as tests/test_upconv5.py scales them"""
    i = UP5_ROWS.index(UP5_BY_ID[row["id"]])
    n, ci, m, co = row["n"], row["ci"], row["m"], row["co"]
    return (rnd(2000 + i, n, ci, *row["uhw"]), rnd(2100 + i, m, ci, 3, 3) / (3 * ci ** 0.5), rnd(2200 + i, m) * 0.2,
            rnd(2300 + i, 9, m) * 0.1 if row["tap_bias"] else None, rnd(2400 + i, co, m, 3, 3) / (3 * m ** 0.5), rnd(2500 + i, co) * 0.2 if row["b2"] else None)


def up5_graph(u, w1, b1, tap_bias, w2, b2, size, dtype=torch.float64, up=up64):
    """the ``reference()`` of tests/test_upconv5.py with the two optional terms:
    relu(conv3x3(conv3x3(up(u); w1) + b1 + [taps of w1 inside the image] tap_bias; w2) + b2)"""
    d = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    m = w1.shape[0]
    t = F.conv2d(up(d(u), size), d(w1), d(b1), padding=1)
    if tap_bias is not None:
        t = t + F.conv2d(torch.ones(1, 1, *size, dtype=dtype), d(tap_bias).t().reshape(m, 1, 3, 3), padding=1)
    return F.relu(F.conv2d(t, d(w2), d(b2), padding=1))


@functools.lru_cache(maxsize=None)
def _up5_ref(rid):
    row = UP5_BY_ID[rid]
    return up5_graph(*up5_inputs(row), row["HW"])


def up5_ref(row):
    return _up5_ref(row["id"])


def up5_layout(row):
    """-> (c0 of u, ld of u, c0 of out, ld of out)"""
    c0u, ldu = (32, row["ci"] + 64) if row["u_slice"] else (0, row["ci"])
    return c0u, ldu, row["out_c0"], row["out_c0"] + row["co"] + (8 if row["out_c0"] else 4)


def ring_mask(ref):
    ring = torch.zeros_like(ref, dtype=torch.bool)
    ring[..., 0, :] = ring[..., -1, :] = ring[..., :, 0] = ring[..., :, -1] = True
    return ring


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("row", UP5_ROWS, ids=lambda r: r["id"])
def test_upconv5x5(P, row, prec, monkeypatch):
    n, (H, W), co = row["n"], row["HW"], row["co"]
    u_t, w1, b1, tb, w2, b2 = up5_inputs(row)
    c0u, ldu, c0o, ldo = up5_layout(row)
    cw5 = P.compose_upconv5x5(w1, b1, tb, w2, b2, DEV, P.L.PREC_NAMES[prec])
    u = src_feat(P, u_t, c0u, ldu)
    out = dst_feat(P, n, H, W, co, c0o, ldo)
    assert P.upconv5x5_supported(u, H, W, cw5)
    names, ring_fix = [], P._upconv5x5_ring

    def ring_after_main(*a):      # the main kernel's name, before the ring fix launches its own (the lines' 1x1 conv)
        names.append(last_kernel(P))
        return ring_fix(*a)
    monkeypatch.setattr(P, "_upconv5x5_ring", ring_after_main)
    P.upconv5x5(u, H, W, cw5, out=out, act=P.ACT_RELU)
    assert names == [f"upconv5x5_kernel<32,{prec}>"]
    got, ref = read(out), up5_ref(row)
    ring = ring_mask(ref)
    close(got, ref, UP5_TOL[prec], f"b upconv5x5 {row['id']} {prec} interior", ~ring)
    close(got, ref, UP5_TOL[prec], f"b upconv5x5 {row['id']} {prec} ring", ring)


# ---- c. conv2d_ups -----------------------------------------------------------------------------------------------------------------------
# prv2_conv2d_ups: the 8 x 32-pixel halo kernel (3x3 s1 p1, bf16 modes, width >= 24, height >= 4) with cout > 64, source channels % 32 == 0
# and <= cin, no limit on the source step.  The first c1 input channels are interpolated from u, the rest come from the concat buffer x
# (c1 == cin: there is no x).  ln: a channels-first LayerNorm between the bias and the activation (fused: cout <= 128); res: added last
def C(id, n, hw, HW, c1, cin, cout, act="gelu", ln=False, res=False, u_slice=False, out_c0=0, raises=False):
    return dict(id=id, n=n, hw=hw, HW=HW, c1=c1, cin=cin, cout=cout, act=act, ln=ln, res=res, u_slice=u_slice, out_c0=out_c0, raises=raises)


UPS_ROWS = [
    C("step-1", 1, (24, 32), (24, 32), 64, 98, 98, res=True),           # u of the output's size: every tap sits on a source pixel
    C("step-2", 1, (48, 64), (24, 32), 32, 66, 98, res=True),           # down-sampling: the four taps of neighbouring outputs share nothing
    C("source-1-row", 1, (1, 16), (8, 32), 32, 34, 98, act="none"),
    C("source-1-col", 1, (12, 1), (24, 32), 32, 32, 96, act="relu"),    # every input channel is interpolated (UpsOnly)
    C("ln-cout128-strip", 1, (12, 35), (24, 70), 64, 98, 128, ln=True),  # width 70 = 2 x 32 + a remainder strip of 6
    C("ln-cout98", 2, (12, 16), (24, 32), 32, 66, 98, ln=True),
    C("u-slice", 1, (10, 17), (20, 33), 64, 98, 98, res=True, u_slice=True),
    C("out-slice", 1, (10, 17), (20, 33), 64, 98, 98, ln=True, out_c0=8),
    C("ln-cout194-rejected", 1, (12, 16), (24, 32), 32, 66, 194, ln=True, raises=True),   # "fused LayerNorm needs cout <= 128"
]
UPS_BY_ID = {r["id"]: r for r in UPS_ROWS}
UPS_TOL = {"bf16x3": 3e-5, "bf16": 2e-2}     # the op's own bars (tests/test_hip_ops.py)


def ups_inputs(row):
    """-> (u [n, c1, h, w], rest [n, cin - c1, H, W] or None, w, bias, (ln weight, ln bias) or None, res or None)"""
    i = UPS_ROWS.index(UPS_BY_ID[row["id"]])
    n, c1, cin, cout, HW = row["n"], row["c1"], row["cin"], row["cout"], row["HW"]
    return (rnd(3000 + i, n, c1, *row["hw"]), rnd(3100 + i, n, cin - c1, *HW) if cin > c1 else None, rnd(3200 + i, cout, cin, 3, 3) / (9 * cin) ** 0.5,
            rnd(3300 + i, cout), (rnd(3400 + i, cout).abs() + 0.5, rnd(3500 + i, cout)) if row["ln"] else None, rnd(3600 + i, n, cout, *HW) if row["res"] else None)


def ups_graph(row, u, rest, w, b, ln, res, dtype=torch.float64, up=up64):
    """act(LayerNorm?(conv3x3([up(u) | rest]; w) + b)) + res in ``dtype``"""
    x = up(u.to(dtype), row["HW"])
    y = F.conv2d(x if rest is None else torch.cat([x, rest.to(dtype)], 1), w.to(dtype), b.to(dtype), padding=1)
    if ln is not None:
        mean = y.mean(1, keepdim=True)
        var = (y - mean).pow(2).mean(1, keepdim=True)
        y = (y - mean) / torch.sqrt(var + LN_EPS) * ln[0].to(dtype).view(1, -1, 1, 1) + ln[1].to(dtype).view(1, -1, 1, 1)
    y = ACTS[row["act"]](y)
    return y if res is None else y + res.to(dtype)


@functools.lru_cache(maxsize=None)
def _ups_ref(rid):
    row = UPS_BY_ID[rid]
    return ups_graph(row, *ups_inputs(row))


def ups_ref(row):
    return _ups_ref(row["id"])


def ups_layout(row):
    """-> (c0 of u, ld of u, c0 of out, ld of out)"""
    c0u, ldu = (32, row["c1"] + 64) if row["u_slice"] else (0, row["c1"])
    return c0u, ldu, row["out_c0"], row["out_c0"] + roundup(row["cout"], 4) + (8 if row["out_c0"] else 4)


def ups_operands(P, row, prec):
    n, (H, W), c1, cin, cout = row["n"], row["HW"], row["c1"], row["cin"], row["cout"]
    u_t, rest, w_t, b_t, ln, res_t = ups_inputs(row)
    c0u, ldu, c0o, ldo = ups_layout(row)
    cw = P.pack_conv(w_t.to(DEV), b_t.to(DEV), pad=1, prec=P.L.PREC_NAMES[prec])
    u = src_feat(P, u_t, c0u, ldu)

    def concat():      # [NaN: where up(u) would go | rest | zero pad channels]
        buf = torch.zeros(n, H, W, roundup(cin, 4))
        buf[..., :c1] = NAN
        if rest is not None:
            buf[..., c1:cin] = rest.permute(0, 2, 3, 1)
        return P.Feat(buf.to(DEV), cin)
    kw = dict(act=act_id(P, row["act"]), ln=tuple(t.to(DEV) for t in ln) if ln else None,
              res=src_feat(P, res_t, 0, roundup(cout, 4), fill=0.0) if res_t is not None else None)
    return cw, u, concat, (lambda: dst_feat(P, n, H, W, cout, c0o, ldo)), kw


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("row", [r for r in UPS_ROWS if not r["raises"]], ids=lambda r: r["id"])
def test_conv2d_ups(P, row, prec):
    """the fused loader == upsample_bilinear into the concat buffer + conv2d, bit for bit, without reading the buffer's first c1 channels;
    and the pair against float64 at the op's bars"""
    (H, W), c1, cin = row["HW"], row["c1"], row["cin"]
    cw, u, concat, dst, kw = ups_operands(P, row, prec)
    xr, want = concat(), dst()
    P.upsample_bilinear(u, H, W, out=xr.slice(0, c1))
    P.conv2d(xr, cw, want, **kw)
    assert "ups" not in last_kernel(P)
    x, out = concat() if cin > c1 else P.UpsOnly(u, H, W), dst()
    lib = P.L.load()
    assert lib.prv2_conv2d_ups_supported(ctypes.byref(P._conv_desc(x, cw, out.ld)), ctypes.byref(P._ups_src(u)))
    P.conv2d_ups(x, u, cw, out, **kw)
    assert "ups" in last_kernel(P)
    got = read(out)
    close(got, ups_ref(row), UPS_TOL[prec], f"c conv2d_ups {row['id']} {prec}")
    assert torch.equal(got, read(want)), float((got - read(want)).abs().max())


@pytest.mark.parametrize("row", [r for r in UPS_ROWS if r["raises"]], ids=lambda r: r["id"])
def test_conv2d_ups_rejects(P, row):
    cw, u, concat, dst, kw = ups_operands(P, row, "bf16x3")
    out = dst()
    with pytest.raises(RuntimeError, match="fused LayerNorm needs cout <= 128"):
        P.conv2d_ups(concat(), u, cw, out, **kw)
    assert bool(torch.isnan(read(out)).all()), "a rejected call wrote its destination"
