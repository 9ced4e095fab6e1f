"""CPU side of tests/test_halo_conv_gpu.py: its tables, float64 references and data are sound before any kernel runs.  Nothing here loads the library.

* the kernel string every row expects per mode, against a restatement of the dispatch rules: conv3x3_halo_supported / conv3x3_halo16_usable
  (csrc/conv3x3.hip), the c256 rung's refusal of gamma / mul / res2 (conv_goes_c256), conv_plan's strip rule and ConvStrip::SECOND_LAUNCH naming
  the generic kernel in f32 mode (csrc/igemm.hip), has_tail_tile (csrc/igemm.h), the tile-width rule of launch_conv3x3_halo / _halo16;
* the edges the tables claim, as assertions: cchunks parities per tile width, main / strip tile counts mod 8, jv per wave half for every cout
  (the jv == 0 half included), the store path (16-byte or scalar) of every row, decode()'s XCD remap a permutation for every tile count;
* references finite and of the right shape; discrimination (dropping any declared operand, the last two input channels of a tail-step row, the last
  source row / column of a partial tile moves the reference by >= 100 x the row's bar); a plain float32 evaluation within 1/4 of the bar; one-pass
  LayerNorm statistics missing the bar on the offset rows;
* gelu_fast (csrc/common.h) restated in float32 numpy against float64 erf GELU on [-8, 8]: measured maximum 4.70e-7 (common.h claims 4.7e-7 for the
  device's v_rcp_f32 / v_exp_f32), below 1/20 of the 3e-5 bar;
* the bf16 emulation errors recorded in EMU, recomputed; no bar above 2e-2;
* the case counts: 3 modes x the conv2d table, 2 x the pre / tail tables, nothing skipped.

erf GELU against tanh GELU: the two differ by at most 4.7e-4 anywhere (test_gelu_variants_differ_by_what_the_rows_can_see prints it), i.e. by
at most ~16 x a 3e-5 bar at scale 1 -- no well-conditioned row can show 100 x: amplifying the difference (gamma, mul) amplifies the fp32 error of a
correct kernel by the same factor and scale with it.  The GELU rows are therefore held to the figure the functions allow: the swap moves every GELU
row by >= GELU_SWAP_MIN x its bar, so a kernel on the wrong variant fails by that factor."""
import math

import numpy as np
import pytest
import torch

import test_halo_conv_gpu as G

DISC = 100.0            # share of the bar a dropped piece must move the reference by (tests/test_gate_tail_host.py)
GELU_SWAP_MIN = 2.0     # ... and what erf -> tanh GELU must (see the head of the file)


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))


def cdiv(a, b):
    return -(-a // b)


# ---- dispatch rules, restated ---------------------------------------------------------------------------------------------------------------

def ldx_of(row):
    xs = G.opts(row)["xs"]
    return xs[1] if xs is not None else G.roundup(row.cin, 4)


def halo_supported(row):
    """conv3x3_halo_supported: 3x3 / s1 / p1 (every row), width >= 24, height >= 4, image extent below 2^31 elements"""
    return row.w >= 24 and row.h >= 4 and row.h * row.w * ldx_of(row) < 2 ** 31


def halo16_usable(row, mode):
    """conv3x3_halo16_usable: the bf16 modes, image extent below 2^29 elements (no PRV2_HALO_MFMA32)"""
    return mode != "f32" and row.h * row.w * ldx_of(row) < 2 ** 29


def has_tail_tile(row, mode):
    return mode != "f32" and row.cin > 32 and row.cin % 32 == 2


def goes_c256(row, mode):
    """conv_goes_c256 + conv3x3_c256_eligible: 256 output channels, bf16 modes, whole slabs, width >= 16 -- unless gamma / mul / res2, or an addend without LN"""
    o = G.opts(row)
    return (row.cout == 256 and mode != "f32" and row.cin >= 32 and row.cin % 32 == 0 and row.w >= 16 and not (o["gamma"] or o["mul"] or o["res2"])
            and (not o["pre"] or o["ln"]))


def strip_rem(w):
    """conv_plan: a remainder of 1..8 columns behind the 32-pixel tile columns is a strip (width >= 64)"""
    rem = w % 32
    return rem if 1 <= rem <= 8 and w >= 64 else 0


def bn_of(cout):
    return 32 if cout <= 32 else (64 if cout <= 64 else 128)


def tiles_n_of(cout):
    return cdiv(cout, 128) if cout > 64 else 1


def generic_of_strip(row):
    """conv_plan_generic on the strip's window (3x3: neither 1x1 rung): 128 columns only for wide layers with a fused LN or more than 128 tiles"""
    tiles_m = cdiv(row.n * row.h * strip_rem(row.w), 128)
    narrow = row.cout > 64 and not G.opts(row)["ln"] and tiles_m * cdiv(row.cout, 128) <= 128
    return "I128" if row.cout > 64 and not narrow else "I64"


def dispatch(row, mode):
    if goes_c256(row, mode):
        return f"conv3x3_c256_kernel<256,{mode}>"
    assert halo_supported(row)
    if row.entry != "conv2d":
        assert halo16_usable(row, mode), "conv2d_pre / conv2d_tail need the 16x16x32 halo kernels"
    if halo16_usable(row, mode):   # (with its strip, if any: ConvStrip::MERGED)
        return G.KERNEL[G.H_OF[bn_of(row.cout)]].format(mode)
    if strip_rem(row.w):           # ConvStrip::SECOND_LAUNCH: the generic kernel's launch is the last one
        return G.KERNEL[generic_of_strip(row)]
    return G.KERNEL[G.F_OF[bn_of(row.cout)]]


def main_tiles(row):
    tiles_x = row.w // 32 if strip_rem(row.w) else cdiv(row.w, 32)
    return row.n * cdiv(row.h, 8) * tiles_x * tiles_n_of(row.cout)


def strip_tiles(row):
    return row.n * cdiv(row.h, 32) * tiles_n_of(row.cout) if strip_rem(row.w) else 0


def xcd_remap(t, ntiles):
    """decode() of halo16_body / the block remap of conv3x3_halo_kernel"""
    q, r, xcd = ntiles >> 3, ntiles & 7, t & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (t >> 3)


def jv_of(cout):
    """per N-tile, per wave half: the 16-column blocks with at least one real channel (halo16_body's jv; narrow kernels: one 'half')"""
    bn = bn_of(cout)
    wn_count, nj = (2, 4) if bn == 128 else (1, bn // 16)
    return [tuple(min(nj, max(0, (cout - tn * bn - wn * (bn // wn_count) + 15) >> 4)) for wn in range(wn_count)) for tn in range(tiles_n_of(cout))]


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------

def test_tables_are_explicit_and_complete():
    assert len({r.id for r in G.ALL_ROWS}) == len(G.ALL_ROWS)
    assert all(r.n in (1, 3) and r.h <= 73 and r.w <= 73 and r.cin <= 260 for r in G.ALL_ROWS)
    assert all(r.entry == "conv2d" for r in G.CONV_ROWS) and all(r.entry == "pre" for r in G.PRE_ROWS) and all(r.entry == "tail" for r in G.TAIL_ROWS)
    # no row skipped: 3 modes x the conv2d table, 2 x the pre / tail tables
    assert len(G.CONV_CASES) == 3 * len(G.CONV_ROWS) and {m for _, m in G.CONV_CASES} == {"f32", "bf16x3", "bf16"}
    assert len(G.PRE_CASES) == 2 * len(G.PRE_ROWS) and len(G.TAIL_CASES) == 2 * len(G.TAIL_ROWS)
    assert {m for _, m in G.PRE_CASES + G.TAIL_CASES} == {"bf16x3", "bf16"}
    assert G.TOL == {"f32": 2e-5, "bf16x3": 3e-5} and G.BF16_CAP == 2e-2 and G.BF16_EMU_TOL == 3e-5 and G.GENERIC_TOL == 2e-5
    src = open(G.__file__).read()
    assert "mark.skip" not in src and "pytest.skip" not in src and "xfail" not in src and "importorskip" not in src
    for ids in (G.REPEAT_IDS, G.BATCH_IDS, G.GENERIC_IDS):
        assert all(i in G.ROW_BY_ID for i in ids) and len(ids) >= 5
    assert all(G.ROW_BY_ID[i].n == 3 for i in G.BATCH_IDS) and all(G.ROW_BY_ID[i].entry == "conv2d" for i in G.GENERIC_IDS)
    # conv2d_pre / conv2d_tail take no input ReLU, gamma, mul or res2; the tail no residual either (ops.conv2d_tail)
    for r in G.PRE_ROWS + G.TAIL_ROWS:
        o = G.opts(r)
        assert not (o["relu_in"] or o["gamma"] or o["mul"] or o["res2"]) and r.cout % 4 == 0
    assert all(not G.opts(r)["res"] and r.cout <= 128 for r in G.TAIL_ROWS)


@pytest.mark.parametrize("row", G.ALL_ROWS, ids=G.row_id)
def test_expected_kernel_is_what_the_dispatch_rules_give(row):
    for mode in G.modes_of(row):
        assert G.expected_kernel(row, mode) == dispatch(row, mode), (row.id, mode)
    if row.entry != "conv2d":
        assert row.kern[0] is None


def test_geometry_rows_contain_the_edges_they_claim():
    shapes = [(n, h, w) for n, h, w, _ in G.GEOM_SHAPES]
    for s in [(1, 4, 24), (3, 5, 25), (1, 8, 32), (1, 9, 33), (1, 8, 65), (1, 9, 72), (1, 33, 66), (3, 5, 73), (3, 16, 64)]:
        assert s in shapes
    assert [strip_rem(w) for _, _, w, _ in G.GEOM_SHAPES] == [0, 0, 0, 0, 1, 8, 2, 0, 0, 0, 0, 0, 2]
    assert [bool(strip_rem(w)) for _, _, w, _ in G.GEOM_SHAPES] == [s for _, _, _, s in G.GEOM_SHAPES]
    assert {(r.n, r.h, r.w, bn_of(r.cout)) for r in G.GEOMETRY} == {(n, h, w, bn) for n, h, w in shapes for bn in (32, 64, 128)}
    by_bn = {bn: [r for r in G.GEOMETRY if bn_of(r.cout) == bn] for bn in (32, 64, 128)}
    for bn in (32, 64):
        assert [main_tiles(r) for r in by_bn[bn]] == [1, 3, 1, 4, 2, 4, 10, 9, 12, 7, 8, 9, 30]
        assert [strip_tiles(r) for r in by_bn[bn]] == [0, 0, 0, 0, 1, 1, 2, 0, 0, 0, 0, 0, 6]
    assert all(tiles_n_of(r.cout) == 2 for r in by_bn[128])
    assert [main_tiles(r) for r in by_bn[128]] == [2, 6, 2, 8, 4, 8, 20, 18, 24, 14, 16, 18, 60]
    assert [strip_tiles(r) for r in by_bn[128]] == [0, 0, 0, 0, 2, 2, 4, 0, 0, 0, 0, 0, 12]   # 2, 4, 12: no multiple of 8 with tiles_n = 2
    assert all(s % 8 for s in [strip_tiles(r) for r in by_bn[128]] if s)
    # tile counts below 8, equal to 8, and not a multiple of 8 above it; q = 1, r = 4
    counts = {main_tiles(r) for r in G.ALL_ROWS}
    assert {1, 3, 7, 8, 9, 12} <= counts and {c % 8 for c in counts} >= {0, 1, 2, 3, 4, 6, 7}
    assert (12 >> 3, 12 & 7) == (1, 4)
    # the second strip tile of 33 rows has one live row; 65 = 2 tiles + one live strip column; 73 = 64 + 9
    assert 33 % 32 == 1 and 65 % 32 == 1 and 73 % 32 == 9 and 9 % 8 == 1 and 33 % 32 == 1


def test_xcd_remap_is_a_permutation_for_every_tile_count_of_the_rows():
    counts = {main_tiles(r) for r in G.ALL_ROWS} | {strip_tiles(r) for r in G.ALL_ROWS if strip_tiles(r)}
    assert min(counts) == 1 and max(counts) >= 60
    for nt in sorted(counts):
        assert sorted(xcd_remap(t, nt) for t in range(nt)) == list(range(nt)), nt


def test_input_channel_rows_contain_the_edges_they_claim():
    conv = G.CONV_ROWS
    for cin in (4, 6, 20, 32, 36, 34, 66, 98, 130, 258):
        assert any(r.cin == cin for r in conv), cin
    assert any(r.cin == 258 and r.cout == 32 for r in conv)
    # the tail step: cchunks = slabs walked by the 9-tap loop; its halo buffer is cchunks & 1 on the 128-column kernel, 0 on the narrow ones
    tail_rows = [r for r in G.ALL_ROWS if has_tail_tile(r, "bf16x3")]
    cch = lambda r: G.roundup(r.cin, 32) // 32 - 1  # noqa: E731
    by_bn = {bn: sorted({cch(r) for r in tail_rows if bn_of(r.cout) == bn}) for bn in (32, 64, 128)}
    assert by_bn[128] == [1, 2, 3, 4] and {c & 1 for c in by_bn[128]} == {0, 1}
    assert by_bn[32] == [1, 2, 8] and by_bn[64] == [1, 2]
    for bn in (32, 64, 128):   # ... in main tiles and in strip tiles, both parities
        assert {cch(r) & 1 for r in tail_rows if bn_of(r.cout) == bn and strip_rem(r.w)} == {0, 1}
        assert {cch(r) & 1 for r in tail_rows if bn_of(r.cout) == bn and not strip_rem(r.w)} >= ({0, 1} if bn != 64 else set())
    assert any(G.opts(r)["relu_in"] for r in tail_rows if bn_of(r.cout) == 128) and any(G.opts(r)["relu_in"] for r in tail_rows if bn_of(r.cout) == 32)
    assert {r.entry for r in tail_rows} == {"conv2d", "pre", "tail"}
    assert not any(has_tail_tile(r, "f32") for r in G.ALL_ROWS)
    # source slices: 16-byte aligned, the loader's pad channels inside the buffer; both kinds (cin % 4 == 0 and != 0)
    sl = [r for r in conv if G.opts(r)["xs"] is not None]
    assert {r.cin % 4 == 0 for r in sl} == {True, False}
    for r in sl:
        c0, ld = G.opts(r)["xs"]
        assert c0 % 4 == 0 and ld % 4 == 0 and c0 > 0 and c0 + G.roundup(r.cin, 4) < ld
    # dense cin % 4 != 0 rows: the pad channels [cin, roundup(cin, 4)) exist and hold BIG
    assert any(r.cin % 4 and G.opts(r)["xs"] is None for r in conv) and math.isfinite(G.BIG) and G.BIG >= 1e30


def test_output_channel_rows_contain_the_edges_they_claim():
    dense = {r.cout for r in G.CONV_ROWS if G.opts(r)["ys"] is None}
    assert {8, 20, 32, 33, 40, 64, 66, 98, 128, 130, 194, 256} <= dense
    assert {c: jv_of(c) for c in (8, 20, 32, 33, 40, 64, 66, 98, 128, 130, 194, 256)} == {
        8: [(1,)], 20: [(2,)], 32: [(2,)], 33: [(3,)], 40: [(3,)], 64: [(4,)], 66: [(4, 1)], 98: [(4, 3)], 128: [(4, 4)],
        130: [(4, 4), (1, 0)],     # the second N-tile: one block in the lower wave half, NONE in the upper
        194: [(4, 4), (4, 1)], 256: [(4, 4), (4, 4)]}
    assert any(0 in half for c in dense for half in jv_of(c))
    strip_couts = {r.cout for r in G.CONV_ROWS if strip_rem(r.w)}
    assert {33, 98, 130, 194} <= strip_couts
    r256 = G.ROW_BY_ID["co256-gamma"]
    assert G.opts(r256)["gamma"] and not goes_c256(r256, "bf16x3") and tiles_n_of(256) == 2
    assert goes_c256(G.R("x", "conv2d", *G.S933, 32, 256, ("F128", "H128")), "bf16x3")   # (without gamma the row would leave this file's kernels)
    # store paths, row by row
    expect = {"co98": True, "co98-slice": False, "co33": True, "co33-slice-c0-2": False, "co64-slice": True, "co66-mul-wide": False, "co130": True,
              "ep64-all": True, "ep-ln-co98": True, "co33-strip": True}
    assert {i: G.vec_epi(G.ROW_BY_ID[i]) for i in expect} == expect
    assert G.dst_layout(G.ROW_BY_ID["co98"]) == (0, 100) and G.dst_layout(G.ROW_BY_ID["co33-slice-c0-2"])[0] % 4 == 2
    for r in G.ALL_ROWS:
        c0, ld = G.dst_layout(r)
        padded = r.cout % 4 != 0
        slices = [(c0, ld)] + [G.operand_layout(r) for k in ("mul", "res", "res2") if G.opts(r)[k]]
        assert G.vec_epi(r) == all(a % 4 == 0 and b % 4 == 0 and (not padded or b == G.roundup(r.cout, 4)) for a, b in slices)
        assert c0 + r.cout + (4 if r.entry == "tail" else 0) <= ld
        if r.entry == "tail":
            assert G.vec_epi(r) and ld == c0 + r.cout + 4 and (c0 + r.cout) % 4 == 0
        if r.entry == "pre":
            a, b = G.operand_layout(r)
            assert a % 4 == 0 and b % 4 == 0 and b >= r.cout
    scalar = [r for r in G.CONV_ROWS if not G.vec_epi(r)]
    assert len(scalar) >= 3 and any(G.opts(r)["mul"] for r in scalar)
    wide = [r for r in G.ALL_ROWS if G.opts(r)["wide"]]
    for k in ("mul", "res", "res2", "pre"):
        assert any(G.opts(r)[k] for r in wide), k
    assert all(G.operand_layout(r)[1] > r.cout + 4 for r in wide)


def test_epilogue_rows_contain_the_paths_they_claim():
    def lean(r):   # the block-uniform ``simple`` of halo16_body's store loop
        o = G.opts(r)
        return G.vec_epi(r) and not (o["gamma"] or o["mul"] or o["res2"] or (o["ln"] and o["res"]))
    for bn in (32, 64, 128):
        rows = [r for r in G.EPILOGUE if bn_of(r.cout) == bn and (r.h, r.w) == (9, 33)]
        kinds = {(G.opts(r)["ln"], G.opts(r)["res"]) for r in rows if lean(r)}
        assert kinds == {(False, False), (True, False), (False, True)}, bn                      # the three lean loops
        assert {G.opts(r)["act"] for r in rows if lean(r)} >= set(G.ACTS), bn                   # all five activations through act_apply_bf
        gen = [G.opts(r) for r in rows if not lean(r)]
        assert any(o["gamma"] for o in gen) and any(o["mul"] and not o["gamma"] for o in gen) and any(o["res2"] and not o["mul"] for o in gen)
        assert any(o["ln"] and o["res"] and not o["mul"] for o in gen) and any(o["act"] == "gelu" for o in gen)       # erf GELU of epi_store
        assert any(all(o[k] for k in ("ln", "gamma", "mul", "res", "res2")) for o in gen) and any(not o["bias"] for o in gen)
        assert any(not G.opts(r)["bias"] for r in rows if lean(r))
        assert any(G.opts(r)["bias_offset"] == 40.0 and G.opts(r)["ln"] for r in rows)
    r20 = G.ROW_BY_ID["ep-ln-co20"]
    assert G.opts(r20)["ln"] and r20.cout == 20 and 16 + 8 > r20.cout   # group b = 16: ln_row_stats' scalar remainder
    pre = [G.opts(r) for r in G.PRE_ROWS]
    assert any(o["ln"] for o in pre) and any(o["res"] for o in pre) and any(not o["ln"] and not o["res"] for o in pre)
    assert any(strip_rem(r.w) for r in G.PRE_ROWS) and any(has_tail_tile(r, "bf16") for r in G.PRE_ROWS) and any(tiles_n_of(r.cout) == 2 for r in G.PRE_ROWS)
    assert {bn_of(r.cout) for r in G.PRE_ROWS} == {bn_of(r.cout) for r in G.TAIL_ROWS} == {32, 64, 128}
    tail = [G.opts(r) for r in G.TAIL_ROWS]
    assert any(o["ln"] for o in tail) and any(not o["ln"] for o in tail) and any(strip_rem(r.w) for r in G.TAIL_ROWS)
    assert max(r.cout for r in G.TAIL_ROWS) == 128   # (130: refused by the entry point -- test_conv2d_tail_refuses_more_than_128_channels)


# ---- references ----------------------------------------------------------------------------------------------------------------------------------

def ln_one_pass(y, lnw, lnb, eps=1e-6):
    """E[y^2] - mean^2: what a one-pass epilogue would compute"""
    u = y.mean(1, keepdim=True)
    var = (y * y).mean(1, keepdim=True) - u * u
    return (y - u) / torch.sqrt(var.clamp(min=0) + eps) * lnw.view(1, -1, 1, 1) + lnb.view(1, -1, 1, 1)


def strict_tol(row):
    return G.TOL["f32"] if row.entry == "conv2d" else G.TOL["bf16x3"]   # the smallest bar the row is held to


@pytest.mark.parametrize("row", G.ALL_ROWS, ids=G.row_id)
def test_reference(row):
    o, d = G.opts(row), G.inputs(row)
    ref = G.reference(row)
    assert G.reference(row) is ref   # computed once, shared
    assert ref.dtype == torch.float64 and ref.shape == (row.n, row.cout + (4 if row.entry == "tail" else 0), row.h, row.w) and bool(torch.isfinite(ref).all())
    scale = scale_of(ref)
    # a plain fp32 evaluation stays within 1/4 of the smallest bar: the inputs do not make a correct fp32 kernel fail
    e32 = float((G.evaluate(row, dt=torch.float32).double() - ref).abs().max())
    assert e32 <= strict_tol(row) * scale / 4, (e32, strict_tol(row) * scale)
    # discrimination: every declared piece matters by >= 100 x the (largest fp32-class) bar
    bar = G.TOL["bf16x3"] * scale
    moved = lambda **kw: float((G.evaluate(row, **kw) - ref).abs().max())  # noqa: E731
    for key in ("bias", "pre", "ln", "gamma", "mul", "res", "res2", "relu_in"):
        if o[key]:
            assert moved(drop=(key,)) >= DISC * bar, (key, moved(drop=(key,)), bar)
    if o["act"] != "none":
        assert moved(drop=("act",)) >= DISC * bar
    if o["act"] == "gelu":
        swap = moved(gelu="tanh")
        print(f"gelu swap {row.id}: {swap / bar:.1f} x the bar")
        assert swap >= GELU_SWAP_MIN * bar, (swap, bar)
    if has_tail_tile(row, "bf16x3"):   # the two channels of the tail step
        x2 = d["x"].clone()
        x2[:, -2:] = 0
        assert moved(x=x2) >= DISC * bar, (moved(x=x2), bar)
        for k in (1, 2):               # ... each of them
            x1 = d["x"].clone()
            x1[:, -k] = 0
            assert moved(x=x1) >= DISC * bar
    if row.h % 8 or row.w % 32:        # a partial tile: its last source row / column
        xr, xc = d["x"].clone(), d["x"].clone()
        xr[:, :, -1, :] = 0
        xc[:, :, :, -1] = 0
        assert moved(x=xr) >= DISC * bar and moved(x=xc) >= DISC * bar
    if row.entry == "tail":            # the pair is the two maps in this order, then zeros
        assert float(ref[:, -2:].abs().max()) == 0.0 and float((ref[:, -4] - ref[:, -3]).abs().max()) >= DISC * bar
        up = torch.nn.functional.interpolate(d["p1"].double(), (row.h, row.w), mode="bilinear", align_corners=True)
        assert torch.equal(ref[:, -4:-3], up) and torch.equal(ref[:, -4, 0, 0], d["p1"][:, 0, 0, 0].double()) and torch.equal(ref[:, -4, -1, -1], d["p1"][:, 0, -1, -1].double())
    if o["bias_offset"]:
        assert float(d["b"].min()) > 38.0
        one = float((G.evaluate(row, dt=torch.float32, ln=ln_one_pass).double() - ref).abs().max())
        print(f"offset {row.id}: two-pass fp32 {e32 / scale:.2e}, one-pass {one / scale:.2e} of the scale (bars 2e-5 / 3e-5)")
        assert one > G.TOL["bf16x3"] * scale, (one, bar)


def test_gelu_variants_differ_by_what_the_rows_can_see():
    v = torch.linspace(-8, 8, 1 << 20, dtype=torch.float64)
    d = (torch.nn.functional.gelu(v, approximate="tanh") - torch.nn.functional.gelu(v)).abs()
    i = int(d.argmax())
    print(f"|tanh GELU - erf GELU| max {float(d[i]):.3e} at v = {float(v[i]):.3f}: {float(d[i]) / 3e-5:.1f} x a 3e-5 bar at scale 1")
    assert 3e-4 <= float(d[i]) <= 6e-4


def gelu_fast32(v):
    """csrc/common.h::gelu_fast in float32, with exact division and exp2 in place of v_rcp_f32 / v_exp_f32"""
    f = np.float32
    assert v.dtype == np.float32
    x = v * f(0.70710678118654752440)
    ax = np.abs(x)
    t = f(1.0) / (f(1.0) + f(0.3275911) * ax)
    p = f(1.061405429) * t
    p = (p - f(1.453152027)) * t
    p = (p + f(1.421413741)) * t
    p = (p - f(0.284496736)) * t
    p = (p + f(0.254829592)) * t
    r = f(1.0) - p * np.exp2(ax * ax * f(-1.44269504088896340736))
    out = f(0.5) * v * (f(1.0) + np.copysign(r, x))
    assert out.dtype == np.float32
    return out


def test_gelu_fast_stays_within_its_share_of_the_bar():
    v = np.linspace(-8.0, 8.0, (1 << 21) + 1).astype(np.float32)
    ref = torch.nn.functional.gelu(torch.from_numpy(v).double()).numpy()
    err = float(np.abs(gelu_fast32(v).astype(np.float64) - ref).max())
    print(f"gelu_fast (float32 numpy) against float64 erf GELU on [-8, 8]: max |error| {err:.3e}")
    assert err <= 3e-5 / 20, err
    assert err <= 1e-6       # the order of common.h's 4.7e-7


# ---- bf16 mode -------------------------------------------------------------------------------------------------------------------------------------

def test_every_row_records_its_emulation_error():
    assert set(G.EMU) == {r.id for r in G.ALL_ROWS}


@pytest.mark.parametrize("row", G.ALL_ROWS, ids=G.row_id)
def test_bf16_emulation_error_is_the_recorded_one(row):
    e = G.emulation_error(row)
    emu = G.EMU[row.id]
    print(f"bf16 emulation {row.id}: {e:.3e}")
    assert abs(e - emu) <= 0.02 * emu, (e, emu)                         # recorded to 3 digits
    assert 10 * G.TOL["bf16x3"] <= G.bf16_bar(emu) <= G.BF16_CAP        # a bf16 bar, not a bf16x3 one, and never above the project's 2e-2
    assert bool(torch.isfinite(G.emulation(row)).all()) and G.emulation(row).shape == G.reference(row).shape
