"""CPU side of tests/test_upconv_kernels_gpu.py: its tables, float64 references and tolerances are sound before any kernel runs.  A
restatement of ac_scale / ac_tap (csrc/common.h) in numpy float32 and of the tile choice of prv2_upconv3x3 / prv2_upconv5x5 gives the
source footprint of every tile: every row's claimed maximum is recomputed, the tables are shown to reach 11 x 17 on both upconv3x3 tile
shapes and 11 x 16 on upconv5x5's, and the bound the kernels are built on -- no tile needs more than LR x LC = 11 x 17 source pixels,
consecutive entries of the column table advance by at most one source column -- is enumerated over every admitted pair of sizes up to
SIZES outputs per axis, so that a later change of TH / TW / LR / LC or of the 0.6 limit fails here instead of corrupting a tile.  Every row
is admitted by a restatement of its *_shape_ok predicate (the rejection row is not), the float32 oracle of every row stays inside half of
the row's tolerance, the bf16 emulation's error is a quarter of the bar it sets (under half of it where the bar is capped at the op's earlier
6e-3), and a deliberately wrong float64 variant misses the reference by 100 tolerances.  Nothing here loads the library."""
import numpy as np
import pytest
import torch

import test_upconv_kernels_gpu as G

f32 = np.float32
LR, LC = 11, 17                     # csrc/upconv.hip upc::LR, LC == csrc/upconv5.hip upc5::LR, LC
TILE_WIDE, TILE_STEEP = (16, 28), (14, 24)      # upc::TH0 x TW0 (both steps <= 0.5f), upc::TH1 x TW1 (a step in (0.5f, 0.6f])
TILE_5, HALO_5 = (14, 24), 2        # upc5::TH x TW, the 5x5 kernel's reach
CARRY = 0.15                        # the interpolation weight from which a row's last footprint row and column count as ``carried``
SIZES = 1400                        # the enumeration's largest output size per axis


# ---- ac_scale / ac_tap and the tiles, float32 as the library computes them ---------------------------------------------------------------
def ac_scale(n_in, n_out):
    return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0.0)


def ac_taps(n_in, n_out):
    """-> (i0, i1, w1) of ac_tap(dst, ac_scale(n_in, n_out), n_in) for dst = 0 .. n_out - 1"""
    src = ac_scale(n_in, n_out) * np.arange(n_out, dtype=f32)
    assert src.dtype == f32
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    return i0, i0 + (i0 < n_in - 1), src - i0.astype(f32)


def axis_footprints(n_in, n_out, tile, halo):
    """per tile along one axis: (first source index = rbase / cbase, number of source indices, the largest weight w1 any output of the tile gives
    the LAST of them) -- the outputs t tile - halo .. t tile + tile - 1 + halo, clamped to the image (both kernels clamp before they call
    ac_tap).  A weight of 0: the last index is staged and read, but a wrong value there would not show (a step of exactly 1/2 on whole tiles)"""
    i0, i1, w1 = ac_taps(n_in, n_out)
    res = []
    for t in range(-(-n_out // tile)):
        lo, hi = max(t * tile - halo, 0), min(t * tile + tile - 1 + halo, n_out - 1)
        sel = (i1[lo:hi + 1] == i1[hi]) & (i1[lo:hi + 1] > i0[lo:hi + 1])
        res.append((int(i0[lo]), int(i1[hi] - i0[lo] + 1), float(w1[lo:hi + 1][sel].max()) if sel.any() else 1.0 if i0[hi] == i1[hi] == i0[lo] else 0.0))
    return res


def upconv3_tile(hw, HW):
    """prv2_upconv3x3: wide = usy <= 0.5f && usx <= 0.5f"""
    return TILE_WIDE if ac_scale(hw[0], HW[0]) <= f32(0.5) and ac_scale(hw[1], HW[1]) <= f32(0.5) else TILE_STEEP


def footprint(hw, HW, tile, halo):
    """-> (rows, columns, rbase, cbase, tile row, tile column, weight of the last row, of the last column): the largest extents over the tiles and,
    of the tiles that have them, the one whose last row / column weighs most -- both in ONE tile, the axes being independent"""
    rows, cols = axis_footprints(hw[0], HW[0], tile[0], halo), axis_footprints(hw[1], HW[1], tile[1], halo)
    mr, mc = max(e for _, e, _ in rows), max(e for _, e, _ in cols)
    ty = max((i for i, (_, e, _) in enumerate(rows) if e == mr), key=lambda i: (rows[i][2], -i))
    tx = max((i for i, (_, e, _) in enumerate(cols) if e == mc), key=lambda i: (cols[i][2], -i))
    return mr, mc, rows[ty][0], cols[tx][0], ty, tx, rows[ty][2], cols[tx][2]


def upconv3_shape_ok(hw, HW, n, cin, ldu, cout):
    """upconv_shape_ok of csrc/upconv.hip (the bf16 modes are the only ones the table runs)"""
    return (n > 0 and HW[0] >= 2 and HW[1] >= 2 and cout > 0 and cin >= 32 and cin % 32 == 0 and ldu % 4 == 0 and ldu >= cin and hw[0] >= 1 and hw[1] >= 1
            and ac_scale(hw[0], HW[0]) <= f32(0.6) and ac_scale(hw[1], HW[1]) <= f32(0.6) and hw[0] * hw[1] * ldu < 2 ** 29 and G.roundup(cout, 128) * 9 * cin < 2 ** 29)


def upconv5_shape_ok(hw, HW, n, cin, ldu, cout):
    """upconv5_shape_ok of csrc/upconv5.hip"""
    return (n > 0 and HW[0] >= 5 and HW[1] >= 5 and 0 < cout <= 32 and cout % 4 == 0 and cin >= 32 and cin % 32 == 0 and ldu % 4 == 0 and ldu >= cin
            and hw[0] >= 2 and hw[1] >= 2 and ac_scale(hw[0], HW[0]) <= f32(0.5) and ac_scale(hw[1], HW[1]) <= f32(0.5) and hw[0] * hw[1] * ldu < 2 ** 29
            and 128 * 25 * cin < 2 ** 29)


def ups_shape_ok(hw, HW, c1, ldu, cin, ldx, cout):
    """ups_shape_ok of csrc/igemm.hip on top of halo16_shape_ok (igemm.h): the 3x3 s1 p1 layers of the bf16 modes the table packs"""
    return (HW[0] * HW[1] * ldx < 2 ** 29 and HW[1] >= 24 and HW[0] >= 4 and cout > 64 and c1 > 0 and c1 % 32 == 0 and c1 <= cin and ldu % 4 == 0 and ldu >= c1
            and hw[0] >= 1 and hw[1] >= 1 and hw[0] * hw[1] * ldu < 2 ** 29)


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- a. upconv3x3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.UPC_ROWS, ids=lambda r: r["id"])
def test_upconv3x3_row(row):
    hw, HW, n, cin, cout = row["hw"], row["HW"], row["n"], row["cin"], row["cout"]
    u, w, b, add = G.upc_inputs(row)
    ref, emu, emu_err = G.upc_ref(row)
    assert ref.shape == (n, cout, *HW) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert G.upc_ref(row)[0] is ref     # computed once
    assert (b is not None) == row["bias"] and (add is not None) == (row["add"] is not None)
    # contract, tile and footprint
    c0u, ldu, c0o, ldo, c0a, lda = G.upc_layout(row)
    assert upconv3_shape_ok(hw, HW, n, cin, ldu, cout)
    assert c0u % 4 == 0 and c0o % 4 == 0 and c0a % 4 == 0 and ldo % 4 == 0 and lda % 4 == 0      # 16-byte aligned rows
    assert c0u + cin <= ldu and c0o + cout < ldo and lda > cout                                   # a sentinel channel beside every destination
    assert row["u_slice"] == (ldu > cin) and (not row["u_slice"] or 0 < c0u < c0u + cin < ldu)
    assert row["tile"] == upconv3_tile(hw, HW)
    mr, mc, rbase, cbase, ty, tx, wr, wc = footprint(hw, HW, row["tile"], 1)
    assert (mr, mc) == row["foot"] and mr <= LR and mc <= LC
    assert row["carried"] == (row["foot"] == (LR, LC) and min(wr, wc) >= CARRY) and (row["carried"] or row["foot"] != (LR, LC) or wr == wc == 0.0)
    scale = G.scale_of(ref)
    tol = G.UPC_TOL_X3 * scale
    # the float32 oracle -- the same graph in float32 -- stays inside half of the bf16x3 bar
    assert maxdiff(G.upc_graph(row, u, w, b, add, torch.float32), ref) <= 0.5 * tol
    # the bf16 emulation: its error sets the bar of bf16 mode against float64, a quarter of which it therefore is -- unless four times the
    # error would pass the op's earlier 6e-3, which then stays the bar (the emulation is 0.9e-3 .. 2.5e-3 of the scale from float64 on these
    # rows, so the cap holds on about half of them): there the emulation, plus the distance the kernel may keep from it, still has to lie
    # inside HALF of the bar.  Either way a kernel within 2e-5 of the emulation cannot fail the bar against float64
    bar = G.upc_tol_bf16(row)
    assert emu_err == G.relerr(emu, ref) and bar == min(4.0 * emu_err, G.UPC_TOL_BF16_CAP) <= G.UPC_TOL_BF16_CAP
    assert emu_err <= 0.25 * bar or bar == G.UPC_TOL_BF16_CAP
    assert G.UPC_TOL_X3 <= emu_err and emu_err + G.UPC_TOL_X3 <= 0.5 * bar
    # discrimination: a lost last footprint row / column of the tile that reaches the maximum -- over the whole output, and in the outputs
    # of THAT tile, where it shows if and only if the row is ``carried``
    if row["foot"] == (LR, LC):
        (th, tw), (y0, x0) = row["tile"], (ty * row["tile"][0], tx * row["tile"][1])
        for axis, first in ((2, rbase + LR - 1), (3, cbase + LC - 1)):
            bad = u.clone()
            bad.index_fill_(axis, torch.tensor([first]), 0.0)
            d = (G.upc_graph(row, bad, w, b, add) - ref).abs()
            in_tile = float(d[:, :, y0:y0 + th, x0:x0 + tw].max())
            assert first < u.shape[axis] and float(d.max()) >= 100 * tol
            assert in_tile >= 100 * tol if row["carried"] else in_tile == 0.0
    # ... the two steps applied to each other's axis (the identity when they are equal)
    (sy, sx) = ((hw[0] - 1) / (HW[0] - 1), (hw[1] - 1) / (HW[1] - 1))
    assert maxdiff(G.upc_graph(row, u, w, b, add, up=lambda t, size: G.up_steps(t, size, sy, sx)), ref) <= 1e-12 * scale
    if (ac_scale(hw[0], HW[0]) <= f32(0.5)) != (ac_scale(hw[1], HW[1]) <= f32(0.5)):
        assert maxdiff(G.upc_graph(row, u, w, b, add, up=lambda t, size: G.up_steps(t, size, sx, sy)), ref) >= 100 * tol


def test_upconv3x3_table_covers_what_it_claims():
    rows = G.UPC_ROWS
    assert len({r["id"] for r in rows}) == len(rows)
    full = [r for r in rows if r["foot"] == (LR, LC)]
    assert {r["tile"] for r in full} == {TILE_WIDE, TILE_STEEP}                                  # 11 x 17 on each tile shape ...
    assert {r["tile"] for r in full if r["carried"]} == {TILE_WIDE, TILE_STEEP}                  # ... with a weight on the last row and column ...
    by = G.UPC_BY_ID
    for hw, HW, tile in (((18, 30), (35, 59), TILE_WIDE), ((18, 30), (30, 50), TILE_STEEP)):      # ... in tile row 1, tile column 1: not a tile at the origin
        assert footprint(hw, HW, tile, 1)[:6] == (LR, LC, 7, 13, 1, 1)
    assert footprint((30, 53), (61, 107), TILE_WIDE, 1)[4:6] == (2, 2)
    assert {by[i]["cin"] // 32 for i in ("full-16x28-1slab", "carried-16x28", "full-16x28-3slabs")} == {1, 2, 3}   # both final stage parities on the full footprint
    assert {r["cin"] // 32 for r in rows} >= {1, 2, 3}
    mixed = [r for r in rows if (ac_scale(r["hw"][0], r["HW"][0]) <= f32(0.5)) != (ac_scale(r["hw"][1], r["HW"][1]) <= f32(0.5))]
    assert [r["id"] for r in mixed] == ["mixed-rows-fine", "mixed-cols-fine"] and all(r["tile"] == TILE_STEEP for r in mixed)
    assert mixed[0]["hw"] == mixed[1]["hw"][::-1] and mixed[0]["HW"] == mixed[1]["HW"][::-1]
    assert {r["hw"] for r in rows} >= {(1, 3), (3, 1), (1, 1)}                                  # ac_scale == 0: every tap has i1 == i0
    assert {r["cout"] for r in rows if r["cout"] < 32} == {8, 20} and any(r["cout"] % 4 for r in rows) and any(r["n"] > 1 for r in rows)
    assert by["pyramid-25x33"]["n"] * by["pyramid-25x33"]["cout"] * 49 * 65 == max(r["n"] * r["cout"] * r["HW"][0] * r["HW"][1] for r in rows)
    for tile in (TILE_WIDE, TILE_STEEP):                                                          # every layout on either tile shape
        lay = [r for r in rows if r["tile"] == tile and r["foot"] == (LR, LC)]
        assert any(r["u_slice"] for r in lay) and any(r["out_c0"] for r in lay) and {r["add"] for r in lay} == {None, "sep", "inplace"}
    assert all(r["bias"] and r["act"] == "gelu" for r in rows if r["add"] == "sep") and not any(r["bias"] for r in rows if r["add"] == "inplace")
    assert {r["act"] for r in rows} == {"none", "relu", "gelu"}


# ---- b. upconv5x5 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.UP5_ROWS, ids=lambda r: r["id"])
def test_upconv5x5_row(row):
    hw, HW, n, ci, co = row["uhw"], row["HW"], row["n"], row["ci"], row["co"]
    inputs = G.up5_inputs(row)
    ref = G.up5_ref(row)
    assert ref.shape == (n, co, *HW) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all()) and G.up5_ref(row) is ref
    assert (inputs[3] is not None) == row["tap_bias"] and (inputs[5] is not None) == row["b2"]
    c0u, ldu, c0o, ldo = G.up5_layout(row)
    assert upconv5_shape_ok(hw, HW, n, ci, ldu, co)
    assert c0u % 4 == 0 and c0o % 4 == 0 and ldo % 4 == 0 and c0u + ci <= ldu and c0o + co < ldo
    mr, mc, _, _, _, _, wr, wc = footprint(hw, HW, TILE_5, HALO_5)
    assert (mr, mc) == row["foot"] and mr <= LR and mc <= LC and row["carried"] == ((mr, mc) == (LR, LC - 1) and min(wr, wc) >= CARRY)
    tol = G.UP5_TOL["bf16x3"] * G.scale_of(ref)
    assert maxdiff(G.up5_graph(*inputs, HW, dtype=torch.float32), ref) <= 0.5 * tol
    ring = G.ring_mask(ref)
    assert bool(ring.any()) and bool((~ring).any())
    # discrimination, interior and ring separately: the half-pixel convention
    bad = (G.up5_graph(*inputs, HW, up=lambda t, size: G.up64(t, size, align_corners=False)) - ref).abs()
    assert float(bad[ring].max()) >= 100 * tol and float(bad[~ring].max()) >= 100 * tol


def test_upconv5x5_graph_is_the_reference_of_test_upconv5():
    import test_upconv5 as T5
    row = G.UP5_BY_ID["not-x2"]
    assert torch.equal(T5.reference(*G.up5_inputs(row), row["HW"]), G.up5_ref(row))


def test_upconv5x5_table_covers_what_it_claims():
    rows, by = G.UP5_ROWS, G.UP5_BY_ID
    assert len({r["id"] for r in rows}) == len(rows)
    assert any(r["foot"] == (11, 16) and r["carried"] for r in rows)                             # the kernel's maximum (the enumeration below)
    assert {r["uhw"] for r in rows} >= {(2, 2), (3, 4)} and {r["HW"] for r in rows} >= {(5, 5), (5, 7)}    # h, w >= 5 and u.h, u.w >= 2 at their ends
    assert by["x4"]["HW"][0] == 4 * by["x4"]["uhw"][0] and by["not-x2"]["HW"][0] != 2 * by["not-x2"]["uhw"][0]
    assert {r["co"] for r in rows} >= {4, 20, 32} and {r["ci"] // 32 for r in rows} >= {1, 2, 3}
    assert not by["no-tap-bias"]["tap_bias"] and not by["no-b2"]["b2"] and by["u-slice"]["u_slice"] and by["out-slice"]["out_c0"]
    assert not upconv5_shape_ok((2, 2), (4, 5), 1, 32, 32, 32) and not upconv5_shape_ok((1, 2), (5, 5), 1, 32, 32, 32) and not upconv5_shape_ok((2, 2), (5, 5), 1, 32, 32, 2)


# ---- c. conv2d_ups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.UPS_ROWS, ids=lambda r: r["id"])
def test_conv2d_ups_row(row):
    hw, HW, n, c1, cin, cout = row["hw"], row["HW"], row["n"], row["c1"], row["cin"], row["cout"]
    c0u, ldu, c0o, ldo = G.ups_layout(row)
    # the shape contract admits every row; what rejects the rejection row is conv_fill_params' "fused LayerNorm needs cout <= 128"
    assert ups_shape_ok(hw, HW, c1, ldu, cin, G.roundup(cin, 4), cout)
    assert row["raises"] == (row["ln"] and cout > 128)
    assert c0u % 4 == 0 and c0o % 4 == 0 and ldo % 4 == 0 and c0u + c1 <= ldu and c0o + cout < ldo
    inputs = G.ups_inputs(row)
    assert (inputs[1] is None) == (cin == c1) and (inputs[4] is not None) == row["ln"] and (inputs[5] is not None) == row["res"]
    if row["raises"]:
        return
    ref = G.ups_ref(row)
    assert ref.shape == (n, cout, *HW) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all()) and G.ups_ref(row) is ref
    tol = G.UPS_TOL["bf16x3"] * G.scale_of(ref)
    assert maxdiff(G.ups_graph(row, *inputs, dtype=torch.float32), ref) <= 0.5 * tol
    if hw != HW:    # (at the identity size both conventions copy the source)
        assert maxdiff(G.ups_graph(row, *inputs, up=lambda t, size: G.up64(t, size, align_corners=False)), ref) >= 100 * tol


def test_conv2d_ups_table_covers_what_it_claims():
    rows, by = G.UPS_ROWS, G.UPS_BY_ID
    assert len({r["id"] for r in rows}) == len(rows)
    assert by["step-1"]["hw"] == by["step-1"]["HW"] and (by["step-1"]["c1"], by["step-1"]["cin"], by["step-1"]["cout"]) == (64, 98, 98)
    assert all(a > b for a, b in zip(by["step-2"]["hw"], by["step-2"]["HW"]))
    assert by["source-1-row"]["hw"][0] == 1 and by["source-1-col"]["hw"][1] == 1 and by["source-1-col"]["c1"] == by["source-1-col"]["cin"]
    ln = [r for r in rows if r["ln"] and not r["raises"]]
    assert {r["cout"] for r in ln} >= {128, 98} and all(r["act"] == "gelu" for r in ln)
    assert by["ln-cout128-strip"]["HW"][1] == 70 and 0 < 70 % 32 <= 8 and by["ln-cout98"]["HW"][1] % 32 == 0      # with and without a remainder strip
    assert by["u-slice"]["u_slice"] and by["out-slice"]["out_c0"] and [r["cout"] for r in rows if r["raises"]] == [194]


# ---- the footprint bound itself --------------------------------------------------------------------------------------------------------
def axis_extremes(n_out, limit, min_in, tiles):
    """every admitted source size of ONE axis with n_out outputs (ac_scale <= limit, n_in >= min_in), vectorised over the source size:
    -> (largest footprint per (tile, halo) of ``tiles``, largest advance of i0 between neighbouring outputs, the admitted steps)"""
    k = np.arange(min_in - 1, n_out, dtype=np.int32)                   # n_in - 1
    s = k.astype(f32) / f32(n_out - 1)
    k, s = k[s <= f32(limit)], s[s <= f32(limit)]
    src = s[:, None] * np.arange(n_out, dtype=f32)[None, :]
    assert src.dtype == f32
    i0 = np.minimum(src.astype(np.int32), k[:, None])
    i1 = i0 + (i0 < k[:, None])
    ext = []
    for tile, halo in tiles:
        t = np.arange(-(-n_out // tile))
        lo, hi = np.maximum(t * tile - halo, 0), np.minimum(t * tile + tile - 1 + halo, n_out - 1)
        ext.append(int((i1[:, hi] - i0[:, lo] + 1).max()) if len(k) else 0)
    return ext, int(np.diff(i0, axis=1).max()) if len(k) and n_out > 1 else 0, s


def test_no_tile_needs_more_than_the_staged_footprint():
    """upconv3x3: rows on 16- and 14-output tiles and columns on 28- and 24-output tiles for steps <= 0.5f (either tile shape may serve such an
    axis: the other axis decides), rows on 14 and columns on 24 for steps in (0.5f, 0.6f]; upconv5x5: 14 / 24 with a two-pixel halo, steps <=
    0.5f, from 5 outputs and 2 sources.  The bound is reached, exactly, by either tile shape at the steps it is made for -- and upconv5x5 stops at 16 columns"""
    top = {"wide": [0, 0, 0, 0], "steep": [0, 0], "five": [0, 0]}
    steps = set()
    for n_out in range(2, SIZES + 1):
        ext, adv, s = axis_extremes(n_out, 0.5, 1, [(16, 1), (28, 1), (14, 1), (24, 1)])
        top["wide"] = [max(a, b) for a, b in zip(top["wide"], ext)]
        ext6, adv6, s6 = axis_extremes(n_out, 0.6, 1, [(14, 1), (24, 1)])
        top["steep"] = [max(a, b) for a, b in zip(top["steep"], ext6)]
        assert adv <= 1 and adv6 <= 1, n_out       # the walk's ``if (ci != c)``: one source column per table entry at the most
        steps.update((float(s.max()), float(s6.max())))
        if n_out >= 5:
            ext5, adv5, _ = axis_extremes(n_out, 0.5, 2, [(TILE_5[0], HALO_5), (TILE_5[1], HALO_5)])
            top["five"] = [max(a, b) for a, b in zip(top["five"], ext5)]
            assert adv5 <= 1
    assert float(f32(0.5)) in steps and float(f32(0.6)) in steps        # the steps that round to exactly 0.5f (2 k + 1 outputs) and 0.6f (3 / 5)
    assert ac_scale(4, 6) == f32(0.6) and ac_scale(301, 501) == f32(0.6) and ac_scale(300, 599) == f32(0.5)
    assert top["wide"][:2] == [LR, LC] and top["steep"] == [LR, LC], top
    assert top["wide"][2] <= LR and top["wide"][3] <= LC, top            # (the smaller tile at the finer steps: the mixed side of ``wide``)
    assert top["five"] == [LR, LC - 1], top


def test_the_restatement_of_ac_tap_is_align_corners():
    """the float32 taps against float64 index arithmetic, away from the sizes where rounding moves a tap across a pixel (weight ~ 0 there)"""
    for n_in, n_out in ((18, 35), (30, 59), (18, 30), (30, 50), (25, 49), (30, 61), (53, 107), (1, 2), (3, 6)):
        i0, i1, w1 = ac_taps(n_in, n_out)
        src = np.arange(n_out, dtype=np.float64) * (n_in - 1) / (n_out - 1)
        off = np.abs(src - np.round(src)) > 1e-4
        assert np.array_equal(i0[off], np.minimum(np.floor(src), n_in - 1).astype(np.int32)[off]) and np.array_equal(i1, np.minimum(i0 + 1, n_in - 1))
        assert float(np.abs(w1 - (src - i0)).max()) <= 1e-4
