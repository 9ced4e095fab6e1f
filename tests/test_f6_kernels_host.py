"""CPU side of tests/test_f6_kernels_gpu.py: the emulation, the tables, the rows' claims and the planted data are sound before any kernel runs.
Nothing here loads the library.

* the quantiser of tests/f6_emulation.py: all 64 e2m3 codes reproduced, ties to the even code, saturation, the E8M0 clamp to [1, 254]; away from ties it
  agrees with tools/studies/split_arith_study.py::mx_quant (which takes the lower neighbour on ties: tie="down" agrees everywhere);
* the edges the rows claim, against a plain restatement of the launch arithmetic of prv2_conv3x3_f6 (f6_emulation.stage1_walks: tile count, blocks =
  min(ceil(ntiles / 8), 32) * 8, the per-XCD chunk, each workgroup's K), the superslab parities, and the remainder branch of the stage-2 block map;
* EMU / EMU_TAIL recomputed; S_row <= 2e-5 on every row; the fp32-accumulated emulation stays under the S_row / 3 bar;
* the planted data: zero blocks, power-of-two maxima, exact ties, the position of the maximum, the outlier, the large edges, slices and strides;
* discrimination: planted errors IN THE EMULATION -- the two corrections swapped, the residual block quantised with q6(x)'s scale, a halo column / row
  taken from the linear-memory neighbour, the tile at position k + 1 of a walk convolved with tile k's first superslab -- move the result by more than
  the bar on every row that claims the edge."""
import importlib.util
import os

import numpy as np
import pytest

import f6_emulation as E
import test_f6_kernels_gpu as G

SMALL = 2000   # pixels: rows up to this size run the whole-image planted errors (the tile-walk rows run the per-tile one)


def study():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("split_arith_study", os.path.join(root, "tools", "studies", "split_arith_study.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the quantiser ------------------------------------------------------------------------------------------------------------------------------------

def test_quantiser_reproduces_all_64_codes():
    assert len(E.E2M3_VALUES) == 64 and len(set(E.E2M3_VALUES[:32])) == 32
    assert list(E.GRID[:9]) == [0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0] and E.GRID[16] == 2.0 and E.GRID[24] == 4.0 and E.GRID[31] == 7.5
    assert np.array_equal(E.E2M3_VALUES[32:], -E.E2M3_VALUES[:32]) and np.all(np.diff(E.GRID) > 0)
    assert np.array_equal(E.GRID, study().E2M3)
    for e in (-126, -20, 0, 3, 100):   # every code is a fixed point at every block scale 2^e (a 7.5-magnitude element pins the scale; -126: the clamped code 1)
        for c in range(64):
            v = np.zeros(32)
            v[0], v[1] = 7.5 * 2.0 ** e, E.E2M3_VALUES[c] * 2.0 ** e
            assert int(E.block_codes(v)[0]) == e + 127 and np.array_equal(E.q6(v), v), (e, c)


def test_quantiser_ties_to_even_and_saturates():
    mids = (E.GRID[:-1] + E.GRID[1:]) / 2
    even = E.round_e2m3(mids)
    assert np.array_equal(even, np.where(np.arange(31) % 2 == 0, E.GRID[:-1], E.GRID[1:]))   # the neighbour with the even code
    assert np.array_equal(E.round_e2m3(mids, "down"), E.GRID[:-1]) and np.array_equal(E.round_e2m3(mids, "up"), E.GRID[1:])
    eps = 2.0 ** -30
    assert np.array_equal(E.round_e2m3(mids + eps), E.GRID[1:]) and np.array_equal(E.round_e2m3(mids - eps), E.GRID[:-1])
    assert np.array_equal(E.round_e2m3(np.array([7.5, 7.75, 7.999, 8.0, 100.0])), np.full(5, 7.5))
    # a block whose maximum is 7.99 of its scale unit: saturates, sign kept
    v = np.zeros(32)
    v[0], v[1] = np.float32(7.99), -np.float32(7.9)
    q = E.q6(v)
    assert q[0] == 7.5 and q[1] == -7.5


def test_e8m0_clamp():
    f = np.float32
    assert list(E.e8m0_of(np.array([0.0, 1e-45, 2.0 ** -126, 2.0 ** -124, 1.0, 4.0, np.nextafter(f(4), f(0)), 3.0e38], dtype=f))) == [1, 1, 1, 1, 125, 127, 126, 252]
    assert int(E.e8m0_of(f(np.inf))) == 253 <= 254       # (never 255)
    z = E.q6(np.zeros(64))
    assert np.array_equal(z, np.zeros(64)) and not np.signbit(z).any()
    # for every normal maximum the scale is 2^(floor(log2 max) - 2)
    m = np.array([0.3, 1.0, 1.999, 2.0, 5.0, 1e-20, 1e20], dtype=f)
    assert np.array_equal(E.e8m0_of(m) - 127, np.floor(np.log2(m.astype(np.float64))) - 2)


def test_quantiser_agrees_with_the_study_away_from_ties():
    S = study()
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((4096, 64)) * np.exp(2 * rng.standard_normal((4096, 1)))).astype(np.float32)
    v[::7, :32] = 0.0
    want = S.mx_quant(v, S.E2M3, 2).astype(np.float64)
    assert np.array_equal(E.q6(v, tie="down"), want)
    even = E.q6(v)
    sc = np.repeat(2.0 ** (E.block_codes(v.astype(np.float64)) - 127.0), 32, axis=-1)
    a = np.abs(v.astype(np.float64)) / sc
    tie = np.isin(a, (E.GRID[:-1] + E.GRID[1:]) / 2)
    assert np.array_equal(even[~tie], want[~tie]) and (~tie).mean() > 0.99
    # ... and on exact ties the two differ exactly where the lower neighbour's code is odd
    t = np.concatenate([(E.GRID[:-1] + E.GRID[1:]) / 2, [7.5]]).astype(np.float32)
    d = E.q6(t) != S.mx_quant(t, S.E2M3, 2)
    assert np.array_equal(d[:31], np.arange(31) % 2 == 1) and not d[31]


def test_emulation_is_the_documented_sum():
    """one pixel, one tap by hand: x w = f16 x f16 w + q6 x q6(w - f16 w) + q6(x - f16 x) q6 w with the weight scale undone"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 1, 16, 64)).astype(np.float32)
    w = np.zeros((256, 64, 3, 3), dtype=np.float32)
    w[:, :, 1, 1] = rng.standard_normal((256, 64)).astype(np.float32) / 8
    ws = E.w_scale_of(w)
    assert ws in (2.0, 4.0, 8.0)
    xs = np.maximum(x, 0).astype(np.float64)
    wc = (w[:, :, 1, 1] * np.float32(ws)).astype(np.float64)
    xh, wh = xs.astype(np.float16).astype(np.float64), wc.astype(np.float16).astype(np.float64)
    want = (xh @ wh.T + E.q6(xs) @ E.q6(wc - wh).T + E.q6(xs - xh) @ E.q6(wc).T) / ws
    assert np.abs(E.conv(x, w, True) - want).max() < 1e-13       # (float64 summation order only)
    assert G.distance(E.conv_f32(x, w, True).astype(np.float64), want) < 1e-6
    assert 1e-7 < G.distance(want, E.exact(x, w, True)) < 1e-4    # (one tap of 64 channels: the scheme's error, nothing coarser)
    # the caller's power-of-two x_scale changes nothing in range
    assert np.abs(E.conv(x, w, True, x_scale=2.0 ** 7) - want).max() < 1e-13 and np.abs(E.conv(x, w, True, x_scale=2.0 ** -3) - want).max() < 1e-13


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------------

def test_tables_are_explicit_and_complete():
    ids = [r.id for r in G.ALL_ROWS]
    assert len(set(ids)) == len(ids)
    assert set(G.EMU) == {r.id for r in G.CONV_ROWS} and set(G.EMU_TAIL) == {r.id for r in G.TAIL_ROWS}
    assert all(r.id.startswith("t-") for r in G.TAIL_ROWS + [G.TAPS]) and not any(r.id.startswith("t-") for r in G.CONV_ROWS + [G.TIE])
    assert all(r.cin % 64 == 0 and r.w >= 16 for r in G.ALL_ROWS)          # the kernels' contract
    assert G.TAIL_TOL == 2e-5 and G.S_MAX == 2e-5
    src = open(G.__file__).read()
    assert "mark.skip" not in src and "pytest.skip" not in src and "xfail" not in src and "importorskip" not in src and "os.environ" not in src and "getenv" not in src and "monkeypatch" not in src
    # buffers stay a few MB
    assert max(r.n * r.h * r.w * max(r.cin, 272) * 4 for r in G.ALL_ROWS) < 12 << 20


def ntiles_of(r):
    return E.tile_grid(r.n, r.h, r.w)[2]


def k_histogram(ntiles):
    h = {}
    for wk in E.stage1_walks(ntiles):
        h[len(wk)] = h.get(len(wk), 0) + 1
    return h


# row -> (tile count, workgroups, {K: how many workgroups walk K tiles})
WALK_CLAIMS = {
    "g-1x8x16": (1, 8, {1: 1, 0: 7}),             # empty workgroups
    "g-1x7x97": (7, 8, {1: 7, 0: 1}),
    "g-2x9x17": (8, 8, {1: 8}),
    "g-1x24x48": (9, 16, {1: 9, 0: 7}),           # chunk 2: XCD 4's chunk is ragged (one tile), XCDs 5 .. 7 are empty
    "w257-c64": (257, 256, {2: 7, 1: 243, 0: 6}),
    "w257-c192": (257, 256, {2: 7, 1: 243, 0: 6}),
    "w514-c64": (514, 256, {3: 7, 2: 244, 1: 5}),
    "w514-c192": (514, 256, {3: 7, 2: 244, 1: 5}),
    "wimg-c64": (260, 256, {2: 7, 1: 246, 0: 3}),
    "wimg-c192": (260, 256, {2: 7, 1: 246, 0: 3}),
}


def test_walk_rows_contain_the_edges_they_claim():
    for rid, (nt, blocks, hist) in WALK_CLAIMS.items():
        r = G.ROW_BY_ID[rid]
        assert ntiles_of(r) == nt, rid
        walks = E.stage1_walks(nt)
        assert len(walks) == blocks == min(E.cdiv(nt, 8), 32) * 8 and k_histogram(nt) == hist, (rid, k_histogram(nt))
        assert sorted(t for wk in walks for t in wk) == list(range(nt)), rid              # every tile exactly once
        chunk = E.cdiv(nt, 8)
        for b, wk in enumerate(walks):                                                     # a workgroup stays inside its XCD's chunk
            assert all((b & 7) * chunk <= t < min(((b & 7) + 1) * chunk, nt) for t in wk)
    assert {nt for nt, _, _ in WALK_CLAIMS.values()} >= {1, 7, 8, 9, 257, 514}
    for r in G.CONV_ROWS:                                                                  # ... and no other row walks
        if r.id not in WALK_CLAIMS:
            assert ntiles_of(r) <= 8 or r.id == "g-1x24x48-c192", r.id
    # the rows of many small images: consecutive tiles of a workgroup lie in different images, 4 tiles each
    r = G.ROW_BY_ID["wimg-c64"]
    assert E.tile_grid(1, r.h, r.w)[2] == 4
    two = [wk for wk in E.stage1_walks(260) if len(wk) == 2]
    assert len(two) == 7 and all(E.tile_origin(a, r.n, r.h, r.w)[0] != E.tile_origin(b, r.n, r.h, r.w)[0] for a, b in two)
    # rows beyond 256 tiles run at one and at three superslabs: the halo double buffer changes parity from tile to tile in both
    assert {(nt > 256, G.ROW_BY_ID[i].cin) for i, (nt, _, _) in WALK_CLAIMS.items() if nt > 256} == {(True, 64), (True, 192)}
    assert (64 // 64) & 1 == 1 and (192 // 64) & 1 == 1


def test_geometry_and_channel_rows_contain_the_edges_they_claim():
    shapes = {(r.n, r.h, r.w) for r in G.CONV_ROWS}
    assert {(1, 1, 16), (1, 8, 16), (1, 9, 17), (1, 7, 31), (1, 16, 32), (1, 24, 48), (2, 9, 17)} <= shapes
    assert [ntiles_of(G.ROW_BY_ID[i]) for i in ("g-1x1x16", "g-1x8x16", "g-1x9x17", "g-1x7x31", "g-1x16x32", "g-1x24x48", "g-2x9x17")] == [1, 1, 4, 2, 4, 9, 8]
    # 24 x 48: the middle tile (1, 1) of 3 x 3 has its whole 10 x 18 halo inside the image
    assert E.tile_origin(4, 1, 24, 48) == (0, 8, 16) and 8 - 1 >= 0 and 8 + 8 < 24 and 16 - 1 >= 0 and 16 + 16 < 48
    # superslab counts 1, 2, 3, 4, 8: both parities of the halo buffer at a tile's end (and of the epilogue's free buffer)
    assert {r.cin // 64 for r in G.CONV_ROWS} == {1, 2, 3, 4, 8}
    assert {(r.cin // 64) & 1 for r in G.CONV_ROWS if ntiles_of(r) > 1} == {0, 1}
    assert {r.cin for r in G.TAIL_ROWS} == {256, 512}
    # slices
    o = lambda i: G.opts(G.ROW_BY_ID[i])  # noqa: E731
    for i in ("xs-end", "xs-end-c192", "t-xs-f32-end"):
        c0, ld = o(i)["xs"]
        assert c0 > 0 and c0 + G.ROW_BY_ID[i].cin == ld                       # ends at the last channel of the wider buffer
    for i in ("xs-mid", "t-xs"):
        c0, ld = o(i)["xs"]
        assert c0 > 0 and c0 + G.ROW_BY_ID[i].cin < ld
    for r in G.ALL_ROWS:
        op = G.opts(r)
        for k in ("xs", "ys", "rs", "ps"):
            if op.get(k) is not None:
                c0, ld = op[k]
                assert c0 % 4 == 0 and ld % 4 == 0 and c0 + (r.cin if k == "xs" else 256) <= ld, (r.id, k)
        if op.get("x2") and op["xs"] is not None:
            assert op["xs"][0] % 8 == 0
    assert sum(G.opts(r)["rs"][1] > 256 for r in G.ALL_ROWS) >= len(G.ALL_ROWS) - 1 and G.TAIL_DEFAULTS["ps"][1] > 256
    assert o("y-dense")["ys"] is None and o("y-slice-4")["ys"][0] == 4 and G.CONV_DEFAULTS["ys"][0] > 0
    conv = [G.opts(r) for r in G.CONV_ROWS]
    assert any(not c["res"] and c["bias"] for c in conv) and any(not c["bias"] and c["res"] for c in conv) and any(not c["bias"] and not c["res"] for c in conv)
    assert any(not c["relu_in"] for c in conv) and any(c["x2out"] and c["res"] for c in conv) and any(c["x2out"] and not c["res"] for c in conv)
    # scales: the caller's and the packed weight scale are powers of two other than 1, in both directions
    assert {np.sign(c["x_log2"]) for c in conv} == {-1, 0, 1}
    ws = {i: E.w_scale_of(G.conv_inputs(G.ROW_BY_ID[i])["w"]) for i in ("g-1x9x17", "wscale-down", "wscale-up")}
    assert ws["wscale-down"] < 1 < ws["g-1x9x17"] < ws["wscale-up"], ws
    tails = [G.opts(r) for r in G.TAIL_ROWS]
    for key, vals in (("x2", {True, False}), ("pre", {True, False}), ("res", {True, False}), ("act", {"relu", "none"}), ("gate_bias", {True, False})):
        assert {t[key] for t in tails} == vals, key
    assert {t["ln_eps"] for t in tails} == {1e-6, 1e-2}
    assert {(r.cin, G.opts(r)["x2"]) for r in G.TAIL_ROWS} >= {(256, True), (512, True), (512, False)}
    assert G.opts(G.TAPS)["taps"] and not G.opts(G.TAPS)["pre"]


def test_stage2_rows_reach_the_remainder_branch():
    counts = {r.id: ntiles_of(r) for r in G.TAIL_ROWS}
    assert {1, 7, 9, 15} <= set(counts.values()) and 8 in counts.values()
    assert {c & 7 for c in counts.values()} >= {0, 1, 7} and (15 >> 3, 15 & 7) == (1, 7) and (9 >> 3, 9 & 7) == (1, 1)
    for nt in sorted(set(counts.values()) | {ntiles_of(G.TAPS)}):
        assert sorted(E.stage2_tile(b, nt) for b in range(nt)) == list(range(nt)), nt
    # with a remainder the map is not the identity beyond 8 tiles: a kernel without the branch would write other tiles
    assert [E.stage2_tile(b, 9) for b in range(9)] != list(range(9)) and [E.stage2_tile(b, 15) for b in range(15)] != list(range(15))


# ---- EMU ------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", G.CONV_ROWS, ids=lambda r: r.id)
def test_conv_row_errors_are_the_recorded_ones(row):
    s, a = G.scheme_error(row), G.accumulation_error(row)
    print(f"{row.id}: S_row {s:.3e}, A_row {a:.3e} = {3 * a / s:.2f} of the bar S_row / 3")
    es, ea = G.EMU[row.id]
    assert abs(s - es) <= 0.02 * es and abs(a - ea) <= 0.02 * ea, (s, a)       # recorded to 3 digits
    assert 0 < s <= G.S_MAX
    assert a <= s / 3 / 4, "fp32 accumulation alone takes more than a quarter of the bar: choose other data"
    assert np.isfinite(G.conv_emulation(row)).all() and G.conv_emulation(row).shape == (row.n, row.h, row.w, 256)
    assert G.conv_emulation(row) is G.conv_emulation(row)                      # computed once, shared
    if row.n * row.h * row.w > SMALL:
        G.conv_emulation.cache_clear(), G.conv_exact.cache_clear(), G.conv_inputs.cache_clear()


@pytest.mark.parametrize("row", G.TAIL_ROWS, ids=lambda r: r.id)
def test_tail_row_errors_are_the_recorded_ones(row):
    g = G.graph_error(row)
    print(f"{row.id}: emulated graph vs exact {g:.3e}")
    assert abs(g - G.EMU_TAIL[row.id]) <= 0.02 * G.EMU_TAIL[row.id], g
    assert 0 < g <= G.S_MAX and 4 * g > 2e-6       # (a bar a bf16x3 epilogue can meet: test_gate_tail_gpu.py's kernels use ~ 0.1 of 2e-5)
    d, o = G.tail_inputs(row), G.opts(row)
    if o["x2"]:
        assert np.array_equal(E.x2_value(d["x"]), d["x"])
    else:
        assert not np.array_equal(E.x2_value(d["x"]), d["x"])                  # mul's low bits matter: hi + lo is not the fp32 value
    # every declared operand matters by far more than the bar
    ref, y = G.tail_emulation(row), E.conv(d["x"], d["w"])
    args = dict(bias=d["b"], pre=d["pre"] if o["pre"] else None, lnw=d["lnw"], lnb=d["lnb"], ln_eps=o["ln_eps"], act=o["act"], gate_w=d["gw"],
                gate_b=d["gb"] if o["gate_bias"] else None, mul=d["x"][..., :256], res=d["res"] if o["res"] else None)
    drops = [k for k in ("pre", "gate_b", "res") if args[k] is not None] + ["bias"]
    for k in drops:
        assert G.distance(E.gate_tail(y, **dict(args, **{k: None})), ref) > 100 * G.TAIL_TOL, k
    assert G.distance(E.gate_tail(y, **dict(args, act="none" if o["act"] == "relu" else "relu")), ref) > 100 * G.TAIL_TOL
    assert G.distance(E.gate_tail(y, **dict(args, ln_eps=1e-2 if o["ln_eps"] == 1e-6 else 1e-6)), ref) > 10 * G.TAIL_TOL


# ---- planted data ---------------------------------------------------------------------------------------------------------------------------------------------------

def xprime(row):
    d, o = G.conv_inputs(row), G.opts(row)
    return E.scaled_input(d["x"], o["relu_in"], 2.0 ** o["x_log2"])


def test_zero_block_rows():
    for rid, relu in (("zero-block", True), ("zero-block-c128-norelu", False)):
        row = G.ROW_BY_ID[rid]
        xs = xprime(row)
        bm = np.abs(xs.reshape(*xs.shape[:3], -1, 32)).max(-1)
        codes = E.block_codes(xs)
        assert (bm[:, :, 1::2, 1] == 0).all() and (codes[:, :, 1::2, 1] == 1).all()                      # the all-zero block: the clamped code
        assert (G.conv_inputs(row)["x"][:, :, 0::3, 0:32] < 0).all()                                    # the all-negative block ...
        assert (bm[:, :, 0::3, 0] == 0).all() == relu and (codes[:, :, 0::3, 0] == 1).all() == relu     # ... is all zero under the ReLU only
        assert (bm[:, :, 0::2, 1] > 0).all()
        r = xs - E.f16(xs)
        assert np.array_equal(E.q6(xs)[:, :, 1::2, 32:64], np.zeros_like(xs[:, :, 1::2, 32:64]))
        assert (E.block_codes(r)[:, :, 1::2, 1] == 1).all()


def test_outlier_row():
    xs = xprime(G.ROW_BY_ID["outlier"])
    b = np.abs(xs.reshape(*xs.shape[:3], -1, 32))
    rest = np.delete(b, 7, axis=-1).max(-1)
    assert (b[..., 0, 7] >= 2.0 ** 8 * rest[..., 0]).all()
    x = G.conv_inputs(G.ROW_BY_ID["outlier"])["x"]
    ratio = np.abs(x[..., 7]) / np.abs(np.delete(x[..., :32], 7, axis=-1)).max(-1)
    assert np.median(ratio) >= 2.0 ** 10    # 2^12 times the typical rest
    # the rest of such a block quantises to zero in q6(x): only the fp16 part carries it
    assert (np.delete(E.q6(xs)[..., :32], 7, axis=-1) == 0).mean() > 0.95


def test_pow2_row():
    xs = xprime(G.ROW_BY_ID["pow2"])
    bm = np.abs(xs.reshape(*xs.shape[:3], -1, 32)).max(-1)
    below = float(np.nextafter(np.float32(4), np.float32(0)))
    assert (bm[..., 0] == 4.0).all() and (bm[..., 1] == below).all() and below < 4.0
    codes = E.block_codes(xs)
    assert (codes[..., 0] == 127).all() and (codes[..., 1] == 126).all()      # one ulp apart, one binade of scale apart
    q = E.q6(xs)
    assert (q[..., 3] == 4.0).all()                                           # 4 in units of 2^0: exact
    assert (q[..., 40] == 3.75).all() and (np.abs(q[..., 32:64]) <= 3.75).all()   # 4 - ulp in units of 2^-1 is 7.99..: saturates at 7.5 x 2^-1


def test_f16exact_row():
    xs = xprime(G.ROW_BY_ID["f16exact"])
    r = xs - E.f16(xs)
    assert not r.any() and (E.block_codes(r) == 1).all() and not E.split_x(G.conv_inputs(G.ROW_BY_ID["f16exact"])["x"], True)[2].any()


def test_range_rows_plant_the_maximum_where_they_claim():
    for rid, pos in (("rng-00", (0, 0, 0, 5)), ("rng-last", (0, 8, 16, 33)), ("rng-blk", (0, 4, 9, 127))):
        row = G.ROW_BY_ID[rid]
        xs = np.abs(xprime(row))
        assert np.unravel_index(int(xs.argmax()), xs.shape) == pos and (xs == xs.max()).sum() == 1 and xs.max() == 37.5
        d, o = G.conv_inputs(row), G.opts(row)
        assert E.range_word(d["x"], o["relu_in"], 1.0) == int(np.float32(37.5).view(np.uint32))
    # (8, 16): the one live pixel of the last ragged tile of 9 x 17; channel 127: the last 32-channel block of the second superslab
    assert E.tile_origin(3, 1, 9, 17) == (0, 8, 16) and 127 // 32 == 3
    assert xprime(G.ROW_BY_ID["rng-blk"]).min() == -37.5                       # a negative maximum: |.|, no ReLU on that row
    for row in G.CONV_ROWS:                                                    # negative inputs under every input ReLU
        if G.opts(row)["data"] != "edges":
            assert (G.conv_inputs(row)["x"] < 0).mean() > 0.2 or G.opts(row)["data"] == "outlier", row.id


def test_edge_rows_hold_large_values_where_the_linear_neighbour_is():
    for rid in ("edge-1x9x17", "edge-2x8x16"):
        x = G.conv_inputs(G.ROW_BY_ID[rid])["x"]
        inner = np.abs(x[:, 1:-1, 1:-1]).mean()
        assert np.abs(x[:, :, 0]).mean() > 8 * inner and np.abs(x[:, :, -1]).mean() > 8 * inner
        assert np.abs(x[:, 0]).mean() > 8 * inner and np.abs(x[:, -1]).mean() > 8 * inner and (x >= 0).all()
    assert G.ROW_BY_ID["edge-2x8x16"].n == 2


def test_tie_row_sits_exactly_on_the_ties():
    row = G.TIE
    d = G.conv_inputs(row)
    xs = xprime(row)
    assert (E.f16(xs) == 1.5).all()
    r = xs - 1.5
    assert (E.block_codes(r) == 127 - 14).all()                               # every residual block's scale is 2^-14
    a = np.abs(r) / G.TIE_UNIT
    assert np.isin(a, G.TIE_MIDS).all()
    for blk in a.reshape(-1, 32)[:: 17]:
        assert sorted(blk) == sorted(G.TIE_MIDS)                              # all 31 midpoints (and 7.5) in every block
    assert (r > 0).any() and (r < 0).any()
    # weights: fp16-exact, one-hot per output channel, scale 1: w - f16 w = 0 and q6 w = w
    w = d["w"]
    assert E.w_scale_of(w) == 1.0 and ((w != 0).sum(axis=(1, 2, 3)) == 1).all() and set(np.unique(w)) == {0.0, 1.0}
    wh, qwr, qw = E.split_w(w, 1.0)
    assert np.array_equal(wh, qw) and not qwr.any()
    # the result minus the fp16 part is the quantised residual alone, and the tie rule shows in half of the elements
    ref = G.conv_emulation(row)
    q_even, q_down = E.q6(r), E.q6(r, tie="down")
    assert np.array_equal(ref[:, :, :, :64], 1.5 + q_even) and (q_even != q_down).mean() > 0.4
    assert float(np.abs(E.conv(d["x"], w, True, tie="down") - ref).max()) == 0.5 * G.TIE_UNIT
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)     # every expected value is an fp32 number: the comparison can be exact


# ---- discrimination: planted errors in the emulation ------------------------------------------------------------------------------------------------------------

def small(row):
    return row.n * row.h * row.w <= SMALL


def moved(row, **kw):
    d, o = G.conv_inputs(row), G.opts(row)
    y = G.conv_finish(E.conv(d["x"], d["w"], o["relu_in"], 2.0 ** o["x_log2"], **kw), row)
    return G.distance(y, G.conv_emulation(row))


def bar_of(row):
    return 0.0 if row is G.TIE else G.EMU[row.id][0] / 3


SMALL_ROWS = [r for r in G.CONV_ROWS + [G.TIE] if small(r)]


@pytest.mark.parametrize("row", SMALL_ROWS, ids=lambda r: r.id)
def test_planted_errors_move_the_emulation_by_more_than_the_bar(row):
    bar = bar_of(row)
    m = moved(row, swap=True)
    print(f"{row.id}: corrections swapped: {m / bar if bar else float('inf'):.0f} x the bar")
    assert m > 10 * bar and m > 0
    if G.opts(row)["data"] != "f16exact":                 # (a zero residual has no scale to get wrong)
        m = moved(row, resid_codes="main")
        print(f"{row.id}: residual on q6(x)'s scale: {m / bar if bar else float('inf'):.1f} x the bar")
        assert m > bar and m > 0
    if row.h >= 2:
        m = moved(row, pad=lambda p: E.pad_linear(p, "x"))
        print(f"{row.id}: halo column from the linear-memory neighbour: {m / bar if bar else float('inf'):.0f} x the bar")
        assert m > 100 * bar and m > 0
    if row.n >= 2:
        m = moved(row, pad=lambda p: E.pad_linear(p, "y"))
        print(f"{row.id}: halo row from the neighbouring image: {m / bar if bar else float('inf'):.0f} x the bar")
        assert m > 100 * bar and m > 0


def test_rows_claiming_the_halo_edges_exist():
    assert sum(r.h >= 2 for r in SMALL_ROWS) >= 20 and sum(r.n >= 2 for r in SMALL_ROWS) >= 4
    assert {G.opts(r)["data"] for r in SMALL_ROWS if r.n >= 2} >= {"randn", "edges"}


@pytest.mark.parametrize("rid", [i for i, (nt, _, _) in WALK_CLAIMS.items() if nt > 256])
def test_a_stale_first_superslab_moves_every_walked_tile(rid):
    """the tile at position k + 1 of a workgroup's walk convolved with tile k's first superslab (channels 0 .. 63 of its halo): per tile, by far above the bar"""
    row = G.ROW_BY_ID[rid]
    d, o = G.conv_inputs(row), G.opts(row)
    n, h, w = row.n, row.h, row.w
    tx, ty, nt = E.tile_grid(n, h, w)
    ws = E.w_scale_of(d["w"])
    full = lambda p: np.pad(p, ((0, 0), (1, 1 + ty * E.TH - h), (1, 1 + tx * E.TW - w), (0, 0)))  # noqa: E731  (the zero halo, out to whole tiles)
    xp = [full(p) for p in E.split_x(d["x"], o["relu_in"], 2.0 ** o["x_log2"])]
    wp = E.split_w(d["w"], ws)
    scale = max(1.0, float(np.abs(G.conv_emulation(row)).max()))
    bar = G.EMU[rid][0] / 3

    def patch(t, src=None):
        img, y0, x0 = E.tile_origin(t, n, h, w)
        out = [p[img:img + 1, y0:y0 + E.TH + 2, x0:x0 + E.TW + 2].copy() for p in xp]
        if src is not None:
            for a, b in zip(out, patch(src)[0]):
                a[..., :64] = b[..., :64]
        lh, lw = min(E.TH, h - y0), min(E.TW, w - x0)
        return out, (lh, lw)

    walks = [wk for wk in E.stage1_walks(nt) if len(wk) >= 2]
    assert len(walks) >= 7 and max(len(wk) for wk in walks) == (3 if nt > 512 else 2)
    pairs = [(wk[k], wk[k + 1]) for wk in walks[:3] + walks[-2:] + [wk for wk in walks if len(wk) == 3][:2] for k in range(len(wk) - 1)]
    worst = np.inf
    for prev, t in pairs:
        (good, (lh, lw)), stale = patch(t), patch(t, prev)[0]
        dy = (E.conv_valid(stale, wp) - E.conv_valid(good, wp))[0, :lh, :lw] / ws / 2.0 ** o["x_log2"]
        worst = min(worst, float(np.abs(dy).max()) / scale)
    print(f"{rid}: a stale first superslab moves a walked tile by >= {worst / bar:.0f} x the bar ({len(pairs)} tiles)")
    assert worst > 100 * bar
    G.conv_emulation.cache_clear(), G.conv_exact.cache_clear(), G.conv_inputs.cache_clear()
