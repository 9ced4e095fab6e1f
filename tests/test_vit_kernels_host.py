"""CPU side of tests/test_vit_kernels_gpu.py: its format helpers, tables, float64 references and tolerances are sound before any kernel runs --
ss_encode / ss_decode are the header's format, every GEMM row takes the route it names (a restatement of gemm_ss_impl's predicates in
csrc/gemm_ss.hip), every attention shape hits the edge it is listed for, the float32 emulation of every GEMM, attention and LayerNorm case
stays inside half of the case's tolerance, and each deliberately wrong variant misses the reference by ten tolerances.  No GPU, no library."""
import numpy as np
import pytest
import torch

import test_vit_kernels_gpu as G


def miss(got, ref, tol):
    """max |got - ref| / tol"""
    return float(((got.double() - ref.double()).abs() / torch.as_tensor(tol, dtype=torch.float64)).max())


# ---- the format ----------------------------------------------------------------------------------------------------------------------
def test_format_round_trips_and_the_key_is_a_function_of_the_global_row():
    x = G.rnd(1, 40, 96) * 3
    hi, lo = G.ss_decode(G.ss_encode(x))
    assert torch.equal(hi, G.bf16(x)) and torch.equal(lo, G.bf16(x - hi)) and float((hi + lo - x).abs().max()) <= 2.0 ** -17 * float(x.abs().max())
    # one row's values on rows of different keys: the same eight slots per group in another order
    row = x[:1]
    slots = {r: G.ss_encode(row, row0=r).view(torch.int32).view(3, 8, 4) for r in (0, 2, 3, 6, 14, 16)}
    assert torch.equal(slots[0], slots[16]) and torch.equal(slots[2], slots[3]) and not torch.equal(slots[0], slots[2])
    for r, key in ((2, 1), (6, 3), (14, 7)):
        assert torch.equal(slots[r], slots[0][:, torch.arange(8) ^ key])
    # logical slots 0..3 are hi, 4..7 lo, eight channels each, in channel order (key 0)
    words = G.ss_encode(row).view(torch.int16).view(3, 8, 8)
    assert torch.equal(words[:, :4].reshape(-1), G.bf16(row).to(torch.bfloat16).view(torch.int16).reshape(-1))
    # row0 shifts the key: rows 5.. of a tensor == the same rows encoded alone at row0 = 5
    assert torch.equal(G.ss_encode(x)[5:].view(torch.int32), G.ss_encode(x[5:], row0=5).view(torch.int32))
    assert not torch.equal(G.ss_encode(x)[5:].view(torch.int32), G.ss_encode(x[5:]).view(torch.int32))
    hi5, lo5 = G.ss_decode(G.ss_encode(x)[5:], row0=5)
    assert torch.equal(hi5, hi[5:]) and torch.equal(lo5, lo[5:])
    # all eight keys within rows 0..15
    assert sorted(set(G.ss_key(torch.arange(16)).tolist())) == list(range(8))


def test_split_inputs_hold_what_they_are_listed_for():
    hi, lo = G.split(torch.tensor(G.SPECIALS))
    named = dict(zip(G.SPECIALS, zip(hi.tolist(), lo.tolist())))
    assert named[1.0] == (1.0, 0.0) and named[0.15625] == (0.15625, 0.0) and named[-2.5] == (-2.5, 0.0)
    assert named[1 + 3 * 2.0 ** -9] == (1 + 2.0 ** -7, -(2.0 ** -9)) and named[1 + 2.0 ** -8] == (1.0, 2.0 ** -8)
    assert named[1 + 2.0 ** -7 + 2.0 ** -8] == (1 + 2.0 ** -6, -(2.0 ** -8))
    assert all(np.isfinite(v).all() for v in named.values())
    for case in G.SPLIT_CASES:
        rows, c, ldx = case
        buf = G.split_input(case)
        assert c % 32 == 0 and ldx % 4 == 0 and bool(torch.isfinite(buf[:, :c]).all()) and bool(torch.isnan(buf[:, c:]).all())
    assert any(c[2] > c[1] for c in G.SPLIT_CASES) and any(c[0] >= 16 for c in G.SPLIT_CASES)
    x = G.tiny_input()
    assert 1e-39 < float(x.abs().min()) < 2.0 ** -126 and float(x.abs().max()) < 1e-29
    hi, lo = G.split(x)      # the bound is the format's own (sharp just above a power of two): the CPU split, which keeps subnormals, meets it
    assert miss(hi.double() + lo.double(), x, G.tiny_tol(x)) <= 1.0


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def ln_variant(c):
    """V of layernorm_kernel<V, true> (prv2_layernorm_ss)"""
    return 1 if c <= 256 else 2 if c <= 512 else 4 if c <= 1024 else 8


def test_layernorm_cases_sit_on_both_sides_of_every_boundary():
    cs = [c for _, c, _ in G.LN_CASES]
    assert all(c % 32 == 0 and c <= 2048 and ldx >= c and ldx % 4 == 0 for _, c, ldx in G.LN_CASES)
    for edge in (256, 512, 1024):
        assert edge in cs and edge + 32 in cs and ln_variant(edge) != ln_variant(edge + 32)
    assert 2048 in cs and {ln_variant(c) for c in cs} == {1, 2, 4, 8}
    assert any(rows > 4 and rows % 4 for rows, _, _ in G.LN_CASES) and any(ldx > c for _, c, ldx in G.LN_CASES)
    assert all(c % 32 or c > 2048 for c in G.LN_REFUSED)


@pytest.mark.parametrize("case", G.LN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_layernorm_emulation_within_half_the_tolerance(case):
    ref = G.ln_ref(case)
    assert miss(G.ln_emulation(case), ref, G.ln_tol(ref)) <= 0.5


# ---- GEMM rows -----------------------------------------------------------------------------------------------------------------------
def launch_of(M, K, N, env, y_ss, gelu):
    """gemm_ss_impl's choices (csrc/gemm_ss.hip) for one call"""
    force = int(env.get(G.TILE_ENV, 0))
    t256 = G.cdiv(M, 256) * G.cdiv(N, 256)
    big = force == 256 if force else (t256 >= 180 and t256 / (G.cdiv(t256, 256) * 256) >= 0.75)
    if big:
        tm, tn = G.cdiv(M, 256), G.cdiv(N, 256)
        blocked = tn % 8 == 0 and tm >= 8
        grid = (G.roundup(tm, 4) if blocked else tm) * tn
        persist = int(env.get(G.PERSIST_ENV, 1)) != 0 and (y_ss or not gelu)
        return dict(tile=256, stages=2, blocked=blocked, ids=grid, idle=grid - tm * tn, persist=persist, workgroups=min(grid, 256) if persist else grid,
                    ppb=int(env.get(G.PPB_ENV, 2)))
    tm, tn = G.cdiv(M, 128), G.cdiv(N, 128)
    if not force and tm * tn < 256:      # small
        tiles = G.cdiv(M, 64) * G.cdiv(N, 64)
        return dict(tile=64, stages=4 if tiles <= 256 else 2, blocked=False, ids=tiles, idle=0, persist=False, workgroups=tiles)
    blocked = tn % 8 == 0 and tm >= 64
    grid = (G.roundup(tm, 4) if blocked else tm) * tn
    return dict(tile=128, stages=2, blocked=blocked, ids=grid, idle=grid - tm * tn, persist=False, workgroups=grid)


def test_every_gemm_row_takes_the_route_it_names():
    routes = set()
    for c in G.GEMM_CASES:
        assert c.M > 0 and c.K % 32 == 0 and c.N % 8 == 0 and (not c.heads or c.N == 192 * c.heads)
        assert c.epis and all((e not in ("E5", "E6", "E7") or c.N % 32 == 0) for e in c.epis)
        if c.M > 300:
            assert c.K <= 96
        for env in c.envs:
            for epi in c.epis:
                e = G.EPI[epi]
                got = launch_of(c.M, c.K, c.N, env, e.ss, e.gelu)
                assert got["tile"] == c.tile, (c, env)
                want_persist = env.get(G.PERSIST_ENV) == "1" and (e.ss or not e.gelu)
                assert got["persist"] == want_persist, (c, env, epi)
                if c.route == "64x4":
                    assert got["stages"] == 4 and not env
                elif c.route == "64x2":
                    assert got["stages"] == 2 and not env and G.cdiv(c.M, 128) * G.cdiv(c.N, 128) < 256
                elif c.route in ("128", "256"):
                    assert not got["blocked"]
                elif c.route in ("128-blocked", "256-blocked"):
                    assert got["blocked"] and got["idle"] > 0 and got["idle"] % G.cdiv(c.N, c.tile) == 0
                elif c.route == "256-walk":
                    assert got["blocked"] and got["persist"] and got["ids"] > 256 == got["workgroups"] and got["idle"] > 0 and got["ppb"] in (1, 2)
                    assert (c.K // 32) % 2 == 1      # an odd slab count: the stage parity differs from tile to tile
                routes.add((c.route, got["persist"]))
    assert {r for r, _ in routes} == {"64x4", "64x2", "128", "128-blocked", "256", "256-blocked", "256-walk"}
    assert ("256", True) in routes and ("256", False) in routes
    slabs = [c.K // 32 for c in G.GEMM_CASES if c.route == "64x4"]
    assert min(slabs) == 1 and max(slabs) > 4       # fewer slabs than the four stages; the ring wraps
    assert sorted(c.M for c in G.GEMM_CASES if c.M > 300) == [1025, 2050, 4400, 8200]
    assert {e for c in G.GEMM_CASES if c.M > 1025 for e in c.epis} == {"E4", "E6"}
    assert {c.envs[i].get(G.PPB_ENV) for c in G.GEMM_CASES if c.route == "256-walk" for i in range(len(c.envs))} == {"1", "2"}
    assert {e for c in G.GEMM_CASES for e in c.epis} == set(G.EPI)


def test_gelu_fast_restatement_and_its_term():
    d, g = G.gelu_term()
    print(f"[vit] gelu_fast: max error {d:.3e} over [-8, 8]")
    assert 0 < d <= 6e-7 and g == 2 * d
    v = np.array([0.0, -0.0, 1.0, -1.0, 8.0, -8.0, 30.0, -30.0], dtype=np.float32)
    assert np.allclose(G.gelu_fast32(v), G.gelu64(torch.from_numpy(v).double()).numpy(), atol=6e-7) and G.gelu_fast32(v).dtype == np.float32


@pytest.mark.parametrize("ci", range(len(G.GEMM_CASES)), ids=lambda ci: f"{G.GEMM_CASES[ci].M}x{G.GEMM_CASES[ci].K}x{G.GEMM_CASES[ci].N}")
def test_gemm_emulation_within_half_the_tolerance(ci):
    for epi in G.GEMM_CASES[ci].epis:
        ref, tol = G.gemm_ref(ci, epi)
        share = miss(G.gemm_emulation(ci, epi), ref, tol)
        print(f"[vit] gemm emulation {G.gemm_run_id((ci, 0, epi))}: {share:.3f}")
        assert share <= 0.5, (ci, epi, share)


SMALL_GEMMS = [ci for ci, c in enumerate(G.GEMM_CASES) if c.M <= 300]


def worst_miss(mutant, epis):
    return max((miss(G.gemm_emulation(ci, epi, **mutant), *G.gemm_ref(ci, epi)) for ci in SMALL_GEMMS for epi in G.GEMM_CASES[ci].epis if epi in epis),
               default=0.0)


@pytest.mark.parametrize("name,mutant,epis", [
    ("the lo hi product dropped", dict(drop_lo_hi=True), ("E0", "E1", "E3", "E5")),
    ("the q scale in front of the bias", dict(scale_first=True), ("E7",)),
    ("the swizzle key from row instead of row >> 1", dict(a_key=lambda row: row & 7), ("E0", "E1")),
    ("hi and lo slots exchanged", dict(a_swap=True), ("E0", "E1")),
    ("GELU in front of the bias", dict(gelu_first=True), ("E2", "E6")),
], ids=lambda v: v.replace(" ", "-") if isinstance(v, str) else None)
def test_wrong_gemm_variants_miss_by_ten_tolerances(name, mutant, epis):
    worst = worst_miss(mutant, epis)
    print(f"[vit] {name}: {worst:.1f} tolerances")
    assert worst >= 10, (name, worst)


# ---- attention shapes --------------------------------------------------------------------------------------------------------------------
# shape -> (keys in the masked tile (0: none), full key tiles, live waves of the last query block, a later image starts at an odd global row)
ATT_EDGES = {
    (1, 1, 1): (1, 0, 1, False),
    (2, 33, 1): (33, 0, 2, True),
    (1, 63, 2): (63, 0, 2, False),          # only a masked tile
    (1, 64, 1): (0, 1, 2, False),           # no masked tile
    (3, 65, 2): (1, 1, 3, True),            # one key masked in; the third wave holds one query
    (1, 127, 1): (63, 1, 4, False),
    (1, 128, 1): (0, 2, 4, False),
    (2, 129, 3): (1, 2, 1, True),           # one query in the second query block: three waves retire
    (1, 193, 1): (1, 3, 3, False),
    (1, 257, 2): (1, 4, 1, False),
}


def test_every_attention_shape_hits_its_edge():
    assert list(ATT_EDGES) == G.ATT_SHAPES
    for (b, n, h), (masked, full, live, odd) in ATT_EDGES.items():
        assert (n % G.AT_BK, n // G.AT_BK) == (masked, full)
        last_block = n - (G.cdiv(n, G.AT_BQ) - 1) * G.AT_BQ
        assert G.cdiv(last_block, 32) == live
        assert any((i * n) % 2 for i in range(b)) == odd
        keys = G.spike_keys(n)
        if n >= 3:
            assert keys[:2] == [2, n - 1] and len(set(keys)) == len(keys) <= len(G.SPIKE_FACTORS)
            assert all(4 <= f <= 6 for f in G.SPIKE_FACTORS)
            first_of_last = (n - 1) // G.AT_BK * G.AT_BK
            assert first_of_last in keys and (masked == 0 or all(k >= full * G.AT_BK for k in (n - 1, first_of_last)))
            inp = G.att_inputs((b, n, h))
            for j, key in enumerate(keys):      # the spike key wins its query's row by a wide margin
                s = (inp.q[:, :, G.spike_query(j, n)] * inp.k[:, :, key]).sum(-1) / 8
                assert float(s.min()) > 15
        else:
            assert keys == []
        inp = G.att_inputs((b, n, h))
        ld = inp.bias_rows.shape[2]
        assert ld == G.roundup(n, G.AT_BK) + G.ATT_LD_EXTRA.get((b, n, h), 0) and ld % 4 == 0
        assert bool(torch.isnan(inp.bias_rows[:, :, n:]).all()) and bool(torch.isfinite(inp.bias_rows[:, :, :n]).all())
        assert float(inp.bias.max()) < 0
        hi, lo = G.ss_decode(inp.qkv_ss)
        assert float((hi + lo - torch.cat([inp.qkv[:, :h * 64] * np.float32(G.Q_SCALE), inp.qkv[:, h * 64:]], 1)).abs().max()) < 1e-3
    assert any(masked == 1 and live == 1 and h > 1 for (_, _, h), (masked, _, live, _) in ATT_EDGES.items())
    assert G.ATT_DENSE_IMAGE[1] % 4 and set(G.ATT_LD_EXTRA) <= set(G.ATT_SHAPES) and G.ATT_DENSE_IMAGE in G.ATT_SHAPES and G.ATT_BF16_ONCE in G.ATT_SHAPES


@pytest.mark.parametrize("shape", G.ATT_SHAPES, ids=G.att_id)
def test_attention_emulation_within_half_the_bar(shape):
    inp = G.att_inputs(shape)
    for with_bias in (False, True):
        ref = G.att_ref(shape, with_bias)
        for out_ss in (False, True):
            share = miss(G.attention_split32(inp.q, inp.k, inp.v, inp.bias if with_bias else None, out_ss), ref, G.att_tol(ref, G.BF16_BAR))
            print(f"[vit] attention emulation {G.att_id(shape)} bias {with_bias} ss {out_ss}: {share:.3f}")
            assert share <= 0.5
        f32 = G.as_rows(((inp.q @ inp.k.transpose(-1, -2)) * 0.125 + (inp.bias if with_bias else 0)).softmax(-1) @ inp.v)
        assert miss(f32, ref, G.att_tol(ref, G.F32_BAR)) <= 0.5


def phantom_key(inp):
    """one key too many: score 0 (zero k row, its bias column never added), zero v"""
    b, h, n, _ = inp.q.shape
    s = torch.cat([inp.q.double() @ inp.k.double().transpose(-1, -2) / 8 + inp.bias.double(), torch.zeros(b, h, n, 1, dtype=torch.float64)], -1)
    return G.as_rows(s.softmax(-1)[..., :n] @ inp.v.double())


def last_key_lost(inp):
    return G.attention64(inp.q, inp.k[:, :, :-1], inp.v[:, :, :-1], inp.bias[:, :, :-1])


def bias_not_in_base_2(inp):
    """the bias added to base-2 scores as it is: worth bias ln 2 in the natural domain"""
    return G.attention64(inp.q, inp.k, inp.v, inp.bias.double() * np.log(2.0))


def heads_major(inp):
    """qkv rows read as [heads][3][64] instead of [3][heads][64]"""
    b, h, n, _ = inp.q.shape
    q, k, v = (t.permute(0, 2, 1, 3) for t in inp.qkv.reshape(b, n, h, 3, 64).unbind(3))
    return G.attention64(q, k, v, inp.bias)


def lo_hi_dropped(inp):
    return G.attention_split32(inp.q, inp.k, inp.v, inp.bias, drop_lo_hi=True)


ATT_MUTANTS = [("one phantom key", phantom_key, 1), ("the last key lost", last_key_lost, 1), ("bias x 1 instead of x log2 e", bias_not_in_base_2, 1),
               ("the head order [heads][3]", heads_major, 2), ("the lo hi product of the scores dropped", lo_hi_dropped, 1)]


@pytest.mark.parametrize("name,mutant,min_heads", ATT_MUTANTS, ids=[m[0].replace(" ", "-") for m in ATT_MUTANTS])
def test_wrong_attention_variants_miss_by_ten_bars(name, mutant, min_heads):
    shapes = [s for s in G.ATT_SHAPES if s[1] >= 33 and s[2] >= min_heads]
    assert len(shapes) >= 3
    for shape in shapes:
        ref = G.att_ref(shape, True)
        m = miss(mutant(G.att_inputs(shape)), ref, G.att_tol(ref, G.BF16_BAR))
        print(f"[vit] {name} at {G.att_id(shape)}: {m:.1f} bars")
        assert m >= 10, (name, shape, m)


# ---- the bias image and the block ----------------------------------------------------------------------------------------------------------
def test_bias_image_restatement():
    for heads, n, ld in G.PACK_CASES:
        assert ld >= n and G.image_bytes(heads, n) % (heads * 8 * 64 * 16) == 0
        rows = G.pack_input((heads, n, ld))
        img = G.bias_image(rows.numpy(), n).reshape(heads, -1, G.cdiv(n, G.AT_BK), 8, 64, 4)
        assert img.size * 4 == G.image_bytes(heads, n) and np.isfinite(img).all()
        # every (q, key) once, every other word zero
        assert int((img != 0).sum()) == heads * n * n
        want = rows[0, n - 1, n - 1].item() * np.float32(1.4426950408889634)
        q, key = n - 1, n - 1
        t, g, half, e = (key % 64) // 32, (key % 32) // 8, (key % 8) // 4, key % 4
        assert img[0, q // 32, key // 64, 4 * t + g, 32 * half + q % 32, e] == np.float32(want)
    assert [c[2] == c[1] for c in G.PACK_CASES].count(True) == 1 and any(c[2] > c[1] for c in G.PACK_CASES)


def test_block_emulation_sets_a_tolerance_that_discriminates():
    ref, tol = G.block64(), G.block_tol()
    top = float(ref.abs().max())
    print(f"[vit] block: emulation error {tol / 4:.3e}, tolerance {tol:.3e}, max|ref| {top:.3f}")
    assert 0 < tol <= 4 * G.BF16_BAR * max(1.0, top)       # no looser than four of the attention kernels' own bars
    wrong = miss(G.block64(1 / G.Q_SCALE), ref, tol)        # the q scale in front of the qkv bias
    print(f"[vit] block, the q scale in front of the bias: {wrong:.1f} tolerances")
    assert wrong >= 10
