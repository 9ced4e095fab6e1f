"""CPU side of tests/test_gate_tail_gpu.py: its tables, float64 references and data are sound before any kernel runs -- the expected kernel of
every row against a restatement of the dispatch predicates (gate_conv_shape_ok / gate_narrow_shape_ok of csrc/conv3x3_gate.hip, the strip rule of
conv_plan in csrc/igemm.hip), finite references of the right shape, discrimination (dropping any operand a row declares moves the reference by
>= 100 x the row's bar), a plain fp32 evaluation within 1/4 of the bar, the one-pass statistics missing it by >= 10 x on the offset case, the caps
on the data, the bf16 emulation errors recorded beside the bf16 cases, and the float64 roi_align against oracle.ops.roi_align.  Nothing here
loads the library."""
import pytest
import torch
import torch.nn.functional as F

import test_gate_tail_gpu as G
from oracle import ops as o_ops

ALL_TAIL = list(dict.fromkeys(G.SHAPE_CASES + G.OPERAND_CASES + G.STRESS_CASES + G.SLICE_CASES + [c for c, _ in G.BF16_CASES]))


def scale_of(ref):
    return max(1.0, float(ref.abs().max()))


# ---- dispatch predicates, restated ------------------------------------------------------------------------------------------------------

def gate_conv_shape_ok(h, w, cin, cout, ldx):
    """c256_shape_ok + gate_conv_shape_ok: 3x3 s1 p1 (every case), image below 2^29 elements, 256 columns, width >= one tile, whole slabs, bf16 modes"""
    return h * w * ldx < 2 ** 29 and cout == 256 and w >= 16 and cin >= 32 and cin % 32 == 0


def gate_narrow_shape_ok(h, w, cin, cout, ldx, ldy):
    """halo16_shape_ok + gate_narrow_shape_ok: the 8 x 32-pixel kernels' width and height terms, 32 / 128 columns, whole slabs"""
    return h * w * ldx < 2 ** 29 and w >= 24 and h >= 4 and cout in (32, 128) and cin >= 32 and cin % 32 == 0 and h * w * ldy < 2 ** 29


def strip_width(w):
    """conv_plan: a remainder of 1..8 columns behind the 32-pixel tile columns is a merged strip of 32 x 8 tiles (width >= 64)"""
    rem = w % 32
    return rem if rem != 0 and rem <= 8 and w >= 64 else 0


def dispatch(case):
    """ln_gate_impl's order: gate weights at 32 / 128 columns -> conv2d_impl (fmt must be 0) -> ConvHalo::GATE; else the 256-column contract"""
    cout, x_x2, _ = G.FAMILIES[case.fam]
    o = G.row_of(case)
    if o["gate"] and cout != 256:
        if x_x2 or not gate_narrow_shape_ok(case.h, case.w, case.cin, cout, case.cin, cout):
            return "reject"
        return {128: "h128", 32: "h32"}[cout]
    if not gate_conv_shape_ok(case.h, case.w, case.cin, cout, case.cin):
        return "reject"
    if x_x2 and (not o["gate"] or o["relu_in"]):
        return "reject"      # a pre-split input is taken by the gate kernel only (no input ReLU)
    return ("gx2" if x_x2 else "gate") if o["gate"] else "plain"


def test_tables_are_explicit_and_complete():
    assert set(G.OPERAND_TABLE) == set(G.FAMILIES) == set(G.FAMILY_KERNEL)
    for fam, rows in G.OPERAND_TABLE.items():
        assert set(rows) == set(G.ROWS), fam
        assert rows["all"] == G.FAMILY_KERNEL[fam]
    for cases in (G.SHAPE_CASES, G.OPERAND_CASES, G.STRESS_CASES, G.SLICE_CASES, [c for c, _ in G.BF16_CASES]):
        assert len({G.case_id(c) for c in cases}) == len(cases)
    assert {(c.fam, c.row) for c in G.OPERAND_CASES} == {(f, r) for f in G.FAMILIES for r in G.ROWS}
    assert {(c.fam, c.data) for c in G.STRESS_CASES} == {(f, d) for f in G.FAMILIES for d in ("offset", "zero", "sat")}
    assert {c.fam for c in G.SLICE_CASES} == set(G.FAMILIES) and any(c.data == "concat" for c in G.SLICE_CASES)
    assert all(c.n in (1, 3) for c in ALL_TAIL)
    assert G.TOL == 2e-5 and G.UNIT_TOL == 4e-5 and G.TAP_TOL == 3e-6 and G.BF16_CAP == 2e-2


def test_shape_lists_contain_the_edges_they_claim():
    hw = [(s[1], s[2]) for s in G.C256_SHAPES]
    assert hw == [(1, 16), (3, 16), (8, 16), (9, 17), (7, 31), (8, 32), (13, 33)]
    assert any(h % 8 == 0 and w % 16 == 0 for h, w in hw) and any(w % 16 == 1 for h, w in hw) and any(h < 8 for h, w in hw) and any(h == 1 for h, w in hw)
    assert any(h > 8 and w > 16 for h, w in hw)                                                   # several tiles on both axes
    assert {s[3] // 32 for s in G.C256_SHAPES} == {1, 2, 3, 4, 16}
    ragged = [s for s in G.C256_SHAPES if s[1] % 8 or s[2] % 16]
    assert {s[3] for s in ragged} == {32, 64, 96, 128, 512}                                       # every slab count on a ragged shape
    nhw = [(s[1], s[2]) for s in G.NARROW_SHAPES]
    assert nhw == [(4, 24), (5, 25), (8, 32), (9, 33), (8, 65), (9, 72), (5, 73)]
    assert {s[3] for s in G.NARROW_SHAPES} == {32, 96, 256}
    assert min(h for h, w in nhw) == 4 and min(w for h, w in nhw) == 24 and (8, 32) in nhw        # the contract's lower edge, the exact tile
    assert [strip_width(w) for h, w in nhw] == [0, 0, 0, 0, 1, 8, 0]                              # a strip with one live column, a full one, 73 = 64 + 9: none
    assert any(w % 32 == 1 and not strip_width(w) for h, w in nhw)                                # one live column in an ordinary tile
    for fam, s in G.OPS_SHAPE.items():
        assert s[0] == 3 and (s[1] % 8 and (s[2] % 16 if fam.startswith("c256") else strip_width(s[2])))
        y0, x0, bh, bw = G.ZERO_BLOCK
        assert y0 + bh <= s[1] and x0 + bw <= s[2] and bh >= 3 and bw >= 3


@pytest.mark.parametrize("case", ALL_TAIL, ids=G.case_id)
def test_expected_kernel_is_what_the_dispatch_predicates_give(case):
    assert G.expected_kernel(case) == dispatch(case)
    if case.row == "all":
        assert G.expected_kernel(case) == G.FAMILY_KERNEL[case.fam]


# ---- references ----------------------------------------------------------------------------------------------------------------------------

def ln32(y, lnw, lnb, eps):
    u = y.mean(1, keepdim=True)
    var = (y - u).pow(2).mean(1, keepdim=True)
    return (y - u) / torch.sqrt(var + eps) * lnw.view(1, -1, 1, 1) + lnb.view(1, -1, 1, 1)


def ln32_one_pass(y, lnw, lnb, eps):
    """E[y^2] - mean^2 in fp32: what a one-pass epilogue would compute"""
    u = y.mean(1, keepdim=True)
    var = (y * y).mean(1, keepdim=True) - u * u
    return (y - u) / torch.sqrt(var.clamp(min=0) + eps) * lnw.view(1, -1, 1, 1) + lnb.view(1, -1, 1, 1)


def eval32(case, ln=ln32):
    d, o = G.tail_inputs(case), G.row_of(case)
    x, mul = G.operand_values(case, d)
    y = F.conv2d(F.relu(x) if o["relu_in"] else x, d["w0"], None, padding=1)
    return G.tail_finish(y, d, o, mul, dt=torch.float32, ln=ln)


RUNNING = [c for c in ALL_TAIL if G.expected_kernel(c) != "reject"]


@pytest.mark.parametrize("case", RUNNING, ids=G.case_id)
def test_tail_reference(case):
    cout = G.FAMILIES[case.fam][0]
    d, o = G.tail_inputs(case), G.row_of(case)
    ref, stats = G.tail_ref(case)
    assert G.tail_ref(case)[0] is ref   # computed once, shared
    assert ref.dtype == torch.float64 and ref.shape == (case.n, cout, case.h, case.w) and bool(torch.isfinite(ref).all())
    bar = G.TOL * scale_of(ref)
    # caps on the data
    assert 0.25 <= stats["cut"] <= 0.75, stats["cut"]
    if o["gate"]:
        z = stats["z"]
        if case.data == "sat":
            q = cout // 4
            assert float((z[:, :q] > 50).double().mean()) == 1.0 and float((z[:, q:2 * q] < -50).double().mean()) == 1.0
            assert float((z > 50).double().mean()) >= 0.2 and float((z < -50).double().mean()) >= 0.2
            assert float(z[:, 2 * q:].abs().max()) <= 8.0
            m = d["mul"].double()
            assert float((ref[:, :q] - (G.x2_reconstruct(d["mul"]) if G.FAMILIES[case.fam][2] else d["mul"]).double()[:, :q] - d["res"].double()[:, :q]).abs().max()) <= 1e-40
            assert float((ref[:, q:2 * q] - d["res"].double()[:, q:2 * q]).abs().max()) <= 1e-40 * float(m.abs().max())
        else:
            assert float(z.abs().max()) <= 8.0, float(z.abs().max())
    # a plain fp32 evaluation stays within 1/4 of the bar: the inputs do not make a correct fp32 kernel fail
    e32 = float((eval32(case).double() - ref).abs().max())
    assert e32 <= bar / 4, (e32, bar)
    # discrimination: every declared piece matters by >= 100 x the bar
    y, mul = G.tail_conv(case), G.operand_values(case, d)[1]
    moved = lambda o2, y2=None, mul2=None: float((G.tail_finish(y if y2 is None else y2, d, o2, mul if mul2 is None else mul2) - ref).abs().max())  # noqa: E731
    for key in ("bias", "gate_bias", "mul", "res", "pre"):
        if o[key]:
            assert moved(dict(o, **{key: False})) >= 100 * bar, (key, moved(dict(o, **{key: False})), bar)
    if o["gate"]:
        assert float((G.tail_finish(y, d, dict(o, gate=False, mul=False, res=False), mul) - ref).abs().max()) >= 100 * bar
    if o["act"] == "relu":
        assert moved(dict(o, act="none")) >= 100 * bar
    if o["relu_in"]:
        assert moved(o, y2=G.conv64(G.operand_values(case, d)[0], d["w0"], False)) >= 100 * bar
    if o["ln_eps"] != 1e-6:
        assert moved(dict(o, ln_eps=1e-6)) >= 100 * bar, (moved(dict(o, ln_eps=1e-6)), bar)
    if case.data == "sat" and G.FAMILIES[case.fam][2]:   # mul as hi + lo (256 columns) against mul as it is
        assert moved(o, mul2=d["mul"]) >= 100 * bar, (moved(o, mul2=d["mul"]), bar)
    if case.data == "sat" and not G.FAMILIES[case.fam][2]:   # ... and the other way round at 32 / 128 columns
        assert moved(o, mul2=G.x2_reconstruct(d["mul"])) >= 100 * bar
    if case.data == "offset":
        one = float((eval32(case, ln=ln32_one_pass).double() - ref).abs().max())
        print(f"offset {G.case_id(case)}: two-pass fp32 {e32 / scale_of(ref):.2e}, one-pass {one / scale_of(ref):.2e} of the scale")
        assert one >= 10 * bar, (one, bar)
    if case.data == "zero":
        y0, x0, bh, bw = G.ZERO_BLOCK
        inner = (slice(None), slice(None), slice(y0 + 1, y0 + bh - 1), slice(x0 + 1, x0 + bw - 1))
        assert float((y[inner]).abs().max()) == 0.0            # the interior of the block sees only zeros: conv + bias is exactly the bias
        other = G.tail_finish(y, d, dict(o, ln_eps=1e-6), mul)
        assert float((other - ref)[inner].abs().max()) >= 100 * bar


@pytest.mark.parametrize("case,emu", G.BF16_CASES, ids=lambda v: G.case_id(v) if isinstance(v, G.Case) else f"emu{v:.2e}")
def test_bf16_emulation_error_is_the_recorded_one(case, emu):
    ref = G.tail_ref(case)[0]
    got = G.tail_emulate_bf16(case)
    e = float((got - ref).abs().max()) / scale_of(ref)
    print(f"bf16 emulation {G.case_id(case)}: {e:.3e}")
    assert abs(e - emu) <= 0.02 * emu, (e, emu)                   # recorded to 3 digits
    assert 100 * G.TOL <= G.bf16_bar(emu) <= G.BF16_CAP          # a bf16 bar, not a bf16x3 one, and never above the project's 2e-2


def test_x2_pack_is_the_format_of_the_header():
    v = G.rnd(3, 2, 3, 5, 16) * 7
    c = G.x2_pack(v)
    assert c.shape == v.shape and c.dtype == torch.float32
    assert torch.equal(G.x2_unpack(c), G.x2_reconstruct(v))
    # per 8 channels: 4 dwords of hi (element 2i in the low half), then 4 dwords of lo
    d = c.view(torch.int32)[0, 0, 0]
    hi = v[0, 0, 0].to(torch.bfloat16).float()
    assert torch.equal((d[:4] << 16).view(torch.float32), hi[0:8:2]) and torch.equal((d[:4] & -65536).view(torch.float32), hi[1:8:2])
    lo = (v[0, 0, 0] - hi).to(torch.bfloat16).float()
    assert torch.equal((d[4:8] << 16).view(torch.float32), lo[0:8:2]) and torch.equal((d[12:16] & -65536).view(torch.float32), lo[9:16:2])


# ---- tap tables ------------------------------------------------------------------------------------------------------------------------------

def test_tap_case_list_covers_what_it_claims():
    cases = G.TAP_CASES + G.TAP_SLICE_CASES
    assert {(c.kb, c.tile) for c in G.TAP_CASES} == {(k, t) for k in G.TAP_KNOTS for t in G.TAP_TILES}
    assert {(c.cout, c.frames) for c in G.TAP_CASES} == {(256, 1), (256, 2), (32, 1), (32, 2)}
    assert {(c.cout, c.frames) for c in G.TAP_SLICE_CASES} == {(256, 1), (32, 2)} and all(c.slices for c in G.TAP_SLICE_CASES)
    assert all(4 <= c.cin <= 8 for c in cases) and G.TAP_MAP[0] <= 12 and G.TAP_MAP[1] <= 16
    assert (0.5, 0.5) in G.TAP_KNOTS and all(0 < b <= 0.5 for kb in G.TAP_KNOTS for b in kb)
    assert len({G.tap_id(c) for c in cases}) == len(cases)


@pytest.mark.parametrize("case", G.TAP_CASES + G.TAP_SLICE_CASES, ids=G.tap_id)
def test_tap_case(case):
    H, W = G.TAP_MAP
    (oh, ow), s = case.tile, G.TAP_SCALE
    boxes = G.tap_boxes(case)
    # the arithmetic of PRV2_CHECK_TAPS (ops.CoarseTaps.gather): ROI bin == knot spacing
    b = boxes[:, -4:]
    bin_w, bin_h = (b[:, 2] - b[:, 0]) * s / ow, (b[:, 3] - b[:, 1]) * s / oh
    assert float((bin_h - case.kb[0]).abs().max()) < 1e-4 and float((bin_w - case.kb[1]).abs().max()) < 1e-4
    # inside the frame; the four corners are touched exactly
    assert float(b[:, :2].min()) >= 0.0 and float(b[:, 2].max()) <= W / s + 1e-4 and float(b[:, 3].max()) <= H / s + 1e-4
    assert b[0, 0] == 0 and b[0, 1] == 0 and abs(float(b[3, 2]) - W / s) < 1e-4 and abs(float(b[3, 3]) - H / s) < 1e-4
    # the last box starts exactly on a knot (sample (0, 0) = coarse pixel (3, 5))
    assert abs(float(b[6, 0]) * s - 0.5 + 0.5 * case.kb[1] - 5) < 1e-5 and abs(float(b[6, 1]) * s - 0.5 + 0.5 * case.kb[0] - 3) < 1e-5
    ref = G.tap_ref(case)
    assert ref.shape == (len(boxes), case.cout, oh, ow) and bool(torch.isfinite(ref).all())
    g = G.tap_g(case)
    assert g.shape == (case.frames, H, W, 9 * case.cout) and g.dtype == torch.float32
    bar = G.TAP_TOL * scale_of(ref)
    if case.frames > 1:   # tiles of both frames interleaved, one index below 0 and one >= B; the frame column matters for every tile
        f = boxes[:, 0].tolist()
        assert min(f) < 0 and max(f) >= case.frames and {0.0, 1.0} <= set(f) and f[:4] == [0.0, 1.0, 0.0, 1.0]
        swapped = boxes.clone()
        swapped[:, 0] = 1.0 - boxes[:, 0].clamp(0, 1)
        per_box = (G.tap_ref(case, swapped) - ref).abs().flatten(1).max(1).values
        assert float(per_box.min()) >= 100 * bar, (per_box, bar)
    assert float(ref.abs().max()) > 0.5


def test_roi_align64_is_the_oracle_roi_align():
    """the float64 restatement against oracle.ops.roi_align (fp32 throughout, torchvision's CPU kernel semantics) on every tap case's boxes, to
    1e-6: handed the oracle's own fp32 sample positions, so that what is compared is the rules (alignment, one sample per bin, clamps) and the
    interpolation.  With float64 positions the two are up to 4e-6 apart on the boxes whose coordinates are no dyadic numbers -- the fp32
    rounding of positions up to 16 coarse pixels, which the kernels under test carry too and which TAP_TOL has to absorb"""
    worst = 0.0
    for case in G.TAP_CASES:
        feat_, _, boxes = G.tap_inputs(case)
        b = boxes.clone()
        b[:, 0] = b[:, 0].clamp(0, case.frames - 1)
        want = o_ops.roi_align(feat_, b, case.tile, G.TAP_SCALE)
        got = G.roi_align64(feat_.double(), boxes, *case.tile, G.TAP_SCALE, pos=torch.float32)
        assert got.shape == want.shape
        assert float((got - want.double()).abs().max()) <= 1e-6 * scale_of(want), G.tap_id(case)
        got64 = G.roi_align64(feat_.double(), boxes, *case.tile, G.TAP_SCALE)
        worst = max(worst, float((got64 - want.double()).abs().max()) / scale_of(want))
    print(f"float64 positions against the fp32 oracle: {worst:.2e} of the scale")
    assert worst <= G.TAP_TOL / 2


def test_roi_align64_clamp_rules():
    """x <= 0 -> 0; lo >= n - 1 -> lo = hi = n - 1; below -1 or above n: zero"""
    v = torch.tensor([-1.5, -1.0, -0.3, 0.0, 2.25, 10.0, 10.7, 11.0, 11.5], dtype=torch.float64)
    lo, hi, l, inside = G.roi_axis64(v, 11)
    assert lo.tolist() == [0, 0, 0, 0, 2, 10, 10, 10, 10] and hi.tolist() == [1, 1, 1, 1, 3, 10, 10, 10, 10]
    assert l.tolist() == [0.0, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 0.0] and inside.tolist() == [False, True, True, True, True, True, True, True, False]


def test_unit_reference():
    for h, w in G.FOLD_SHAPES + [G.UNIT_SHAPE]:
        d = G.unit_inputs(h, w)
        b = d["boxes"]
        bin_w, bin_h = (b[:, 2] - b[:, 0]) * G.TAP_SCALE / w, (b[:, 3] - b[:, 1]) * G.TAP_SCALE / h
        assert float((bin_h - G.FOLD_KB[0]).abs().max()) < 1e-4 and float((bin_w - G.FOLD_KB[1]).abs().max()) < 1e-4
        assert float(b.min()) >= 0 and float(b[:, 2].max()) <= G.FOLD_MAP[1] / G.TAP_SCALE and float(b[:, 3].max()) <= G.FOLD_MAP[0] / G.TAP_SCALE
    assert (5 % 8, 17 % 16) == (5, 1) and (3 < 8, 16 % 16) == (True, 0) and G.FOLD_SHAPES == [(5, 17), (3, 16)] and G.UNIT_SHAPE == (9, 17)
    h, w = G.UNIT_SHAPE
    ref = G.unit_ref(h, w)
    assert ref.shape == (3, G.F_, h, w) and bool(torch.isfinite(ref).all())
    # the coarse half matters: without the ROI channels the unit is far from the reference
    d = G.unit_inputs(h, w)
    xe = G.x2_reconstruct(d["x"]).double()
    y = F.conv2d(xe, d["wf"][:, :G.F_].double(), d["bf"].double(), padding=1)
    t = F.relu(G.ln64(y, d["lnw"].double(), d["lnb"].double(), 1e-6))
    z = torch.einsum("oc,nchw->nohw", d["w3"].double(), t) + d["b3"].double().view(1, -1, 1, 1)
    assert float((xe * torch.sigmoid(z) + d["res"].double() - ref).abs().max()) >= 100 * G.UNIT_TOL * scale_of(ref)
