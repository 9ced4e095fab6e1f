"""Temporal stabilisation, the host side: the numpy specification temporal.temporal_step_host (hand-checked values, every branch, the
special pixels, the flicker property), TemporalStabilizer on CPU tensors, the C ABI / ctypes / torch-op plumbing, the argument checks
that need no GPU, the CLI's argument errors and Tester.run with the flag on a CPU stub model."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from patchrefinerv2_amd import temporal as T  # noqa: E402

F32 = np.float32
INF, NAN = float("inf"), float("nan")
SYMBOLS = ("prv2_temporal_workspace_bytes", "prv2_temporal_step")


def _grey(h, w, value=0.5):
    return np.full((3, h, w), value, dtype=F32)


def _ramp(h, w, lo=1.0, hi=4.0):
    """a static scene: a smooth ramp in metres"""
    return (lo + (hi - lo) * (np.arange(h * w, dtype=np.float64).reshape(h, w) / (h * w - 1))).astype(F32)


def _step(x, image, state, **kw):
    out, state, row = T.temporal_step_host(x, image, state, **kw)
    return out, state, T.stats_dict(row, x.size)


def test_luma_is_the_point_clouds_bytes_weighted():
    from patchrefinerv2_amd.output import color_bytes, sample_indices
    img = np.zeros((3, 2, 3), dtype=F32)
    img[0] = [[0.0, 1.0, 0.5], [0.25, NAN, 2.0]]
    img[1] = [[0.0, 1.0, 0.5], [0.5, 0.1, -1.0]]
    img[2] = [[0.0, 1.0, 0.5], [1.0, 0.9, 0.3]]
    L = T.luma_host(img, 2, 3)
    # bytes: 0.5 * 255 = 127.5 -> 128 (ties to even); 0.25 -> 63.75 -> 64; NaN -> 0; 2.0 -> 255; -1 -> 0; 0.1 -> 25.5 -> 26 (fp32: 25.500002);
    # 0.9 -> 229.5 -> 230 (fp32 229.50002); 0.3 -> 76.5 -> 77 (fp32 76.50001)
    want = [[0, 255, 128], [(77 * 64 + 150 * 128 + 29 * 255 + 128) >> 8, (150 * 26 + 29 * 230 + 128) >> 8, (77 * 255 + 29 * 77 + 128) >> 8]]
    assert L.dtype == np.uint8 and L.tolist() == want
    # an image of another size is sampled as the cloud samples it
    big = np.random.default_rng(0).random((3, 5, 7)).astype(F32)
    sy, sx = sample_indices(2, 5), sample_indices(3, 7)
    r, g, b = (color_bytes(big[c][sy][:, sx] * F32(255)).astype(int) for c in range(3))
    assert np.array_equal(T.luma_host(big, 2, 3), (77 * r + 150 * g + 29 * b + 128) >> 8)
    with pytest.raises(ValueError, match="image"):
        T.luma_host(np.zeros((2, 3)), 2, 3)


def test_hand_checked_2x3():
    """six pixels are fewer than the minimum count of 64, so the second frame is a scene cut: out = x -- but the masks, the five sums
    and the change sums are all there to check by hand"""
    img0, img1 = _grey(2, 3, 0.5), _grey(2, 3, 0.5)
    img1[:, 0, 2] = 0.6  # luma 128 -> 153: not static at tau = 6
    y = np.array([[1.0, 2.0, 4.0], [2.0, 1.0, 8.0]], dtype=F32)
    x = np.array([[1.5, 2.0, 4.0], [0.5, NAN, 8.25]], dtype=F32)
    out, st, s0 = _step(y, img0, None)
    assert s0["reset"] and s0["n"] == 0 and s0["n_gate"] == 0 and s0["sums"] == (0, 0, 0, 0) and s0["change_before"] == 0.0
    assert np.array_equal(out, y) and np.array_equal(st[1], np.full((2, 3), 128, np.uint8))
    out, st, s1 = _step(x, img1, st)
    # gate: (0, 2) fails the luma test and (1, 1) is NaN -> 4 gated pixels.  Fit mask |x - y| <= y / 2: (0, 0) 0.5 <= 0.5, (0, 1) 0 <= 1,
    # (1, 0) 1.5 > 1 is out, (1, 2) 0.25 <= 4 -> m = (0, 0), (0, 1), (1, 2): qx = 384, 512, 2112; qy = 256, 512, 2048
    assert s1["reset"] and not s1["fitted"] and s1["scale"] == 1.0 and s1["shift"] == 0.0
    assert s1["n_gate"] == 4 and s1["n"] == 3 and s1["static_fraction"] == 4 / 6
    assert s1["sums"] == (384 + 512 + 2112, 384 ** 2 + 512 ** 2 + 2112 ** 2, 384 * 256 + 512 * 512 + 2112 * 2048, 256 + 512 + 2048)
    # change: 0.5 / 1 -> 32768; 0; 1.5 / 2 -> 49152; 0.25 / 8 -> 2048
    assert s1["change_before_sum"] == 32768 + 0 + 49152 + 2048 == s1["change_after_sum"]
    assert s1["change_before"] == (32768 + 49152 + 2048) / (65536.0 * 4)
    assert out.tobytes() == x.tobytes() and st[0] is out and st[1][0, 2] == 153


def _fit_case(h=8, w=16):
    y = _ramp(h, w, 1.0, 3.0)
    y = np.rint(y * 256).astype(F32) / F32(256)  # on the fixed-point grid: the fit sees the values themselves
    return y, _grey(h, w)


def test_fit_recovers_an_exact_scale_and_shift():
    y, img = _fit_case()
    x = ((y.astype(np.float64) - 0.25) / 1.25)
    x = (np.rint(x * 256) / 256).astype(F32)
    _, st, _ = _step(y, img, None)
    for anchor in (1.0, 0.5, 0.0):
        out, _, s = _step(x, img, st, alpha=0.0, anchor=anchor)
        assert not s["reset"] and s["fitted"] and s["n"] == s["n_gate"] == y.size
        # the fit of the rounded x: close to 1.25 and 0.25, scaled towards the identity by the anchor
        assert abs(s["scale"] - (1 + anchor * 0.25)) < 2e-3 * max(anchor, 1e-9) + 1e-15
        assert abs(s["shift"] - anchor * 0.25) < 4e-3 * max(anchor, 1e-9) + 1e-15
        want = (np.float64(s["scale"]) * x.astype(np.float64) + np.float64(s["shift"])).astype(F32)
        assert out.tobytes() == want.tobytes()  # alpha = 0: no blend
        if anchor == 0.0:
            assert s["scale"] == 1.0 and s["shift"] == 0.0 and out.tobytes() == x.tobytes()
        if anchor == 1.0:
            assert np.abs(out - y).max() < 6e-3 and s["change_after"] < s["change_before"] / 20


def test_the_normal_equations_by_hand():
    """two depth levels: the sums and the 2 x 2 solution in closed form"""
    h, w = 8, 16
    y = np.where(np.arange(h * w).reshape(h, w) % 2 == 0, 2.0, 4.0).astype(F32)
    x = np.where(y == 2.0, 1.5, 3.5).astype(F32)  # y = x + 0.5
    img = _grey(h, w)
    _, st, _ = _step(y, img, None)
    out, _, s = _step(x, img, st, alpha=0.5, rho=0.25, anchor=1.0)
    assert s["n"] == 128 and s["sums"] == (64 * (384 + 896), 64 * (384 ** 2 + 896 ** 2), 64 * (384 * 512 + 896 * 1024), 64 * (512 + 1024))
    assert s["fitted"] and s["scale"] == 1.0 and s["shift"] == 0.5
    assert out.tobytes() == y.tobytes()  # aligned exactly: r = 0, w = alpha, the blend of equal values
    assert s["change_before_sum"] == 64 * (16384 + 8192) and s["change_after_sum"] == 0


def test_first_frame_and_shape_change_reset():
    x, img = _ramp(8, 16), _grey(8, 16)
    out, st, s = _step(x, img, None)
    assert s["reset"] and out.tobytes() == x.tobytes() and s["scale"] == 1.0 and s["shift"] == 0.0 and not s["fitted"]
    out2, st2, s2 = _step(x * F32(1.02), img, st, anchor=1.0)
    assert not s2["reset"] and s2["fitted"]
    x3 = _ramp(8, 20)
    out3, st3, s3 = _step(x3, _grey(8, 20), st2)  # another shape: as without a state
    assert s3["reset"] and s3["n_gate"] == 0 and out3.tobytes() == x3.tobytes() and st3[0].shape == (8, 20)


def test_scene_cut():
    y, img = _fit_case(16, 16)  # 256 pixels, minimum count 64
    _, st, _ = _step(y, img, None)
    cut = _grey(16, 16)
    cut[:, :, 4:] = 0.9  # three quarters of the image changed: 64 static pixels are just enough
    x = y * F32(1.1)
    _, _, s = _step(x, cut, st)
    assert s["n_gate"] == 64 and not s["reset"] and s["fitted"]
    cut[:, 0, 3] = 0.9  # one more
    out, st2, s = _step(x, cut, st)
    assert s["n_gate"] == 63 and s["n"] == 63 and s["reset"] and not s["fitted"] and out.tobytes() == x.tobytes()
    assert s["change_before_sum"] == s["change_after_sum"] > 0
    assert np.array_equal(st2[1], T.luma_host(cut, 16, 16)) and st2[0] is out


def test_constant_map_is_identity():
    img = _grey(8, 16)
    y, x = np.full((8, 16), 2.0, F32), np.full((8, 16), 2.5, F32)
    _, st, _ = _step(y, img, None)
    out, _, s = _step(x, img, st, alpha=0.5, rho=0.25)
    assert not s["reset"] and not s["fitted"] and s["n"] == 128 and s["scale"] == 1.0 and s["shift"] == 0.0  # det = 0
    # identity, then the blend: r = 0.5 / 2 = 0.25, r / rho = 1, w = 0.25, out = 2.5 + 0.25 * (2 - 2.5) = 2.375
    assert np.all(out == F32(2.375))
    assert s["change_before_sum"] == 128 * 16384 and s["change_after_sum"] == 128 * 12288


def test_fitted_scale_out_of_bounds_is_identity():
    img = _grey(8, 16)
    x = np.rint(_ramp(8, 16, 1.0, 1.2) * 256).astype(F32) / F32(256)
    y = F32(3) * x - F32(2)  # slope 3 inside the fit gate |x - y| <= y / 2
    _, st, _ = _step(y, img, None)
    out, _, s = _step(x, img, st, alpha=0.0, anchor=1.0)
    assert not s["reset"] and s["n"] == 128 and not s["fitted"] and s["scale"] == 1.0 and s["shift"] == 0.0 and out.tobytes() == x.tobytes()
    y2 = F32(1.9) * x - F32(0.9)  # slope 1.9: inside the bounds
    _, st, _ = _step(y2, img, None)
    assert _step(x, img, st, anchor=1.0)[2]["fitted"]


def test_alpha_tau_and_parameter_checks():
    rng = np.random.default_rng(5)
    y, _ = _fit_case(16, 32)
    img0 = rng.random((3, 16, 32)).astype(F32)
    img1 = np.clip(img0 + rng.integers(-3, 4, size=(1, 16, 32)).astype(F32) / F32(255), 0, 1).astype(F32)
    x = y * F32(1.03) + F32(0.01)
    _, st, _ = _step(y, img0, None)
    dl = np.abs(T.luma_host(img1, 16, 32).astype(int) - st[1].astype(int))
    assert dl.min() == 0 and 2 <= dl.max() <= 6
    for tau in (0, 1, 255):
        _, _, s = _step(x, img1, st, tau=tau)
        assert s["n_gate"] == int((dl <= tau).sum())
    assert _step(x, img1, st, tau=255)[2]["n_gate"] == y.size
    out0, _, s0 = _step(x, img1, st, alpha=0.0)
    want = (np.float64(s0["scale"]) * x.astype(np.float64) + np.float64(s0["shift"])).astype(F32)
    assert out0.tobytes() == want.tobytes()
    out5, _, s5 = _step(x, img1, st, alpha=0.5)
    assert s5["scale"] == s0["scale"] and s5["change_after_sum"] < s0["change_after_sum"] and out5.tobytes() != out0.tobytes()
    for kw, msg in ((dict(alpha=1.0), "alpha"), (dict(alpha=-0.1), "alpha"), (dict(alpha=NAN), "alpha"), (dict(tau=256), "tau"), (dict(tau=-1), "tau"),
                    (dict(tau=1.5), "tau"), (dict(rho=0.0), "rho"), (dict(rho=INF), "rho"), (dict(rho=NAN), "rho"), (dict(anchor=1.1), "anchor"),
                    (dict(anchor=-0.1), "anchor"), (dict(anchor=NAN), "anchor")):
        with pytest.raises(ValueError, match=msg):
            T.temporal_step_host(x, img1, st, **kw)
        with pytest.raises(ValueError, match=msg):
            T.TemporalStabilizer(**kw)
    with pytest.raises(ValueError, match="h, w"):
        T.temporal_step_host(x[None], img1, None)


def special_pixels(x, y):
    """the pixels that must pass through and stay out of the fit, written into copies of a frame x and its predecessor y"""
    x, y = x.copy(), y.copy()
    flat_x, flat_y = x.reshape(-1), y.reshape(-1)
    for i, v in enumerate((NAN, INF, -INF, 0.0, -1.5, 1024.0, 5000.0, 3.0e38, 1e-4)):
        flat_x[3 + 2 * i] = v
    for i, v in enumerate((NAN, INF, 0.0, -2.0, 1024.0, 2000.0)):
        flat_y[30 + 3 * i] = v
    flat_x[60], flat_y[60] = 1500.0, 1400.0   # both valid and static but beyond the fixed-point cap: blended, not fitted
    flat_x[61], flat_y[61] = 0.001, 0.0012    # q rounds to 0: not fitted
    flat_x[62], flat_y[62] = 0.5, 2.0         # outside the fit gate
    return x, y


def test_special_pixels_pass_through_and_stay_out_of_the_fit():
    y0, img = _fit_case(16, 32)
    x0 = ((y0.astype(np.float64) - 0.1) / 1.05).astype(F32)
    x, y = special_pixels(x0, y0)
    _, st, _ = _step(y, img, None)
    out, _, s = _step(x, img, st, anchor=1.0)
    _, st0, _ = _step(y0, img, None)
    clean = np.ones(x.shape, bool)
    clean.reshape(-1)[[3 + 2 * i for i in range(9)] + [30 + 3 * i for i in range(6)] + [60, 61, 62]] = False
    # the fit is the fit of the clean pixels alone
    xm, ym = np.where(clean, x0, F32(0)), y0
    _, _, sc = _step(np.where(clean, x0, NAN).astype(F32), img, st0, anchor=1.0)
    assert s["fitted"] and s["n"] == int(clean.sum()) == sc["n"] and s["sums"] == sc["sums"] and s["scale"] == sc["scale"] and s["shift"] == sc["shift"]
    bad = ~(np.isfinite(x) & (x > 0))
    assert bad.sum() == 5 and out[bad].tobytes() == x[bad].tobytes()  # NaN, +-inf, 0, negative: bit for bit
    assert s["n_gate"] == x.size - 5 - 4  # the invalid x and the four further invalid y (NaN, inf, 0, -2)
    flat = out.reshape(-1)
    assert flat[3 + 2 * 5] != 1024.0 and abs(flat[3 + 2 * 5] / 1024.0 - 1) < 0.1  # a valid pixel beyond the cap is aligned (and blended)
    assert np.isfinite(flat[3 + 2 * 7]) and flat[60] != 1500.0
    for i in (30, 33, 36, 39):  # an invalid predecessor: aligned only
        want = F32(np.float64(s["scale"]) * np.float64(x.reshape(-1)[i]) + np.float64(s["shift"]))
        assert flat[i] == want
    del xm, ym


def flicker_sequence(frames=8, h=48, w=64, seed=7):
    """a static ramp scene seen by a jittering estimator: +-5 % scale, +-0.03 m shift, 2 mm noise, and a block that moves (its luma and
    its depth change) -> [(x, image)]"""
    rng = np.random.default_rng(seed)
    base = _ramp(h, w, 1.5, 6.0).astype(np.float64)
    tex = rng.random((3, h, w)).astype(F32) * F32(0.5) + F32(0.2)
    seq = []
    for t in range(frames):
        s, b = 1.0 + rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03)
        d, img = base.copy(), tex.copy()
        c0 = 4 + 6 * t
        d[10:22, c0:c0 + 10] = 1.0
        img[:, 10:22, c0:c0 + 10] = 0.95
        seq.append(((s * d + b + rng.normal(0.0, 0.002, size=d.shape)).astype(F32), img))
    return seq


def test_flicker_property():
    """a static scene with jittered scale and shift: with anchor = 1 the summed change after is at most a tenth of the change before,
    and every fit recovers the jitter it has to undo.  At the default anchor 0.9 a tenth of every frame's jitter (up to +-5 % and
    +-0.03 m) stays in, so the bound is looser: the remaining change is at most 0.1 x the jitter between two frames plus the noise, a
    quarter of the change before at the worst"""
    seq = flicker_sequence()
    for anchor, bound in ((1.0, 10.0), (0.9, 4.0)):
        st, before, after = None, 0, 0
        for t, (x, img) in enumerate(seq):
            out, st, s = _step(x, img, st, anchor=anchor)
            assert s["reset"] == (t == 0)
            if t:
                assert s["fitted"] and 0.85 < s["scale"] < 1.15 and s["static_fraction"] > 0.8
                before, after = before + s["change_before_sum"], after + s["change_after_sum"]
        print(f"anchor {anchor}: change before {before} after {after} ratio {before / after:.1f}")
        assert after * bound <= before, (anchor, before, after)


def test_stabilizer_host_route_is_the_specification_and_grouping_does_not_matter():
    seq = flicker_sequence(frames=5, h=24, w=40)
    d = torch.from_numpy(np.stack([x for x, _ in seq]))[:, None]
    img = torch.from_numpy(np.stack([i for _, i in seq]))
    st, want, rows = None, [], []
    for x, im in seq:
        out, st, s = _step(x, im, st)
        want.append(out), rows.append(s)
    for groups in ((1, 1, 1, 1, 1), (2, 3), (5,)):
        stab, outs, stats, k = T.TemporalStabilizer(), [], [], 0
        for n in groups:
            o, s = stab.step(d[k:k + n], img[k:k + n])
            assert o.shape == (n, 1, 24, 40) and o.dtype == torch.float32 and len(s) == n
            outs.append(o), stats.extend(s)
            k += n
        assert torch.cat(outs)[:, 0].numpy().tobytes() == np.stack(want).tobytes() and stats == rows
        y, L = stab.state_host()
        assert y.tobytes() == st[0].tobytes() and np.array_equal(L, st[1])
        stab.reset()
        assert stab.state_host() is None and stab.step(d[:1], img[:1])[1][0]["reset"]
    with pytest.raises(ValueError, match="depth"):
        T.TemporalStabilizer().step(d[0, 0], img[:1])
    with pytest.raises(ValueError, match="image_hr"):
        T.TemporalStabilizer().step(d[:2], img[:1])


def _arg_count(hdr, name):
    m = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr)
    return len(m.group(1).split(","))


def test_entry_points_declared_bound_exported_and_ops_registered():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20 and "Temporal stabilisation" in hdr
    assert re.search(r"#define PRV2_TEMPORAL_STATS 12\b", hdr) and L.TEMPORAL_STATS == T.STATS == ops.TEMPORAL_STATS == 12
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
        assert _arg_count(hdr, name) == len(L.SIGNATURES[name][1]), name
    lib = L.load()
    assert lib.prv2_abi_version() == 20
    assert lib.prv2_temporal_workspace_bytes(8, 1024) == 48 and lib.prv2_temporal_workspace_bytes(9, 1025) == 4 * 48
    assert lib.prv2_temporal_workspace_bytes(0, 4) == -1 and lib.prv2_temporal_workspace_bytes(4096, 8193) == -1  # > 2^25 pixels
    assert lib.prv2_temporal_workspace_bytes(4096, 8192) > 0
    t = torch_ops.load()
    assert "temporal_step_" in torch_ops.OPS and hasattr(ops, "temporal_step")
    t.temporal_step_.default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU implementation to fall into
        t.temporal_step_(torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), 0.5, 6, 0.05, 0.9, torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8),
                         torch.zeros(4, 4, dtype=torch.uint8), False)


def test_entry_point_rejects_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, q, r, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288), ctypes.c_void_p(4100)
    big = 1 << 30  # never dereferenced: every call fails its argument check before a launch

    def step(depth=p, image=p, n=1, h=4, w=4, ih=4, iw=4, alpha=0.5, tau=6, rho=0.05, anchor=0.9, state=q, l0=q, l1=r, present=0, out=r,
             stats=p, ws=p, wsb=big):
        return lib.prv2_temporal_step(depth, image, n, h, w, ih, iw, alpha, tau, rho, anchor, state, l0, l1, present, out, stats, ws, wsb, None)
    for name in ("depth", "image", "state", "l0", "l1", "out", "stats"):
        assert step(**{name: None}) != 0 and "null" in err(), name
    assert step(ws=None) != 0 and "workspace" in err()
    assert step(n=0) != 0 and "frame count" in err()
    assert step(h=0) != 0 and "shape" in err()
    assert step(h=4096, w=8193) != 0 and "2^25" in err()
    assert step(ih=0) != 0 and "image shape" in err()
    for kw, word in ((dict(alpha=1.0), "alpha"), (dict(alpha=-0.5), "alpha"), (dict(alpha=NAN), "alpha"), (dict(tau=256), "tau"), (dict(tau=-1), "tau"),
                     (dict(rho=0.0), "rho"), (dict(rho=INF), "rho"), (dict(rho=NAN), "rho"), (dict(anchor=1.5), "anchor"), (dict(anchor=NAN), "anchor"),
                     (dict(present=2), "state_present"), (dict(l1=q), "luma"), (dict(out=p), "alias"), (dict(state=p), "alias"),
                     (dict(stats=odd), "misaligned"), (dict(ws=odd), "misaligned"), (dict(wsb=47), "prv2_temporal_workspace_bytes")):
        assert step(**kw) != 0 and word in err(), (kw, err())
    with pytest.raises(RuntimeError, match="temporal_step"):
        L.check(step(n=0), "temporal_step")


def test_wrapper_validates_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    d, im, s, l0, l1 = torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        ops.temporal_step(d, im, s, l0, l1, False)
    with pytest.raises(ValueError, match="alpha"):
        ops.temporal_step(d, im, s, l0, l1, False, alpha=1.0)
    with pytest.raises(ValueError, match="tau"):
        ops.temporal_step(d, im, s, l0, l1, False, tau=300)


@pytest.mark.parametrize("flags,message", [
    (["--temporal-stabilize", "--temporal-alpha", "1.0"], "--temporal-alpha"),
    (["--temporal-stabilize", "--temporal-tau", "256"], "--temporal-tau"),
    (["--temporal-stabilize", "--temporal-tau", "1.5"], "--temporal-tau"),
    (["--temporal-stabilize", "--temporal-rho", "0"], "--temporal-rho"),
    (["--temporal-stabilize", "--temporal-anchor", "1.5"], "--temporal-anchor"),
    (["--temporal-stabilize", "--generate-pl"], "per-image"),
])
def test_cli_argument_errors(flags, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", *flags], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


class _StubModel:
    """a CPU 'estimator': frame k's map is a fixed scene times a scale that jitters with k (k is written into the image's corner)"""
    device = "cpu"
    supports_return_device = False
    SCALES = (1.0, 1.04, 0.97, 1.02, 0.95)

    def __init__(self):
        self.calls = []

    def resizer(self, hr):
        return hr

    def __call__(self, mode, cai_mode, process_num, tile_cfg, image_lr, image_hr, **kw):
        self.calls.append(image_hr.shape[0])
        base = torch.from_numpy(_ramp(24, 40, 1.5, 5.0))
        ks = [int(round(float(im[0, 0, 0]) * 255)) for im in image_hr]
        return torch.stack([base * self.SCALES[k] for k in ks])[:, None], {}


def _stub_dataset(n=5):
    tex = np.random.default_rng(1).random((3, 24, 40)).astype(F32)
    items = []
    for k in range(n):
        im = tex.copy()
        im[:, 0, 0] = k / 255.0
        items.append(dict(img_file_basename=f"f{k}", image_hr=torch.from_numpy(im)))
    return items


def test_tester_run_with_the_flag_on_a_cpu_stub(tmp_path):
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    data = _stub_dataset()
    base = _ramp(24, 40, 1.5, 5.0)
    st, want = None, []
    for k, item in enumerate(data):
        out, st, s = _step(base * F32(_StubModel.SCALES[k]), item["image_hr"].numpy(), st, alpha=0.4, anchor=1.0)
        want.append((out, s))
    plain = Tester(None, RunnerInfo(work_dir=str(tmp_path)), data, _StubModel()).run(image_raw_shape=(24, 40))
    assert all("temporal" not in r for r in plain) and [r["name"] for r in plain] == [f"f{k}" for k in range(5)]
    off = Tester(None, RunnerInfo(work_dir=str(tmp_path), temporal_stabilize=False), data, _StubModel()).run(image_raw_shape=(24, 40))
    assert off == plain
    for fb in (1, 2, 5):
        model = _StubModel()
        t = Tester(None, RunnerInfo(work_dir=str(tmp_path), temporal_stabilize=True, temporal_alpha=0.4, temporal_anchor=1.0), data, model)
        res = t.run(image_raw_shape=(24, 40), frame_batch=fb)
        assert model.calls == {1: [1] * 5, 2: [2, 2, 1], 5: [5]}[fb]
        assert [r["name"] for r in res] == [f"f{k}" for k in range(5)]  # dataset order
        for r, p, (out, s) in zip(res, plain, want):
            assert set(r) == set(p) | {"temporal"} and set(r["temporal"]) == set(Tester.TEMPORAL_KEYS)
            assert r["temporal"] == {k: s[k] for k in Tester.TEMPORAL_KEYS}
            assert r["mean"] == float(torch.from_numpy(out).mean())  # the entry (and everything _emit writes) sees the stabilised map
        assert res[0]["temporal"]["reset"] and not any(r["temporal"]["reset"] for r in res[1:])
        moved = [s for _, s in want[1:]]
        assert t.last_eval == dict(temporal_change_before=float(np.mean([s["change_before"] for s in moved])),
                                   temporal_change_after=float(np.mean([s["change_after"] for s in moved])))
        assert t.last_eval["temporal_change_after"] < t.last_eval["temporal_change_before"] / 10
    # the saved PNG holds the stabilised map
    from patchrefinerv2_amd.output import write_png16
    t = Tester(None, RunnerInfo(work_dir=str(tmp_path / "s"), save=True, temporal_stabilize=True, temporal_alpha=0.4, temporal_anchor=1.0), data[:2], _StubModel())
    t.run(image_raw_shape=(24, 40))
    write_png16(str(tmp_path / "want.png"), (want[1][0] * 256).astype("uint16"))
    assert (tmp_path / "s" / "f1_uint16.png").read_bytes() == (tmp_path / "want.png").read_bytes()


def test_tester_rejects_generate_pl_and_several_ranks():
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    data = _stub_dataset(2)
    with pytest.raises(ValueError, match="per-image"):
        Tester(None, RunnerInfo(temporal_stabilize=True), data, _StubModel()).generate_pl(image_raw_shape=(24, 40))
    model = _StubModel()
    with pytest.raises(ValueError, match="one process"):
        Tester(None, RunnerInfo(temporal_stabilize=True, world_size=2), data, model).run(image_raw_shape=(24, 40))
    assert model.calls == []  # rejected before a frame is computed
