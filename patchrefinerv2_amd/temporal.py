"""Temporal stabilisation of depth maps across video frames (not in the reference; include/prv2.h "Temporal stabilisation").

A per-frame metric estimator jitters in global scale and shift from one frame to the next.  The stabiliser sits between the model and
the output stage: every frame is aligned to the previous OUTPUT by a gated least-squares scale and shift (compute_scale_and_shift's
normal equations, losses.py:523-544, with the new frame as the prediction and the previous output as the target) and blended with it
where the image has not changed.  ``anchor`` < 1 lets the sequence leak back to the model's own scale.

temporal_step_host   the specification, in numpy: exact int64 sums, one IEEE float64 operation per step
temporal_motion_host / temporal_warp_host   the optional motion stage in front of it (``motion_range``): integer block matching of the
                     frame's luma against the previous one and the state warped by the blocks' vectors, so that a moving camera
                     no longer gates the frame out (include/prv2.h "Temporal motion")
TemporalStabilizer   the state of one sequence; ``step`` takes the device route (csrc/temporal.hip through ops.temporal_step, or
                     csrc/motion.hip through ops.temporal_motion_step with ``motion``; their bits equal the specification's) for GPU
                     tensors and the specification for CPU tensors
"""
from __future__ import annotations

import math

import numpy as np

from .output import color_bytes, sample_indices

F32, F64, I64 = np.float32, np.float64, np.int64
STATS = 12  # PRV2_TEMPORAL_STATS: 8-byte words of a frame's stats row
MAX_PIXELS = 1 << 25  # (2^18)^2 * 2^25 < 2^63: the bound of the exact sums
DEFAULTS = dict(alpha=0.5, tau=6, rho=0.05, anchor=0.9)
MOTION_STATS = 8  # PRV2_TEMPORAL_MOTION_STATS: 8-byte words of a frame's motion stats row
MOTION_BLOCK = 16  # pixels a side of a block; the quarter map has one pixel per 4 x 4
QNAN = np.uint32(0x7FC00000)  # what the warp gives a pixel whose source left the frame


def check_params(alpha=0.5, tau=6, rho=0.05, anchor=0.9):
    """-> (alpha, tau, rho, anchor) as float, int, float, float; ValueError outside alpha in [0, 1), tau an integer in 0 .. 255,
    rho > 0 finite, anchor in [0, 1]"""
    if not (isinstance(tau, (int, np.integer)) or float(tau) == int(tau)) or not 0 <= int(tau) <= 255:
        raise ValueError(f"temporal: tau {tau}: an integer in 0 .. 255")
    alpha, tau, rho, anchor = float(alpha), int(tau), float(rho), float(anchor)
    if not 0.0 <= alpha < 1.0:
        raise ValueError(f"temporal: alpha {alpha} outside [0, 1)")
    if not (rho > 0.0 and math.isfinite(rho)):
        raise ValueError(f"temporal: rho {rho} must be positive and finite")
    if not 0.0 <= anchor <= 1.0:
        raise ValueError(f"temporal: anchor {anchor} outside [0, 1]")
    return alpha, tau, rho, anchor


def luma_host(image, h, w) -> np.ndarray:
    """uint8 [h, w]: (77 R + 150 G + 29 B + 128) >> 8 of the bytes the point cloud gives the pixels of an [h, w] grid from ``image``
    fp32 [3, ih, iw] (``sample_indices``, ``color_bytes(v * 255)``)"""
    img = np.asarray(image, dtype=F32)
    if img.ndim != 3 or img.shape[0] != 3 or img.shape[1] < 1 or img.shape[2] < 1:
        raise ValueError(f"temporal: image is [3, ih, iw] (got {img.shape})")
    sy, sx = sample_indices(h, img.shape[1]), sample_indices(w, img.shape[2])
    with np.errstate(all="ignore"):
        r, g, b = (color_bytes(img[c][sy][:, sx] * F32(255)).astype(np.int32) for c in range(3))
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)


def _valid(v):
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v > 0)


def _change(v64, y64, g) -> int:
    """sum over g of rint(65536 min(1, |v - y| / y)); a NaN ratio counts as 1"""
    c = np.abs(v64[g] - y64[g]) / y64[g]
    return int(np.rint(65536.0 * np.where(c < 1.0, c, 1.0)).astype(I64).sum())


def stats_dict(row, hw: int, motion_row=None) -> dict:
    """a frame's stats row (int64 [STATS]; words 9 and 10 hold float64 bits) as a dict: ``reset``, ``n`` (pixels of the fit), ``n_gate``
    (gated pixels), ``static_fraction`` = n_gate / (h w), ``scale``, ``shift`` (after the anchor), ``fitted``, ``sums`` = (sum qx,
    sum qx^2, sum qx qy, sum qy), ``change_before_sum`` / ``change_after_sum`` (65536ths) and ``change_before`` / ``change_after`` =
    those / (65536 n_gate), 0 without gated pixels; ``motion``: ``motion_dict(motion_row)``, None when the motion stage is off"""
    row = np.asarray(row, dtype=I64)
    s, b = (float(v) for v in row[9:11].view(F64))
    ng = int(row[2])
    return dict(reset=bool(row[0]), n=int(row[1]), n_gate=ng, static_fraction=ng / float(hw), scale=s, shift=b, fitted=bool(row[11]),
                sums=tuple(int(v) for v in row[3:7]), change_before_sum=int(row[7]), change_after_sum=int(row[8]),
                change_before=int(row[7]) / (65536.0 * ng) if ng else 0.0, change_after=int(row[8]) / (65536.0 * ng) if ng else 0.0,
                motion=None if motion_row is None else motion_dict(motion_row))


def check_motion_range(motion_range) -> int:
    """-> R as int; ValueError unless an integer in 1 .. 16"""
    integral = isinstance(motion_range, (int, np.integer)) or (isinstance(motion_range, float) and motion_range.is_integer())
    if isinstance(motion_range, bool) or not integral or not 1 <= int(motion_range) <= 16:
        raise ValueError(f"temporal: motion_range {motion_range}: an integer in 1 .. 16")
    return int(motion_range)


def motion_blocks(h, w):
    """(nby, nbx): the 16 x 16 blocks of an [h, w] frame"""
    return -(-h // MOTION_BLOCK), -(-w // MOTION_BLOCK)


def quarter_host(L) -> np.ndarray:
    """uint8 [ceil(h / 4), ceil(w / 4)]: (the sum of the 4 x 4 pixels, indices clamped into the frame, + 8) >> 4"""
    L = np.asarray(L, dtype=np.uint8)
    h, w = L.shape
    iy, ix = np.minimum(np.arange(4 * -(-h // 4)), h - 1), np.minimum(np.arange(4 * -(-w // 4)), w - 1)
    p = L[iy][:, ix].astype(np.int32)
    return ((p.reshape(len(iy) // 4, 4, len(ix) // 4, 4).sum(axis=(1, 3)) + 8) >> 4).astype(np.uint8)


def _candidates(r):
    """the (dy, dx) of [-r, r]^2 in the tie order: by dy^2 + dx^2, then dy, then dx"""
    return sorted(((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))


def motion_coarse_host(L, P, motion_range=8):
    """the coarse search of ``temporal_motion_host`` -> (vectors int32 [nby, nbx, 2] in quarter pixels, before the median; S(winner) and
    S(0, 0) int64 [nby, nbx])"""
    R = check_motion_range(motion_range)
    Q, QP = quarter_host(L).astype(np.int32), quarter_host(P).astype(np.int32)
    hq, wq = Q.shape
    nby, nbx = motion_blocks(*np.shape(L))
    I, J = np.arange(-2, 4 * nby + 2), np.arange(-2, 4 * nbx + 2)  # the rows and columns of every block's window: 4 + 4 nb of them
    Qw = Q[np.clip(I, 0, hq - 1)][:, np.clip(J, 0, wq - 1)]

    def sad(dy, dx):
        D = np.abs(Qw - QP[np.clip(I + dy, 0, hq - 1)][:, np.clip(J + dx, 0, wq - 1)])
        C = D.reshape(nby + 1, 4, nbx + 1, 4).sum(axis=(1, 3), dtype=I64)  # 4 x 4 cells; a window is 2 x 2 of them
        return C[:-1, :-1] + C[:-1, 1:] + C[1:, :-1] + C[1:, 1:]

    s0 = sad(0, 0)
    best, vec = s0.copy(), np.zeros((nby, nbx, 2), dtype=np.int32)
    for dy, dx in _candidates(R)[1:]:  # in the tie order, so a strict "<" is the lexicographic rule
        s = sad(dy, dx)
        better = s < best
        best[better] = s[better]
        vec[better] = (dy, dx)
    vec[~(best + 64 < s0)] = 0
    return vec, best, s0


def motion_median_host(v) -> np.ndarray:
    """the component-wise median (the fifth smallest) of the nine vectors of every block's 3 x 3 neighbourhood, block indices clamped"""
    v = np.asarray(v)
    nby, nbx = v.shape[:2]
    nine = [v[np.clip(np.arange(nby) + a, 0, nby - 1)][:, np.clip(np.arange(nbx) + b, 0, nbx - 1)] for a in (-1, 0, 1) for b in (-1, 0, 1)]
    return np.sort(np.stack(nine), axis=0)[4]


def motion_refine_host(L, P, vhat):
    """the refinement of ``temporal_motion_host`` around 4 ``vhat`` -> (m int32 [nby, nbx, 2] in pixels; T(m) with T(0, 0) for a zeroed
    block, and T(0, 0), int64 [nby, nbx])"""
    L, P = np.asarray(L, dtype=np.uint8), np.asarray(P, dtype=np.uint8)
    h, w = L.shape
    nby, nbx = motion_blocks(h, w)
    B = MOTION_BLOCK
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    Li = np.zeros((nby * B, nbx * B), dtype=np.int32)
    Li[:h, :w] = L
    inside = np.zeros((nby * B, nbx * B), dtype=bool)
    inside[:h, :w] = True
    npix = inside.reshape(nby, B, nbx, B).sum(axis=(1, 3), dtype=I64)
    cyx = 4 * np.asarray(vhat, dtype=np.int32)
    cy, cx = (np.repeat(np.repeat(cyx[..., k], B, axis=0), B, axis=1)[:h, :w] for k in (0, 1))  # per pixel: its block's 4 v^

    def sad(sy, sx):  # the blocks' sums of |L[p] - P[clamp(p + s)]|, s per pixel
        D = np.zeros_like(Li)
        D[:h, :w] = np.abs(Li[:h, :w] - P[np.clip(yy + sy, 0, h - 1), np.clip(xx + sx, 0, w - 1)].astype(np.int32))
        return D.reshape(nby, B, nbx, B).sum(axis=(1, 3), dtype=I64)

    t0 = sad(0, 0)
    best, e = None, np.zeros((nby, nbx, 2), dtype=np.int32)
    for ey, ex in _candidates(3):
        t = sad(cy + ey, cx + ex)
        if best is None:
            best = t.copy()
            continue
        better = t < best
        best[better] = t[better]
        e[better] = (ey, ex)
    m = cyx + e
    zero = ~(best + npix < t0)
    m[zero] = 0
    return m, np.where(zero, t0, best), t0


def temporal_motion_host(L, P, motion_range=8):
    """The block motion of a frame against the previous one, all in integers.  ``L``: the frame's luma, ``P``: the previous luma, uint8
    [h, w] -> (m int16 [nby, nbx, 2]: pixel p of the frame was at p + m[p's 16 x 16 block] in the previous frame; row int64
    [MOTION_STATS]: blocks, blocks with m != 0, sum my, sum mx, sum |my| + |mx|, max(|my|, |mx|), sum T(m) (T(0, 0) for a zeroed
    block), sum T(0, 0)).

    Every index that leaves its map is clamped into it.  Q, QP: the quarter maps (``quarter_host``).  Coarse: block (by, bx) owns the
    8 x 8 window of Q at rows 4 by - 2 .. 4 by + 5, columns 4 bx - 2 .. 4 bx + 5; S(d) = sum over the window of |Q[i, j] - QP[i + dy,
    j + dx]| for |dy|, |dx| <= R; the smallest (S, dy^2 + dx^2, dy, dx) wins and is taken if S + 64 < S(0, 0), else (0, 0).  v^ = the
    component-wise median of the 3 x 3 blocks' coarse vectors.  Fine: c = 4 v^ + e, e in [-3, 3]^2; T(c) = sum over the block's npix
    pixels inside the frame of |L[p] - P[p + c]|; the smallest (T, ey^2 + ex^2, ey, ex) wins; m = c if T + npix < T(0, 0), else 0."""
    R = check_motion_range(motion_range)
    L, P = np.asarray(L), np.asarray(P)
    if L.dtype != np.uint8 or P.dtype != np.uint8 or L.ndim != 2 or L.size < 1 or L.shape != P.shape:
        raise ValueError(f"temporal: the lumas are two uint8 [h, w] maps (got {L.dtype} {L.shape}, {P.dtype} {P.shape})")
    coarse, _, _ = motion_coarse_host(L, P, R)
    m, t, t0 = motion_refine_host(L, P, motion_median_host(coarse))
    a = np.abs(m).astype(I64)
    row = np.array([m.shape[0] * m.shape[1], int((m != 0).any(axis=2).sum()), int(m[..., 0].sum()), int(m[..., 1].sum()), int(a.sum()), int(a.max()),
                    int(t.sum()), int(t0.sum())], dtype=I64)
    return m.astype(np.int16), row


def temporal_warp_host(y, P, m):
    """the state moved by the blocks' vectors: yw[p] = y[p + m], Pw[p] = P[p + m] where p + m lies inside the frame; elsewhere yw is the
    quiet NaN 0x7FC00000 (not valid, so the pixel is not gated) and Pw = 0 -> (yw fp32 [h, w], Pw uint8 [h, w])"""
    y, P, m = np.asarray(y, dtype=F32), np.asarray(P, dtype=np.uint8), np.asarray(m).astype(np.int64)
    h, w = y.shape
    B = MOTION_BLOCK
    my, mx = (np.repeat(np.repeat(m[..., k], B, axis=0), B, axis=1)[:h, :w] for k in (0, 1))
    sy, sx = np.arange(h)[:, None] + my, np.arange(w)[None, :] + mx
    ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    sy, sx = np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)
    yw = np.where(ok, y.view(np.uint32)[sy, sx], QNAN).astype(np.uint32).view(F32)
    return yw, np.where(ok, P[sy, sx], 0).astype(np.uint8)


def motion_dict(row):
    """a frame's motion stats row as a dict: ``blocks``, ``moving_fraction`` (blocks with m != 0), ``mean_dy`` / ``mean_dx`` (over all
    blocks, pixels), ``mean_abs`` (of |my| + |mx|), ``max_abs``, ``sad`` / ``sad_zero`` (sum T(m) / sum T(0, 0)); all zero for the
    row of a frame whose motion stage did not run (no state)"""
    row = np.asarray(row, dtype=I64)
    nb = int(row[0])
    d = max(nb, 1)
    return dict(blocks=nb, moving_fraction=int(row[1]) / d, mean_dy=int(row[2]) / d, mean_dx=int(row[3]) / d, mean_abs=int(row[4]) / d,
                max_abs=int(row[5]), sad=int(row[6]), sad_zero=int(row[7]))


def temporal_step_host(x, image, state=None, alpha=0.5, tau=6, rho=0.05, anchor=0.9, motion_range=None):
    """One frame of the specification.  ``x``: the frame's map fp32 [h, w] (metres); ``image``: fp32 [3, ih, iw] in [0, 1], any size;
    ``state``: None or (previous output fp32 [h', w'], previous luma uint8 [h', w']) -> (out fp32 [h, w], state (out, luma),
    row int64 [STATS]: the layout of prv2_temporal_step's stats; ``stats_dict`` names it).  With ``motion_range`` = R (1 .. 16) the
    motion stage runs first and a fourth value is returned, its row int64 [MOTION_STATS] (``motion_dict``): with a state of this shape,
    (y, Lp) = temporal_warp_host(y, Lp, temporal_motion_host(L, Lp, R)) stand in for the state below (the new state is (out, L) as
    ever); without one the stage does not run and the row is all zero.

    valid(v) = finite and > 0.  L = the frame's luma (``luma_host``).  Without a state, or with one of another shape, no pixel is
    gated.  Else g = |L - Lp| <= tau and valid(x) and valid(y); the fit mask m = g and 1 <= qx < 2^18 and 1 <= qy < 2^18 and
    |x - y| <= 0.5 y (float64) with qx = rint(x 256), qy = rint(y 256) in fp32.  The int64 sums over m: n, qx, qx^2, qx qy, qy.
    n < max(64, h w // 100): a reset (no state, or a scene cut), out = x.  Else, in float64, det = a00 a11 - a01 a01 of a00 = sum qx^2,
    a01 = sum qx, a11 = n, b0 = sum qx qy, b1 = sum qy; s = (a11 b0 - a01 b1) / det and b = ((a00 b1 - a01 b0) / det) / 256 when
    det > 0, s in [0.5, 2] and b finite, else s = 1, b = 0; then s = 1 + anchor (s - 1), b = anchor b.  a = fp32(s x + b) where x and
    that value are valid, else x; where g: r = (a - y) / min(a, y), w = alpha / (1 + (r / rho)^2), out = fp32(a + w (y - a)); elsewhere
    out = a.  An invalid x passes through unchanged, NaN included."""
    alpha, tau, rho, anchor = check_params(alpha, tau, rho, anchor)
    if motion_range is not None:
        motion_range = check_motion_range(motion_range)
    mrow = np.zeros(MOTION_STATS, dtype=I64)
    x = np.ascontiguousarray(x, dtype=F32)
    if x.ndim != 2 or x.size < 1:
        raise ValueError(f"temporal: the map is [h, w] (got {x.shape})")
    h, w = x.shape
    if h * w > MAX_PIXELS:
        raise ValueError(f"temporal: a frame of {h} x {w} exceeds 2^25 pixels (the bound of the exact int64 sums)")
    L = luma_host(image, h, w)
    row = np.zeros(STATS, dtype=I64)
    has_prev = state is not None and tuple(state[0].shape) == (h, w)
    x64 = x.astype(F64)
    g = np.zeros((h, w), dtype=bool)
    sums = [0, 0, 0, 0, 0]
    with np.errstate(all="ignore"):
        if has_prev:
            y, Lp = np.asarray(state[0], dtype=F32), np.asarray(state[1], dtype=np.uint8)
            if motion_range is not None:
                m, mrow = temporal_motion_host(L, Lp, motion_range)
                y, Lp = temporal_warp_host(y, Lp, m)
            y64 = y.astype(F64)
            g = (np.abs(L.astype(np.int32) - Lp.astype(np.int32)) <= tau) & _valid(x) & _valid(y)
            qx, qy = np.rint(x * F32(256)), np.rint(y * F32(256))
            cap = F32(2 ** 18)
            m = g & (qx >= 1) & (qx < cap) & (qy >= 1) & (qy < cap) & (np.abs(x64 - y64) <= 0.5 * y64)
            ix, iy = qx[m].astype(I64), qy[m].astype(I64)
            sums = [int(m.sum()), int(ix.sum()), int((ix * ix).sum()), int((ix * iy).sum()), int(iy.sum())]
        n = sums[0]
        reset = n < max(64, (h * w) // 100)
        s, b, fitted = F64(1.0), F64(0.0), False
        if not reset:
            a00, a01, a11, b0, b1 = F64(sums[2]), F64(sums[1]), F64(n), F64(sums[3]), F64(sums[4])
            det = a00 * a11 - a01 * a01
            if det > 0:
                sf = (a11 * b0 - a01 * b1) / det
                bf = ((a00 * b1 - a01 * b0) / det) / F64(256.0)
                if 0.5 <= sf <= 2.0 and np.isfinite(bf):
                    s, b, fitted = F64(1.0) + F64(anchor) * (sf - F64(1.0)), F64(anchor) * bf, True
        if reset:
            out = x.copy()
        else:
            al = (s * x64 + b).astype(F32)
            a = np.where(_valid(x) & _valid(al), al, x)
            A = a.astype(F64)
            q = ((A - y64) / np.minimum(A, y64)) / F64(rho)
            wt = F64(alpha) / (F64(1.0) + q * q)
            out = np.where(g, (A + wt * (y64 - A)).astype(F32), a)
        if has_prev:
            row[7], row[8] = _change(x64, y64, g), _change(out.astype(F64), y64, g)
    row[0], row[1], row[2], row[3:7], row[11] = int(reset), n, int(g.sum()), sums[1:], int(fitted)
    row[9:11] = np.array([s, b], dtype=F64).view(I64)
    return (out, (out, L), row) if motion_range is None else (out, (out, L), row, mrow)


class TemporalStabilizer:
    """The stabiliser of ONE sequence: ``step`` takes the frames in order, however they are grouped into calls (the result does not
    depend on the grouping).  ``reset`` forgets the sequence; a frame of another shape, or on another device, starts a new one.
    ``motion`` puts the motion stage (``temporal_motion_host``, range ``motion_range`` in 1 .. 16) in front of every step."""

    def __init__(self, alpha=0.5, tau=6, rho=0.05, anchor=0.9, motion=False, motion_range=8):
        self.alpha, self.tau, self.rho, self.anchor = check_params(alpha, tau, rho, anchor)
        self.motion_range = check_motion_range(motion_range) if motion else None
        self.reset()

    @property
    def params(self):
        return dict(alpha=self.alpha, tau=self.tau, rho=self.rho, anchor=self.anchor)

    def reset(self):
        self._host = None  # (out, luma) numpy
        self._dev = None   # dict(depth, luma [2, h, w], cur): the device state; luma[cur] is the previous luma

    def step(self, depth, image_hr):
        """``depth``: B frames [B, 1, H, W] (or [B, H, W]) in sequence order; ``image_hr``: [B, 3, ih, iw] in [0, 1] ->
        (out: a tensor like ``depth``, [stats dict per frame] (``stats_dict``; its ``motion`` is None without the motion stage)).  GPU
        tensors take the kernels and cost one device-to-host copy of the stats rows per call, no other synchronisation; CPU tensors
        take ``temporal_step_host``."""
        import torch
        if not isinstance(depth, torch.Tensor) or depth.dim() not in (3, 4) or (depth.dim() == 4 and depth.shape[1] != 1):
            raise ValueError("TemporalStabilizer.step: depth is a tensor [B, 1, H, W] or [B, H, W]")
        h, w = depth.shape[-2:]
        d = depth.reshape(-1, h, w)
        image = torch.as_tensor(image_hr)
        image = image[None] if image.dim() == 3 else image
        if image.dim() != 4 or image.shape[0] != d.shape[0] or image.shape[1] != 3:
            raise ValueError(f"TemporalStabilizer.step: image_hr is [B, 3, ih, iw] with the maps' B = {d.shape[0]} (got {tuple(image.shape)})")
        if h * w > MAX_PIXELS:
            raise ValueError(f"TemporalStabilizer.step: a frame of {h} x {w} exceeds 2^25 pixels (the bound of the exact int64 sums)")
        if d.is_cuda:
            out, rows = self._step_device(d.float().contiguous(), image.to(d.device).float().contiguous())
        else:
            out, rows = self._step_host(d.float().numpy(), image.cpu().float().numpy())
        return out.reshape(depth.shape), [stats_dict(r[:STATS], h * w, r[STATS:] if self.motion_range else None) for r in rows]

    def _step_host(self, d, image):
        import torch
        self._dev = None
        outs, rows = [], []
        for f in range(d.shape[0]):
            out, self._host, *row = temporal_step_host(d[f], image[f], self._host, motion_range=self.motion_range, **self.params)
            outs.append(out), rows.append(np.concatenate(row))  # (the step's row, then the motion row when the stage is on)
        return torch.from_numpy(np.stack(outs)), rows

    def _step_device(self, d, image):
        import torch
        from . import ops
        self._host = None
        n, h, w = d.shape
        st = self._dev
        present = st is not None and tuple(st["depth"].shape) == (h, w) and st["depth"].device == d.device
        if not present:
            st = self._dev = dict(depth=torch.empty((h, w), dtype=torch.float32, device=d.device),
                                  luma=torch.empty((2, h, w), dtype=torch.uint8, device=d.device), cur=0)
        cur = st["cur"]
        if self.motion_range:
            out, stats, mstats, _ = ops.temporal_motion_step(d, image, st["depth"], st["luma"][cur], st["luma"][1 - cur], present,
                                                             motion_range=self.motion_range, **self.params)
            stats = torch.cat((stats, mstats), dim=1)  # one copy to the host for both blocks
        else:
            out, stats = ops.temporal_step(d, image, st["depth"], st["luma"][cur], st["luma"][1 - cur], present, **self.params)
        st["cur"] = cur ^ (n & 1)  # frame f wrote its luma into buffer (f + 1) & 1 of the pair
        return out, stats.cpu().numpy()

    def state_host(self):
        """the state as numpy (output fp32 [h, w], luma uint8 [h, w]), None before the first frame (a device state is copied)"""
        if self._dev is not None:
            return self._dev["depth"].cpu().numpy(), self._dev["luma"][self._dev["cur"]].cpu().numpy()
        return None if self._host is None else (np.asarray(self._host[0]), np.asarray(self._host[1]))
