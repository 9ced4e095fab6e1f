"""Host-side wrappers over the kernels: torch supplies device memory and the stream, nothing else.

``Feat`` is an NHWC activation view (optionally a channel slice of a wider buffer) -- the
mechanism that makes every ``torch.cat`` of the reference free: producers write into slices.

Every wrapper has one shape: validate, allocate, then ONE callable whose two arms are the two routes to the same kernel
(``DISPATCH``: ``_tops().X(...)`` / ``_c("X", ...)``), handed to at most ONE ``PROFILER.launch`` / ``launch_aux`` with the tag, the
FLOP or byte count and the shape string computed once.  Single-frame and B-frame forms of an op share that body and differ in the
entry point's name and a leading frame count.  ``_conv_desc`` / ``_ups_src`` build the two descriptors of the C ABI.
"""
from __future__ import annotations

import ctypes as C
import math
import numpy as np
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from . import lib as L
from .lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_SOFTPLUS, PREC_F32  # noqa: F401


# How the host mirror (frame.py's drivers, the networks under models.py) reaches the kernels: "torch" = through the PyTorch-ROCm custom ops torch.ops.prv2.* (csrc/torch_ops.cpp ->
# libprv2_torch.so: at::Tensor in / out on torch's current stream; ``_tops()``), "ctypes" = straight through the C ABI (lib.py;
# ``_c``).  Every entry point a frame uses exists on both routes; same kernels, same results bit for bit (tests/test_hip_models.py::
# test_models_through_torch_custom_ops) and the same profiler records (tests/test_ops_routes_gpu.py).  The wrappers read DISPATCH when
# they are called.  PRV2_DISPATCH selects the default (INTEGRATION.md has the measured per-frame difference).
DISPATCH = os.environ.get("PRV2_DISPATCH", "torch")
assert DISPATCH in ("ctypes", "torch"), DISPATCH


def _tops():
    from . import torch_ops
    return torch_ops.load()


_CFN: dict = {}  # entry point -> its bound ctypes function (resolved on first use)


def _c(name: str, *args, what: Optional[str] = None):
    """the ctypes route: prv2_<name>(*args, current stream), a non-zero status raised as ``<what> failed`` (``what``: the name to report
    when it is not the entry point's)"""
    fn = _CFN.get(name)
    if fn is None:
        fn = _CFN[name] = getattr(L.load(), "prv2_" + name)
    L.check(fn(*args, torch.cuda.current_stream().cuda_stream), what or name)


def _last_kernel() -> str:
    """a profiler tag evaluated after the launch: the kernel the library dispatched the last call to"""
    return L.load().prv2_last_kernel().decode()


class Profiler:
    """Optional per-launch accounting for bench.py: algorithmic FLOPs (2*MAC) and, when ``timed``,
    HIP events recorded on the launch stream around each matrix-kernel launch."""

    def __init__(self):
        self.enabled = False
        self.timed = False
        self.by_shape = False
        self.records = []  # (kernel tag, executed flops, start event, end event, reference-graph flops)

    def start(self, timed=False, by_shape=False):
        self.enabled, self.timed, self.by_shape, self.records = True, timed, by_shape, []

    def stop(self):
        self.enabled = False
        return self.records

    def launch(self, tag, flops, fn, shape=None, algo=None):
        """``tag``: a string, or a callable evaluated AFTER the launch (the library reports which kernel it dispatched).
        ``flops``: the 2*MAC the launch EXECUTES; ``algo``: the 2*MAC the reference graph spends on the same step when that differs
        (the coarse half of a cat([fine, coarse_roi]) conv is computed once per frame here: coarse_tap_*) -- default: the same."""
        if not self.enabled:
            return fn()
        e0 = e1 = None
        if self.timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
        else:
            fn()
        if callable(tag):
            tag = tag()
        if self.by_shape and shape is not None:
            tag = f"{tag} {shape}"
        self.records.append((tag, flops, e0, e1, flops if algo is None else algo))

    def launch_aux(self, tag, nbytes, fn, shape):
        """memory-bound kernels: only itemised in the per-layer report (by_shape); bytes go into the tag"""
        if not (self.enabled and self.by_shape):
            return fn()
        return self.launch(tag, 0.0, fn, f"{shape} {nbytes / 1e6:.0f}MB")

    def summary(self):
        """{tag: dict(launches, flops (executed), algo (reference graph), ms)} (call after torch.cuda.synchronize())."""
        out = {}
        for tag, fl, e0, e1, al in self.records:
            d = out.setdefault(tag, dict(launches=0, flops=0.0, ms=0.0, algo=0.0))
            d["launches"] += 1
            d["flops"] += fl
            d["algo"] += al
            if e0 is not None:
                d["ms"] += e0.elapsed_time(e1)
        return out


PROFILER = Profiler()


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, Feat):
        return t.ptr
    return t.data_ptr()


def _ld(f) -> int:
    return 0 if f is None else f.ld


def _require_dev(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise ValueError("prv2 ops need float32 tensors on the GPU (no CPU fallback exists)")
        if t is not None and t.device.index != torch.cuda.current_device():
            # kernels are enqueued on the CURRENT device's stream: a tensor of another device would be touched from the
            # wrong queue (the frame drivers enter torch.cuda.device(model.device) themselves)
            raise RuntimeError(f"prv2 op on a {t.device} tensor while the current device is cuda:{torch.cuda.current_device()}: "
                               "wrap the call in torch.cuda.device(tensor.device)")


def roundup(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def _feat_of(y: torch.Tensor, c: int) -> "Feat":
    """the ``Feat`` of an NHWC tensor a torch.ops.prv2 operator allocated: dense, or -- channel counts that are not a multiple of 4 -- the
    first c channels of a buffer whose pixel stride is padded (csrc/torch_ops.cpp::alloc_nhwc)"""
    n, h, w, _ = y.shape
    ld = y.stride(2)
    return Feat(y if ld == y.shape[3] else torch.as_strided(y, (n, h, w, ld), (h * w * ld, w * ld, ld, 1)), c)


class Feat:
    """NHWC fp32 activation [n, h, w, c] living in ``buf`` ([n, h, w, ld]) at channel offset c0."""

    __slots__ = ("buf", "n", "h", "w", "c", "c0", "x2", "aux")

    def __init__(self, buf: torch.Tensor, c: Optional[int] = None, c0: int = 0, x2: bool = False):
        assert buf.dim() == 4 and buf.is_contiguous()
        _require_dev(buf)
        self.buf = buf
        # x2: the bytes are the pre-split "X2" operand format of include/prv2.h (per 8 channels [8 bf16 hi | 8 bf16 lo]) instead of
        # fp32 -- written by a producer for the 256-column conv kernels, its only readers (csrc/conv3x3_gate.hip)
        self.x2 = x2
        self.aux = None  # per-frame derived tensors a consumer attached to this map (fusion.BiDirectionalFusion.prepare_frame)
        self.n, self.h, self.w = buf.shape[0], buf.shape[1], buf.shape[2]
        self.c = buf.shape[3] - c0 if c is None else c
        self.c0 = c0
        assert 0 <= c0 and c0 + self.c <= buf.shape[3]

    @staticmethod
    def alloc_raw(n, h, w, c, device, pad_to: int = 4) -> "Feat":
        """like ``alloc`` but the pad channels are left to the caller (a producer that writes them: ops.depth_pair_fill)"""
        return Feat(torch.empty((n, h, w, roundup(c, pad_to)), device=device, dtype=torch.float32), c)

    @staticmethod
    def alloc(n, h, w, c, device, pad_to: int = 4) -> "Feat":
        ld = roundup(c, pad_to)
        # pad channels are read by the conv loader (x zero weights): they must be finite -- zero just those
        buf = torch.empty((n, h, w, ld), device=device, dtype=torch.float32)
        if ld != c:
            if DISPATCH == "torch":
                _tops().zero_pad_channels_(buf, c)
            else:
                _c("zero_pad_channels", buf.data_ptr(), n * h * w, c, ld)
        return Feat(buf, c)

    @property
    def ld(self) -> int:
        return self.buf.shape[3]

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + 4 * self.c0

    @property
    def device(self):
        return self.buf.device

    def slice(self, c0: int, c: int) -> "Feat":
        assert not self.x2 or (c0 % 8 == 0 and c % 8 == 0)
        return Feat(self.buf, c, self.c0 + c0, self.x2)

    def view(self) -> torch.Tensor:
        """this activation as a (strided) torch tensor [n, h, w, c]: what the torch.ops.prv2 operators take"""
        assert not self.x2, "a pre-split (X2) buffer is not an fp32 tensor"
        return self.buf[..., self.c0:self.c0 + self.c]

    def raw(self) -> torch.Tensor:
        """the same strided tensor whatever the format (an X2 buffer is a float32 CONTAINER: the operator is told by its ``fmt``)"""
        return self.buf[..., self.c0:self.c0 + self.c]

    def batch(self, b0: int, b1: int) -> "Feat":
        return Feat(self.buf[b0:b1], self.c, self.c0, self.x2)

    def x2_to_float(self) -> "Feat":
        """tests / debugging: the fp32 values an X2 buffer stands for (hi + lo per element)"""
        assert self.x2 and self.c0 % 8 == 0 and self.c % 8 == 0
        raw = self.buf[..., self.c0:self.c0 + self.c].contiguous().view(torch.int32)              # [n, h, w, c] dwords
        g = raw.view(self.n, self.h, self.w, self.c // 8, 2, 4)                                   # [.., group, hi | lo, 4 dwords = 8 bf16]
        def unpack(d):                                                                            # 4 dwords -> 8 floats (element 2i = low half)
            lo16 = (d << 16).view(torch.float32)
            hi16 = (d & -65536).view(torch.float32)
            return torch.stack([lo16, hi16], dim=-1).flatten(-2)
        v = unpack(g[..., 0, :]) + unpack(g[..., 1, :])
        return Feat(v.reshape(self.n, self.h, self.w, self.c).contiguous())

    def to_nchw(self) -> torch.Tensor:
        """Debug / boundary helper: dense NCHW copy (through the HIP layout kernel)."""
        if DISPATCH == "torch":
            return _tops().nhwc_to_nchw(self.view())
        out = torch.empty((self.n, self.c, self.h, self.w), device=self.device, dtype=torch.float32)
        _c("nhwc_to_nchw", self.ptr, self.n, self.c, self.h, self.w, self.ld, out.data_ptr())
        return out

    @staticmethod
    def from_nchw(x: torch.Tensor, pad_to: int = 4) -> "Feat":
        _require_dev(x)
        x = x.contiguous()
        n, c, h, w = x.shape
        if DISPATCH == "torch" and pad_to == 4:
            y = _tops().nchw_to_nhwc(x)
            return _feat_of(y, c)
        f = Feat.alloc(n, h, w, c, x.device, pad_to)
        _c("nchw_to_nhwc", x.data_ptr(), n, c, h, w, f.ptr, f.ld)
        return f


@dataclass
class ConvW:
    """A packed convolution / linear weight (prv2_pack_conv_weight layout) + its bias."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    cout: int
    cin: int
    kh: int
    kw: int
    stride: int = 1
    pad: int = 0
    convt_k: int = 0
    prec: int = PREC_F32
    same_pad: bool = False  # timm Conv2dSame / TensorFlow "SAME" padding (prv2_conv_desc.same_pad)


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, pad: Optional[int] = None,
              convt_k: int = 0, bn_scale: Optional[torch.Tensor] = None, prec: int = PREC_F32, device=None,
              same_pad: bool = False) -> ConvW:
    """weight: PyTorch layout [cout, cin, kh, kw] / [cout, cin] (Linear) / [cin, cout, k, k] (ConvTranspose2d)."""
    lib = L.load()
    device = device or weight.device
    w = weight.detach().to(device=device, dtype=torch.float32).contiguous()
    if w.dim() == 2:
        w = w[:, :, None, None]
    if convt_k:
        cin, cout, kh, kw = w.shape
    else:
        cout, cin, kh, kw = w.shape
    if pad is None:
        pad = kh // 2 if not convt_k else 0
    sc = bn_scale.detach().to(device=device, dtype=torch.float32).contiguous() if bn_scale is not None else None
    if DISPATCH == "torch":
        packed = _tops().pack_conv_weight(w, sc, convt_k, prec)
    else:
        nbytes = lib.prv2_packed_weight_bytes(cout, cin, kh, kw, convt_k, prec)
        packed = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
        _c("pack_conv_weight", w.data_ptr(), _ptr(sc), packed.data_ptr(), cout, cin, kh, kw, convt_k, prec)
    b = bias.detach().to(device=device, dtype=torch.float32).contiguous() if bias is not None else None
    return ConvW(packed, b, cout, cin, kh, kw, convt_k if convt_k else stride, pad, convt_k, prec, same_pad)


@dataclass
class ConvWF6:
    """A 256-column 3x3 conv packed for the fp16 + fp6 kernel (prv2_pack_conv3x3_f6_weight) + its bias and power-of-two scales."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    cout: int
    cin: int
    w_scale: float          # the weights were multiplied by this before the fp16 / fp6 split (max |w w_scale| in [1, 2))
    x_scale: float = 1.0    # what the loader multiplies the activations with (calibration: ``range``)
    range: Optional[torch.Tensor] = None  # device uint32[1]: float bits of the largest |relu(x) x_scale| any launch saw
    kh = kw = 3  # (not fields: the one layer shape the kernels take, named as ``ConvW`` names it for ``_conv_desc``)
    stride = pad = 1
    convt_k = 0
    prec = L.PREC_F16F6
    same_pad = False


F16F6 = os.environ.get("PRV2_F16F6", "0") == "1"  # the fp16 + fp6 arithmetic for the layers that have a kernel for it (default: bf16x3)
F6_GATE = os.environ.get("PRV2_F6_GATE", "1") != "0"  # A/B switch of the mode's stage 2: the GatedConvUnit tail kernel (conv3x3_c256_gate_f6_kernel)


class F6Range:
    """The fp16 range guard of the fp16 + fp6 layers.  Every packed layer owns one word of a per-device table; its kernel raises the word
    to the float bits of the largest |relu(x) x_scale| it saw (prv2_conv3x3_f6, ``range_word``).  After a frame (one small D2H behind the
    frame's own synchronisation) ``check`` moves each layer's power-of-two ``x_scale`` so that its largest input sits near 2^8 -- 2^8 of
    head room below fp16's 65504, 22 binades of full-precision values below it -- and tells the caller whether the frame it just
    computed has to be recomputed: a layer saw values beyond fp16's range (its fp16 part saturated: finite but fp6-grade) or its whole
    input sat below 2^-10 (fp16 subnormals)."""
    SLOTS = 256
    moved = False
    TARGET_LOG2, LOW_LOG2, HIGH = 8, -10, 65504.0
    _tables: dict = {}

    @staticmethod
    def _key(device) -> str:
        """one key per physical device: 'cuda' (a config default) and 'cuda:0' (a tensor's .device) are the same table"""
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        return str(d)

    @classmethod
    def slot(cls, device, cw) -> torch.Tensor:
        import weakref
        device = torch.device(cls._key(device))
        ent = cls._tables.setdefault(str(device), dict(table=torch.zeros(cls.SLOTS, dtype=torch.int32, device=device), layers=[]))
        ent["layers"] = [(i, r) for i, r in ent["layers"] if r() is not None]
        used = {i for i, _ in ent["layers"]}
        i = next((k for k in range(cls.SLOTS) if k not in used), None)
        if i is None:
            raise RuntimeError(f"F6Range: all {cls.SLOTS} range words of {device} are taken by live fp16 + fp6 layers")
        ent["layers"].append((i, weakref.ref(cw)))
        ent["table"][i] = 0
        return ent["table"][i:i + 1]

    @classmethod
    def active(cls, device) -> bool:
        ent = cls._tables.get(cls._key(device))
        return bool(ent and any(r() is not None for _, r in ent["layers"]))

    @classmethod
    def check(cls, device, reduce=None) -> list:
        """-> [(layer, seen maximum, old x_scale)] of the layers whose frame must be recomputed (their x_scale is already moved); the
        table is cleared for the next frame.  ``reduce(table)``: an in-place MAX all-reduce over the ranks of a patch-sharded frame (the words are
        float bits of non-negative values: integer order == float order), so that every rank takes the same decision.
        ``cls.moved`` tells the caller whether ANY x_scale changed (captured hipGraphs carry the old scales as kernel arguments: the
        caller drops them, otherwise the next measurement would be taken under a scale this table no longer knows)"""
        cls.moved = False
        ent = cls._tables.get(cls._key(device))
        if not ent:
            return []
        if reduce is not None:
            reduce(ent["table"])
        seen = ent["table"].to("cpu", copy=True).view(torch.float32)  # (synchronises the current stream)
        ent["table"].zero_()
        redo = []
        for i, r in ent["layers"]:
            cw = r()
            m = float(seen[i]) if cw is not None else 0.0
            if m <= 0.0 or not math.isfinite(m):
                if cw is not None and not math.isfinite(m) and m != 0.0:
                    redo.append((cw, m, cw.x_scale))  # (inf / nan inputs: nothing a scale can do -- reported)
                continue
            e = math.floor(math.log2(m))
            if m > cls.HIGH or e < cls.LOW_LOG2:
                redo.append((cw, m, cw.x_scale))
            if m > cls.HIGH / 4 or e < cls.LOW_LOG2 + 6:  # (move early: two binades before the upper, six before the lower limit)
                cw.x_scale = cw.x_scale * 2.0 ** (cls.TARGET_LOG2 - e)
                cls.moved = True
        return redo

    @classmethod
    def clear(cls, device) -> None:
        """forget what the launches so far saw (callers that run the fp16 + fp6 layers outside a guarded frame)"""
        ent = cls._tables.get(cls._key(device))
        if ent:
            ent["table"].zero_()


def pack_conv3x3_f6(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, device=None) -> ConvWF6:
    """weight [256, cin, 3, 3] (cin % 64 == 0) -> the fragment-major fp16 + fp6 image of csrc/conv3x3_f6.hip."""
    lib = L.load()
    device = device or weight.device
    w = weight.detach().to(device=device, dtype=torch.float32).contiguous()
    cout, cin, kh, kw = w.shape
    nbytes = lib.prv2_conv3x3_f6_weight_bytes(cout, cin)
    assert (kh, kw) == (3, 3) and nbytes > 0, (cout, cin, kh, kw)
    amax = float(w.abs().max())
    w_scale = 2.0 ** -math.floor(math.log2(amax)) if amax > 0 else 1.0
    packed = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
    if DISPATCH == "torch":
        _tops().pack_conv3x3_f6_weight(w, w_scale, packed)
    else:
        _c("pack_conv3x3_f6_weight", w.data_ptr(), w_scale, packed.data_ptr(), cout, cin)
    b = bias.detach().to(device=device, dtype=torch.float32).contiguous() if bias is not None else None
    cw = ConvWF6(packed, b, cout, cin, w_scale, 1.0, None)
    cw.range = F6Range.slot(device, cw)
    return cw


def conv3x3_f6_supported(x: Feat, cout: int, cin: int, allow_x2: bool = False) -> bool:
    """shape contract of the fp16 + fp6 kernels (a property of the layer, never of the batch); ``allow_x2``: the gate-tail kernel also takes pre-split input"""
    if (getattr(x, "x2", False) and not allow_x2) or x.c != cin or x.ld % 4:
        return False
    d = _conv_desc(x, ConvWF6(None, None, cout, cin, 1.0), roundup(cout, 4))
    return bool(L.load().prv2_conv3x3_f6_supported(C.byref(d)))


def conv3x3_f6(x: Feat, cw: ConvWF6, out: Optional[Feat] = None, *, relu_in: bool = False, res: Optional[Feat] = None) -> Feat:
    """y = conv3x3(relu?(x)) + bias (+ res) in the fp16 + fp6 arithmetic (include/prv2.h::prv2_conv3x3_f6); ``out`` may be X2."""
    assert x.c == cw.cin and not getattr(x, "x2", False)
    if out is None:
        out = Feat.alloc(x.n, x.h, x.w, cw.cout, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, x.h, x.w, cw.cout)
    assert res is None or ((res.n, res.h, res.w, res.c) == (out.n, out.h, out.w, out.c) and not res.x2)
    d = _conv_desc(x, cw, out.ld, relu_in=relu_in, ld_res=_ld(res), fmt=L.FMT_Y_X2 if out.x2 else 0)
    out_scale = 1.0 / (cw.x_scale * cw.w_scale)

    def call():
        if DISPATCH == "torch":
            _tops().conv3x3_f6(x.view(), cw.w, cw.bias, res.view() if res is not None else None, relu_in, cw.x_scale, out_scale, cw.range, out.raw(), d.fmt)
        else:
            _c("conv3x3_f6", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), _ptr(res), cw.x_scale, out_scale, _ptr(cw.range), out.ptr)

    PROFILER.launch(_last_kernel, 2.0 * x.n * x.h * x.w * cw.cout * cw.cin * 9, call, shape=f"{cw.cin}->{cw.cout} k3s1 {x.n}x{x.h}x{x.w}")
    return out


def conv_out_hw(cw: ConvW, h: int, w: int):
    if cw.convt_k:
        return h * cw.convt_k, w * cw.convt_k
    if cw.same_pad:
        return -(-h // cw.stride), -(-w // cw.stride)
    return (h + 2 * cw.pad - cw.kh) // cw.stride + 1, (w + 2 * cw.pad - cw.kw) // cw.stride + 1


def _conv_desc(x, cw, ldy: int, *, act: int = ACT_NONE, relu_in: bool = False, ld_mul: int = 0, ld_res: int = 0, ld_res2: int = 0,
               ln_eps: float = 1e-6, x_bstride: int = 0, force_generic: bool = False, fmt: int = 0) -> "L.ConvDesc":
    """the prv2_conv_desc of the layer ``cw`` (ConvW / ConvWF6) on the input ``x`` (anything with n, h, w, ld) writing rows of pitch ``ldy``"""
    return L.ConvDesc(n=x.n, h=x.h, w=x.w, cin=cw.cin, cout=cw.cout, kh=cw.kh, kw=cw.kw, stride=cw.stride, pad=cw.pad, ldx=x.ld, ldy=ldy,
                      x_bstride=x_bstride, y_bstride=0, relu_in=int(relu_in), act=act, convt_k=cw.convt_k, ld_mul=ld_mul, ld_res=ld_res,
                      ld_res2=ld_res2, prec=cw.prec, force_generic=int(force_generic), ln_eps=ln_eps, part=0, same_pad=int(cw.same_pad), fmt=fmt)


def _ups_src(u) -> "L.UpsSrc":
    """the prv2_ups_src of a low-resolution map that a kernel interpolates itself"""
    return L.UpsSrc(x=u.ptr, h=u.h, w=u.w, ld=u.ld, channels=u.c, bstride=0)


def _gate_fmt(x, mul=None) -> int:
    """prv2_conv_desc.fmt of the 256-column conv kernels: which of x / mul are pre-split (X2) buffers"""
    return (L.FMT_X_X2 if getattr(x, "x2", False) else 0) | (L.FMT_MUL_X2 if mul is not None and mul.x2 else 0)


def _c256(x: Feat, cw: ConvW) -> bool:
    """does the library run this conv on its 256-channel 3x3 kernel (which fuses the LayerNorm at that width)?"""
    if x.c != cw.cin or x.ld % 4 or cw.cout != 256 or os.environ.get("PRV2_NO_C256"):
        return False
    return bool(L.load().prv2_conv3x3_ln_gate_supported(C.byref(_conv_desc(x, cw, roundup(cw.cout, 4), fmt=_gate_fmt(x)))))


def conv2d(x: Feat, cw: ConvW, out: Optional[Feat] = None, *, relu_in: bool = False, act: int = ACT_NONE,
           gamma: Optional[torch.Tensor] = None, mul: Optional[Feat] = None, res: Optional[Feat] = None,
           res2: Optional[Feat] = None, x_bstride: int = 0, force_generic: bool = False, ln=None,
           ln_eps: float = 1e-6, algo: Optional[float] = None) -> Feat:
    """y = epilogue(conv(x)); see include/prv2.h::prv2_conv2d.  ``ln`` = (weight, bias) of a channels-first
    LayerNorm applied between the bias and the activation (fused when cout <= 128, else a separate row-LN pass).
    ``algo``: the reference graph's FLOPs for this step when they differ from the executed ones (Profiler.launch)."""
    if ln is not None and cw.cout > 128 and not (gamma is None and mul is None and res2 is None and not force_generic and not x_bstride
                                                 and _c256(x, cw)):
        y = conv2d(x, cw, out, relu_in=relu_in, x_bstride=x_bstride, force_generic=force_generic)
        assert gamma is None and mul is None and res is None and res2 is None
        return layernorm_feat(y, ln[0], ln[1], ln_eps, act)
    assert x.c == cw.cin, (x.c, cw.cin)
    oh, ow = conv_out_hw(cw, x.h, x.w)
    if out is None:
        out = Feat.alloc(x.n, oh, ow, cw.cout, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, oh, ow, cw.cout), ((out.n, out.h, out.w, out.c), (x.n, oh, ow, cw.cout))
    d = _conv_desc(x, cw, out.ld, act=act, relu_in=relu_in, ld_mul=_ld(mul), ld_res=_ld(res), ld_res2=_ld(res2), ln_eps=ln_eps,
                   x_bstride=x_bstride, force_generic=force_generic)
    for aux in (mul, res, res2):
        if aux is not None:
            assert (aux.n, aux.h, aux.w, aux.c) == (out.n, out.h, out.w, out.c) and not aux.x2
    assert not getattr(x, "x2", False), "conv2d reads fp32 activations (X2 inputs: conv3x3_ln_gate)"
    if out.x2:  # pre-split output: written by the 256-column conv without LayerNorm (GatedConvUnit.conv -> the unit's concat buffer)
        assert ln is None and gamma is None and mul is None and res2 is None and not force_generic and not x_bstride and _c256(x, cw)
        d.fmt = L.FMT_Y_X2
    ncols = cw.cout * (cw.convt_k ** 2 if cw.convt_k else 1)
    taps = 1 if cw.convt_k else cw.kh * cw.kw
    m_rows = x.n * (x.h * x.w if cw.convt_k else oh * ow)
    halo = (cw.kh == 3 and cw.kw == 3 and cw.stride == 1 and (cw.pad == 1 or cw.same_pad) and not cw.convt_k and x.w >= 24 and x.h >= 4
            and not force_generic)  # only for the f32-mode strip split below; kernel names come from prv2_last_kernel()
    lnw, lnb = (ln[0], ln[1]) if ln is not None else (None, None)

    def call():
        if DISPATCH == "torch":
            v = lambda f: None if f is None else f.view()  # noqa: E731
            _tops().conv2d(x.view(), cw.w, cw.bias, cw.cout, cw.kh, cw.kw, cw.stride, cw.pad, act, relu_in, lnw, lnb, gamma, v(mul), v(res), v(res2),
                           cw.convt_k, cw.prec, ln_eps, cw.same_pad, out.raw(), d.fmt, force_generic, d.part)
        else:
            _c("conv2d", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), _ptr(lnw), _ptr(lnb), _ptr(gamma), _ptr(mul), _ptr(res), _ptr(res2), out.ptr)

    shape = f"{cw.cin}->{cw.cout} k{cw.kh}s{cw.stride}{'T' if cw.convt_k else ''} {x.n}x{x.h}x{x.w}"
    rem = x.w % 32
    if halo and PROFILER.enabled and 0 < rem <= 8 and x.w >= 64 and cw.prec == PREC_F32:
        # f32 mode: the library runs this conv as 32-pixel tiles + a remainder strip on the generic kernel (csrc/igemm.hip;
        # the bf16 modes do both in one launch); when launches are timed the two kernels are issued and accounted separately
        full = 2.0 * m_rows * ncols * cw.cin * taps
        d.part = 1
        PROFILER.launch(_last_kernel, full * (x.w - rem) / x.w, call, shape=shape)
        d.part = 2
        PROFILER.launch(_last_kernel, full * rem / x.w, call, shape=shape + f" strip{rem}")
        return out
    PROFILER.launch(_last_kernel, 2.0 * m_rows * ncols * cw.cin * taps, call, shape=shape, algo=algo)
    return out


UPS_FUSION = os.environ.get("PRV2_UPS_FUSION", "1") != "0"  # A/B and test switch: bilinear upsample fused into the consumer conv's loader


class UpsOnly:
    """the ``x`` of ``conv2d_ups`` when EVERY input channel comes from the upsampled source (u.c == cin): only the output size"""

    def __init__(self, u: Feat, h: int, w: int):
        self.n, self.h, self.w, self.c, self.ld, self.ptr, self.device = u.n, h, w, u.c, u.ld, u.ptr, u.device


def conv2d_ups_supported(x, u: Feat, cw: ConvW) -> bool:
    """can ``conv2d_ups`` fuse the upsample of ``u`` (the first u.c input channels) into this 3x3 conv's loader?  A property of the
    layer (channels, per-image size, arithmetic mode) -- never of the batch."""
    if not UPS_FUSION or type(x) not in (Feat, UpsOnly) or type(u) is not Feat or x.n != u.n or (x.h, x.w) == (u.h, u.w):
        return False
    return bool(L.load().prv2_conv2d_ups_supported(C.byref(_conv_desc(x, cw, roundup(cw.cout, 4))), C.byref(_ups_src(u))))


UPCONV = os.environ.get("PRV2_UPCONV", "1") != "0"  # A/B and test switch: 3x3 convs of an upsampled tensor computed at the low resolution


def upconv3x3_supported(u: Feat, h: int, w: int, cw: ConvW) -> bool:
    """can ``upconv3x3`` take conv3x3(bilinear_align_corners(u -> h x w); cw)?  A property of the layer (channels, per-image sizes, mode)."""
    if not UPCONV or type(u) is not Feat or (cw.kh, cw.kw, cw.stride, cw.pad, cw.convt_k) != (3, 3, 1, 1, 0) or cw.cin != u.c or cw.same_pad:
        return False
    return bool(L.load().prv2_upconv3x3_supported(C.byref(_ups_src(u)), u.n, h, w, cw.cout, cw.prec))


def upconv3x3(u: Feat, h: int, w: int, cw: ConvW, out: Optional[Feat] = None, *, act: int = ACT_NONE, bias: bool = True, add: Optional[Feat] = None) -> Feat:
    """act(conv3x3(bilinear_align_corners(u -> h x w); cw) + bias) computed at u's resolution (include/prv2.h::prv2_upconv3x3): nine tap
    GEMMs on the low-resolution grid, then the four interpolation corners of every tap gathered per output pixel -- 2.3x fewer matrix
    operations than ``conv2d_ups``.  fp32-grade, not bit-identical to it (summation order).  ``add`` [n, h, w, cout]: a pre-activation
    addend -- the direct conv over the REST of a concat input [up(u) | rest] with the other weight columns (it may be ``out`` itself)."""
    assert cw.cin == u.c
    if out is None:
        out = Feat.alloc(u.n, h, w, cw.cout, u.device)
    assert (out.n, out.h, out.w, out.c) == (u.n, h, w, cw.cout)
    b = cw.bias if bias else None

    def call():
        if DISPATCH == "torch":
            _tops().upconv3x3(u.view(), cw.w, b, cw.cout, h, w, act, cw.prec, out.view(), add.view() if add is not None else None)
        else:
            _c("upconv3x3", C.byref(_ups_src(u)), cw.w.data_ptr(), _ptr(b), _ptr(add), _ld(add), u.n, h, w, cw.cout, act, cw.prec, out.ptr, out.ld, 0)

    # executed: the tap GEMMs over every tile's 192-pixel source footprint (16 x 28 output tiles, 32-channel passes); algo: the reference
    # graph's nine taps at the OUTPUT resolution
    wide = (u.h - 1) * 2 <= (h - 1) and (u.w - 1) * 2 <= (w - 1)  # (csrc/upconv.hip: 16 x 28 output tiles up to a source step of 1/2, else 14 x 24)
    tiles = -(-h // 16) * -(-w // 28) if wide else -(-h // 14) * -(-w // 24)
    shape = f"{cw.cin}->{cw.cout} k3s1 {u.n}x{h}x{w} (lowres {u.c}ch {u.h}x{u.w})"
    PROFILER.launch(_last_kernel, 2.0 * u.n * tiles * 192 * 9 * cw.cin * roundup(cw.cout, 32), call, shape=shape, algo=2.0 * u.n * h * w * cw.cout * cw.cin * 9)
    return out


UPCONV5 = os.environ.get("PRV2_UPCONV5", "1") != "0"  # A/B and test switch: output_conv2[0] o output_conv1 o interpolate as one 5x5 conv at the source resolution


def compose_upconv5x5(w1: torch.Tensor, b1: torch.Tensor, tap_bias: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor], device, prec) -> dict:
    """Host side (float64) of ``upconv5x5``: two back-to-back 3x3 convs -- w1 [m, ci, 3, 3] + bias b1 [m] (+ ``tap_bias`` [9, m]: what each tap of the
    first conv adds where it lies inside the image -- the folded bias of an upstream 1x1, fusion.py), w2 [co, m, 3, 3] + b2 -- as
    dict(w5 = packed 5x5 composite, bias_map [5, 5, co], edge = packed 1x1 weights [28 co, ci] of the ring fix).  The algebra:
    tools/studies/composite5x5_ring.py (include/prv2.h::prv2_upconv5x5)."""
    import torch.nn.functional as F
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    w1, w2 = d(w1), d(w2)
    m, ci = w1.shape[:2]
    co = w2.shape[0]
    b1 = d(b1) if b1 is not None else torch.zeros(m, dtype=torch.float64)
    b2 = d(b2) if b2 is not None else torch.zeros(co, dtype=torch.float64)
    tap_bias = d(tap_bias) if tap_bias is not None else torch.zeros(9, m, dtype=torch.float64)
    weff = torch.zeros(co, ci, 5, 5, dtype=torch.float64)
    for y2 in range(3):
        for x2 in range(3):
            weff[:, :, y2:y2 + 3, x2:x2 + 3] += torch.einsum("om,miyx->oiyx", w2[:, :, y2, x2], w1)
    inside = torch.ones(1, 1, 8, 8, dtype=torch.float64)
    tb = b1.view(1, m, 1, 1) + F.conv2d(inside, tap_bias.t().reshape(m, 1, 3, 3), padding=1)
    vb = F.conv2d(tb, w2, b2, padding=1)[0]
    cls = [0, 1, 3, 6, 7]  # rows / columns of the 8 x 8 grid standing for the classes 0, 1, interior, h - 2, h - 1
    bias_map = vb[:, cls][:, :, cls].permute(1, 2, 0).contiguous()

    def edge(k2sel, k1sel):
        we = torch.zeros(5, co, ci, dtype=torch.float64)
        for k2 in range(3):
            for k1 in range(3):
                we[k2 + k1] += k2sel(k2) @ k1sel(k1)
        return we
    zero = torch.zeros(co, ci, dtype=torch.float64)
    groups = [  # (five taps along the edge, corner term at the line's first position, at its last) per edge: top, bottom, left, right
        (edge(lambda k: w2[:, :, 0, k], lambda k: w1[:, :, 2, k]), w2[:, :, 0, 0] @ w1[:, :, 2, 2], w2[:, :, 0, 2] @ w1[:, :, 2, 0]),
        (edge(lambda k: w2[:, :, 2, k], lambda k: w1[:, :, 0, k]), w2[:, :, 2, 0] @ w1[:, :, 0, 2], w2[:, :, 2, 2] @ w1[:, :, 0, 0]),
        (edge(lambda k: w2[:, :, k, 0], lambda k: w1[:, :, k, 2]), zero, zero),
        (edge(lambda k: w2[:, :, k, 2], lambda k: w1[:, :, k, 0]), zero, zero)]
    wedge = torch.cat([torch.cat([we.reshape(5 * co, ci), c0, c1], 0) for we, c0, c1 in groups], 0)  # [28 co, ci]
    return dict(w5=pack_conv(weff.float(), None, pad=2, device=device, prec=prec), bias_map=bias_map.float().contiguous().to(device),
                edge=pack_conv(wedge.float(), None, device=device, prec=prec), cout=co)


def upconv5x5_supported(u: Feat, h: int, w: int, cw5: dict) -> bool:
    if not UPCONV5 or type(u) is not Feat or cw5["w5"].cin != u.c:
        return False
    return bool(L.load().prv2_upconv5x5_supported(C.byref(_ups_src(u)), u.n, h, w, cw5["cout"], cw5["w5"].prec))


def upconv5x5(u: Feat, h: int, w: int, cw5: dict, out: Optional[Feat] = None, *, act: int = ACT_NONE) -> Feat:
    """act(conv3x3(conv3x3(bilinear_align_corners(u -> h x w); W1) + b1; W2) + b2) as ONE 5x5 conv at u's resolution + the bias classes + the
    fix of the one-pixel border ring (include/prv2.h::prv2_upconv5x5 / _lines / _ring; ``compose_upconv5x5``): the 3x3 pair's intermediate
    map is never formed.  fp32-grade, not bit-identical to the two-conv sequence."""
    cw, co = cw5["w5"], cw5["cout"]
    if out is None:
        out = Feat.alloc(u.n, h, w, co, u.device)
    assert (out.n, out.h, out.w, out.c) == (u.n, h, w, co) and not out.x2
    us = _ups_src(u)

    def main():
        if DISPATCH == "torch":
            _tops().upconv5x5(u.view(), cw.w, cw5["bias_map"], co, h, w, act, cw.prec, out.view())
        else:
            _c("upconv5x5", C.byref(us), cw.w.data_ptr(), cw5["bias_map"].data_ptr(), u.n, h, w, co, act, cw.prec, out.ptr, out.ld, 0)

    tiles = -(-h // 14) * -(-w // 24)  # (csrc/upconv5.hip: 14 x 24 output tiles, 192-pixel source footprint, five 160-column kernel-row passes)
    PROFILER.launch(_last_kernel, 2.0 * u.n * tiles * 192 * 25 * cw.cin * 32, main,
                    shape=f"{cw.cin}->(128)->{co} k5 {u.n}x{h}x{w} (lowres {u.c}ch {u.h}x{u.w})", algo=cw5.get("algo_per_px", 0.0) * u.n * h * w)
    _upconv5x5_ring(u, us, h, w, cw5["edge"], out, act)
    return out


def _upconv5x5_ring(u: Feat, us, h: int, w: int, edge: ConvW, out: Feat, act: int):
    """the ring of ``upconv5x5``: the four border lines of up(u) at u's resolution -> tap GEMMs of the edges -> 1-D gather on the ring pixels"""
    if DISPATCH == "torch":
        lines = Feat(_tops().upconv5x5_lines(u.view(), h, w))
        ge = conv2d(lines, edge, algo=0.0)
        _tops().upconv5x5_ring_(out.view(), ge.view(), u.h, u.w, act)
    else:
        lines = Feat(torch.empty((u.n, 1, 2 * u.w + 2 * u.h, u.c), device=u.device, dtype=torch.float32))
        _c("upconv5x5_lines", C.byref(us), u.n, h, w, lines.ptr)
        ge = conv2d(lines, edge, algo=0.0)
        _c("upconv5x5_ring", out.ptr, out.ld, 0, u.n, h, w, out.c, ge.ptr, ge.ld, u.h, u.w, act)


def conv2d_ups(x: Feat, u: Feat, cw: ConvW, out: Optional[Feat] = None, *, act: int = ACT_NONE, res: Optional[Feat] = None, ln=None,
               ln_eps: float = 1e-6) -> Feat:
    """3x3 conv over the VIRTUAL concat [bilinear_align_corners(u -> x.h x x.w) | x[..., u.c:]]: channels [0, u.c) are interpolated
    from the low-resolution ``u`` inside the conv's tile loader (include/prv2.h::prv2_conv2d_ups); ``x`` supplies the rest at
    their usual channel offsets (its first u.c channels are never read).  Bit-identical to upsample_bilinear(u, out=x.slice(0, u.c))
    followed by conv2d(x, cw)."""
    assert x.c == cw.cin and u.c <= x.c and (u.n, x.n) == (x.n, u.n)
    oh, ow = conv_out_hw(cw, x.h, x.w)
    if out is None:
        out = Feat.alloc(x.n, oh, ow, cw.cout, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, oh, ow, cw.cout)
    d, us = _conv_desc(x, cw, out.ld, act=act, ld_res=_ld(res), ln_eps=ln_eps), _ups_src(u)
    lnw, lnb = (ln[0], ln[1]) if ln is not None else (None, None)

    def call():
        if DISPATCH == "torch":
            _tops().conv3x3_ups(None if type(x) is UpsOnly else x.view(), u.view(), cw.w, cw.bias, cw.cout, x.h, x.w, act, lnw, lnb,
                                res.view() if res is not None else None, cw.prec, ln_eps, out.view())
        else:
            _c("conv2d_ups", C.byref(d), x.ptr, C.byref(us), cw.w.data_ptr(), _ptr(cw.bias), _ptr(lnw), _ptr(lnb), _ptr(res), out.ptr)

    PROFILER.launch(_last_kernel, 2.0 * x.n * oh * ow * cw.cout * cw.cin * 9, call, shape=f"{cw.cin}->{cw.cout} k3s1 {x.n}x{x.h}x{x.w} (+up {u.c}ch {u.h}x{u.w})")
    return out


TAIL_FUSION = os.environ.get("PRV2_TAIL_FUSION", "1") != "0"  # A/B and test switch: [pred1 | pred2] tails written by the conv that fills the row


def conv2d_tail_supported(x: Feat, cw: ConvW, out: Feat) -> bool:
    """can ``conv2d_tail`` close the [.. | pred1 | pred2 | 0 | 0] row behind this conv's output slice?  (a property of the layer)"""
    if not TAIL_FUSION or not DIRECT_PLACEMENT or type(x) is not Feat or out.ld != out.c0 + cw.cout + 4 or (out.c0 + cw.cout) % 4:
        return False
    return bool(L.load().prv2_conv2d_tail_supported(C.byref(_conv_desc(x, cw, out.ld))))


def conv2d_tail(x: Feat, cw: ConvW, out: Feat, p1: Feat, p2: Feat, *, act: int = ACT_NONE, ln=None, ln_eps: float = 1e-6) -> Feat:
    """conv2d(x, cw, out, act=, ln=) that also writes (p1, p2, 0, 0) -- the two dense depth maps resized bilinear(align_corners) to
    the output size -- into the four channels behind ``out``'s slice (include/prv2.h::prv2_conv2d_tail); bit-identical to
    conv2d + depth_pair_fill"""
    assert x.c == cw.cin and (out.n, out.h, out.w, out.c) == (x.n, x.h, x.w, cw.cout) and out.ld == out.c0 + cw.cout + 4
    assert p1.c == 1 and p2.c == 1 and p1.ld == 1 and p2.ld == 1 and (p1.n, p1.h, p1.w) == (p2.n, p2.h, p2.w) and p1.n == x.n
    d = _conv_desc(x, cw, out.ld, act=act, ln_eps=ln_eps)
    lnw, lnb = (ln[0], ln[1]) if ln is not None else (None, None)

    def call():
        if DISPATCH == "torch":
            _tops().conv3x3_tail(x.view(), cw.w, cw.bias, cw.cout, act, lnw, lnb, None, p1.buf.view(p1.n, p1.h, p1.w), p2.buf.view(p2.n, p2.h, p2.w),
                                 cw.prec, ln_eps, out.view())
        else:
            _c("conv2d_tail", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), _ptr(lnw), _ptr(lnb), None, p1.ptr, p2.ptr, p1.h, p1.w, out.ptr)

    PROFILER.launch(_last_kernel, 2.0 * x.n * x.h * x.w * cw.cout * cw.cin * 9, call, shape=f"{cw.cin}->{cw.cout} k3s1 {x.n}x{x.h}x{x.w} (+tail)")
    return out


GATE_FUSION = os.environ.get("PRV2_GATE_FUSION", "1") != "0"  # A/B and test switch: GatedConvUnit tail as one kernel
X2_FORMAT = os.environ.get("PRV2_X2", "1") != "0"  # A/B and test switch: the GatedConvUnit's concat buffer in the pre-split operand format
# widths F of a GatedConvUnit the library fuses (prv2_conv3x3_ln_gate); PRV2_GATE_CHANNELS=256 restricts them for A/B runs
GATE_CHANNELS = tuple(int(c) for c in os.environ.get("PRV2_GATE_CHANNELS", "32,128,256").split(","))


def pack_gate(weight: torch.Tensor) -> torch.Tensor:
    """fragment-major image of a C -> C 1x1 conv's weights (C = 32, 128, 256) for ``conv3x3_ln_gate`` (prv2_pack_gate_weight)"""
    w = weight.detach().to(torch.float32).reshape(weight.shape[0], -1).contiguous()
    c = w.shape[0]
    assert w.shape == (c, c) and c in GATE_CHANNELS and w.is_cuda
    if DISPATCH == "torch":
        return _tops().pack_gate_weight(w)
    dst = torch.empty(L.load().prv2_gate_weight_bytes(c) // 4, device=w.device, dtype=torch.float32)
    _require_dev(w)
    _c("pack_gate_weight", w.data_ptr(), dst.data_ptr(), c, c)
    return dst


def conv3x3_ln_gate_supported(x: Feat, cw: ConvW) -> bool:
    """shape contract of the fused kernel (layer shape per image only: the choice never depends on the batch)"""
    if not GATE_FUSION or x.c != cw.cin or x.ld % 4 or cw.cout not in GATE_CHANNELS:
        return False
    return bool(L.load().prv2_conv3x3_ln_gate_supported(C.byref(_conv_desc(x, cw, roundup(cw.cout, 4), fmt=_gate_fmt(x)))))


TAPS_FOLD = os.environ.get("PRV2_TAPS_FOLD", "1") != "0"  # A/B switch: the 256-column gate kernels gather their coarse addend themselves


def conv3x3_ln_gate_taps_supported(x: Feat, cw) -> bool:
    """can the gate kernel that runs this layer take ``CoarseTaps`` tables instead of a gathered ``pre``? (the 256-column kernels)"""
    if not TAPS_FOLD or cw.cout != 256 or x.c != cw.cin or x.ld % 4:
        return False
    return bool(L.load().prv2_conv3x3_ln_gate_taps_supported(C.byref(_conv_desc(x, cw, 256, fmt=_gate_fmt(x)))))


def _tap_tables(taps: "CoarseTaps", boxes: torch.Tensor, spatial_scale: float, n: int) -> "L.TapTables":
    """prv2_tap_tables of ``taps`` for the n tiles ``boxes`` (the checks of ``CoarseTaps.gather``)"""
    assert boxes.dtype == torch.float32 and boxes.is_cuda and boxes.is_contiguous() and tuple(boxes.shape) == (n, 5 if taps.nf else 4)
    assert taps.cout == 256 and not taps.v.x2 and not taps.g.x2
    return L.TapTables(v=taps.v.ptr, g=taps.g.ptr, boxes=boxes.data_ptr(), n_frames=taps.g.n if taps.nf else 0, h=taps.g.h, w=taps.g.w, ldv=taps.v.ld,
                       ldg=taps.g.ld, knot_bh=taps.kb[0], knot_bw=taps.kb[1], spatial_scale=spatial_scale)


def conv3x3_ln_gate(x: Feat, cw: ConvW, ln, gate_w: Optional[torch.Tensor], gate_bias: Optional[torch.Tensor], out: Optional[Feat] = None,
                    *, act: int = ACT_RELU, mul: Optional[Feat] = None, res: Optional[Feat] = None, relu_in: bool = False,
                    ln_eps: float = 1e-6, pre: Optional[Feat] = None, pre_cin: int = 0, taps: Optional["CoarseTaps"] = None,
                    boxes: Optional[torch.Tensor] = None, spatial_scale: float = 1.0) -> Feat:
    """y = mul * sigmoid(conv1x1(act(LN(conv3x3(x) + b))) + gate_bias) (+ res) in one kernel (include/prv2.h::prv2_conv3x3_ln_gate);
    ``gate_w`` None: y = act(LN(conv3x3(x) + b)).  ``pre``: pre-LayerNorm addend [n, h, w, cout] -- the conv's coarse half from
    ``CoarseTaps.gather`` (prv2_conv3x3_ln_gate_pre), standing for ``pre_cin`` further input channels of the reference's conv.
    ``taps`` + ``boxes`` + ``spatial_scale`` instead of ``pre``: the kernel gathers that addend itself (prv2_conv3x3_ln_gate_taps; same bits)."""
    if out is None:
        out = Feat.alloc(x.n, x.h, x.w, cw.cout, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, x.h, x.w, cw.cout) and x.c == cw.cin
    for aux in (mul, res):
        assert aux is None or (aux.n, aux.h, aux.w, aux.c) == (out.n, out.h, out.w, out.c)
    d = _conv_desc(x, cw, out.ld, act=act, relu_in=relu_in, ld_mul=_ld(mul), ld_res=_ld(res), ln_eps=ln_eps, fmt=_gate_fmt(x, mul))
    assert not out.x2 and (res is None or not res.x2)
    flops = 2.0 * x.n * x.h * x.w * cw.cout * (cw.cin * 9 + (cw.cout if gate_w is not None else 0))
    if pre is not None:
        assert taps is None and (pre.n, pre.h, pre.w, pre.c) == (out.n, out.h, out.w, out.c) and not pre.x2
    boxes = boxes.contiguous() if taps is not None else None
    tt = _tap_tables(taps, boxes, spatial_scale, x.n) if taps is not None else None

    def call():
        r = lambda f: None if f is None else f.raw()  # noqa: E731
        if tt is not None and DISPATCH == "torch":
            _tops().conv3x3_ln_gate_taps(x.raw(), cw.w, cw.bias, ln[0], ln[1], gate_w, gate_bias, r(mul), r(res), act, relu_in, cw.prec, ln_eps, out.view(),
                                         d.fmt, taps.v.view(), taps.g.view(), boxes, bool(taps.nf), *taps.kb, float(spatial_scale))
        elif tt is not None:
            _c("conv3x3_ln_gate_taps", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), C.byref(tt), _ptr(ln[0]), _ptr(ln[1]), _ptr(gate_w),
               _ptr(gate_bias), _ptr(mul), _ptr(res), out.ptr)
        elif DISPATCH == "torch":
            _tops().conv3x3_ln_gate(x.raw(), cw.w, cw.bias, ln[0], ln[1], gate_w, gate_bias, r(mul), r(res), act, relu_in, cw.prec, ln_eps, out.view(),
                                    r(pre), d.fmt)
        else:
            _c("conv3x3_ln_gate_pre", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), _ptr(pre), _ld(pre), _ptr(ln[0]), _ptr(ln[1]), _ptr(gate_w),
               _ptr(gate_bias), _ptr(mul), _ptr(res), out.ptr, what="conv3x3_ln_gate")

    has_pre = pre is not None or tt is not None
    coarse = f"(+{pre_cin} coarse)" if has_pre else ""
    PROFILER.launch(_last_kernel, flops, call,
                    shape=f"{cw.cin}{coarse}->{cw.cout}{'->' + str(cw.cout) + ' gate' if gate_w is not None else ''} k3s1 {x.n}x{x.h}x{x.w}",
                    algo=flops + 2.0 * x.n * x.h * x.w * cw.cout * pre_cin * 9 if has_pre else None)
    return out


def conv3x3_ln_gate_f6(x: Feat, cw: ConvWF6, ln, gate_w: torch.Tensor, gate_bias: Optional[torch.Tensor], out: Optional[Feat] = None, *,
                       act: int = ACT_RELU, mul: Optional[Feat] = None, res: Optional[Feat] = None, ln_eps: float = 1e-6,
                       pre: Optional[Feat] = None, pre_cin: int = 0, taps: Optional["CoarseTaps"] = None, boxes: Optional[torch.Tensor] = None,
                       spatial_scale: float = 1.0) -> Feat:
    """``conv3x3_ln_gate`` with the 3x3 conv in the fp16 + fp6 arithmetic (include/prv2.h::prv2_conv3x3_ln_gate_f6): x and mul in one format -- the unit's
    pre-split (X2) ``out`` / concat, or the fp32 concat; LayerNorm, gate GEMM (bf16x3) and final stage are the bf16x3 kernel's.  ``taps`` + ``boxes`` +
    ``spatial_scale`` instead of ``pre``: prv2_conv3x3_ln_gate_f6_taps."""
    x2 = bool(getattr(x, "x2", False))
    assert x.c == cw.cin and (mul is None or bool(mul.x2) == x2)
    if out is None:
        out = Feat.alloc(x.n, x.h, x.w, cw.cout, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, x.h, x.w, cw.cout) and not out.x2 and (res is None or not res.x2)
    for aux in (mul, res, pre):
        assert aux is None or (aux.n, aux.h, aux.w, aux.c) == (out.n, out.h, out.w, out.c)
    d = _conv_desc(x, cw, out.ld, act=act, ld_mul=_ld(mul), ld_res=_ld(res), ln_eps=ln_eps, fmt=_gate_fmt(x, mul))
    out_scale = 1.0 / (cw.x_scale * cw.w_scale)
    flops = 2.0 * x.n * x.h * x.w * cw.cout * (cw.cin * 9 + cw.cout)
    assert pre is None or taps is None
    boxes = boxes.contiguous() if taps is not None else None
    tt = _tap_tables(taps, boxes, spatial_scale, x.n) if taps is not None else None

    def call():
        r = lambda f: None if f is None else f.raw()  # noqa: E731
        if tt is not None and DISPATCH == "torch":
            _tops().conv3x3_ln_gate_f6_taps(x.raw(), cw.w, cw.bias, ln[0], ln[1], gate_w, gate_bias, r(mul), r(res), act, ln_eps, cw.x_scale, out_scale,
                                            cw.range, out.view(), d.fmt, taps.v.view(), taps.g.view(), boxes, bool(taps.nf), *taps.kb, float(spatial_scale))
        elif tt is not None:
            _c("conv3x3_ln_gate_f6_taps", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), C.byref(tt), _ptr(ln[0]), _ptr(ln[1]), _ptr(gate_w),
               _ptr(gate_bias), _ptr(mul), _ptr(res), cw.x_scale, out_scale, _ptr(cw.range), out.ptr)
        elif DISPATCH == "torch":
            _tops().conv3x3_ln_gate_f6(x.raw(), cw.w, cw.bias, r(pre), ln[0], ln[1], gate_w, gate_bias, r(mul), r(res), act, ln_eps, cw.x_scale, out_scale,
                                       cw.range, out.view(), d.fmt)
        else:
            _c("conv3x3_ln_gate_f6", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), _ptr(pre), _ld(pre), _ptr(ln[0]), _ptr(ln[1]), _ptr(gate_w),
               _ptr(gate_bias), _ptr(mul), _ptr(res), cw.x_scale, out_scale, _ptr(cw.range), out.ptr)

    has_pre = pre is not None or tt is not None
    coarse = f"(+{pre_cin} coarse)" if has_pre else ""
    PROFILER.launch(_last_kernel, flops, call, shape=f"{cw.cin}{coarse}->{cw.cout}->{cw.cout} gate k3s1 {x.n}x{x.h}x{x.w}",
                    algo=flops + 2.0 * x.n * x.h * x.w * cw.cout * pre_cin * 9 if has_pre else None)
    return out


def linear(x2d: torch.Tensor, cw: ConvW, out: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
    """rows [M, K] @ W^T (+ epilogue) -> [M, N]; a 1x1 convolution over an M x 1 image."""
    M, K = x2d.shape
    xf = Feat(x2d.view(1, M, 1, K), cw.cin)
    if out is None:
        out = torch.empty((M, cw.cout), device=x2d.device, dtype=torch.float32)
    of = Feat(out.view(1, M, 1, out.shape[1]), cw.cout)
    for k in ("mul", "res", "res2"):
        if kw.get(k) is not None and not isinstance(kw[k], Feat):
            t = kw[k]
            kw[k] = Feat(t.view(1, M, 1, t.shape[1]), cw.cout)
    conv2d(xf, cw, of, **kw)
    return out


def conv2d_cout1(x: Feat, weight: torch.Tensor, bias: Optional[torch.Tensor], k: int, *, act: int = ACT_NONE,
                 scale: float = 1.0, res: Optional[torch.Tensor] = None, clamp0: bool = False,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Single-output-channel conv -> dense [n, 1, h, w] tensor (NCHW == NHWC for one channel)."""
    y = out if out is not None else torch.empty((x.n, 1, x.h, x.w), device=x.device, dtype=torch.float32)
    assert y.is_contiguous() and y.numel() == x.n * x.h * x.w
    def call():
        if DISPATCH == "torch":
            _tops().conv_cout1(x.view(), weight, bias, k, act, scale, res, clamp0, y)
        else:
            _c("conv2d_cout1", x.ptr, x.n, x.h, x.w, x.c, x.ld, weight.data_ptr(), k, _ptr(bias), act, scale, _ptr(res), int(clamp0), y.data_ptr())

    PROFILER.launch("conv_cout1_kernel", 2.0 * x.n * x.h * x.w * x.c * k * k, call)
    return y


def dwconv2d(x: Feat, w_tapmajor: torch.Tensor, bias: Optional[torch.Tensor], k: int, stride: int, relu=False, *,
             act: Optional[int] = None, same_pad: bool = False) -> Feat:
    """depthwise k x k; ``relu`` (bool) or any ``act``; ``same_pad``: timm Conv2dSame (output ceil(h / stride))"""
    act = (ACT_RELU if relu else ACT_NONE) if act is None else act
    if same_pad:
        oh, ow = -(-x.h // stride), -(-x.w // stride)
    else:
        oh = (x.h + 2 * (k // 2) - k) // stride + 1
        ow = (x.w + 2 * (k // 2) - k) // stride + 1
    box = []  # the output: the tensor the torch op allocates, or the Feat allocated here
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().dwconv2d(x.view(), w_tapmajor, bias, k, stride, act, same_pad))  # noqa: E731
    else:
        out = Feat.alloc(x.n, oh, ow, x.c, x.device)
        box.append(out)
        call = lambda: _c("dwconv2d_ex", x.ptr, x.n, x.h, x.w, x.c, x.ld, w_tapmajor.data_ptr(), _ptr(bias), k, stride, act, int(same_pad),  # noqa: E731
                          out.ptr, out.ld, what="dwconv2d")
    PROFILER.launch("dwconv_kernel", 2.0 * x.n * oh * ow * x.c * k * k, call)
    return box[0] if isinstance(box[0], Feat) else _feat_of(box[0], x.c)


def global_avgpool(x: Feat) -> torch.Tensor:
    """[n, c] mean over the pixels (the squeeze of timm's SqueezeExcite: x.mean((2, 3)))"""
    assert x.c % 4 == 0
    box = []  # the output: what the torch op returns, or the buffer allocated here
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().global_avgpool(x.view()))  # noqa: E731
    else:
        out = torch.empty((x.n, x.c), device=x.device, dtype=torch.float32)
        ws = torch.empty(L.load().prv2_global_avgpool_workspace_floats(x.n, x.h * x.w, x.c), device=x.device, dtype=torch.float32)
        box.append(out)
        call = lambda: _c("global_avgpool", x.ptr, x.n, x.h * x.w, x.c, x.ld, out.data_ptr(), ws.data_ptr())  # noqa: E731
    PROFILER.launch_aux("global_avgpool", 4.0 * x.n * x.h * x.w * x.c, call, f"{x.c}ch {x.n}x{x.h}x{x.w}")
    return box[0]


def se_gate(mean: torch.Tensor, w1: torch.Tensor, b1, w2t: torch.Tensor, b2) -> torch.Tensor:
    """sigmoid(W2 silu(W1 mean + b1) + b2) per image: timm SqueezeExcite's conv_reduce -> act -> conv_expand -> gate.
    w1 [cse, c]; w2t [cse, c] = conv_expand's weight transposed."""
    n, c = mean.shape
    cse = w1.shape[0]
    assert w1.shape == (cse, c) and w2t.shape == (cse, c) and w1.is_contiguous() and w2t.is_contiguous()
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().se_gate(mean, w1, b1, w2t, b2))  # noqa: E731
    else:
        g = torch.empty((n, c), device=mean.device, dtype=torch.float32)
        ws = torch.empty((n, cse), device=mean.device, dtype=torch.float32)
        box.append(g)
        call = lambda: _c("se_gate", mean.data_ptr(), n, c, w1.data_ptr(), _ptr(b1), cse, w2t.data_ptr(), _ptr(b2), g.data_ptr(), ws.data_ptr())  # noqa: E731
    PROFILER.launch_aux("se_gate", 4.0 * (n * c + 2 * c * cse), call, f"{c}->{cse}->{c} x{n}")
    return box[0]


def channel_scale_(x: Feat, s: torch.Tensor) -> Feat:
    """x *= s[n, c] in place (the excite of SqueezeExcite)"""
    assert s.shape == (x.n, x.c) and s.is_contiguous() and x.c % 4 == 0
    def call():
        if DISPATCH == "torch":
            _tops().channel_scale_(x.view(), s)
        else:
            _c("channel_scale", x.ptr, x.n, x.h * x.w, x.c, x.ld, s.data_ptr())

    PROFILER.launch_aux("channel_scale", 8.0 * x.n * x.h * x.w * x.c, call, f"{x.c}ch {x.n}x{x.h}x{x.w}")
    return x


def layernorm_rows(x: torch.Tensor, rows: int, c: int, ldx: int, weight, bias, eps: float, act: int, y: torch.Tensor,
                   ldy: int, x_off: int = 0, y_off: int = 0):
    if DISPATCH == "torch":
        _tops().layernorm(torch.as_strided(x, (rows, c), (ldx, 1), x.storage_offset() + x_off), weight, bias, eps, act,
                          torch.as_strided(y, (rows, c), (ldy, 1), y.storage_offset() + y_off))
        return
    _c("layernorm", x.data_ptr() + 4 * x_off, rows, c, ldx, weight.data_ptr(), bias.data_ptr(), eps, act, y.data_ptr() + 4 * y_off, ldy)


def layernorm_feat(x: Feat, weight, bias, eps: float = 1e-6, act: int = ACT_NONE, out: Optional[Feat] = None) -> Feat:
    """channels-first LayerNorm of the reference == row LayerNorm in NHWC (convs.py:21-29)."""
    if out is None:
        out = x
    rows = x.n * x.h * x.w

    def call():
        if DISPATCH == "torch":
            _tops().layernorm(x.view().reshape(rows, x.c) if x.ld == x.c else torch.as_strided(x.buf, (rows, x.c), (x.ld, 1), x.buf.storage_offset() + x.c0),
                              weight, bias, eps, act, torch.as_strided(out.buf, (rows, out.c), (out.ld, 1), out.buf.storage_offset() + out.c0))
        else:
            _c("layernorm", x.ptr, rows, x.c, x.ld, weight.data_ptr(), bias.data_ptr(), eps, act, out.ptr, out.ld)

    PROFILER.launch_aux("layernorm", 8.0 * rows * x.c, call, f"{x.c}ch {x.n}x{x.h}x{x.w}")
    return out


# ---- split-swizzled ("ss") operands of the large ViT linears (csrc/gemm_ss.hip; include/prv2.h "Split-swizzled") --------------
# An ss tensor is carried as a float32 [rows, C] container (same bytes per element as fp32); only the kernels interpret it.
SS_DISABLED = False  # A/B and test switch: keep the ViT blocks on the fp32-operand kernels
SS_MIN_ROWS = 512   # token rows from which the ViT blocks run on the pre-split path (bit-identical to the fp32-operand path;
                    # measured per linear vs gemm16: +25..37 % at 14 k rows, +20 % at 4 k, +30 % / 0 / -8 % (qkv, fc1 / proj / fc2) at
                    # 1037: profiles/r02_gemm_ss_bench.txt)


def split_ss(x2d: torch.Tensor) -> torch.Tensor:
    M, K = x2d.shape
    _require_dev(x2d)
    if DISPATCH == "torch":
        return _tops().split_ss(x2d)
    out = torch.empty((M, K), device=x2d.device, dtype=torch.float32)
    _c("split_ss", x2d.data_ptr(), M, K, x2d.stride(0), out.data_ptr())
    return out


def layernorm_ss(x: torch.Tensor, rows: int, c: int, ldx: int, weight, bias, eps: float, y_ss: torch.Tensor):
    if DISPATCH == "torch":
        return _tops().layernorm_ss(torch.as_strided(x, (rows, c), (ldx, 1)), weight, bias, eps, y_ss)
    _c("layernorm_ss", x.data_ptr(), rows, c, ldx, weight.data_ptr(), bias.data_ptr(), eps, y_ss.data_ptr())


def gemm_ss(a_ss: torch.Tensor, cw: ConvW, out: Optional[torch.Tensor] = None, *, out_ss: bool = False, act: int = ACT_NONE,
            gamma: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rows (split-swizzled) [M, K] @ W^T (+ bias, act, gamma, residual) -> fp32 rows, or split-swizzled rows (out_ss)"""
    M, K = a_ss.shape
    assert cw.prec == L.PREC_BF16X3 and cw.kh == 1 and cw.kw == 1 and cw.cin == K and K % 32 == 0, (cw.prec, cw.cin, K)
    if out is None:
        out = torch.empty((M, cw.cout), device=a_ss.device, dtype=torch.float32)

    def call():
        if DISPATCH == "torch":
            _tops().gemm_ss(a_ss, cw.w, cw.cout, cw.bias, gamma, res, act, out_ss, out)
        else:
            _c("gemm_ss", a_ss.data_ptr(), M, K, cw.w.data_ptr(), cw.cout, _ptr(cw.bias), _ptr(gamma), _ptr(res), res.stride(0) if res is not None else 0, act,
               None if out_ss else out.data_ptr(), out.stride(0), out.data_ptr() if out_ss else None)

    PROFILER.launch(_last_kernel, 2.0 * M * K * cw.cout, call, shape=f"{K}->{cw.cout} k1s1 1x{M}x1")
    return out


QKV_SS = os.environ.get("PRV2_QKV_SS", "1") != "0"  # A/B and test switch: the attention block without the qkv_split pre-pass
Q_SCALE = float(np.float32(0.125) * np.float32(1.4426950408889634))  # hd^-0.5 log2 e at head_dim 64: the float32 product qkv_split_kernel multiplies with


def gemm_ss_qkv(a_ss: torch.Tensor, cw: ConvW, heads: int) -> torch.Tensor:
    """the qkv Linear of an attention block on split-swizzled rows -> split-swizzled [q * hd^-0.5 log2 e | k | v] rows, the operand of
    ``attention_qkv_ss`` (include/prv2.h::prv2_gemm_ss_qkv)"""
    M, K = a_ss.shape
    assert cw.prec == L.PREC_BF16X3 and cw.kh == 1 and cw.kw == 1 and cw.cin == K and K % 32 == 0 and cw.cout == 3 * heads * 64, (cw.prec, cw.cin, K, cw.cout)
    res = []

    def call():
        if DISPATCH == "torch":
            res.append(_tops().gemm_ss_qkv(a_ss, cw.w, cw.cout, cw.bias, heads * 64, Q_SCALE))
            return
        out = torch.empty((M, cw.cout), device=a_ss.device, dtype=torch.float32)
        _c("gemm_ss_qkv", a_ss.data_ptr(), M, K, cw.w.data_ptr(), cw.cout, _ptr(cw.bias), heads * 64, Q_SCALE, out.data_ptr())
        res.append(out)

    PROFILER.launch(_last_kernel, 2.0 * M * K * cw.cout, call, shape=f"{K}->{cw.cout} k1s1 1x{M}x1")
    return res[0]


def attention_qkv_ss(qkv_ss: torch.Tensor, b: int, ntok: int, heads: int, bias=None, out_ss: bool = True) -> torch.Tensor:
    """softmax(q k^T + bias) v on ``gemm_ss_qkv``'s rows (bf16x3); bit-equal to ``attention`` on the fp32 rows of the same Linear"""
    image = isinstance(bias, AttnBiasImage)
    if image:
        assert (bias.heads, bias.ntok) == (heads, ntok)
        bias_t, ld_bias = bias.image, -1
    elif bias is not None:
        _require_dev(bias)
        assert bias.is_contiguous() and bias.shape[0] == heads and bias.shape[1] == ntok
        bias_t, ld_bias = bias, bias.shape[2]
    else:
        bias_t, ld_bias = None, 0
    res = []

    def call():
        if DISPATCH == "torch":
            res.append(_tops().attention_qkv_ss(qkv_ss, b, ntok, heads, bias_t, image, out_ss))
            return
        out = torch.empty((b * ntok, heads * 64), device=qkv_ss.device, dtype=torch.float32)
        _c("attention_qkv_ss", qkv_ss.data_ptr(), b, ntok, heads, 64, _ptr(bias_t), ld_bias, None if out_ss else out.data_ptr(), out.data_ptr() if out_ss else None)
        res.append(out)

    PROFILER.launch("attention_qkvss_kernel", 4.0 * b * heads * ntok * ntok * 64, call)
    return res[0]


def patchify(img: Feat, p: int, ldo: int) -> torch.Tensor:
    gh, gw = img.h // p, img.w // p
    if DISPATCH == "torch":
        return _tops().patchify(img.view(), p, ldo)
    rows = torch.empty((img.n * gh * gw, ldo), device=img.device, dtype=torch.float32)
    _c("patchify", img.ptr, img.n, gh, gw, p, img.ld, rows.data_ptr(), ldo)
    return rows


def assemble_tokens(emb: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, b: int, np_: int, dim: int) -> torch.Tensor:
    if DISPATCH == "torch":
        return _tops().assemble_tokens(emb, cls, pos, b, np_, dim)
    tok = torch.empty((b, np_ + 1, dim), device=emb.device, dtype=torch.float32)
    _c("assemble_tokens", emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), b, np_, dim, tok.data_ptr())
    return tok


class AttnBiasImage:
    """a [heads, ntok, ld] score bias re-ordered once for the bf16x3 attention kernel (include/prv2.h::prv2_pack_attention_bias)"""

    def __init__(self, image: torch.Tensor, heads: int, ntok: int):
        self.image, self.heads, self.ntok = image, heads, ntok


ATT_BIAS_IMAGE = os.environ.get("PRV2_ATT_BIAS_IMAGE", "1") != "0"  # A/B and test switch


def pack_attention_bias(bias: torch.Tensor, ntok: int):
    """bias rows [heads, ntok, ld] -> AttnBiasImage (bf16 modes; same values, the kernel's per-tile log2 e product pre-formed)"""
    _require_dev(bias)
    assert bias.is_contiguous() and bias.dim() == 3 and bias.shape[1] == ntok
    heads = bias.shape[0]
    if DISPATCH == "torch":
        return AttnBiasImage(_tops().pack_attention_bias(bias, ntok), heads, ntok)
    lib = L.load()
    img = torch.empty(lib.prv2_attention_bias_image_bytes(heads, ntok) // 4, device=bias.device, dtype=torch.float32)
    _c("pack_attention_bias", bias.data_ptr(), heads, ntok, bias.shape[2], img.data_ptr())
    return AttnBiasImage(img, heads, ntok)


def attention(qkv: torch.Tensor, b: int, ntok: int, heads: int, prec: int = PREC_F32, bias=None,
              out_ss: bool = False) -> torch.Tensor:
    """``bias``: optional [heads, ntok, ld >= roundup(ntok, 64)] additive score bias shared by the batch (BEiT), or its
    ``AttnBiasImage`` (bf16 modes); ``out_ss``: write the output split-swizzled (the operand format of gemm_ss; bf16x3 only)"""
    out = torch.empty((b * ntok, heads * 64), device=qkv.device, dtype=torch.float32)
    lib = L.load()
    nbytes = lib.prv2_attention_workspace_bytes(b, ntok, heads, prec)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device) if nbytes else None
    image = isinstance(bias, AttnBiasImage)
    if image:
        assert prec != PREC_F32 and (bias.heads, bias.ntok) == (heads, ntok)
        bias_t, ld_bias = bias.image, -1
    elif bias is not None:
        _require_dev(bias)
        assert bias.is_contiguous() and bias.shape[0] == heads and bias.shape[1] == ntok
        bias_t, ld_bias = bias, bias.shape[2]
    else:
        bias_t, ld_bias = None, 0
    res = []  # (the torch ops allocate their own output)

    def call():
        if DISPATCH == "torch":
            res.append(_tops().attention_ss(qkv, b, ntok, heads, bias_t, image) if out_ss else _tops().attention_fwd(qkv, b, ntok, heads, prec, bias_t, image))
        elif out_ss:
            assert prec == L.PREC_BF16X3
            _c("attention_ss", qkv.data_ptr(), b, ntok, heads, 64, _ptr(bias_t), ld_bias, out.data_ptr(), _ptr(ws), nbytes)
        else:
            _c("attention_bias", qkv.data_ptr(), b, ntok, heads, 64, _ptr(bias_t), ld_bias, out.data_ptr(), prec, _ptr(ws), nbytes, what="attention")

    PROFILER.launch("attention_f32_kernel" if prec == PREC_F32 else "attention_bf16x3_kernel", 4.0 * b * heads * ntok * ntok * 64, call)
    return res[0] if res else out


def crop_resize(img_chw: torch.Tensor, tiles: torch.Tensor, ch: int, cw: int, oh: int, ow: int,
                mean: Optional[Sequence[float]], std: Optional[Sequence[float]], out: Feat):
    """img_chw [3,H,W] device; tiles int32 [k,2] device; writes channels 0..2 of ``out`` [k,oh,ow,*].
    B frames: img [B,3,H,W] and tiles int32 [k,3] = (frame, h, w) (prv2_crop_resize_frames)."""
    _require_dev(img_chw)
    assert tiles.dtype == torch.int32 and tiles.is_cuda and img_chw.is_contiguous()
    k = tiles.shape[0]
    frames = img_chw.dim() == 4
    if frames:
        assert tiles.shape[1] == 3, "crop_resize of B frames takes tiles (frame, h, w)"
    if DISPATCH == "torch":
        m, s = (list(v) if v is not None else None for v in (mean, std))
        (_tops().crop_resize_frames if frames else _tops().crop_resize_bilinear)(img_chw, tiles.contiguous(), ch, cw, oh, ow, m, s, out.slice(0, 3).view())
        return
    m, s = ((C.c_float * 3)(*v) if v is not None else None for v in (mean, std))
    _c("crop_resize_frames" if frames else "crop_resize", img_chw.data_ptr(), *img_chw.shape[:-3], img_chw.shape[-2], img_chw.shape[-1], tiles.data_ptr(), k,
       ch, cw, oh, ow, m, s, out.ptr, out.ld)


def bicubic_resize(img_hwc: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """[h, w, 3] uint8 (-> /255) or fp32 RGB image on the device -> [3, oh, ow] fp32 (bicubic, align_corners=True);
    general_dataset.py:55-60."""
    if not img_hwc.is_cuda or img_hwc.dtype not in (torch.uint8, torch.float32):
        raise ValueError("bicubic_resize needs a uint8 or float32 image on the GPU (no CPU fallback exists)")
    assert img_hwc.dim() == 3 and img_hwc.shape[2] == 3
    img_hwc = img_hwc.contiguous()
    if DISPATCH == "torch":
        return _tops().bicubic_resize(img_hwc, oh, ow)
    out = torch.empty((3, oh, ow), device=img_hwc.device, dtype=torch.float32)
    _c("bicubic_resize", img_hwc.data_ptr(), int(img_hwc.dtype == torch.uint8), img_hwc.shape[0], img_hwc.shape[1], out.data_ptr(), oh, ow)
    return out


def roi_align(feat: Feat, boxes: torch.Tensor, spatial_scale: float, oh: int, ow: int, out: Optional[Feat] = None) -> Feat:
    """boxes [k, 4] = (x1, y1, x2, y2) on ONE map (feat.n == 1), or [k, 5] = (frame, x1, y1, x2, y2) on B maps (torchvision's
    format; prv2_roi_align_frames)"""
    frames = boxes.shape[1] == 5
    assert (feat.n == 1 or frames) and boxes.dtype == torch.float32 and boxes.is_cuda and boxes.shape[1] in (4, 5)
    k = boxes.shape[0]
    if out is None:
        out = Feat.alloc(k, oh, ow, feat.c, feat.device)
    nf = (feat.n,) if frames else ()  # (the B-frame entry points take the frame count first; one map: feat.n == 1)
    what = "roi_align_frames" if frames else "roi_align"

    def call():
        if DISPATCH == "torch":
            (_tops().roi_align_frames if frames else _tops().roi_align)(feat.view(), boxes.contiguous(), float(spatial_scale), oh, ow, out.raw(), out.x2)
        else:  # (x2: the pre-split format of the gate kernel's input)
            _c(what.replace("align", "align_x2") if out.x2 else what, feat.ptr, *nf, feat.h, feat.w, feat.c, feat.ld, boxes.data_ptr(), k, spatial_scale, oh, ow,
               out.ptr, out.ld, what=what)

    PROFILER.launch_aux("roi_align", 4.0 * feat.c * (feat.n * feat.h * feat.w + k * oh * ow), call,
                        f"{feat.c}ch {f'{feat.n}x' if frames else ''}{feat.h}x{feat.w}->{k}x{oh}x{ow}{' x2' if out.x2 else ''}")
    return out


def upsample_bilinear(x: Feat, oh: int, ow: int, out: Optional[Feat] = None) -> Feat:
    if out is None:
        out = Feat.alloc(x.n, oh, ow, x.c, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, oh, ow, x.c)

    def call():
        if DISPATCH == "torch":
            _tops().upsample_bilinear_ac(x.view(), oh, ow, out.view())
        else:
            _c("upsample_bilinear", x.ptr, x.n, x.h, x.w, x.c, x.ld, oh, ow, out.ptr, out.ld)

    PROFILER.launch_aux("upsample_bilinear", 4.0 * x.n * x.c * (x.h * x.w + oh * ow), call, f"{x.c}ch {x.n}x{x.h}x{x.w}->{oh}x{ow}")
    return out


def conv2d_pre_supported(h: int, w: int, cw: ConvW, ln: bool) -> bool:
    """can ``conv2d_pre`` add a pre-epilogue addend to this 3x3 conv on h x w images (a property of the layer)?"""
    if ln and cw.cout > 128 and cw.cout != 256:
        return False
    x = SimpleNamespace(n=1, h=h, w=w, ld=roundup(cw.cin, 4))  # (one dense image of the layer's input)
    return bool(L.load().prv2_conv2d_pre_supported(C.byref(_conv_desc(x, cw, roundup(cw.cout, 4)))))


def conv2d_pre(x: Feat, cw: ConvW, pre: Feat, out: Optional[Feat] = None, *, act: int = ACT_NONE, res: Optional[Feat] = None, ln=None,
               ln_eps: float = 1e-6, pre_cin: int = 0) -> Feat:
    """y = act([LN](conv3x3(x) + pre + bias)) (+ res) (include/prv2.h::prv2_conv2d_pre): ``pre`` [n, h, w, cout] is the coarse half of the
    reference's conv over cat([coarse_roi, x]) from ``CoarseTaps.gather``, standing for ``pre_cin`` further input channels"""
    assert x.c == cw.cin and (pre.n, pre.h, pre.w, pre.c) == (x.n, x.h, x.w, cw.cout) and not pre.x2
    if out is None:
        out = Feat.alloc(x.n, x.h, x.w, cw.cout, x.device)
    assert (out.n, out.h, out.w, out.c) == (x.n, x.h, x.w, cw.cout) and not out.x2
    d = _conv_desc(x, cw, out.ld, act=act, ld_res=_ld(res), ln_eps=ln_eps)
    lnw, lnb = (ln[0], ln[1]) if ln is not None else (None, None)
    flops = 2.0 * x.n * x.h * x.w * cw.cout * cw.cin * 9

    def call():
        if DISPATCH == "torch":
            _tops().conv3x3_pre(x.view(), cw.w, cw.bias, pre.view(), cw.cout, act, lnw, lnb, res.view() if res is not None else None, cw.prec, ln_eps, out.view())
        else:
            _c("conv2d_pre", C.byref(d), x.ptr, cw.w.data_ptr(), _ptr(cw.bias), pre.ptr, pre.ld, _ptr(lnw), _ptr(lnb), _ptr(res), out.ptr)

    PROFILER.launch(_last_kernel, flops, call,
                    shape=f"{cw.cin}(+{pre_cin} coarse)->{cw.cout} k3s1 {x.n}x{x.h}x{x.w}", algo=flops + 2.0 * x.n * x.h * x.w * cw.cout * pre_cin * 9)
    return out


CHAIN32 = os.environ.get("PRV2_CHAIN32", "1") != "0"  # A/B and test switch: the fused 32-channel full-resolution chains (csrc/chain32.hip)


def pack_chain32(weight: torch.Tensor, kind: int, device=None) -> torch.Tensor:
    """fragment image of a 32-output-channel conv for the ``chain32_*`` kernels (include/prv2.h::prv2_pack_chain32_weight): kind 0 = first
    conv of a chain (3x3, natural K), 1 = second conv / 1x1 (K in accumulator order), 2 = the [p1 | p2] tail of a 3x3 over 34 channels"""
    w = weight.detach().to(device=device or weight.device, dtype=torch.float32).contiguous()
    assert w.shape[0] == 32 and w.dim() in (2, 4)
    taps = w.shape[2] * w.shape[3] if w.dim() == 4 else 1
    if DISPATCH == "torch":
        return _tops().pack_chain32_weight(w, kind)
    lib = L.load()
    packed = torch.empty(lib.prv2_chain32_weight_bytes(kind, taps) // 4, device=w.device, dtype=torch.float32)
    _c("pack_chain32_weight", w.data_ptr(), w.shape[1], taps, kind, packed.data_ptr())
    return packed


def chain32_consts(device, **rows) -> torch.Tensor:
    """the [9][32] constant table of the ``chain32_*`` kernels: b1, ln1w, ln1b, b2, bg, bo, w3, ln2w, ln2b (missing rows zero)"""
    names = ("b1", "ln1w", "ln1b", "b2", "bg", "bo", "w3", "ln2w", "ln2b")
    assert set(rows) <= set(names)
    t = torch.zeros((9, 32), dtype=torch.float32, device=device)
    for i, n in enumerate(names):
        if rows.get(n) is not None:
            t[i] = rows[n].detach().to(device=device, dtype=torch.float32).reshape(32)
    return t


def _chain32_desc(x: Feat, w1, w2, wg, wo, consts, pre, p1, p2, y: Feat, depth, b3, ln_eps):
    assert x.c == 32 and y.c == 32 and (x.n, x.h, x.w) == (y.n, y.h, y.w) and not x.x2 and not y.x2
    assert pre is None or ((pre.n, pre.h, pre.w, pre.c) == (x.n, x.h, x.w, 32) and not pre.x2)
    return L.Chain32Desc(x=x.ptr, w1=w1.data_ptr(), w2=w2.data_ptr(), wg=wg.data_ptr(), wo=_ptr(wo), consts=consts.data_ptr(), pre=_ptr(pre),
                         p1=_ptr(p1), p2=_ptr(p2), y=y.ptr, depth=_ptr(depth), x_bstride=0, y_bstride=0, n=x.n, h=x.h, w=x.w, ldx=x.ld, ldy=y.ld,
                         ld_pre=pre.ld if pre is not None else 0, b3=b3, ln_eps=ln_eps)


def chain32_c2f(x: Feat, cw: dict, pre: Optional[Feat], out: Optional[Feat] = None, depth: Optional[torch.Tensor] = None, ln_eps: float = 1e-6,
                pre_cin: int = 0):
    """C2FModule's full-resolution tail in one kernel (include/prv2.h::prv2_chain32_c2f): GateresConfUnit2 of ``output_conv2_fusion`` (conv +
    skip, fusion_conv with the coarse half ``pre``, gate), ``out_conv`` and ``output_conv3``.  cw: dict(w1, w2, wg, wo, consts, b3) of
    ``pack_chain32`` / ``chain32_consts`` images.  Returns (last feature [n, h, w, 32], depth [n, 1, h, w])."""
    if out is None:
        out = Feat(torch.empty((x.n, x.h, x.w, 32), device=x.device, dtype=torch.float32))
    if depth is None:
        depth = torch.empty((x.n, 1, x.h, x.w), device=x.device, dtype=torch.float32)
    assert depth.is_contiguous() and depth.numel() == x.n * x.h * x.w

    def call():
        if DISPATCH == "torch":
            _tops().chain32_c2f(x.view(), cw["w1"], cw["w2"], cw["wg"], cw["wo"], cw["consts"], cw["b3"], pre.view() if pre is not None else None, ln_eps,
                                out.view(), depth)
        else:
            _c("chain32_c2f", C.byref(_chain32_desc(x, cw["w1"], cw["w2"], cw["wg"], cw["wo"], cw["consts"], pre, None, None, out, depth, cw["b3"], ln_eps)))

    px = float(x.n * x.h * x.w)
    flops = 2.0 * px * (2 * 9 * 32 * 32 + 2 * 32 * 32 + 32)
    PROFILER.launch(_last_kernel, flops, call, shape=f"32->32->32(+{pre_cin} coarse)->gate->32->1 k3s1 {x.n}x{x.h}x{x.w}",
                    algo=flops + 2.0 * px * 9 * 32 * pre_cin)
    return out, depth


def chain32_enc(x: Feat, cw: dict, pre: Feat, p1: torch.Tensor, p2: torch.Tensor, out: Optional[Feat] = None, ln_eps: float = 1e-6, pre_cin: int = 0) -> Feat:
    """``fusion_layers_1[0]`` + ``fusion_layers_2[0]`` in one kernel (include/prv2.h::prv2_chain32_enc).  cw: dict(w1, w2, wt, consts);
    p1 / p2: dense depth maps at x's size."""
    if out is None:
        out = Feat(torch.empty((x.n, x.h, x.w, 32), device=x.device, dtype=torch.float32))
    _require_dev(p1, p2)
    assert p1.is_contiguous() and p2.is_contiguous() and p1.numel() == p2.numel() == x.n * x.h * x.w

    def call():
        if DISPATCH == "torch":
            _tops().chain32_enc(x.view(), cw["w1"], cw["w2"], cw["wt"], cw["consts"], pre.view(), p1, p2, ln_eps, out.view())
        else:
            _c("chain32_enc", C.byref(_chain32_desc(x, cw["w1"], cw["w2"], cw["wt"], None, cw["consts"], pre, p1, p2, out, None, 0.0, ln_eps)))

    px = float(x.n * x.h * x.w)
    flops = 2.0 * px * (9 * 32 * 32 + 9 * 34 * 32)
    PROFILER.launch(_last_kernel, flops, call, shape=f"32(+{pre_cin} coarse)->32->34->32 k3s1 {x.n}x{x.h}x{x.w}",
                    algo=flops + 2.0 * px * 9 * 32 * pre_cin)
    return out


COARSE_TAPS = os.environ.get("PRV2_COARSE_TAPS", "1") != "0"  # A/B and test switch: coarse half of the cat([fine, coarse_roi]) convs once per frame


class CoarseTaps:
    """The coarse half of one ``cat([fine, coarse_roi])`` 3x3 conv, tabulated once per frame (include/prv2.h::prv2_coarse_tap_knots):
    ``g`` [1, H, W, 9 * cout] = the level's map through the conv's coarse weights, tap-major (a 1x1 GEMM at coarse resolution),
    ``v`` [1, 3H, 3W, cout] = the unmasked tap sum on the knot grid, ``kb`` = (tile height / frame height, tile width / frame width).
    B frames: ``g`` [B, H, W, 9 * cout] -> ``v`` [B, 3H, 3W, cout] in one launch, and ``gather`` takes boxes (frame, x1, y1, x2, y2)."""

    def __init__(self, g: Feat, cout: int, kb):
        assert g.c == 9 * cout and 0 < kb[0] <= 0.5 and 0 < kb[1] <= 0.5
        self.g, self.cout, self.kb = g, cout, (float(kb[0]), float(kb[1]))
        self.nf = (g.n,) if g.n > 1 else ()  # (B frames: the entry points take the frame count first)
        box = []  # the table: the tensor the torch op allocates, or the one allocated here
        if DISPATCH == "torch":
            op = _tops().coarse_tap_knots_frames if self.nf else _tops().coarse_tap_knots
            call = lambda: box.append(op(g.view(), cout, *self.kb))  # noqa: E731
        else:
            v = torch.empty((g.n, 3 * g.h, 3 * g.w, cout), device=g.device, dtype=torch.float32)
            box.append(v)
            call = lambda: _c("coarse_tap_knots_frames" if self.nf else "coarse_tap_knots", g.ptr, *self.nf, g.h, g.w, cout, g.ld, *self.kb,  # noqa: E731
                              v.data_ptr(), cout)
        PROFILER.launch_aux("coarse_tap_knots", 4.0 * g.n * g.h * g.w * 18 * cout, call, f"{cout}ch {f'{g.n}x' if self.nf else ''}{g.h}x{g.w}")
        self.v = Feat(box[0])

    def gather(self, boxes: torch.Tensor, spatial_scale: float, oh: int, ow: int, out: Optional[Feat] = None) -> Feat:
        """the conv's coarse half for the tiles ``boxes`` (as roi_align takes them): [k, oh, ow, cout], zero padding at the tile border
        included (prv2_coarse_tap_gather).  Tables of B frames: boxes (frame, x1, y1, x2, y2) (prv2_coarse_tap_gather_frames)."""
        assert boxes.dtype == torch.float32 and boxes.is_cuda and boxes.shape[1] == (5 if self.nf else 4)
        k = boxes.shape[0]
        # The knot-grid algebra holds when consecutive output pixels are exactly ``kb`` coarse pixels apart (ROI bin == knot spacing): every
        # box must span kb * (g.h, g.w) * (oh, ow) / spatial_scale frame pixels.  The boxes live on the device (no host sync on the frame
        # path): PRV2_CHECK_TAPS=1 verifies them here; the library checks what it can see (knot spacing in (0, 1/2]), fusion.py compares the
        # ROI's output size with its consumer's map before taking this path.
        if os.environ.get("PRV2_CHECK_TAPS"):
            b = boxes.detach().cpu()[:, -4:]
            bin_w = (b[:, 2] - b[:, 0]) * spatial_scale / ow
            bin_h = (b[:, 3] - b[:, 1]) * spatial_scale / oh
            assert float((bin_h - self.kb[0]).abs().max()) < 1e-4 and float((bin_w - self.kb[1]).abs().max()) < 1e-4, \
                ("CoarseTaps.gather: ROI bin size differs from the knot spacing the table was built for", float(bin_h[0]), float(bin_w[0]), self.kb)
        if out is None:
            out = Feat(torch.empty((k, oh, ow, self.cout), device=self.g.device, dtype=torch.float32))
        assert (out.n, out.h, out.w, out.c) == (k, oh, ow, self.cout) and not out.x2
        g, v, nf = self.g, self.v, self.nf

        def call():
            if DISPATCH == "torch":
                (_tops().coarse_tap_gather_frames if nf else _tops().coarse_tap_gather)(v.view(), g.view(), *self.kb, boxes.contiguous(), float(spatial_scale),
                                                                                        oh, ow, out.view())
            else:
                _c("coarse_tap_gather_frames" if nf else "coarse_tap_gather", v.ptr, g.ptr, *nf, g.h, g.w, self.cout, v.ld, g.ld, *self.kb, boxes.data_ptr(), k,
                   spatial_scale, oh, ow, out.ptr, out.ld)

        PROFILER.launch_aux("coarse_tap_gather", 4.0 * self.cout * (9 * g.n * g.h * g.w + k * oh * ow), call,
                            f"{self.cout}ch {f'{g.n}x' if nf else ''}{g.h}x{g.w}->{k}x{oh}x{ow}")
        return out


def coarse_tap_weight(w_coarse: torch.Tensor) -> torch.Tensor:
    """[cout, cin, 3, 3] coarse-half weights of a conv -> the 1x1 GEMM weights [9 * cout, cin] whose output is tap-major
    (row tap * cout + co = w[co, :, ky, kx]): G of ``CoarseTaps``"""
    co, ci = w_coarse.shape[:2]
    return w_coarse.permute(2, 3, 0, 1).reshape(9 * co, ci).contiguous()


DIRECT_PLACEMENT = os.environ.get("PRV2_DIRECT_PLACEMENT", "1") != "0"  # A/B and test switch: ROI levels / depth pairs written by their producers


class RoiSource:
    """A level of the coarse pyramid as seen by one batch of tiles: ``roi_align(feat.repeat(K), boxes, (h, w), scale)`` that has
    not been materialised.  Its consumers are concat buffers (the [coarse | fine] inputs of the fusion convs): ``write(dst)``
    gathers straight into a destination slice -- reading the small, L2-resident coarse map again is cheaper than writing the
    K-tile ROI once and copying it into each consumer (1 + 2 x (read + write) of K x c x h x w floats -> 2 writes)."""

    def __init__(self, feat: Feat, boxes: torch.Tensor, spatial_scale: float, oh: int, ow: int):
        self.feat, self.boxes, self.scale = feat, boxes, spatial_scale
        self.n, self.h, self.w, self.c = boxes.shape[0], oh, ow, feat.c
        self._mat: Optional[Feat] = None

    @property
    def device(self):
        return self.feat.device

    def write(self, dst: Feat):
        assert (dst.n, dst.h, dst.w, dst.c) == (self.n, self.h, self.w, self.c)
        if not DIRECT_PLACEMENT:
            return upsample_bilinear(self.materialize(), dst.h, dst.w, out=dst)
        roi_align(self.feat, self.boxes, self.scale, self.h, self.w, out=dst)

    def materialize(self) -> Feat:
        if self._mat is None:
            self._mat = roi_align(self.feat, self.boxes, self.scale, self.h, self.w)
        return self._mat


def conv_border_bias(y: Feat, tap_bias: torch.Tensor):
    """y -= the folded bias of the 3x3 taps that the zero padding hides at the image border (include/prv2.h::prv2_conv_border_bias)"""
    assert tap_bias.shape == (9, y.c) and tap_bias.is_contiguous()

    def call():
        if DISPATCH == "torch":
            _tops().conv_border_bias_(y.view(), tap_bias)
        else:
            _c("conv_border_bias", y.ptr, y.n, y.h, y.w, y.c, y.ld, tap_bias.data_ptr())

    PROFILER.launch_aux("conv_border_bias", 8.0 * y.n * 2 * (y.h + y.w) * y.c, call, f"{y.c}ch {y.n}x{y.h}x{y.w}")


def depth_pair_fill(p1: Feat, p2: Feat, buf: Feat, c0: int):
    """channels c0, c0 + 1 of ``buf`` <- (p1, p2) resized to the buffer's size, channels c0 + 2, c0 + 3 (the pad) <- 0"""
    assert p1.c == 1 and p2.c == 1 and p1.ld == 1 and p2.ld == 1 and (p1.n, p1.h, p1.w) == (p2.n, p2.h, p2.w) == (buf.n, p1.h, p1.w)
    assert buf.ld == buf.c0 + c0 + 4 and (buf.c0 + c0) % 4 == 0, (buf.ld, buf.c0, c0)

    def call():
        if DISPATCH == "torch":
            _tops().depth_pair_fill(p1.buf.view(p1.n, p1.h, p1.w), p2.buf.view(p2.n, p2.h, p2.w), buf.buf[..., buf.c0 + c0:buf.c0 + c0 + 4])
        else:
            _c("depth_pair_fill", p1.ptr, p2.ptr, p1.n, p1.h, p1.w, buf.h, buf.w, buf.ptr + 4 * c0, buf.ld)

    PROFILER.launch_aux("depth_pair_fill", 16.0 * buf.n * buf.h * buf.w, call, f"{buf.n}x{p1.h}x{p1.w}->{buf.h}x{buf.w}")


def blend_paste(avg, cnt, pred, mask, tiles, th, tw):
    if DISPATCH == "torch":
        return _tops().blend_init(avg, cnt, pred.contiguous(), mask, tiles.contiguous(), th, tw)
    _c("blend_paste", avg.data_ptr(), cnt.data_ptr(), avg.shape[0], avg.shape[1], pred.data_ptr(), pred.shape[-2], pred.shape[-1], mask.data_ptr(),
       tiles.data_ptr(), tiles.shape[0], th, tw)


def blend_update(avg, cnt, pred, mask, tiles, th, tw):
    if DISPATCH == "torch":
        return _tops().blend_update(avg, cnt, pred.contiguous(), mask, tiles.contiguous(), th, tw)
    _c("blend_update", avg.data_ptr(), cnt.data_ptr(), avg.shape[0], avg.shape[1], pred.data_ptr(), pred.shape[-2], pred.shape[-1], mask.data_ptr(),
       tiles.data_ptr(), tiles.shape[0], th, tw)


def _blend_frames(step, maps, pred, mask, tiles, th, tw, kind="frames"):
    """one pass step (``step``: "paste" / "update") of the blend for B maps [B, H, W] -- ``maps`` = (avg, cnt), or (avg, cnt, m2, ntl) with
    the overlap statistics (``kind`` "stats": prv2_blend_*_stats): pred [B, k, ph, pw] and tiles int32 [B, k, 2] are frame f's slice of
    frame-major lists (any frame stride: ``preds.view(B, n, ph, pw)[:, o:o + k]``, no copies)"""
    B, k = pred.shape[0], pred.shape[1]
    assert maps[0].dim() == 3 and tiles.shape[:2] == (B, k) and pred.stride(1) == pred.shape[2] * pred.shape[3] and tiles.stride(1) == 2
    if DISPATCH == "torch":
        return getattr(_tops(), f"blend_{'init' if step == 'paste' else step}_{kind}")(*maps, pred, mask, tiles, th, tw)
    _c(f"blend_{step}_{kind}", *(t.data_ptr() for t in maps), B, maps[0].shape[1], maps[0].shape[2], pred.data_ptr(), pred.shape[-2], pred.shape[-1],
       pred.stride(0) if B > 1 else k * pred.shape[2] * pred.shape[3], mask.data_ptr(), tiles.data_ptr(), tiles.stride(0) // 2 if B > 1 else k, k, th, tw)


def blend_paste_frames(avg, cnt, pred, mask, tiles, th, tw):
    _blend_frames("paste", (avg, cnt), pred, mask, tiles, th, tw)


def blend_update_frames(avg, cnt, pred, mask, tiles, th, tw):
    _blend_frames("update", (avg, cnt), pred, mask, tiles, th, tw)


def blend_resize(avg, cnt, oh, ow):
    """[H, W] maps, or B maps [B, H, W] in one launch (prv2_blend_resize_frames)"""
    frames = avg.dim() == 3
    if DISPATCH == "torch":
        return (_tops().blend_resize_frames if frames else _tops().blend_resize)(avg, cnt, oh, ow)
    a, c = (torch.empty((*avg.shape[:-2], oh, ow), device=avg.device, dtype=torch.float32) for _ in range(2))
    _c("blend_resize_frames" if frames else "blend_resize", avg.data_ptr(), cnt.data_ptr(), *avg.shape, a.data_ptr(), c.data_ptr(), oh, ow)
    return a, c


def _as_frames(avg, pred, tiles):
    """B = 1 inputs of the statistics ops as a batch of one: maps [H, W] -> [1, H, W], pred [k, (1,) ph, pw] -> [1, k, ph, pw],
    tiles [k, 2] -> [1, k, 2] (views)"""
    if avg.dim() == 2:
        avg = avg[None]
        pred = pred.reshape(1, pred.shape[0], pred.shape[-2], pred.shape[-1])
        tiles = tiles[None]
    return avg, pred, tiles


def _blend_stats(step, avg, cnt, m2, ntl, pred, mask, tiles, th, tw):
    """one pass step of the blend with the overlap statistics m2 / ntl: maps [H, W] with pred [k, ph, pw] / tiles [k, 2], or B maps
    [B, H, W] with frame-major slices pred [B, k, ph, pw] / tiles [B, k, 2] as ``blend_paste_frames``"""
    a3, pred, tiles = _as_frames(avg, pred, tiles)
    _blend_frames(step, (a3, *(t.view(a3.shape) for t in (cnt, m2, ntl))), pred, mask, tiles, th, tw, "stats")


def blend_paste_stats(avg, cnt, m2, ntl, pred, mask, tiles, th, tw):
    """paste: avg = p, cnt = ct, m2 = 0, ntl = 1 under every tile"""
    _blend_stats("paste", avg, cnt, m2, ntl, pred, mask, tiles, th, tw)


def blend_update_stats(avg, cnt, m2, ntl, pred, mask, tiles, th, tw):
    """update: avg / cnt as ``blend_update``; ntl += 1 under every tile, m2 += ct (p - avg_old)(p - avg_new) where ct > 0"""
    _blend_stats("update", avg, cnt, m2, ntl, pred, mask, tiles, th, tw)


def blend_resize_stats(avg, cnt, m2, ntl, oh, ow):
    """``blend_resize`` of [H, W] or [B, H, W] maps plus ntl (nearest) and m2 (the nearest pixel's m2 / cnt times the resampled cnt)
    -> (avg, cnt, m2, ntl) at [(B,) oh, ow]"""
    one = avg.dim() == 2
    a3, c3, s3, n3 = (t[None] if one else t for t in (avg, cnt, m2, ntl))
    B = a3.shape[0]
    if DISPATCH == "torch":
        out = _tops().blend_resize_stats(a3, c3, s3, n3, oh, ow)
    else:
        out = tuple(torch.empty((B, oh, ow), device=avg.device, dtype=torch.float32) for _ in range(4))
        _c("blend_resize_stats", a3.data_ptr(), c3.data_ptr(), s3.data_ptr(), n3.data_ptr(), B, a3.shape[1], a3.shape[2], *(t.data_ptr() for t in out), oh, ow)
    return tuple(t[0] for t in out) if one else tuple(out)


def blend_uncertainty(cnt, m2):
    """the weighted standard deviation of the overlapping tile predictions: sqrt(max(m2, 0) / cnt) where cnt > 0, 0 elsewhere"""
    return (m2.clamp(min=0) / cnt).sqrt_().masked_fill_(cnt <= 0, 0.0)


def add(a: Feat, b: Feat, out: Optional[Feat] = None) -> Feat:
    assert (a.n, a.h, a.w, a.c) == (b.n, b.h, b.w, b.c)
    if out is None:
        out = Feat.alloc(a.n, a.h, a.w, a.c, a.device)
    if DISPATCH == "torch":
        _tops().add_nhwc(a.view(), b.view(), out.view())
        return out
    _c("add", a.ptr, a.ld, b.ptr, b.ld, a.n * a.h * a.w, a.c, out.ptr, out.ld)
    return out


def zoe_attractor(attr: Feat, bins: Feat, alpha: float = 300.0) -> Feat:
    assert (attr.n, attr.h, attr.w) == (bins.n, bins.h, bins.w)
    if DISPATCH == "torch":
        y = _tops().zoe_attractor(attr.view(), bins.view(), alpha)
        return _feat_of(y, bins.c)
    out = Feat.alloc(bins.n, bins.h, bins.w, bins.c, bins.device)
    _c("zoe_attractor", attr.ptr, attr.ld, attr.c, bins.ptr, bins.ld, bins.c, alpha, bins.n * bins.h * bins.w, out.ptr, out.ld)
    return out


def zoe_logbinom_depth(pt: Feat, centers: Feat, min_temp: float, max_temp: float) -> torch.Tensor:
    assert pt.c == 4 and (pt.n, pt.h, pt.w) == (centers.n, centers.h, centers.w)
    if DISPATCH == "torch":
        return _tops().zoe_bins_head(pt.view(), centers.view(), min_temp, max_temp)
    depth = torch.empty((pt.n, 1, pt.h, pt.w), device=pt.device, dtype=torch.float32)
    _c("zoe_logbinom_depth", pt.ptr, pt.ld, centers.ptr, centers.ld, centers.c, min_temp, max_temp, pt.n * pt.h * pt.w, depth.data_ptr())
    return depth


# ------------------------------------------------------------------------------------------------------------------
# Edge-aware evaluation (csrc/edges.hip): frames [B, H, W] on the device, both dispatch routes.  Masks are bool tensors.
# ------------------------------------------------------------------------------------------------------------------
EDGE_PRE = {None: L.EDGE_PRE_NONE, "none": L.EDGE_PRE_NONE, "log": L.EDGE_PRE_LOG, "inv": L.EDGE_PRE_INV}


def _edge_frames(x, dtype=None):
    """[H, W] or [B, H, W] -> contiguous [B, H, W] (of ``dtype`` when given)"""
    if x.dim() == 2:
        x = x[None]
    assert x.dim() == 3 and x.is_cuda, x.shape
    return (x if dtype is None else x.to(dtype)).contiguous()


def _edge_ws(x):
    n = L.load().prv2_edges_workspace_bytes(*x.shape)
    return torch.empty((n,), dtype=torch.uint8, device=x.device)


def depth_preprocess(depth, preprocess="log"):
    """extract_edges' preprocessing (metric.py:184-198) of fp32 frames [B, H, W] -> fp32 [B, H, W]"""
    if preprocess not in EDGE_PRE:
        raise ValueError(f"Invalid depth preprocessing. ({preprocess})")
    d = _edge_frames(depth, torch.float32)
    if DISPATCH == "torch":
        return _tops().depth_preprocess(d, EDGE_PRE[preprocess])
    out, ws = torch.empty_like(d), _edge_ws(d)
    _c("depth_preprocess", d.data_ptr(), *d.shape, EDGE_PRE[preprocess], out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def canny(image, sigma=1.0, low_threshold=0.1, high_threshold=0.2):
    """metrics.canny of fp32 frames [B, H, W] -> bool [B, H, W] (bit-identical to the host on the same input)"""
    from .metrics import gaussian_weights
    x, gw = _edge_frames(image, torch.float32), gaussian_weights(sigma)
    if DISPATCH == "torch":
        return _tops().canny(x, gw.tolist(), float(low_threshold), float(high_threshold))
    out, ws = torch.empty(x.shape, dtype=torch.bool, device=x.device), _edge_ws(x)
    _c("canny", x.data_ptr(), *x.shape, gw.ctypes.data, len(gw) - 1, low_threshold, high_threshold, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def edt_sq(mask):
    """exact squared distance to the nearest set pixel of each frame: bool [B, H, W] -> int32 [B, H, W] (INT32_MAX: empty frame)"""
    m = _edge_frames(mask, torch.bool)
    if DISPATCH == "torch":
        return _tops().edt_sq(m)
    out, ws = torch.empty(m.shape, dtype=torch.int32, device=m.device), _edge_ws(m)
    _c("edt_sq", m.data_ptr(), *m.shape, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def binary_dilate(mask, k):
    """k x k binary dilation (zero padding, k in 3 / 5 / 7) of bool [B, H, W]"""
    m = _edge_frames(mask, torch.bool)
    if DISPATCH == "torch":
        return _tops().binary_dilate(m, k)
    out = torch.empty_like(m)
    _c("binary_dilate", m.data_ptr(), *m.shape, k, out.data_ptr())
    return out


def boundary_stats(gt_edges, pred_edges, valid, d2_target, d2_pred, gt_ext, pred_ext, th_edges_acc=10.0):
    """the per-frame statistics of compute_boundary_metrics -> float64 [B, 8]: TP, FP, FN, TN, n_bde, n_gt, sum_acc, sum_comp
    (include/prv2.h prv2_boundary_stats)"""
    g, p, v, ge, pe = (_edge_frames(t, torch.bool) for t in (gt_edges, pred_edges, valid, gt_ext, pred_ext))
    dt, dp = _edge_frames(d2_target, torch.int32), _edge_frames(d2_pred, torch.int32)
    if DISPATCH == "torch":
        return _tops().boundary_stats(g, p, v, dt, dp, ge, pe, float(th_edges_acc))
    out, ws = torch.empty((g.shape[0], 8), dtype=torch.float64, device=g.device), _edge_ws(g)
    _c("boundary_stats", g.data_ptr(), p.data_ptr(), v.data_ptr(), dt.data_ptr(), dp.data_ptr(), ge.data_ptr(), pe.data_ptr(), *g.shape,
       float(th_edges_acc), out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


# ------------------------------------------------------------------------------------------------------------------
# Output stage (csrc/output.hip): frames [B, H, W] on the device, both dispatch routes.  Scanline buffers are uint8
# [B, prv2_rows_bytes(H, W, bpp)]: frame f's deflate-ready PNG image is rows[f, :H * (1 + bpp * W)].
# ------------------------------------------------------------------------------------------------------------------
def _rows(x, bpp):
    return torch.empty((x.shape[0], L.load().prv2_rows_bytes(x.shape[1], x.shape[2], bpp)), dtype=torch.uint8, device=x.device)


def _opt_frames(t, like, dtype):
    if t is None:
        return None
    t = _edge_frames(t, dtype)
    if t.shape != like.shape:
        raise ValueError(f"shape {tuple(t.shape)} does not match the frames {tuple(like.shape)}")
    return t


def order_stats(value, ranks, mask=None, invalid_val=-99.0, gate=None, gate_thr=0.0):
    """exact order statistics of the valid pixels of fp32 frames [B, H, W] -> (counts int64 [B], values fp32 [B, len(ranks)]), both
    on the device.  valid: ``mask`` (bool) when given, value != invalid_val otherwise; with ``gate`` also not (gate < gate_thr).
    ranks: k >= 0 the k-th smallest, k < 0 counted from the largest, clamped into the frame's valid count (include/prv2.h
    prv2_order_stats)"""
    v = _edge_frames(value, torch.float32)
    m, g = _opt_frames(mask, v, torch.bool), _opt_frames(gate, v, torch.float32)
    ranks = [int(r) for r in ranks]
    if DISPATCH == "torch":
        return _tops().order_stats(v, m, float(invalid_val), g, float(gate_thr), ranks)
    lib = L.load()
    ws = torch.empty((lib.prv2_output_workspace_bytes(v.shape[0]),), dtype=torch.uint8, device=v.device)
    counts = torch.empty((v.shape[0],), dtype=torch.int64, device=v.device)
    out = torch.empty((v.shape[0], len(ranks)), dtype=torch.float32, device=v.device)
    rk = np.asarray(ranks, dtype=np.int64)
    _c("order_stats", v.data_ptr(), _ptr(m), float(invalid_val), _ptr(g), float(gate_thr), *v.shape, rk.ctypes.data, len(ranks), counts.data_ptr(),
       out.data_ptr(), ws.data_ptr(), ws.numel())
    return counts, out


def colorize_rows(value, norm, lut, invalid_mask=None, invalid_val=-99.0, background_rgb=(128, 128, 128)):
    """metrics.colorize of fp32 frames [B, H, W] between norm[f] = (vmin, vmax) (device fp32 [B, 2]) through the colour table
    ``lut`` (device uint8 [N + 3, 4]) -> RGB scanline buffer"""
    v = _edge_frames(value, torch.float32)
    m = _opt_frames(invalid_mask, v, torch.bool)
    bg = int(background_rgb[0]) | int(background_rgb[1]) << 8 | int(background_rgb[2]) << 16
    norm = norm.to(torch.float32).contiguous()
    if DISPATCH == "torch":
        return _tops().colorize_rows(v, m, float(invalid_val), norm, lut, bg)
    if tuple(norm.shape) != (v.shape[0], 2) or lut.dtype != torch.uint8 or lut.dim() != 2 or lut.shape[1] != 4 or not lut.is_contiguous():
        raise ValueError("colorize_rows: norm is fp32 [B, 2], lut uint8 [N + 3, 4]")
    rows = _rows(v, 3)
    _c("colorize_rows", v.data_ptr(), _ptr(m), float(invalid_val), *v.shape, norm.data_ptr(), lut.data_ptr(), lut.shape[0] - 3, bg, rows.data_ptr(), rows.shape[1])
    return rows


def quantize16_rows(value, scale=256.0):
    """(value * scale).astype(uint16) of fp32 frames [B, H, W] as big-endian 16-bit scanlines (saturating; NaN -> 0)"""
    v = _edge_frames(value, torch.float32)
    if DISPATCH == "torch":
        return _tops().quantize16_rows(v, float(scale))
    rows = _rows(v, 2)
    _c("quantize16_rows", v.data_ptr(), *v.shape, float(scale), rows.data_ptr(), rows.shape[1])
    return rows


def pl_uncertainty_rows(uncertainty, count_map, params, lut):
    """tester.pseudo_label_uncertainty on the device -> (16-bit scanlines of floor(u * 256), RGB scanlines of u through ``lut``);
    params: device float64 [B, 5] = lo, hi, thr, umin, umax (include/prv2.h prv2_pl_uncertainty_rows)"""
    u = _edge_frames(uncertainty, torch.float32)
    c = _opt_frames(count_map, u, torch.float32)
    if DISPATCH == "torch":
        return _tops().pl_uncertainty_rows(u, c, params, lut)
    if tuple(params.shape) != (u.shape[0], 5) or params.dtype != torch.float64 or not params.is_contiguous():
        raise ValueError("pl_uncertainty_rows: params is float64 [B, 5]")
    r16, rgb = _rows(u, 2), _rows(u, 3)
    _c("pl_uncertainty_rows", u.data_ptr(), c.data_ptr(), *u.shape, params.data_ptr(), lut.data_ptr(), lut.shape[0] - 3, r16.data_ptr(), r16.shape[1],
       rgb.data_ptr(), rgb.shape[1])
    return r16, rgb


def mask_rows(mask):
    """bool frames [B, H, W] as 0 / 255 gray scanlines"""
    m = _edge_frames(mask, torch.bool)
    if DISPATCH == "torch":
        return _tops().mask_rows(m)
    rows = _rows(m, 1)
    _c("mask_rows", m.data_ptr(), *m.shape, rows.data_ptr(), rows.shape[1])
    return rows


def upsample_bilinear_map(x, oh, ow):
    """F.interpolate(mode='bilinear', align_corners=False) of fp32 maps [B, h, w] -> [B, oh, ow]"""
    x = _edge_frames(x, torch.float32)
    if DISPATCH == "torch":
        return _tops().upsample_bilinear_map(x, int(oh), int(ow))
    y = torch.empty((x.shape[0], int(oh), int(ow)), dtype=torch.float32, device=x.device)
    _c("upsample_bilinear_map", x.data_ptr(), *x.shape, y.data_ptr(), int(oh), int(ow))
    return y


def deflate_rows(rows, length):
    """zlib streams of byte frames that are on the device: ``rows`` uint8 [B, stride] (a scanline buffer: stride a multiple of
    16), ``length`` <= stride valid bytes per frame -> (out uint8 [B, prv2_deflate_bound(length)], out_bytes int64 [B]), both on
    the device: frame f's stream is out[f, :out_bytes[f]].  zlib.decompress restores rows[f, :length]; the stream is not zlib's
    own (include/prv2.h prv2_deflate_rows) and is the same on every call."""
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("deflate_rows: rows is a contiguous GPU uint8 [B, stride] tensor")
    length = int(length)
    if DISPATCH == "torch":
        return _tops().deflate_rows(rows, length)
    lib = L.load()
    bound, wsb = lib.prv2_deflate_bound(length), lib.prv2_deflate_workspace_bytes(rows.shape[0], length)
    if bound < 0 or wsb < 0:
        raise ValueError(f"deflate_rows: bad length {length} or frame count {rows.shape[0]}")
    out = torch.empty((rows.shape[0], bound), dtype=torch.uint8, device=rows.device)
    out_bytes = torch.empty((rows.shape[0],), dtype=torch.int64, device=rows.device)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=rows.device)
    _c("deflate_rows", rows.data_ptr(), rows.shape[0], length, rows.shape[1], out.data_ptr(), bound, out_bytes.data_ptr(), ws.data_ptr(), wsb)
    return out, out_bytes


# ------------------------------------------------------------------------------------------------------------------
# Geometry export (csrc/pointcloud.hip): PLY vertex records and surface-normal scanlines of frames [B, H, W], both dispatch
# routes.  The host specification is output.pointcloud_host / output.normal_map_host.
# ------------------------------------------------------------------------------------------------------------------
def _camera(intrinsics, depth_range, what):
    """(fx, fy, cx, cy), (lo, hi) as Python floats that hold float32 values (the kernels' arithmetic is fp32)"""
    k = [float(np.float32(v)) for v in np.asarray(intrinsics, dtype=np.float64).reshape(-1)]
    if len(k) != 4 or not all(math.isfinite(v) for v in k) or k[0] <= 0 or k[1] <= 0:
        raise ValueError(f"{what}: intrinsics are finite fx, fy, cx, cy with fx, fy > 0 (got {intrinsics})")
    lo, hi = (float(np.float32(v)) for v in depth_range)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f"{what}: the depth range (lo, hi) must not be NaN")
    return k, (lo, hi)


_NO_IMAGE = object()  # the export samples no image


def _scene_inputs(what, depth, intrinsics, depth_range, image=_NO_IMAGE, edge_thr=None, max_width=False):
    """the arguments every export computed from a depth map shares, checked -> (frames fp32 [B, H, W], image fp32 [B, 3, Hi, Wi] or
    None, k, lo, hi, edge_thr or None) with the scalars as Python floats that hold float32 values.  ``max_width``: the frames' rows
    must fit prv2_stereo_max_width()"""
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dim() not in (2, 3):
        raise ValueError(f"{what}: depth is a GPU tensor [H, W] or [B, H, W]")
    d = _edge_frames(depth, torch.float32)
    k, (lo, hi) = _camera(intrinsics, depth_range, what)
    thr = None
    if edge_thr is not None:
        thr = float(np.float32(edge_thr))
        if math.isnan(thr):
            raise ValueError(f"{what}: edge_thr must not be NaN")
    if max_width:
        limit = L.load().prv2_stereo_max_width()
        if d.shape[2] > limit:
            raise ValueError(f"{what}: a row of {d.shape[2]} columns is wider than the {limit} the kernel keeps in LDS (prv2_stereo_max_width)")
    if image is _NO_IMAGE:
        return d, None, k, lo, hi, thr
    if not isinstance(image, torch.Tensor) or not image.is_cuda or image.device != d.device:
        raise ValueError(f"{what}: image is a GPU tensor on the depth map's device")
    img = (image[None] if image.dim() == 3 else image).to(torch.float32).contiguous()
    if img.dim() != 4 or img.shape[0] != d.shape[0] or img.shape[1] != 3 or img.shape[2] < 1 or img.shape[3] < 1:
        raise ValueError(f"{what}: image is [B, 3, Hi, Wi] with the depth map's B = {d.shape[0]} (got {tuple(image.shape)})")
    return d, img, k, lo, hi, thr


def _cloud_inputs(what, depth, image, intrinsics, depth_range, edge_thr, stride):
    """``_scene_inputs`` of pointcloud_pack and mesh_pack, and their stride"""
    if int(stride) < 1:
        raise ValueError(f"{what}: stride {int(stride)} < 1")
    return (*_scene_inputs(what, depth, intrinsics, depth_range, image, edge_thr), int(stride))


def _record_buffer(what, out, d, bound):
    """``out``, or a new uint8 [B, bound] buffer on the device of the frames ``d``; ``out`` must be a contiguous uint8 [B, >= bound]"""
    if out is None:
        return torch.empty((d.shape[0], bound), dtype=torch.uint8, device=d.device)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != d.device or out.dim() != 2 or not out.is_contiguous()
            or out.shape[0] != d.shape[0] or out.shape[1] < bound):
        raise ValueError(f"{what} is a contiguous GPU uint8 [{d.shape[0]}, >= {bound}] tensor")
    return out


def pointcloud_pack(depth, image, intrinsics, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1, out=None):
    """the PLY vertex records of fp32 depth frames [B, H, W] -> (vertex bytes uint8 [B, bound], counts int64 [B]), both on the
    device: frame f's cloud is the first 15 * counts[f] bytes of row f (float x, y, z + uchar r, g, b per kept pixel, row-major
    pixel order), bound = 15 * ceil(H / stride) * ceil(W / stride); the bytes behind a frame's records are not written.
    ``image``: fp32 [B, 3, Hi, Wi] ([3, Hi, Wi] for one frame), any size, sampled nearest.  ``intrinsics``: fx, fy, cx, cy in
    pixels of the [H, W] grid; ``depth_range``: (lo, hi), valid is lo < Z < hi; ``edge_thr``: the flying-pixel threshold
    (<= 0: off).  ``out``: a uint8 [B, >= bound] buffer to write into (include/prv2.h prv2_pointcloud_count / _pack)."""
    d, img, k, lo, hi, thr, stride = _cloud_inputs("pointcloud_pack", depth, image, intrinsics, depth_range, edge_thr, stride)
    lib = L.load()
    out = _record_buffer("pointcloud_pack: out", out, d, lib.prv2_pointcloud_bound(d.shape[1], d.shape[2], stride))
    if DISPATCH == "torch":
        return out, _tops().pointcloud_pack(d, img, k, lo, hi, thr, stride, out)
    wsb = lib.prv2_pointcloud_workspace_bytes(*d.shape)
    if wsb < 0:
        raise ValueError(f"pointcloud_pack: bad frame shape {tuple(d.shape)}")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=d.device)
    counts = torch.empty((d.shape[0],), dtype=torch.int64, device=d.device)
    _c("pointcloud_count", d.data_ptr(), *d.shape, *k, lo, hi, thr, stride, counts.data_ptr(), ws.data_ptr(), wsb)
    _c("pointcloud_pack", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], *k, lo, hi, thr, stride, ws.data_ptr(), wsb,
       out.data_ptr(), out.shape[1])
    return out, counts


def mesh_pack(depth, image, intrinsics, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1, out_vertices=None, out_faces=None):
    """the triangle mesh of fp32 depth frames [B, H, W] -> (vertex bytes uint8 [B, vbound], N int64 [B], face bytes uint8
    [B, fbound], M int64 [B]), all on the device.  The vertices are ``pointcloud_pack``'s (same arguments, same bytes); frame f's
    faces are the first 13 * M[f] bytes of row f (uchar 3 + three little-endian int32 vertex indices per face, cells in row-major
    order; the rule is output.mesh_faces_host), fbound = 26 * (ceil(H / stride) - 1) * (ceil(W / stride) - 1); the bytes behind
    a frame's records are not written.  The kept pixels are counted once: the vertex records and the index map of the faces read
    the same offsets.  ``out_vertices`` / ``out_faces``: uint8 [B, >= bound] buffers to write into (include/prv2.h "Mesh
    export")."""
    d, img, k, lo, hi, thr, stride = _cloud_inputs("mesh_pack", depth, image, intrinsics, depth_range, edge_thr, stride)
    lib = L.load()
    cwsb, wsb = lib.prv2_pointcloud_workspace_bytes(*d.shape), lib.prv2_mesh_workspace_bytes(*d.shape, stride)
    if cwsb < 0 or wsb < 0:
        raise ValueError(f"mesh_pack: bad frame shape {tuple(d.shape)}")
    verts = _record_buffer("mesh_pack: out_vertices", out_vertices, d, lib.prv2_pointcloud_bound(d.shape[1], d.shape[2], stride))
    faces = _record_buffer("mesh_pack: out_faces", out_faces, d, lib.prv2_mesh_bound(d.shape[1], d.shape[2], stride))
    if DISPATCH == "torch":
        n, m = _tops().mesh_pack(d, img, k, lo, hi, thr, stride, verts, faces)
        return verts, n, faces, m
    cws = torch.empty((cwsb,), dtype=torch.uint8, device=d.device)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=d.device)
    n = torch.empty((d.shape[0],), dtype=torch.int64, device=d.device)
    m = torch.empty((d.shape[0],), dtype=torch.int64, device=d.device)
    _c("pointcloud_count", d.data_ptr(), *d.shape, *k, lo, hi, thr, stride, n.data_ptr(), cws.data_ptr(), cwsb)
    _c("pointcloud_pack", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], *k, lo, hi, thr, stride, cws.data_ptr(), cwsb,
       verts.data_ptr(), verts.shape[1])
    _c("mesh_index", d.data_ptr(), *d.shape, lo, hi, thr, stride, cws.data_ptr(), cwsb, ws.data_ptr(), wsb)
    _c("mesh_count", d.data_ptr(), *d.shape, thr, stride, m.data_ptr(), ws.data_ptr(), wsb)
    _c("mesh_pack", d.data_ptr(), *d.shape, thr, stride, ws.data_ptr(), wsb, faces.data_ptr(), faces.shape[1])
    return verts, n, faces, m


def mesh_adaptive_pack(depth, image, intrinsics, depth_range=(0.0, math.inf), edge_thr=0.05, tolerance=0.01, block=32, out_vertices=None,
                       out_faces=None):
    """the adaptive triangle mesh of fp32 depth frames [B, H, W] -> (vertex bytes uint8 [B, vbound], N int64 [B], face bytes uint8
    [B, fbound], M int64 [B]), all on the device: a right-triangulated irregular network over the pixel grid, large triangles where
    the depth at a hypotenuse midpoint is within ``tolerance`` (relative, along the ray) of a flat triangle's, pixel-sized ones at
    depth edges and holes; ``block``: the side of the hierarchy's blocks in cells, a power of two in [2, 64].  The rule is
    output.mesh_adaptive_host.  Frame f's vertices are the first 15 * N[f] bytes of row f (``pointcloud_pack``'s records of the
    pixels a face uses, row-major) and its faces the first 13 * M[f] bytes (``mesh_pack``'s records, indices into that list);
    vbound = 15 * H * W, fbound = 26 * (H - 1) * (W - 1); the bytes behind a frame's records are not written.  ``out_vertices`` /
    ``out_faces``: uint8 [B, >= bound] buffers to write into (include/prv2.h "Adaptive mesh export")."""
    from .output import mesh_adaptive_arguments
    tol, block = mesh_adaptive_arguments(tolerance, block)
    d, img, k, lo, hi, thr = _scene_inputs("mesh_adaptive_pack", depth, intrinsics, depth_range, image, edge_thr)
    lib = L.load()
    wsb = lib.prv2_mesh_adaptive_workspace_bytes(*d.shape, block)
    if wsb < 0:
        raise ValueError(f"mesh_adaptive_pack: bad frame shape {tuple(d.shape)}")
    verts = _record_buffer("mesh_adaptive_pack: out_vertices", out_vertices, d, lib.prv2_mesh_adaptive_vertex_bound(d.shape[1], d.shape[2]))
    faces = _record_buffer("mesh_adaptive_pack: out_faces", out_faces, d, lib.prv2_mesh_adaptive_face_bound(d.shape[1], d.shape[2]))
    if DISPATCH == "torch":
        n, m = _tops().mesh_adaptive_pack(d, img, k, lo, hi, thr, tol, block, verts, faces)
        return verts, n, faces, m
    ws = torch.empty((wsb,), dtype=torch.uint8, device=d.device)
    n = torch.empty((d.shape[0],), dtype=torch.int64, device=d.device)
    m = torch.empty((d.shape[0],), dtype=torch.int64, device=d.device)
    _c("mesh_adaptive_count", d.data_ptr(), *d.shape, lo, hi, thr, tol, block, n.data_ptr(), m.data_ptr(), ws.data_ptr(), wsb)
    _c("mesh_adaptive_pack", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], *k, lo, hi, thr, tol, block, ws.data_ptr(), wsb,
       verts.data_ptr(), verts.shape[1], faces.data_ptr(), faces.shape[1])
    return verts, n, faces, m


def normal_rows(depth, intrinsics, depth_range=(0.0, math.inf)):
    """the camera-facing surface normals of fp32 depth frames [B, H, W] as RGB scanlines (n * 0.5 + 0.5 in bytes; (0, 0, 0)
    where there is no normal) -> scanline buffer (include/prv2.h prv2_normal_rows)"""
    d, _, k, lo, hi, _ = _scene_inputs("normal_rows", depth, intrinsics, depth_range)
    if DISPATCH == "torch":
        return _tops().normal_rows(d, k, lo, hi)
    rows = _rows(d, 3)
    _c("normal_rows", d.data_ptr(), *d.shape, *k, lo, hi, rows.data_ptr(), rows.shape[1])
    return rows


# ------------------------------------------------------------------------------------------------------------------
# Stereo export (csrc/stereo.hip): the right-eye view of frames [B, H, W] as scanlines, or its source-column maps, both dispatch
# routes.  The host specification is output.stereo_source_host / output.stereo_image_host.
# ------------------------------------------------------------------------------------------------------------------
STEREO_LAYOUTS = {"right": 0, "sbs": 1, "anaglyph": 2}  # PRV2_STEREO_RIGHT / _SBS / _ANAGLYPH


def _stereo_inputs(what, depth, intrinsics, baseline, convergence, depth_range, edge_thr, image=_NO_IMAGE):
    """``_scene_inputs`` of stereo_rows and stereo_source, and their baseline and convergence -> (frames, image or None, fx, baseline,
    convergence, lo, hi, edge_thr)"""
    d, img, k, lo, hi, thr = _scene_inputs(what, depth, intrinsics, depth_range, image, edge_thr, max_width=True)
    base, conv = float(np.float32(baseline)), float(np.float32(convergence))
    if not math.isfinite(base):
        raise ValueError(f"{what}: baseline {baseline} must be finite")
    if math.isnan(conv) or conv == 0.0:
        raise ValueError(f"{what}: convergence {convergence}: a distance other than 0 (inf: parallel axes)")
    return d, img, k[0], base, conv, lo, hi, thr


def stereo_source(depth, intrinsics, baseline, convergence=math.inf, depth_range=(0.0, math.inf), edge_thr=0.05):
    """the source columns of the right-eye view of fp32 depth frames [B, H, W] -> (src, filled), int32 [B, H, W] on the device: the
    source column every column of the view shows (-1: a hole), and the same with the holes filled from the farther side
    (output.stereo_source_host; include/prv2.h prv2_stereo_source).  ``intrinsics``: fx, fy, cx, cy of the [H, W] grid (fx is used);
    ``baseline``: metres to the right; ``convergence``: the depth that keeps its column (inf: parallel axes)."""
    d, _, fx, base, conv, lo, hi, thr = _stereo_inputs("stereo_source", depth, intrinsics, baseline, convergence, depth_range, edge_thr)
    if DISPATCH == "torch":
        return tuple(_tops().stereo_source(d, fx, base, conv, lo, hi, thr))
    src, filled = torch.empty(d.shape, dtype=torch.int32, device=d.device), torch.empty(d.shape, dtype=torch.int32, device=d.device)
    _c("stereo_source", d.data_ptr(), *d.shape, fx, base, conv, lo, hi, thr, src.data_ptr(), filled.data_ptr())
    return src, filled


def stereo_rows(depth, image, intrinsics, baseline, convergence=math.inf, depth_range=(0.0, math.inf), edge_thr=0.05, layout="right"):
    """the right-eye view of fp32 depth frames [B, H, W] as RGB scanlines -> scanline buffer uint8 [B, prv2_rows_bytes(H, Wout, 3)],
    Wout = 2 W for ``layout`` 'sbs' (left | right), W for 'right' and 'anaglyph' (red of the left eye, green and blue of the right);
    output.stereo_image_host is the specification (include/prv2.h prv2_stereo_rows).  ``image``: fp32 [B, 3, Hi, Wi] ([3, Hi, Wi]
    for one frame), any size, sampled nearest; the other arguments as ``stereo_source``."""
    if layout not in STEREO_LAYOUTS:
        raise ValueError(f"stereo_rows: layout {layout!r}: one of {tuple(STEREO_LAYOUTS)}")
    d, img, fx, base, conv, lo, hi, thr = _stereo_inputs("stereo_rows", depth, intrinsics, baseline, convergence, depth_range, edge_thr, image)
    if DISPATCH == "torch":
        return _tops().stereo_rows(d, img, fx, base, conv, lo, hi, thr, STEREO_LAYOUTS[layout])
    wout = d.shape[2] * (2 if layout == "sbs" else 1)
    rows = torch.empty((d.shape[0], L.load().prv2_rows_bytes(d.shape[1], wout, 3)), dtype=torch.uint8, device=d.device)
    _c("stereo_rows", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], fx, base, conv, lo, hi, thr, STEREO_LAYOUTS[layout],
       rows.data_ptr(), rows.shape[1])
    return rows


# ------------------------------------------------------------------------------------------------------------------
# Depth-of-field export (csrc/bokeh.hip): frames [B, H, W] re-rendered through a thin lens, as fp32 planes or as scanlines, both
# dispatch routes.  The host specification is output.bokeh_render_host / output.bokeh_image_host.
# ------------------------------------------------------------------------------------------------------------------
def bokeh_max_radius() -> int:
    """the largest ``max_radius`` the kernel takes (include/prv2.h prv2_bokeh_max_radius)"""
    return int(L.load().prv2_bokeh_max_radius())


def _bokeh_inputs(what, depth, image, intrinsics, aperture, focus, focus_point, max_radius, depth_range):
    """``_scene_inputs`` of bokeh_render and bokeh_rows, and their lens -> (frames, image, fx, aperture, focus (0.0: use the focus
    point), u, v, max_radius, lo, hi)"""
    d, img, k, lo, hi, _ = _scene_inputs(what, depth, intrinsics, depth_range, image)
    ap, rm = float(np.float32(aperture)), float(np.float32(max_radius))
    if not (math.isfinite(ap) and ap >= 0.0):
        raise ValueError(f"{what}: aperture {aperture}: finite and not below 0 (metres)")
    if not 0.0 <= rm <= bokeh_max_radius():
        raise ValueError(f"{what}: max_radius {max_radius}: in [0, {bokeh_max_radius()}] pixels (prv2_bokeh_max_radius)")
    zf = 0.0
    if focus is not None:
        zf = float(np.float32(focus))
        if not (math.isfinite(zf) and zf > 0.0):
            raise ValueError(f"{what}: focus {focus}: a finite distance greater than 0 (None: the focus point)")
    u, v = (float(np.float32(c)) for c in focus_point)
    if not (0.0 <= u <= 1.0 and 0.0 <= v <= 1.0):
        raise ValueError(f"{what}: focus point {tuple(focus_point)} outside [0, 1]^2")
    return d, img, k[0], ap, zf, u, v, rm, lo, hi


def bokeh_render(depth, image, intrinsics, aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0, depth_range=(0.0, math.inf)):
    """fp32 depth frames [B, H, W] re-rendered through a thin lens -> (out fp32 [B, 3, H, W], focus fp32 [B]), both on the device:
    output.bokeh_render_host is the specification (include/prv2.h prv2_bokeh_render).  ``image``: fp32 [B, 3, Hi, Wi] ([3, Hi, Wi]
    for one frame), any size, sampled nearest.  ``intrinsics``: fx, fy, cx, cy of the [H, W] grid (fx is used); ``aperture``: the
    lens diameter in metres; ``focus``: the distance in focus, or None for the depth at ``focus_point`` (u, v) in [0, 1]^2, read on
    the device; ``max_radius``: the cap of the circle of confusion in pixels (<= ``bokeh_max_radius()``).  ``focus``: the distance
    every frame used, NaN where its focus pixel was not valid (that frame is the image itself)."""
    d, img, fx, ap, zf, u, v, rm, lo, hi = _bokeh_inputs("bokeh_render", depth, image, intrinsics, aperture, focus, focus_point, max_radius,
                                                          depth_range)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().bokeh_render(d, img, fx, ap, zf, u, v, rm, lo, hi))  # noqa: E731
    else:
        out = torch.empty((d.shape[0], 3, d.shape[1], d.shape[2]), dtype=torch.float32, device=d.device)
        used = torch.empty((d.shape[0],), dtype=torch.float32, device=d.device)
        box.extend((out, used))
        call = lambda: _c("bokeh_render", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], fx, ap, zf, u, v, rm, lo, hi,  # noqa: E731
                          out.data_ptr(), used.data_ptr())
    # per pixel: the map and the three colour samples read, three planes written (the window is re-read from cache and LDS)
    PROFILER.launch_aux("bokeh_render", d.numel() * 28.0, call, f"{d.shape[0]}x{d.shape[1]}x{d.shape[2]} r{rm:g}")
    return box[0], box[1]


def bokeh_rows(depth, image, intrinsics, aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0, depth_range=(0.0, math.inf)):
    """``bokeh_render`` as RGB scanlines -> (scanline buffer uint8 [B, prv2_rows_bytes(H, W, 3)], focus fp32 [B]): the bytes of
    output.bokeh_image_host (include/prv2.h prv2_bokeh_rows); the arguments as ``bokeh_render``."""
    d, img, fx, ap, zf, u, v, rm, lo, hi = _bokeh_inputs("bokeh_rows", depth, image, intrinsics, aperture, focus, focus_point, max_radius,
                                                          depth_range)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().bokeh_rows(d, img, fx, ap, zf, u, v, rm, lo, hi))  # noqa: E731
    else:
        rows = _rows(d, 3)
        used = torch.empty((d.shape[0],), dtype=torch.float32, device=d.device)
        box.extend((rows, used))
        call = lambda: _c("bokeh_rows", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], fx, ap, zf, u, v, rm, lo, hi,  # noqa: E731
                          rows.data_ptr(), rows.shape[1], used.data_ptr())
    PROFILER.launch_aux("bokeh_rows", d.numel() * 19.0, call, f"{d.shape[0]}x{d.shape[1]}x{d.shape[2]} r{rm:g}")
    return box[0], box[1]


# ------------------------------------------------------------------------------------------------------------------
# Novel-view export (csrc/view.hip): frames [B, H, W] seen from a list of camera poses, as source maps or as scanlines, both
# dispatch routes.  The host specification is output.view_source_host / output.view_image_host; output.view_poses makes the poses.
# ------------------------------------------------------------------------------------------------------------------
def view_max_face() -> int:
    """the pixel centres a face's box may span each way before it is dropped (include/prv2.h prv2_view_max_face)"""
    return int(L.load().prv2_view_max_face())


def _view_inputs(what, depth, intrinsics, poses, depth_range, edge_thr, image=_NO_IMAGE):
    """``_scene_inputs`` of view_source and view_rows, and their poses -> (frames, image or None, k, poses fp32 [NV, 12] on the
    frames' device, lo, hi, edge_thr, workspace bytes)"""
    d, img, k, lo, hi, thr = _scene_inputs(what, depth, intrinsics, depth_range, image, edge_thr, max_width=True)
    if isinstance(poses, torch.Tensor):
        p = poses.detach().to(torch.float32)
    else:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float32)))
    if p.dim() == 1:
        p = p[None]
    if p.dim() != 2 or p.shape[0] < 1 or p.shape[1] != 12:
        raise ValueError(f"{what}: poses are [NV, 12] (or [12]): row-major 3 x 4 matrices [R | t] (got {tuple(p.shape)})")
    nbytes = L.load().prv2_view_workspace_bytes(d.shape[0], min(p.shape[0], 2 ** 31 - 1), d.shape[1], d.shape[2])
    if nbytes <= 0:
        raise ValueError(f"{what}: {d.shape[0]} frames x {p.shape[0]} views of {d.shape[1]} x {d.shape[2]} exceed 2^29 pixels")
    return d, img, k, p.to(d.device).contiguous(), lo, hi, thr, int(nbytes)


def view_source(depth, intrinsics, poses, depth_range=(0.0, math.inf), edge_thr=0.05):
    """fp32 depth frames [B, H, W] seen from the camera poses ``poses`` ([NV, 12] or [12], a host array or a tensor: row-major
    [R | t] of output.view_poses; uploaded here) -> (src, filled int32 [B, NV, H, W], iz fp32 [B, NV, H, W]) on the device: the source
    pixel y * W + x every pixel of every view shows (-1: a hole), the same with the holes filled from the farther side, and the
    winners' 1 / Zc (0: a hole) -- output.view_source_host for every (frame, pose); include/prv2.h prv2_view_source.
    ``intrinsics``: fx, fy, cx, cy of the [H, W] grid."""
    d, _, k, p, lo, hi, thr, nbytes = _view_inputs("view_source", depth, intrinsics, poses, depth_range, edge_thr)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().view_source(d, k, p, lo, hi, thr))  # noqa: E731
    else:
        shape = (d.shape[0], p.shape[0], d.shape[1], d.shape[2])
        box.extend((torch.empty(shape, dtype=torch.int32, device=d.device), torch.empty(shape, dtype=torch.int32, device=d.device),
                    torch.empty(shape, dtype=torch.float32, device=d.device)))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=d.device)
        call = lambda: _c("view_source", d.data_ptr(), *d.shape, *k, p.data_ptr(), p.shape[0], lo, hi, thr, box[0].data_ptr(),  # noqa: E731
                          box[1].data_ptr(), box[2].data_ptr(), ws.data_ptr(), nbytes)
    # per view pixel: the key cleared, about seven 8-byte minima at the identity pose, the key read, three maps written
    PROFILER.launch_aux("view_source", d.numel() * p.shape[0] * 84.0, call, f"{d.shape[0]}x{p.shape[0]}x{d.shape[1]}x{d.shape[2]}")
    return box[0], box[1], box[2]


def view_rows(depth, image, intrinsics, poses, depth_range=(0.0, math.inf), edge_thr=0.05):
    """``view_source``'s views as RGB scanlines -> scanline buffers uint8 [B, NV, prv2_rows_bytes(H, W, 3)]: the bytes of
    output.view_image_host for every (frame, pose) (include/prv2.h prv2_view_rows).  ``image``: fp32 [B, 3, Hi, Wi] ([3, Hi, Wi] for
    one frame), any size, sampled nearest; the other arguments as ``view_source``."""
    d, img, k, p, lo, hi, thr, nbytes = _view_inputs("view_rows", depth, intrinsics, poses, depth_range, edge_thr, image)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().view_rows(d, img, k, p, lo, hi, thr))  # noqa: E731
    else:
        rows = torch.empty((d.shape[0], p.shape[0], L.load().prv2_rows_bytes(d.shape[1], d.shape[2], 3)), dtype=torch.uint8, device=d.device)
        box.append(rows)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=d.device)
        call = lambda: _c("view_rows", d.data_ptr(), img.data_ptr(), *d.shape, img.shape[2], img.shape[3], *k, p.data_ptr(), p.shape[0], lo, hi,  # noqa: E731
                          thr, rows.data_ptr(), rows.shape[2], ws.data_ptr(), nbytes)
    PROFILER.launch_aux("view_rows", d.numel() * p.shape[0] * 87.0, call, f"{d.shape[0]}x{p.shape[0]}x{d.shape[1]}x{d.shape[2]}")
    return box[0]


# ------------------------------------------------------------------------------------------------------------------
# Temporal stabilisation (csrc/temporal.hip): the frames of a sequence aligned to and blended with the previous output, both dispatch
# routes.  The host specification is temporal.temporal_step_host; temporal.TemporalStabilizer keeps the state.
# ------------------------------------------------------------------------------------------------------------------
TEMPORAL_STATS = L.TEMPORAL_STATS


def _temporal_args(fn, depth, image, state_depth, luma_prev, luma_next):
    """the tensor checks the temporal steps share -> (n, h, w)"""
    from .temporal import MAX_PIXELS
    tensors = dict(depth=depth, image=image, state_depth=state_depth, luma_prev=luma_prev, luma_next=luma_next)
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != depth.device:
            raise ValueError(f"{fn}: {name} is a GPU tensor on the maps' device (temporal.temporal_step_host is the host's)")
        want = torch.uint8 if name.startswith("luma") else torch.float32
        if t.dtype != want or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be a contiguous {want} tensor (got {t.dtype}, strides {t.stride()})")
    if depth.dim() != 3 or depth.numel() == 0:
        raise ValueError(f"{fn}: depth is [n, H, W] (got {tuple(depth.shape)})")
    n, h, w = depth.shape
    if h * w > MAX_PIXELS:
        raise ValueError(f"{fn}: a frame of {h} x {w} exceeds 2^25 pixels (the bound of the exact int64 sums)")
    if image.dim() != 4 or image.shape[0] != n or image.shape[1] != 3 or image.shape[2] < 1 or image.shape[3] < 1:
        raise ValueError(f"{fn}: image is [n, 3, Hi, Wi] with the maps' n = {n} (got {tuple(image.shape)})")
    for name in ("state_depth", "luma_prev", "luma_next"):
        if tuple(tensors[name].shape) != (h, w):
            raise ValueError(f"{fn}: {name} {tuple(tensors[name].shape)} is not the frames' [{h}, {w}]")
    if luma_prev.data_ptr() == luma_next.data_ptr():
        raise ValueError(f"{fn}: the two luma buffers must differ")
    return n, h, w


def temporal_step(depth, image, state_depth, luma_prev, luma_next, state_present, alpha=0.5, tau=6, rho=0.05, anchor=0.9):
    """n frames of a sequence, in order: ``depth`` fp32 [n, H, W] and ``image`` fp32 [n, 3, Hi, Wi] on the GPU -> (out fp32 [n, H, W],
    stats int64 [n, 12] on the device: the rows ``temporal.stats_dict`` names; include/prv2.h prv2_temporal_step).  The state is
    updated in place: ``state_depth`` fp32 [H, W] (read when ``state_present``; leaves with the last output), ``luma_prev`` /
    ``luma_next`` two distinct uint8 [H, W] buffers (frame f reads the previous luma from the first when f is even and writes its own
    into the other; the state leaves in ``luma_prev`` for an even n, in ``luma_next`` for an odd one).  Four launches per frame on the
    current stream, no host synchronisation; the same bits however a sequence is cut into calls."""
    from .temporal import check_params
    alpha, tau, rho, anchor = check_params(alpha, tau, rho, anchor)
    n, h, w = _temporal_args("temporal_step", depth, image, state_depth, luma_prev, luma_next)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().temporal_step_(depth, image, alpha, tau, rho, anchor, state_depth, luma_prev, luma_next,  # noqa: E731
                                                         bool(state_present)))
    else:
        wsb = L.load().prv2_temporal_workspace_bytes(h, w)
        if wsb < 0:
            raise ValueError(f"temporal_step: bad frame shape {tuple(depth.shape)}")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=depth.device)
        out = torch.empty_like(depth)
        stats = torch.empty((n, TEMPORAL_STATS), dtype=torch.int64, device=depth.device)
        box.extend((out, stats))
        call = lambda: _c("temporal_step", depth.data_ptr(), image.data_ptr(), n, h, w, image.shape[2], image.shape[3], alpha, tau, rho,  # noqa: E731
                          anchor, state_depth.data_ptr(), luma_prev.data_ptr(), luma_next.data_ptr(), int(bool(state_present)), out.data_ptr(),
                          stats.data_ptr(), ws.data_ptr(), wsb)
    # per pixel: the fit reads x, y, Lp and the image's three samples and writes L; the apply reads x, y, L, Lp and writes out
    PROFILER.launch_aux("temporal_step", n * h * w * 39.0, call, f"{n}x{h}x{w}")
    return box[0], box[1]


def temporal_motion_step(depth, image, state_depth, luma_prev, luma_next, state_present, alpha=0.5, tau=6, rho=0.05, anchor=0.9,
                         motion_range=8):
    """``temporal_step`` with the motion stage in front (include/prv2.h prv2_temporal_motion_step; csrc/motion.hip): the same arguments
    and state, ``motion_range`` = R in 1 .. 16 -> (out, stats, motion stats int64 [n, 8]: the rows ``temporal.motion_dict`` names,
    vectors int16 [n, ceil(H / 16), ceil(W / 16), 2]: the blocks' (my, mx)), the last three on the device.  A frame with a state costs
    six launches before the step's four; the bits equal ``temporal.temporal_step_host(motion_range=R)``'s."""
    from .temporal import check_motion_range, check_params
    alpha, tau, rho, anchor = check_params(alpha, tau, rho, anchor)
    motion_range = check_motion_range(motion_range)
    n, h, w = _temporal_args("temporal_motion_step", depth, image, state_depth, luma_prev, luma_next)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().temporal_motion_step_(depth, image, alpha, tau, rho, anchor, motion_range, state_depth,  # noqa: E731
                                                                luma_prev, luma_next, bool(state_present)))
    else:
        wsb = L.load().prv2_temporal_motion_workspace_bytes(h, w)
        if wsb < 0:
            raise ValueError(f"temporal_motion_step: bad frame shape {tuple(depth.shape)}")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=depth.device)
        out = torch.empty_like(depth)
        stats = torch.empty((n, TEMPORAL_STATS), dtype=torch.int64, device=depth.device)
        mstats = torch.empty((n, L.TEMPORAL_MOTION_STATS), dtype=torch.int64, device=depth.device)
        vectors = torch.empty((n, -(-h // 16), -(-w // 16), 2), dtype=torch.int16, device=depth.device)
        box.extend((out, stats, mstats, vectors))
        call = lambda: _c("temporal_motion_step", depth.data_ptr(), image.data_ptr(), n, h, w, image.shape[2], image.shape[3], alpha, tau,  # noqa: E731
                          rho, anchor, motion_range, state_depth.data_ptr(), luma_prev.data_ptr(), luma_next.data_ptr(),
                          int(bool(state_present)), out.data_ptr(), stats.data_ptr(), mstats.data_ptr(), vectors.data_ptr(), ws.data_ptr(), wsb)
    # per pixel: the step's 39 bytes, the luma pass (12 read, 1 written), the warp (5 read, 5 written) and the refinement's windows (~3)
    PROFILER.launch_aux("temporal_motion_step", n * h * w * 65.0, call, f"{n}x{h}x{w}")
    return box[0], box[1], box[2], box[3]


# ------------------------------------------------------------------------------------------------------------------
# Ground-truth evaluation (csrc/evalgt.hip): the device half of UnrealStereo4kDataset and the sums behind compute_metrics, both
# dispatch routes.
# ------------------------------------------------------------------------------------------------------------------
def u8_image(src, swap_rb=True):
    """uint8 [H, W, 3] on the device -> fp32 [3, H, W] = float(src) / 255 (correctly rounded), channels reversed with ``swap_rb``
    (u4k_dataset.py:125-147: bit-equal to ``image.astype(np.float32)[:, :, ::-1].copy() / 255.0`` + to_tensor)"""
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
        raise ValueError("u8_image: src is a GPU uint8 [H, W, 3] tensor")
    src = src.contiguous()
    if DISPATCH == "torch":
        return _tops().u8_image(src, bool(swap_rb))
    dst = torch.empty((3, src.shape[0], src.shape[1]), dtype=torch.float32, device=src.device)
    _c("u8_image", src.data_ptr(), src.shape[0], src.shape[1], int(bool(swap_rb)), dst.data_ptr())
    return dst


def disp_gt(disp, factor, th=1.0):
    """fp32 disparity [H, W] -> (depth = factor / disp fp32 [H, W], boundary uint8 [H, W] = metrics.get_boundaries(disp, th, 0)) in
    one pass (u4k_dataset.py:128-129,216)"""
    if not isinstance(disp, torch.Tensor) or not disp.is_cuda or disp.dtype != torch.float32 or disp.dim() != 2:
        raise ValueError("disp_gt: disp is a GPU fp32 [H, W] tensor")
    disp = disp.contiguous()
    if DISPATCH == "torch":
        return _tops().disp_gt(disp, float(factor), float(th))
    depth, boundary = torch.empty_like(disp), torch.empty(disp.shape, dtype=torch.uint8, device=disp.device)
    _c("disp_gt", disp.data_ptr(), *disp.shape, float(factor), float(th), depth.data_ptr(), boundary.data_ptr())
    return depth, boundary


def _mask_u8(t, like, name):
    if t is None:
        return None
    t = _edge_frames(t)
    if t.dtype not in (torch.bool, torch.uint8):
        t = t != 0
    if t.shape != like.shape:
        raise ValueError(f"depth_metrics: {name} has shape {tuple(t.shape)}, the frames {tuple(like.shape)}")
    return t


GT_KINDS = {"eth3d": 0, "mid": 1, "cityscapes": 2}  # enum prv2_gt_kind (datasets.ImageDataset's gt_format names)
CITYSCAPES_FACTOR = float(np.float32(0.209313 * 2262.52))  # general_dataset.py:144: baseline x focal length, met by a float32 array


def gt_decode(src, kind, factor=CITYSCAPES_FACTOR, doffs=0.0, th=1.0, flip=False, byteswap=False):
    """the general dataset's ground truth (general_dataset.py:103-151) from the raw samples [H, W] on the device, one pass ->
    (depth fp32 [H, W], boundary uint8 [H, W] = metrics.get_boundaries(<the map the reference takes its edges from>, th, 0)).
    ``kind``: 'eth3d' (fp32 depth; non-finite -> 0), 'mid' (fp32 PFM disparity; depth = factor / (disp + doffs) / 1000, 0 at +inf;
    ``flip``: rows bottom-to-top, ``byteswap``: the file's byte order is not the host's) or 'cityscapes' (uint16 disparity samples;
    ``factor`` defaults to the reference's constant) -- include/prv2.h prv2_gt_decode."""
    if kind not in GT_KINDS:
        raise ValueError(f"gt_decode: kind {kind!r} is not one of {sorted(GT_KINDS)}")
    want = torch.uint16 if kind == "cityscapes" else torch.float32
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != want or src.dim() != 2:
        raise ValueError(f"gt_decode: src is a GPU {want} [H, W] tensor for kind {kind!r}")
    src = src.contiguous()
    if DISPATCH == "torch":
        return _tops().gt_decode(src, GT_KINDS[kind], float(factor), float(doffs), float(th), bool(flip), bool(byteswap))
    depth = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    boundary = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    _c("gt_decode", src.data_ptr(), GT_KINDS[kind], *src.shape, float(factor), float(doffs), float(th), int(bool(flip)), int(bool(byteswap)),
       depth.data_ptr(), boundary.data_ptr())
    return depth, boundary


def depth_metrics(gt, pred, boundary=None, region=None, min_depth=1e-3, max_depth=80.0, crop=None):
    """the sums of compute_metrics (metric.py:11-149) of fp32 frames [B, H, W] -> float64 [B, S, 12] on the device, S = 3 (all /
    inside / outside) with a ``region`` map, else 1; ``crop`` = (y0, y1, x0, x1), None: the whole frame.  The twelve sums: include/prv2.h
    prv2_depth_metrics.  Bit-identical from call to call."""
    g, p = _edge_frames(gt, torch.float32), _edge_frames(pred, torch.float32)
    if g.shape != p.shape:
        raise ValueError(f"depth_metrics: gt {tuple(g.shape)} and pred {tuple(p.shape)} differ in shape")
    b, r = _mask_u8(boundary, g, "boundary"), _mask_u8(region, g, "region")
    y0, y1, x0, x1 = (0, g.shape[1], 0, g.shape[2]) if crop is None else (int(v) for v in crop)
    if DISPATCH == "torch":
        return _tops().depth_metrics(g, p, b, r, float(min_depth), float(max_depth), y0, y1, x0, x1)
    lib = L.load()
    wsb = lib.prv2_depth_metrics_workspace_bytes(*g.shape)
    if wsb < 0:
        raise ValueError(f"depth_metrics: bad frame shape {tuple(g.shape)}")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=g.device)
    out = torch.empty((g.shape[0], 3 if r is not None else 1, 12), dtype=torch.float64, device=g.device)
    _c("depth_metrics", g.data_ptr(), p.data_ptr(), _ptr(b), _ptr(r), *g.shape, float(min_depth), float(max_depth), y0, y1, x0, x1, out.data_ptr(), ws.data_ptr(), wsb)
    return out


def depth_metrics_lowres(gt, pred, boundary=None, region=None, min_depth=1e-3, max_depth=80.0, crop=None):
    """``depth_metrics`` for a prediction [B, h, w] of another resolution than gt [B, H, W]: every prediction value is sampled in the
    scoring kernel (bilinear, align_corners=False, the operations of F.interpolate on the device), the resized map is never written
    (include/prv2.h prv2_depth_metrics_lowres).  Equal shapes run ``depth_metrics``' kernel: the same bits."""
    g, p = _edge_frames(gt, torch.float32), _edge_frames(pred, torch.float32)
    if g.shape[0] != p.shape[0]:
        raise ValueError(f"depth_metrics_lowres: gt {tuple(g.shape)} and pred {tuple(p.shape)} differ in their frame count")
    b, r = _mask_u8(boundary, g, "boundary"), _mask_u8(region, g, "region")
    y0, y1, x0, x1 = (0, g.shape[1], 0, g.shape[2]) if crop is None else (int(v) for v in crop)
    if DISPATCH == "torch":
        return _tops().depth_metrics_lowres(g, p, b, r, float(min_depth), float(max_depth), y0, y1, x0, x1)
    lib = L.load()
    wsb = lib.prv2_depth_metrics_workspace_bytes(*g.shape)
    if wsb < 0:
        raise ValueError(f"depth_metrics_lowres: bad frame shape {tuple(g.shape)}")
    ws = torch.empty((wsb,), dtype=torch.uint8, device=g.device)
    out = torch.empty((g.shape[0], 3 if r is not None else 1, 12), dtype=torch.float64, device=g.device)
    _c("depth_metrics_lowres", g.data_ptr(), p.data_ptr(), _ptr(b), _ptr(r), *g.shape, p.shape[1], p.shape[2], float(min_depth), float(max_depth),
       y0, y1, x0, x1, out.data_ptr(), ws.data_ptr(), wsb)
    return out


# ------------------------------------------------------------------------------------------------------------------
# ETHDataset (estimator/datasets/eth_dataset.py): the image stage (csrc/gather.hip) and the edge area its get_metrics splits every
# metric by (csrc/evalgt.hip), both dispatch routes.
# ------------------------------------------------------------------------------------------------------------------
def u8_image_resize(src_hwc_u8, oh, ow):
    """uint8 RGB [h, w, 3] on the device -> fp32 [3, oh, ow]: bytes / 255, then F.interpolate(mode='bilinear', align_corners=True) in
    PyTorch's fp32 operations (eth_dataset.py:133,150-161; include/prv2.h prv2_u8_image_resize).  (oh, ow) == (h, w) gives
    ``u8_image(swap_rb=False)``'s bits."""
    src = src_hwc_u8
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
        raise ValueError("u8_image_resize: src is a GPU uint8 [H, W, 3] tensor")
    oh, ow = int(oh), int(ow)
    if oh < 1 or ow < 1:
        raise ValueError(f"u8_image_resize: bad size {oh} x {ow}")
    src = src.contiguous()
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().u8_image_resize(src, oh, ow))  # noqa: E731
    else:
        dst = torch.empty((3, oh, ow), dtype=torch.float32, device=src.device)
        box.append(dst)
        call = lambda: _c("u8_image_resize", src.data_ptr(), src.shape[0], src.shape[1], dst.data_ptr(), oh, ow)  # noqa: E731
    PROFILER.launch_aux("u8_image_resize", 12.0 * oh * ow + 3.0 * src.shape[0] * src.shape[1], call, f"{src.shape[0]}x{src.shape[1]}->{oh}x{ow}")
    return box[0]


def image_edge_region(image_chw, H, W, frac=0.5):
    """fp32 image [3, h, w] on the device -> uint8 0/1 [H, W]: the edge area of ETHDataset.get_metrics
    (eth_dataset.py:261-272) -- Sobel gradient magnitude summed over the channels, >= ``frac`` x its maximum, widened by the 3 x 3
    blur and resized (bilinear, align_corners=True) to the ground truth's shape, > 0.  Exact integer logic after the gradient, the
    same bits on every call (include/prv2.h prv2_image_edge_region)."""
    img = image_chw
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.float32:
        raise ValueError("image_edge_region: image is a GPU fp32 [3, h, w] tensor")
    if img.dim() != 3 or img.shape[0] != 3:
        raise ValueError(f"image_edge_region: image of shape {tuple(img.shape)}, expected [3, h, w]")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"image_edge_region: bad size {H} x {W}")
    img = img.contiguous()
    h, w = img.shape[1:]
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().image_edge_region(img, H, W, float(frac)))  # noqa: E731
    else:
        wsb = L.load().prv2_image_edge_region_workspace_bytes(h, w)
        if wsb < 0:
            raise ValueError(f"image_edge_region: bad image shape {tuple(img.shape)}")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=img.device)
        region = torch.empty((H, W), dtype=torch.uint8, device=img.device)
        box.append(region)
        call = lambda: _c("image_edge_region", img.data_ptr(), h, w, float(frac), region.data_ptr(), H, W, ws.data_ptr(), wsb)  # noqa: E731
    PROFILER.launch_aux("image_edge_region", 21.0 * h * w + 1.0 * H * W, call, f"{h}x{w}->{H}x{W}")
    return box[0]


# ------------------------------------------------------------------------------------------------------------------
# CityScapesDataset (estimator/datasets/cityscapes_dataset.py): the ground-truth decode and the two pixel sets of its get_metrics
# (csrc/evalgt.hip), kornia's Canny on the colour segmentation map (csrc/edges.hip), both dispatch routes.  The host specification is
# metrics.seg_canny / metrics.cityscapes_masks.
# ------------------------------------------------------------------------------------------------------------------
def cityscapes_gt(disp_u16, seg_u8, factor):
    """uint16 disparity samples [H, W] and the RGB bytes [H, W, 3] of the colour segmentation map (or None) on the device, one pass
    -> (depth fp32 [H, W], boundary uint8 [H, W], seg fp32 [3, H, W] holding 0 .. 255, or None): gt_decode('cityscapes')'s depth with
    ``factor``, -1 in the noisy bands (the last ceil(H / 4) rows, the first W // 16 and the last ceil(W / 16) columns), 0 at the sky
    class (R == 70 and G == 130); boundary = metrics.get_boundaries(<that map>, 1, 0) (cityscapes_dataset.py:153-174, :300;
    include/prv2.h prv2_cityscapes_gt)."""
    d = disp_u16
    if not isinstance(d, torch.Tensor) or not d.is_cuda or d.dtype != torch.uint16 or d.dim() != 2:
        raise ValueError("cityscapes_gt: disp is a GPU uint16 [H, W] tensor")
    d = d.contiguous()
    s = seg_u8
    if s is not None:
        if not isinstance(s, torch.Tensor) or not s.is_cuda or s.dtype != torch.uint8 or s.device != d.device:
            raise ValueError("cityscapes_gt: seg is a GPU uint8 [H, W, 3] tensor on disp's device, or None")
        if tuple(s.shape) != tuple(d.shape) + (3,):
            raise ValueError(f"cityscapes_gt: seg of shape {tuple(s.shape)}, expected {tuple(d.shape) + (3,)}")
        s = s.contiguous()
    box = []
    if DISPATCH == "torch":
        def call():
            depth, boundary, seg = _tops().cityscapes_gt(d, s, float(factor))
            box.extend((depth, boundary, seg if s is not None else None))
    else:
        depth = torch.empty(d.shape, dtype=torch.float32, device=d.device)
        boundary = torch.empty(d.shape, dtype=torch.uint8, device=d.device)
        seg = None if s is None else torch.empty((3,) + tuple(d.shape), dtype=torch.float32, device=d.device)
        box.extend((depth, boundary, seg))
        call = lambda: _c("cityscapes_gt", d.data_ptr(), _ptr(s), *d.shape, float(factor), depth.data_ptr(), boundary.data_ptr(), _ptr(seg))  # noqa: E731
    PROFILER.launch_aux("cityscapes_gt", (7.0 if s is None else 22.0) * d.numel(), call, f"{d.shape[0]}x{d.shape[1]}")
    return box[0], box[1], box[2]


def seg_canny(seg_chw, low_threshold=0.1, high_threshold=0.2):
    """fp32 colour segmentation map [3, H, W] (0 .. 255) on the device -> bool [H, W]: ``kornia.filters.canny(seg)[1] > 0`` with
    kornia's defaults (cityscapes_dataset.py:333-334), equal to metrics.seg_canny on the same input pixel for pixel (include/prv2.h
    prv2_seg_canny states the arithmetic).  H, W >= 3: the blur's reflect pad of 2 needs three pixels."""
    from .metrics import seg_canny_weights
    x = seg_chw
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("seg_canny: seg is a GPU fp32 [3, H, W] tensor")
    if x.dim() != 3 or x.shape[0] != 3:
        raise ValueError(f"seg_canny: seg of shape {tuple(x.shape)}, expected [3, H, W]")
    h, w = x.shape[1:]
    if h < 3 or w < 3:
        raise ValueError(f"seg_canny: {h} x {w}: the reflect pad of 2 needs at least 3 x 3 pixels")
    x = x.contiguous()
    gw = seg_canny_weights()
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().seg_canny(x, [float(v) for v in gw], float(low_threshold), float(high_threshold)))  # noqa: E731
    else:
        ws = torch.empty((L.load().prv2_edges_workspace_bytes(1, h, w),), dtype=torch.uint8, device=x.device)
        out = torch.empty((h, w), dtype=torch.bool, device=x.device)
        box.append(out)
        call = lambda: _c("seg_canny", x.data_ptr(), h, w, gw.ctypes.data, float(low_threshold), float(high_threshold), out.data_ptr(),  # noqa: E731
                          ws.data_ptr(), ws.numel())
    PROFILER.launch_aux("seg_canny", 80.0 * h * w, call, f"{h}x{w}")
    return box[0]


def cityscapes_masks(seg_edges, gt_edges, hr_region):
    """bool / uint8 maps [H, W] on the device -> (edge_mask, flatten), uint8 0/1 [H, W], one pass: edge_mask = seg_edges and the
    7 x 7 dilation of gt_edges, flatten = not edge_mask and not hr_region (cityscapes_dataset.py:360-365 without the valid-depth
    test, which the scoring kernel makes; include/prv2.h prv2_cityscapes_masks)."""
    maps = []
    for name, t in (("seg_edges", seg_edges), ("gt_edges", gt_edges), ("hr_region", hr_region)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.bool, torch.uint8) or t.dim() != 2:
            raise ValueError(f"cityscapes_masks: {name} is a GPU bool / uint8 [H, W] tensor")
        if maps and (t.shape != maps[0].shape or t.device != maps[0].device):
            raise ValueError(f"cityscapes_masks: {name} {tuple(t.shape)} does not match seg_edges {tuple(maps[0].shape)} on its device")
        maps.append(t.contiguous())
    s, g, r = maps
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().cityscapes_masks(s, g, r))  # noqa: E731
    else:
        edge, flatten = torch.empty(s.shape, dtype=torch.uint8, device=s.device), torch.empty(s.shape, dtype=torch.uint8, device=s.device)
        box.extend((edge, flatten))
        call = lambda: _c("cityscapes_masks", s.data_ptr(), g.data_ptr(), r.data_ptr(), *s.shape, edge.data_ptr(), flatten.data_ptr())  # noqa: E731
    PROFILER.launch_aux("cityscapes_masks", 5.0 * s.numel(), call, f"{s.shape[0]}x{s.shape[1]}")
    return box[0], box[1]


# ------------------------------------------------------------------------------------------------------------------
# KittiDataset / ScanNetDataset (estimator/datasets/kitti_dataset.py, scannet_dataset.py): the ground truth of a 16-bit depth PNG,
# re-gridded as it is decoded (csrc/evalgt.hip), both dispatch routes.  The host specification is metrics.depth16_decode_spec.
# ------------------------------------------------------------------------------------------------------------------
def depth16_gt(src_u16, out_hw=None, divisor=256.0, window=None, nearest=False, th=1.0):
    """the uint16 samples [sh, sw] of a depth PNG on the device, one pass -> (depth fp32 [H, W] = float32(sample) / divisor, boundary
    uint8 [H, W] = metrics.get_boundaries(depth, th, 0)), (H, W) = ``out_hw`` (None: the source's shape).  ``window=(top, left)``: output
    (y, x) is source (top + y, left + x) -- KITTI's kb-crop (kitti_dataset.py:123-131, divisor 256); None is (0, 0).  ``nearest=True``:
    the grid of PIL's ``resize((W, H), Image.NEAREST)`` (metrics.pil_nearest_index) -- ScanNet's ground truth at the image's size
    (scannet_dataset.py:112-118, divisor 1000).  include/prv2.h prv2_depth16_gt."""
    s = src_u16
    if not isinstance(s, torch.Tensor) or not s.is_cuda or s.dtype != torch.uint16 or s.dim() != 2:
        raise ValueError("depth16_gt: src is a GPU uint16 [H, W] tensor")
    if nearest and window is not None:
        raise ValueError("depth16_gt: give window or nearest=True, not both")
    sh, sw = s.shape
    H, W = (sh, sw) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    top, left = (0, 0) if window is None else (int(window[0]), int(window[1]))
    if H < 1 or W < 1 or sh < 1 or sw < 1 or H * W >= 2 ** 31:
        raise ValueError(f"depth16_gt: bad shape {sh} x {sw} -> {H} x {W}")
    if not nearest and (top < 0 or left < 0 or top + H > sh or left + W > sw):
        raise ValueError(f"depth16_gt: the window of {H} x {W} at ({top}, {left}) lies outside the {sh} x {sw} source")
    if not float(divisor) > 0:
        raise ValueError(f"depth16_gt: divisor {divisor} is not positive")
    s = s.contiguous()
    box = []
    if DISPATCH == "torch":
        call = lambda: box.extend(_tops().depth16_gt(s, H, W, float(divisor), top, left, bool(nearest), float(th)))  # noqa: E731
    else:
        depth = torch.empty((H, W), dtype=torch.float32, device=s.device)
        boundary = torch.empty((H, W), dtype=torch.uint8, device=s.device)
        box.extend((depth, boundary))
        call = lambda: _c("depth16_gt", s.data_ptr(), sh, sw, int(bool(nearest)), top, left, H, W, float(divisor), float(th),  # noqa: E731
                          depth.data_ptr(), boundary.data_ptr())
    PROFILER.launch_aux("depth16_gt", 7.0 * H * W, call, f"{sh}x{sw}->{H}x{W}")
    return box[0], box[1]


# ------------------------------------------------------------------------------------------------------------------
# Scale-and-shift-invariant evaluation (estimator/models/losses.py:523-544, :600-700; csrc/ssi_eval.hip), both dispatch routes.
# ------------------------------------------------------------------------------------------------------------------
SSI_VALUES = L.SSI_VALUES


def ssi_metrics(gt, pred, min_depth=1e-3, max_depth=80.0, crop=None):
    """fp32 frames gt [B, H, W] and pred [B, H, W] (or [B, h, w]: sampled inside the kernels as ``depth_metrics_lowres`` samples it) ->
    float64 [B, 41] on the device: the scale / shift of compute_scale_and_shift for the values and for the vertical / horizontal
    stride-2 differences, the mask count N, the normal-equation sums, the sums behind ssi_l1 / ssi_gm / gm / ssi_gm_inv and the twelve
    sums of ``depth_metrics`` on the aligned prediction (the layout: include/prv2.h prv2_ssi_metrics).  The mask is
    min_depth < gt < max_depth inside ``crop`` = (y0, y1, x0, x1), None: the whole frame.  Two passes, no host synchronisation;
    bit-identical from call to call and for a frame alone or in a batch."""
    g, p = _edge_frames(gt, torch.float32), _edge_frames(pred, torch.float32)
    if g.shape[0] != p.shape[0]:
        raise ValueError(f"ssi_metrics: gt {tuple(g.shape)} and pred {tuple(p.shape)} differ in their frame count")
    y0, y1, x0, x1 = (0, g.shape[1], 0, g.shape[2]) if crop is None else (int(v) for v in crop)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().ssi_metrics(g, p, float(min_depth), float(max_depth), y0, y1, x0, x1))  # noqa: E731
    else:
        wsb = L.load().prv2_ssi_metrics_workspace_bytes(*g.shape)
        if wsb < 0:
            raise ValueError(f"ssi_metrics: bad frame shape {tuple(g.shape)}")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=g.device)
        out = torch.empty((g.shape[0], SSI_VALUES), dtype=torch.float64, device=g.device)
        box.append(out)
        call = lambda: _c("ssi_metrics", g.data_ptr(), p.data_ptr(), *g.shape, p.shape[1], p.shape[2], float(min_depth), float(max_depth),  # noqa: E731
                          y0, y1, x0, x1, out.data_ptr(), ws.data_ptr(), wsb)
    PROFILER.launch_aux("ssi_metrics", 2.0 * (4.0 * g.numel() + 4.0 * p.numel()), call, f"{g.shape[0]}x{g.shape[1]}x{g.shape[2]}<-{p.shape[1]}x{p.shape[2]}")
    return box[0]


# ------------------------------------------------------------------------------------------------------------------
# Boundary F1 evaluation (the scale-invariant boundary F1 of Depth Pro; csrc/boundary_eval.hip), both dispatch routes.
# ------------------------------------------------------------------------------------------------------------------
BOUNDARY_MAX_THRESHOLDS = L.BOUNDARY_MAX_THRESHOLDS


def boundary_f1(gt, pred, min_depth=1e-3, max_depth=80.0, crop=None, thresholds=None):
    """fp32 frames gt [B, H, W] and pred [B, H, W] (or [B, h, w]: sampled inside the kernel as ``depth_metrics_lowres`` samples it) ->
    float64 [B, 2 + 12 T] on the device: n_h, n_v, then per threshold and direction (L, T, R, B) the counts tp, np, ng of the
    occluding-boundary pairs (the definition and the layout: include/prv2.h "Boundary F1 evaluation"; metrics.boundary_from_values
    makes the scores).  The mask is min_depth < gt < max_depth inside ``crop`` = (y0, y1, x0, x1), None: the whole frame.
    ``thresholds``: 1 .. 16 finite ratios > 1, None: metrics.boundary_thresholds().  One pass, no host synchronisation; integer counts:
    bit-identical from call to call and for a frame alone or in a batch."""
    g, p = _edge_frames(gt, torch.float32), _edge_frames(pred, torch.float32)
    if g.shape[0] != p.shape[0]:
        raise ValueError(f"boundary_f1: gt {tuple(g.shape)} and pred {tuple(p.shape)} differ in their frame count")
    if thresholds is None:
        from .metrics import boundary_thresholds
        thresholds = boundary_thresholds()
    th = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
    if not 1 <= th.size <= BOUNDARY_MAX_THRESHOLDS:
        raise ValueError(f"boundary_f1: {th.size} thresholds, not in [1, {BOUNDARY_MAX_THRESHOLDS}]")
    y0, y1, x0, x1 = (0, g.shape[1], 0, g.shape[2]) if crop is None else (int(v) for v in crop)
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().boundary_f1(g, p, float(min_depth), float(max_depth), y0, y1, x0, x1, [float(t) for t in th]))  # noqa: E731
    else:
        wsb = L.load().prv2_boundary_f1_workspace_bytes(*g.shape)
        if wsb < 0:
            raise ValueError(f"boundary_f1: bad frame shape {tuple(g.shape)}")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=g.device)
        out = torch.empty((g.shape[0], L.boundary_values(th.size)), dtype=torch.float64, device=g.device)
        box.append(out)
        call = lambda: _c("boundary_f1", g.data_ptr(), p.data_ptr(), *g.shape, p.shape[1], p.shape[2], float(min_depth), float(max_depth),  # noqa: E731
                          y0, y1, x0, x1, th.ctypes.data, int(th.size), out.data_ptr(), ws.data_ptr(), wsb)
    PROFILER.launch_aux("boundary_f1", 4.0 * g.numel() + 4.0 * p.numel(), call, f"{g.shape[0]}x{g.shape[1]}x{g.shape[2]}<-{p.shape[1]}x{p.shape[2]} T{th.size}")
    return box[0]


# ------------------------------------------------------------------------------------------------------------------
# Sparsification curves of a per-pixel uncertainty (AUSE / AURG; csrc/sparsify.hip), both dispatch routes.
# ------------------------------------------------------------------------------------------------------------------
SPARSIFY_MAX_LEVELS = L.SPARSIFY_MAX_LEVELS


def _sparsify_frames(t, name):
    """an fp32 map [H, W] or [B, H, W] -> contiguous [B, H, W]; anything else is the caller's error (nothing is converted)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"sparsify: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"sparsify: {name} has dtype {t.dtype}, expected torch.float32")
    if t.dim() not in (2, 3):
        raise ValueError(f"sparsify: {name} has shape {tuple(t.shape)}, expected [H, W] or [B, H, W]")
    return (t[None] if t.dim() == 2 else t).contiguous()


def sparsify(gt, pred, uncert, count=None, min_count=0.0, min_depth=1e-3, max_depth=80.0, levels=20):
    """fp32 frames gt, pred, uncert (and count) [B, H, W] of one shape -> float64 [B, 1 + 10 L] on the device: n, the 3 L thresholds of
    the uncertainty / e_rel / e_sq ordering and the seven rows of L sums over the kept sets S_k (the layout and the definition:
    include/prv2.h prv2_sparsify).  Host tensors, another dtype, other dims, maps of different shapes and ``levels`` outside [1, 64] are
    rejected before anything is launched.  No host synchronisation; bit-identical from call to call and for a frame alone or in a batch."""
    g = _sparsify_frames(gt, "gt")
    p, u = _sparsify_frames(pred, "pred"), _sparsify_frames(uncert, "uncert")
    c = None if count is None else _sparsify_frames(count, "count")
    for name, t in (("pred", p), ("uncert", u), ("count", c)):
        if t is not None and t.shape != g.shape:
            raise ValueError(f"sparsify: {name} {tuple(t.shape)} does not match gt {tuple(g.shape)}: resize the maps to one shape first")
    levels = int(levels)
    if not 1 <= levels <= SPARSIFY_MAX_LEVELS:
        raise ValueError(f"sparsify: {levels} levels out of range [1, {SPARSIFY_MAX_LEVELS}]")
    for name, t in (("gt", g), ("pred", p), ("uncert", u), ("count", c)):
        if t is not None and (not t.is_cuda or t.device != g.device):
            raise ValueError(f"sparsify: {name} must be a GPU tensor on gt's device (there is no CPU path; "
                             "metrics.compute_uncertainty_metrics is the host's)")
    wsb = L.load().prv2_sparsify_workspace_bytes(*g.shape, levels)
    if wsb < 0:
        raise ValueError(f"sparsify: bad frame shape {tuple(g.shape)}")
    box = []
    if DISPATCH == "torch":
        call = lambda: box.append(_tops().sparsify(g, p, u, c, float(min_count), float(min_depth), float(max_depth), levels))  # noqa: E731
    else:
        ws = torch.empty((wsb,), dtype=torch.uint8, device=g.device)
        out = torch.empty((g.shape[0], L.sparsify_values(levels)), dtype=torch.float64, device=g.device)
        box.append(out)
        call = lambda: _c("sparsify", g.data_ptr(), p.data_ptr(), u.data_ptr(), _ptr(c), float(min_count), *g.shape, float(min_depth),  # noqa: E731
                          float(max_depth), levels, out.data_ptr(), ws.data_ptr(), ws.numel())
    PROFILER.launch_aux("sparsify", (42.0 + 60.0 * -(-levels // 8)) * g.numel(), call, f"{g.shape[0]}x{g.shape[1]}x{g.shape[2]} L{levels}")
    return box[0]
