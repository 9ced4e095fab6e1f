/*
 * prv2.h -- C ABI of the MI355X (gfx950) hot path of patch-refined depth inference.
 *
 * The reference (zhyever/PatchRefinerV2) is pure Python/PyTorch: it has no FFI.  The seam this
 * library sits behind is therefore the set of torch ops the reference's hot path dispatches
 * (SURVEY.md 2.1 / 8b).  Each entry point below names the reference call site(s) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless the name ends in _host or the type says otherwise;
 *   - activations are NHWC: element (n,y,x,c) lives at base[n*bstride + (y*W + x)*ld + c];
 *     ``ld`` (pixel stride, in floats) lets a producer write straight into a channel slice of
 *     a wider concatenation buffer, which is how every torch.cat on the path is made free;
 *   - ``stream`` is a hipStream_t passed as void*; all work is enqueued, nothing synchronises;
 *   - return value: 0 on success, non-zero on a rejected argument or a HIP error;
 *     prv2_last_error() returns the message of the calling thread's last failure;
 *   - no allocation, no hidden global state, graph-capture safe.
 */
#ifndef PRV2_H
#define PRV2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRV2_ABI_VERSION 20

enum prv2_act { PRV2_ACT_NONE = 0, PRV2_ACT_RELU = 1, PRV2_ACT_GELU = 2, PRV2_ACT_SIGMOID = 3, PRV2_ACT_SOFTPLUS = 4,
                PRV2_ACT_SILU = 5 /* x * sigmoid(x): EfficientNet refiner encoder (timm 'swish') */ };

/* arithmetic of the matrix kernels */
enum prv2_prec {
  PRV2_PREC_F32 = 0,    /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate            */
  PRV2_PREC_BF16X3 = 1, /* operands split hi+lo bf16; hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 */
  PRV2_PREC_BF16 = 2,   /* plain bf16 operands (fast, ~1e-3 relative; not the parity path)          */
  PRV2_PREC_F16F6 = 3   /* fp16 product + two block-scaled fp6 (e2m3) corrections: what prv2_conv3x3_f6 computes in and reports through
                         * prv2_last_kernel(); the other entry points do not take it                  */
};

int prv2_abi_version(void);
const char* prv2_last_error(void);
/* Name of the device kernel the calling thread's last successful prv2_conv2d dispatched to, as "name<BN,prec>"
 * (e.g. "conv3x3_halo16_kernel<128,bf16x3>", "gemm16_kernel<64,bf16x3>"): what bench.py's roofline attributes time to.
 * Which kernel runs a layer depends on the layer's shape PER IMAGE, never on the batch size (so results do not depend on
 * how tiles are batched).  When a call issues two kernels (f32 mode: 3x3 tiles + remainder strip) it names the last.
 * prv2_dwconv2d_ex (and prv2_dwconv2d through it) and prv2_conv2d_cout1 report theirs the same way, with the kernel size in the
 * first slot: "dwconv_strip_kernel<K,f32>" (stride 1, 8 pixels per thread) / "dwconv_kernel<K,f32>", and
 * "conv_cout1_k3_kernel<32,f32>" (32-channel slabs) / "conv_cout1_k1_kernel<0,f32>". */
const char* prv2_last_kernel(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear layer with fused epilogue.
 * Replaces nn.Conv2d / nn.Linear / nn.ConvTranspose2d(k==stride) on the path:
 *   fusion convs     estimator/models/blocks/convs.py:39-41,70; bi_directional_fusion_model.py:40-51
 *   DPT head convs   external/depth_anything_v2/dpt.py:51-81, util/blocks.py:45-47
 *   ViT linears      external/depth_anything_v2/dinov2_layers/attention.py:44,46; mlp.py:30,32
 *
 *   y[m, n] = epilogue( sum_{ky,kx,c} pre(x[pix(m) + (ky,kx), c]) * w[n, ky, kx, c] )
 *   epilogue: v = acc + bias[n]; [v = LN_row(v) * ln_weight[n] + ln_bias[n]]; v = act(v); v *= gamma[n];
 *             v = mul[m,n] * v; v += res[m,n] + res2[m,n]
 *   (every pointer optional).  pre = ReLU when relu_in != 0.  Zero padding.
 *   LN_row = the channels-first LayerNorm of the fusion convs (convs.py:21-29, biased variance, eps ln_eps) over the
 *   cout channels of the pixel, fused when cout <= 128 (the whole row sits in one workgroup tile).
 *
 * Weights are pre-packed by prv2_pack_conv_weight(): [cout_pad][kh*kw][cin_pad] with
 * cin_pad = roundup(cin, 32), cout_pad = roundup(cout, 128), zero filled.
 * convt_k > 0 turns the call into ConvTranspose2d(kernel=stride=convt_k): kh=kw=1, the GEMM has
 * convt_k^2 * cout columns ordered (ky, kx, co) and each column block is scattered to
 * output pixel (y*k+ky, x*k+kx).
 * ------------------------------------------------------------------------------------------ */
typedef struct prv2_conv_desc {
  int32_t n, h, w;       /* input batch / spatial size                                   */
  int32_t cin, cout;
  int32_t kh, kw, stride, pad;
  int32_t ldx, ldy;      /* pixel strides (floats)                                       */
  int64_t x_bstride;     /* image stride of x in floats (0 => h*w*ldx)                   */
  int64_t y_bstride;     /* image stride of y in floats (0 => oh*ow*ldy)                 */
  int32_t relu_in;       /* apply ReLU to x while loading                                */
  int32_t act;           /* enum prv2_act                                                */
  int32_t convt_k;       /* 0, or k for ConvTranspose2d(k, stride=k)                     */
  int32_t ld_mul, ld_res, ld_res2;
  int32_t prec;          /* enum prv2_prec                                               */
  int32_t force_generic; /* != 0: never use the LDS-halo 3x3 kernel (tests / A-B)        */
  float ln_eps;          /* epsilon of the fused LayerNorm (used when ln_weight != NULL) */
  int32_t part;          /* f32 mode: 3x3 halo convs whose width is 32k + (1..8) run as 32-pixel tiles + a remainder strip
                          * (generic kernel): 0 = both (default), 1 = the tiles only, 2 = the strip only (per-kernel timing).
                          * The bf16 modes do tiles and strip in one launch: part must be 0.                             */
  int32_t same_pad;      /* != 0: TensorFlow "SAME" padding as timm's Conv2dSame (the reference's stem surgery builds one,
                          * patchrefinerplus.py:152-158): out = ceil(in / stride), total = max((out-1)*stride + k - in, 0),
                          * low = total / 2, the rest goes to the high side; ``pad`` is ignored.  Not for convt_k.          */
  int32_t fmt;           /* PRV2_FMT_* bits: operands in the pre-split "X2" activation format -- per 8 channels
                          * [8 x bf16 hi | 8 x bf16 lo] (32 bytes = the bytes of 8 floats; hi = RNE bf16 of v, lo = RNE bf16 of v - hi),
                          * i.e. exactly what the bf16x3 kernels' loaders make of an fp32 input, stored by the producer so that the
                          * consumer only copies.  Taken by the 256-column kernels (prv2_conv3x3_ln_gate / prv2_conv2d layers it routes
                          * there): X_X2 + MUL_X2 by the gate kernel, Y_X2 by the plain conv without LayerNorm.  A layer's result does not
                          * depend on the format (``mul`` counts as hi + lo either way).  0 everywhere else.                        */
} prv2_conv_desc;
#define PRV2_FMT_X_X2 1   /* x is X2 (gate kernel: the GatedConvUnit's [out | coarse ROI] concat)            */
#define PRV2_FMT_MUL_X2 2 /* mul is X2 (gate kernel: ``out``, the first half of that concat; goes together with X_X2) */
#define PRV2_FMT_Y_X2 4   /* y is written X2 (256-column conv, no LayerNorm: GatedConvUnit.conv writing ``out``) */

/* host-side helpers: sizes of the packed weight buffers (in bytes) */
int64_t prv2_packed_weight_bytes(int32_t cout, int32_t cin, int32_t kh, int32_t kw, int32_t convt_k, int32_t prec);

/* w_src: device fp32, PyTorch layout [cout][cin][kh][kw] (Conv2d / Linear with kh=kw=1) or
 * [cin][cout][k][k] when convt_k>0 (ConvTranspose2d).  bn_scale (optional, [cout]) is folded in. */
int prv2_pack_conv_weight(const float* w_src, const float* bn_scale, void* w_packed, int32_t cout, int32_t cin,
                          int32_t kh, int32_t kw, int32_t convt_k, int32_t prec, void* stream);

int prv2_conv2d(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias,
                const float* ln_weight, const float* ln_bias, const float* gamma, const float* mul, const float* res,
                const float* res2, float* y, void* stream);

/* 3x3 / stride 1 / pad 1 convolution whose first ``channels`` input channels are a bilinear(align_corners=True) UPSAMPLE of a
 * low-resolution tensor, interpolated while the conv stages its input tile -- the upsampled tensor is never written:
 *   UpSample.forward_hardcode   estimator/models/blocks/fusion_model.py:15-24   x = cat[interpolate(x1, size, 'bilinear',
 *                               align_corners=True), x2, pred1, pred2] -> DoubleConv: the first conv reads channels [0, c1) from x1
 *   C2FModule output_conv1      bi_directional_fusion_model.py:139-142,201      conv3x3(interpolate(path_1, scale 2, align_corners))
 * x (NHWC, d->ldx) supplies the channels [channels, d->cin) at their usual offsets (its first ``channels`` channels are not
 * read; x may equal u->x when channels == d->cin).  Same arithmetic, bit for bit, as prv2_upsample_bilinear into x followed by
 * prv2_conv2d.  Contract (prv2_conv2d_ups_supported(d, u) != 0): bf16 modes, 3x3 s1 p1, cout > 64 and != 256-with-cin%32==0 routing
 * aside the layer must be one the 128-column halo kernel takes (width >= 24 ...), channels % 32 == 0, 0 < channels <= cin,
 * u->ld % 4 == 0, 16-byte aligned, no input ReLU. */
typedef struct prv2_ups_src {
  const float* x;        /* low-resolution source, NHWC [n, h, w, ld], channels [0, channels) used */
  int32_t h, w, ld;
  int32_t channels;
  int64_t bstride;       /* image stride in floats (0 => h*w*ld) */
} prv2_ups_src;
int prv2_conv2d_ups_supported(const prv2_conv_desc* d, const prv2_ups_src* u);
int prv2_conv2d_ups(const prv2_conv_desc* d, const float* x, const prv2_ups_src* u, const void* w_packed, const float* bias,
                    const float* ln_weight, const float* ln_bias, const float* res, float* y, void* stream);

/* 3x3 / stride 1 / pad 1 convolution of a bilinear(align_corners=True) UPSAMPLE (factor >= 5/3) of u, computed at u's resolution
 * (csrc/upconv.hip) -- the layers prv2_conv2d_ups interpolates inside its loader, with 2.3x fewer matrix operations:
 *   C2FModule output_conv1      bi_directional_fusion_model.py:139-142,201   conv3x3(interpolate(path_1, scale 2, align_corners=True))
 *   UpSample.forward_hardcode   fusion_model.py:15-24                        the interpolate(x1) part of DoubleConv.0(cat[x1, x2, pred1, pred2])
 * The conv is linear and its input an interpolation of u, so  conv3x3(up(u); W)(p) = sum_tap [p + d_tap inside] Bil(G_tap; s(p + d_tap))
 * with G_tap = W[:, :, tap] . u at LOW resolution (MFMA) and the 36 corner terms per output gathered on the VALU.
 *     y[n, h, w, 0 .. cout) = act(conv3x3(interpolate(u, (h, w), 'bilinear', align_corners=True)) + bias + add)
 * w_packed: prv2_pack_conv_weight(cout, cin = u->channels, 3, 3) -- for a conv over a concat [up(u) | rest], the weight columns of
 * the upsampled part; ``add`` (NHWC [n, h, w, ld_add >= cout], or NULL) is then prv2_conv2d of ``rest`` with the other columns,
 * activation NONE -- it may be y itself (every output element is read by the thread that writes it).
 * Same split products and fp32 accumulation as the other bf16 kernels; the taps / corners are summed in another order than
 * upsample -> conv (fp32-grade, not bit-identical).  Contract (prv2_upconv3x3_supported != 0): bf16 modes, u->channels % 32 == 0,
 * source step (u->h - 1) / (h - 1) and (u->w - 1) / (w - 1) <= 0.6 pixel (16 x 28 output tiles up to 1/2 -- the x2 upsamples --,
 * 14 x 24 up to 3/5: DepthAnything's 256 -> 448 head resolution), 16-byte aligned NHWC rows. */
int prv2_upconv3x3_supported(const prv2_ups_src* u, int32_t n, int32_t h, int32_t w, int32_t cout, int32_t prec);
int prv2_upconv3x3(const prv2_ups_src* u, const void* w_packed, const float* bias, const float* add, int32_t ld_add, int32_t n, int32_t h,
                   int32_t w, int32_t cout, int32_t act, int32_t prec, float* y, int32_t ldy, int64_t y_bstride, void* stream);

/* TWO back-to-back 3x3 convs (no activation in between) of a bilinear(align_corners=True) x2 UPSAMPLE as ONE 5x5 conv computed at u's
 * resolution (csrc/upconv5.hip) -- C2FModule's ``output_conv2[0] o output_conv1 o interpolate`` (with refinenet1.out_conv folded into
 * output_conv1): bi_directional_fusion_model.py:139-146 (interpolate + out_conv), :169-173 (definitions), :201-203 (use):
 *     v = act(conv3x3(conv3x3(up(u); W1) + b1(p); W2) + b2)  =  act(conv5x5(up(u); Weff) + bias_map(p) - ring_fix(p)),   Weff[d] = sum_{d1+d2=d} W2[d2] W1[d1]
 * 205 k instead of 332 k MACs per output pixel in the reference's terms; the 128-channel full-resolution intermediate is never formed.
 *   prv2_upconv5x5       y = act(conv5x5(interpolate(u, (h, w))) + bias_map[class(y)][class(x)]) for every pixel EXCEPT the one-pixel border
 *                        ring, which is written WITHOUT the activation (the ring fix below finishes it).  w_packed:
 *                        prv2_pack_conv_weight(cout, cin = u->channels, 5, 5) of Weff; bias_map: device fp32 [5][5][cout], row / column
 *                        classes (0, 1, interior, h - 2, h - 1): the inner conv's (position dependent) bias seen through the outer conv's
 *                        zero padding -- data independent.  cout <= 32.
 *   prv2_upconv5x5_lines lines[n][2 uw + 2 uh][channels] = the border lines of up(u) at u's resolution: output row 0, row h - 1 (uw positions
 *                        each), column 0, column w - 1 (uh each) -- align_corners samples of u's first / last rows and columns.
 *   prv2_upconv5x5_ring  the 5x5 form over the zero-padded map includes inner-conv outputs one pixel OUTSIDE the image, which the outer conv's
 *                        zero padding hides: on the ring  y = act(y - fix),  fix = per edge a 1-D five-tap conv of the border line -- as tap
 *                        GEMMs at u's resolution: g_edges[n][2 uw + 2 uh][ldg] = prv2_conv2d (1x1) of ``lines`` with the weights
 *                        [(edge * 7 + j) * cout + c][ci], edge = top, bottom, left, right; j < 5: sum_{k1 + k2 - 2 = j - 2} W2[edge's outer taps k2]
 *                        W1[edge's inner taps k1]; j = 5 / 6: the corner term at the row edges' first / last pixel (the outside corner position
 *                        is in both edges' sums).  tools/studies/composite5x5_ring.py: the float64 algebra (4e-15).
 * Contract (prv2_upconv5x5_supported != 0): bf16 modes, u->channels % 32 == 0, cout % 4 == 0 and <= 32, source step <= 1/2 (x2 upsamples),
 * h, w >= 5, 16-byte aligned NHWC rows.  fp32-grade, not bit-identical to the two-conv sequence. */
int prv2_upconv5x5_supported(const prv2_ups_src* u, int32_t n, int32_t h, int32_t w, int32_t cout, int32_t prec);
int prv2_upconv5x5(const prv2_ups_src* u, const void* w_packed, const float* bias_map, int32_t n, int32_t h, int32_t w, int32_t cout,
                   int32_t act, int32_t prec, float* y, int32_t ldy, int64_t y_bstride, void* stream);
int prv2_upconv5x5_lines(const prv2_ups_src* u, int32_t n, int32_t h, int32_t w, float* lines, void* stream);
int prv2_upconv5x5_ring(float* y, int32_t ldy, int64_t y_bstride, int32_t n, int32_t h, int32_t w, int32_t cout, const float* g_edges,
                        int32_t ldg, int32_t uh, int32_t uw, int32_t act, void* stream);

/* prv2_conv2d (3x3 / stride 1 / pad 1, bias, [LayerNorm,] activation, [+ res]) that ALSO writes the two depth maps every fusion
 * level appends to its features behind its own output channels: y[pixel][cout .. cout + 3] = (p1, p2, 0, 0), p1 / p2 dense
 * [n, ph, pw] resized bilinear(align_corners=True) to the output size -- the ``torch.cat([f, pred1, pred2])`` of
 * fusion_model.py:91-118 / bi_directional_fusion_model.py:424-436 closed by the conv that fills the rest of the row, instead of a
 * prv2_depth_pair_fill launch of 16-byte stores into 400-byte rows.  Same arithmetic as prv2_conv2d + prv2_depth_pair_fill.
 * Contract (prv2_conv2d_tail_supported(d) != 0): bf16 modes, 3x3 s1 p1, width >= 24, height >= 4, cout % 4 == 0 and <= 128 (the
 * widths whose LayerNorm the halo kernels fuse), ldy >= cout + 4, LayerNorm or residual but not both. */
int prv2_conv2d_tail_supported(const prv2_conv_desc* d);
int prv2_conv2d_tail(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* ln_weight,
                     const float* ln_bias, const float* res, const float* p1, const float* p2, int32_t ph, int32_t pw, float* y,
                     void* stream);

/* GatedConvUnit tail in one kernel (estimator/models/blocks/bi_directional_fusion_model.py:44-51 ``fusion_conv`` =
 * Conv3x3(2F -> F) . LayerNorm(channels_first) . ReLU . Conv1x1(F -> F) . Sigmoid, and :70-80 ``out * fusion (+ xs[0])``):
 *     fused = act(LN(conv3x3(x) + bias))                              (d->act: NONE or RELU; ln_eps from d)
 *     y     = mul * sigmoid(conv1x1(fused) + gate_bias) (+ res)
 * gate_w_packed == NULL: y = act(LN(conv3x3(x) + bias)) -- the 256-channel conv with the LayerNorm fused (prv2_conv2d fuses it
 * for cout <= 128 only); mul / res / gate_bias must then be NULL and d->act may be any activation.
 * Shape contract (prv2_conv3x3_ln_gate_supported(d) != 0): 3x3, stride 1, pad 1, cin % 32 == 0, bf16 modes; cout == 256 (F of the
 * refinenets: 8 x 16-pixel x 256-channel tiles, width >= 16), or -- with gate weights -- cout == 128 / 32 (the full-resolution
 * output_conv2_fusion block of the DepthAnything / ZoeDepth fusion configs: 8 x 32-pixel tiles, width >= 24, height >= 4); x / y / mul / res NHWC fp32 with pixel strides ldx / ldy / ld_mul / ld_res (multiples of 4, 16-byte aligned).
 * w_packed: prv2_pack_conv_weight image of the 3x3 weights; gate_w_packed: prv2_pack_gate_weight image (prv2_gate_weight_bytes(cout)
 * bytes) of the 1x1 weights [cout][cout].  Same arithmetic as the unfused sequence conv2d -> layernorm -> conv2d(1x1, sigmoid, mul,
 * res) (split products, accumulation order); the row statistics are reduced in a different (fixed) order. */
int prv2_conv3x3_ln_gate_supported(const prv2_conv_desc* d);
int64_t prv2_gate_weight_bytes(int32_t channels);
int prv2_pack_gate_weight(const float* w_src, void* w_packed, int32_t cout, int32_t cin, void* stream);
int prv2_conv3x3_ln_gate(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* ln_weight,
                         const float* ln_bias, const void* gate_w_packed, const float* gate_bias, const float* mul, const float* res,
                         float* y, void* stream);

/* prv2_conv3x3_ln_gate with a pre-LayerNorm addend: fused = act(LN(conv3x3(x) + bias + pre)), pre NHWC fp32 [n, h, w, ld_pre >= cout]
 * (ld_pre % 4 == 0, 16-byte aligned) -- the coarse half of the unit's ``fusion_conv.0`` from prv2_coarse_tap_gather, x being the fine
 * half only (cin = F instead of 2F).  pre == NULL: prv2_conv3x3_ln_gate. */
int prv2_conv3x3_ln_gate_pre(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* pre,
                             int32_t ld_pre, const float* ln_weight, const float* ln_bias, const void* gate_w_packed, const float* gate_bias,
                             const float* mul, const float* res, float* y, void* stream);

/* prv2_conv2d (3x3 / stride 1 / pad 1) with an addend in front of the epilogue: v = acc + pre[m, n] + bias[n]; [LayerNorm;] act; [+ res]
 * -- ``fusion_layers_1[l](cat([c, f]))`` (bi_directional_fusion_model.py:424-426; FusionUnet encoder_layers_1, fusion_model.py:91-95)
 * run over the fine half f only, with the coarse half of the conv from prv2_coarse_tap_gather as ``pre`` [n, h, w, ld_pre >= cout].
 * Contract (prv2_conv2d_pre_supported(d) != 0): bf16 modes, 3x3 s1 p1, width >= 24, height >= 4, cout % 4 == 0 (the layers the
 * 16x16x32 halo kernels or the 256-column kernel run); a fused LayerNorm needs cout <= 128 or == 256. */
int prv2_conv2d_pre_supported(const prv2_conv_desc* d);
int prv2_conv2d_pre(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* pre, int32_t ld_pre,
                    const float* ln_weight, const float* ln_bias, const float* res, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * The 32-channel FULL-RESOLUTION tail of BiDirectionalFusion: two consecutive 3x3 convs with everything between and behind them in
 * ONE kernel (csrc/chain32.hip; 8 x 16-pixel tiles, the first conv's output stays in LDS; bf16x3 arithmetic):
 *   prv2_chain32_c2f   C2FModule ``output_conv2_fusion`` (GatedFusionBlock with one input, upscale=False) + ``output_conv3``
 *                      bi_directional_fusion_model.py:56-82,116-146 (unit / block), :171-180 (definitions), :203-204 (use)
 *        o     = conv3x3(relu(x); W1) + b1 + x                            GateresConfUnit2.conv + skip_add
 *        f     = relu(LN(conv3x3(o; W2) + b2 + pre))                      fusion_conv.0-.2 over cat([o, c_feat]); pre = its coarse half
 *        y     = Wo (o * sigmoid(Wg f + bg)) + bo                         fusion_conv.3, gate, out_conv         -> y  [n, h, w, 32]
 *        depth = w3 . y + b3                                              output_conv3 (1x1 -> 1)              -> depth [n, h, w]
 *   prv2_chain32_enc   ``fusion_layers_1[0]`` + ``fusion_layers_2[0]`` (SingleConvCNNLN)   bi_directional_fusion_model.py:424-431
 *        f = gelu(LN(conv3x3(x; W1) + b1 + pre))                          over cat([c, x]); pre = the coarse half (prv2_coarse_tap_gather)
 *        y = gelu(LN(conv3x3(cat([f, p1, p2]); W2) + b2))                 p1 / p2: dense [n, h, w] depth maps at the level's size
 * Weight images: prv2_pack_chain32_weight(w_src [32][cin_total][taps] fp32 PyTorch layout, kind) -> prv2_chain32_weight_bytes(kind, taps)
 *   kind 0: the FIRST conv (taps 9; input channels [0, 32) of w_src);  kind 1: the second conv (taps 9) and the 1x1 gate / out_conv
 *   (taps 1) -- K in accumulator order;  kind 2: the [p1 | p2] tail of a 3x3 over 34 channels (channels 32, 33 of w_src).
 *   prv2_chain32_c2f: w1 kind 0, w2 kind 1, wg / wo kind 1 (taps 1);  prv2_chain32_enc: w1 kind 0, w2 kind 1, wg = kind 2 of W2.
 * consts: device fp32 [9][32] = b1, LN1 weight, LN1 bias, b2, bg, bo, w3, LN2 weight, LN2 bias (rows a mode does not use: zeros);
 *   LN1 is the chain's FIRST LayerNorm (c2f: behind the second conv; enc: behind the first), LN2 enc's second.
 * Same split products / fp32 accumulation as prv2_conv2d's bf16x3 kernels; not bit-identical to the unfused sequence (LayerNorm sums
 * in another order; ``o`` enters the gate product as hi + lo, as ``mul`` does in prv2_conv3x3_ln_gate).
 * ------------------------------------------------------------------------------------------ */
typedef struct prv2_chain32_desc {
  const float* x;        /* NHWC input [n, h, w, ldx >= 32]                                */
  const void* w1;
  const void* w2;
  const void* wg;
  const void* wo;        /* c2f only                                                       */
  const float* consts;
  const float* pre;      /* [n, h, w, ld_pre >= 32] (c2f: may be NULL)                     */
  const float* p1;       /* enc only                                                       */
  const float* p2;
  float* y;              /* NHWC output [n, h, w, ldy >= 32] (a channel slice is fine)     */
  float* depth;          /* c2f only (may be NULL)                                         */
  int64_t x_bstride;     /* image strides in floats (0 => h*w*ld)                          */
  int64_t y_bstride;
  int32_t n, h, w;
  int32_t ldx, ldy, ld_pre;
  float b3, ln_eps;
} prv2_chain32_desc;
int64_t prv2_chain32_weight_bytes(int32_t kind, int32_t taps);
int prv2_pack_chain32_weight(const float* w_src, int32_t cin_total, int32_t taps, int32_t kind, void* w_packed, void* stream);
int prv2_chain32_c2f(const prv2_chain32_desc* d, void* stream);
int prv2_chain32_enc(const prv2_chain32_desc* d, void* stream);

/* The 256-channel 3x3 conv of a GatedConvUnit / ResidualConvUnit in the fp16 + block-scaled-fp6 arithmetic (csrc/conv3x3_f6.hip;
 * PRV2_PREC_F16F6) -- estimator/models/blocks/bi_directional_fusion_model.py:40-43 (self.conv = ReLU, Conv2d 3x3), :58-64 (out =
 * self.conv(x) + x); the same layer prv2_conv2d runs in bf16x3 on conv3x3_c256_kernel:
 *     y[n, h, w, 0 .. 256) = out_scale * conv3x3(q(relu?(x) * x_scale); q(W * w_scale)) + bias + res        (fp32 NHWC, or X2 with d->fmt = PRV2_FMT_Y_X2)
 * where each product x w is taken as f16(x) f16(w) + q6(x) q6(w - f16 w) + q6(x - f16 x) q6(w), q6 = fp6 e2m3 with one power-of-two
 * scale per 32 channels, fp32 accumulation: two v_mfma_f32_16x16x32_f16 and one v_mfma_scale_f32_16x16x128_f8f6f4 per 64 channels and tap
 * instead of six bf16 MFMAs.  rms error of a dot product against float64 1.2e-5 (bf16x3: 4.4e-6) -- fp32-grade, wider than TF32.
 * x_scale / w_scale: powers of two chosen by the caller so that |relu(x) x_scale| and |W w_scale| stay inside fp16's range (values
 * beyond 65504 are clamped in the fp16 part and carried by the fp6 residual: finite, imprecise); out_scale = 1 / (x_scale w_scale).
 * range_word (device, or NULL): receives atomicMax of the float bits of max |relu(x) x_scale| the launch saw -- the caller's range monitor.
 * Contract (prv2_conv3x3_f6_supported(d) != 0): 3x3 s1 p1, cout = 256, cin % 64 == 0, width >= 16, d->act = NONE, no LayerNorm / gate /
 * mul; d->relu_in and d->ld_res as for prv2_conv2d.  w_packed: prv2_pack_conv3x3_f6_weight (PyTorch [256][cin][3][3] fp32). */
int prv2_conv3x3_f6_supported(const prv2_conv_desc* d);
int64_t prv2_conv3x3_f6_weight_bytes(int32_t cout, int32_t cin);
int prv2_pack_conv3x3_f6_weight(const float* w_src, float w_scale, void* w_packed, int32_t cout, int32_t cin, void* stream);
int prv2_conv3x3_f6(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* res, float x_scale,
                    float out_scale, uint32_t* range_word, float* y, void* stream);
/* The GatedConvUnit tail with its 3x3 conv in the same fp16 + fp6 arithmetic (csrc/conv3x3_f6.hip: conv3x3_c256_gate_f6_kernel) -- what
 * prv2_conv3x3_ln_gate_pre computes on conv3x3_c256_gate_x2_kernel (bi_directional_fusion_model.py:44-51, 70-80):
 *     y = mul * sigmoid(conv1x1(act(LN(out_scale * conv3x3(q(x * x_scale); q(W * w_scale)) + bias + pre))) + gate_bias) (+ res)
 * The LayerNorm, the 256 x 256 gate GEMM (bf16x3) and the final stage are conv3x3_gate.hip's epilogue, unchanged (csrc/conv3x3_gate_epi.h).
 * Contract: prv2_conv3x3_f6_supported(d); x and mul in ONE format -- pre-split (d->fmt = PRV2_FMT_X_X2 | PRV2_FMT_MUL_X2: the unit's ``out`` / its X2 concat) or
 * fp32 (d->fmt = 0: the [out | coarse ROI] concat of the configs whose ROI gather resizes, mul = its first half) --, no input ReLU, fp32 y;
 * ln_weight / ln_bias / gate_w_packed (prv2_pack_gate_weight) required; pre (or NULL) as for prv2_conv3x3_ln_gate_pre; w_packed:
 * prv2_pack_conv3x3_f6_weight of the conv's weights over what x holds (the fine half W[:, :256] with ``pre``, all 512 input channels of the concat form). */
int prv2_conv3x3_ln_gate_f6(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const float* pre, int32_t ld_pre,
                            const float* ln_weight, const float* ln_bias, const void* gate_w_packed, const float* gate_bias, const float* mul,
                            const float* res, float x_scale, float out_scale, uint32_t* range_word, float* y, void* stream);

/* prv2_conv3x3_ln_gate_pre / prv2_conv3x3_ln_gate_f6 with the addend GATHERED INSIDE the kernel: instead of ``pre`` they take the tables
 * prv2_coarse_tap_gather would have read (v, g of prv2_coarse_tap_knots[_frames] for cout = 256 channels) and the tiles' boxes, and the
 * epilogue of the 256-column gate kernels runs the gather's column walk (csrc/coarse_taps_walk.h) for its 8 x 16 pixels -- the addend is
 * never written to or read from HBM.  Image i of the conv is tile i of ``boxes`` ([d->n, 4] (x1, y1, x2, y2), or [d->n, 5] with the frame
 * index in front when n_frames >= 1; n_frames = 0: single-frame tables), gathered at the conv's own d->h x d->w.  Bit-identical to the
 * same call with pre = prv2_coarse_tap_gather[_frames](...).  Contract: that of the entry point it stands for, with gate weights,
 * d->cout = 256 (prv2_conv3x3_ln_gate_taps_supported(d) != 0); the tables' contract is prv2_coarse_tap_gather's.  (Additive: the ABI stays at 20.) */
typedef struct prv2_tap_tables {
  const float* v;        /* [B, 3h, 3w, ldv] knots (prv2_coarse_tap_knots)                 */
  const float* g;        /* [B, h, w, ldg >= 9 * 256] tap-major                            */
  const float* boxes;    /* device fp32 [d->n, 4 or 5]                                     */
  int32_t n_frames;      /* 0: single-frame tables and 4-column boxes                      */
  int32_t h, w;          /* coarse size                                                    */
  int32_t ldv, ldg;
  float knot_bh, knot_bw;
  float spatial_scale;
} prv2_tap_tables;
int prv2_conv3x3_ln_gate_taps_supported(const prv2_conv_desc* d);
int prv2_conv3x3_ln_gate_taps(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const prv2_tap_tables* taps,
                              const float* ln_weight, const float* ln_bias, const void* gate_w_packed, const float* gate_bias,
                              const float* mul, const float* res, float* y, void* stream);
int prv2_conv3x3_ln_gate_f6_taps(const prv2_conv_desc* d, const float* x, const void* w_packed, const float* bias, const prv2_tap_tables* taps,
                                 const float* ln_weight, const float* ln_bias, const void* gate_w_packed, const float* gate_bias,
                                 const float* mul, const float* res, float x_scale, float out_scale, uint32_t* range_word, float* y,
                                 void* stream);

/* Convolution with ONE output channel (direct, HBM-bound):
 *   final_conv 3x3 -> 1 + clamp(update_base + offset, 0)   bi_directional_fusion_model.py:438-442, fusion_model.py:113-118
 *   output_conv2.2 1x1 32->1 + Sigmoid * max_depth          external/depth_anything_v2/dpt.py:111-113,190
 *   output_conv3 1x1 32->1                                   bi_directional_fusion_model.py:178-179
 * w: device fp32 PyTorch layout [1][cin][k][k].  y = post( act(conv + bias) * scale + res ), post = max(.,0) if clamp0.
 * y / res are dense [n, h, w] (ld 1). */
int prv2_conv2d_cout1(const float* x, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t ldx, const float* wgt,
                      int32_t k, const float* bias, int32_t act, float scale, const float* res, int32_t clamp0,
                      float* y, void* stream);

/* Depthwise kxk convolution, k in {3, 5, 7}, pad k/2 (+folded BatchNorm bias, optional ReLU) for the refiner encoders
 * (timm, un-vendored; lightweight_refiner.py:260-262,296): MobileNetV4 (3x3 / 5x5) and ConvNeXt (7x7, conv_dw).
 * w: device, TAP-MAJOR [k*k][c] with the BN scale already folded (so that a lane's 4 channels are one float4); bias [c]. */
int prv2_dwconv2d(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ldx, const float* wgt,
                  const float* bias, int32_t k, int32_t stride, int32_t relu, float* y, int32_t ldy, void* stream);
/* The same with any enum prv2_act and, when same_pad != 0, TensorFlow "SAME" padding (see prv2_conv_desc.same_pad):
 * the depthwise convs of timm's tf_efficientnet_* (Conv2dSame; v2_eff_u4k.py:94).  Output ceil(h/stride) x ceil(w/stride). */
int prv2_dwconv2d_ex(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ldx, const float* wgt,
                     const float* bias, int32_t k, int32_t stride, int32_t act, int32_t same_pad, float* y, int32_t ldy,
                     void* stream);

/* Squeeze-and-excitation pieces of the EfficientNet refiner encoder (timm SqueezeExcite, un-vendored):
 *   prv2_global_avgpool: out[n][c] = mean over the h*w pixels of image n (x.mean((2, 3)));  out is dense [n][c];
 *                        workspace: prv2_global_avgpool_workspace_floats(n, hw, c) floats (partial sums of the two-stage,
 *                        fixed-order -- run-to-run deterministic -- reduction).
 *   prv2_se_gate:        g[n][:] = sigmoid(W2 silu(W1 mean[n][:] + b1) + b2), the conv_reduce / conv_expand bottleneck in fp32;
 *                        w1 [cse][c] (PyTorch layout), w2t [cse][c] = conv_expand's weight TRANSPOSED, biases optional,
 *                        workspace n*cse floats.
 *   prv2_channel_scale:  x[n, pix, c] *= s[n][c]  in place (x * gate). */
int64_t prv2_global_avgpool_workspace_floats(int32_t n, int64_t hw, int32_t c);
int prv2_global_avgpool(const float* x, int32_t n, int64_t hw, int32_t c, int32_t ldx, float* out, float* workspace, void* stream);
int prv2_se_gate(const float* mean, int32_t n, int32_t c, const float* w1, const float* b1, int32_t cse, const float* w2t,
                 const float* b2, float* g, float* workspace, void* stream);
int prv2_channel_scale(float* x, int32_t n, int64_t hw, int32_t c, int32_t ldx, const float* s, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row LayerNorm (+activation).  Rows of ``c`` contiguous floats with strides ldx / ldy.
 * Replaces nn.LayerNorm(eps=1e-6) on tokens (dinov2.py:95, block.py:56,68) and -- because the
 * activations are NHWC -- the channels-first LayerNorm of the fusion convs (convs.py:21-29)
 * including the GELU / ReLU that follows it (convs.py:70-72, bi_directional_fusion_model.py:49-50).
 * ------------------------------------------------------------------------------------------ */
int prv2_layernorm(const float* x, int64_t rows, int32_t c, int32_t ldx, const float* weight, const float* bias,
                   float eps, int32_t act, float* y, int32_t ldy, void* stream);

/* ------------------------------------------------------------------------------------------
 * ViT token plumbing (external/depth_anything_v2/dinov2.py:212-231, patch_embed.py:69-82)
 * ------------------------------------------------------------------------------------------ */
/* img NHWC [b, gh*p, gw*p, 3] (ld 3..) -> rows [b*gh*gw, ldo] with (ky, kx, c) column order, zero padded to ldo */
int prv2_patchify(const float* img, int32_t b, int32_t gh, int32_t gw, int32_t p, int32_t ldi, float* rows,
                  int32_t ldo, void* stream);
/* tokens[b, 0] = cls + pos[0]; tokens[b, 1+i] = emb[b, i] + pos[1+i] */
int prv2_assemble_tokens(const float* emb, const float* cls, const float* pos, int32_t b, int32_t np, int32_t dim,
                         float* tokens, void* stream);
/* softmax((q*scale) k^T) v per (batch, head); qkv rows are [3][heads][hd] as produced by the qkv
 * Linear (attention.py:49-62).  hd must be 64.  out rows are [heads][hd]. */
int prv2_attention(const float* qkv, int32_t b, int32_t ntok, int32_t heads, int32_t hd, float* out, int32_t prec,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* The same with an additive score bias shared by the batch: softmax((q*scale) k^T + bias[head]) v -- the relative position
 * bias of the MiDaS BEiT blocks (torch.hub MiDaS midas/backbones/beit.py attention_forward; called by
 * external/zoedepth/models/base_models/midas.py:267).  bias: [heads][ntok][ld_bias] fp32, ld_bias >= roundup(ntok, 64),
 * a multiple of 4, rows 16-byte aligned (pad keys are never read past ntok's 64-key tile and are masked).  bias == NULL: no bias. */
/* The bias of a (model, resolution) is a constant: prv2_pack_attention_bias re-orders its rows once into the image the bf16x3 kernel
 * reads with coalesced loads (per head, block of 32 queries and tile of 64 keys: the values in accumulator order, pre-multiplied by
 * log2 e -- the product the kernel otherwise forms per tile; same bits).  Passed to prv2_attention_bias / prv2_attention_ss as
 * ``bias`` with ld_bias == PRV2_ATTENTION_BIAS_IMAGE (bf16 modes). */
#define PRV2_ATTENTION_BIAS_IMAGE (-1)
int64_t prv2_attention_bias_image_bytes(int32_t heads, int32_t ntok);
int prv2_pack_attention_bias(const float* bias, int32_t heads, int32_t ntok, int32_t ld_bias, float* image, void* stream);
int prv2_attention_bias(const float* qkv, int32_t b, int32_t ntok, int32_t heads, int32_t hd, const float* bias, int32_t ld_bias,
                        float* out, int32_t prec, void* workspace, int64_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * Split-swizzled ("ss") operand format and the dense layers that consume it (csrc/gemm_ss.hip) -- the ViT blocks'
 * Linear layers (attention.py:44,46; mlp.py:30,32) at large token counts, PRV2_PREC_BF16X3 only.
 * A row of C channels (C % 32 == 0) occupies 4*C bytes like fp32: per 32 channels one 128-byte group of eight 16-byte
 * slots, logical slot s = 0..3: bf16 hi of channels 8s..8s+7, s = 4..7: bf16 lo of channels 8(s-4)..; stored at
 * slot s ^ ((row >> 1) & 7) (the image prv2_pack_conv_weight gives the weights).  Producers write it directly:
 *   prv2_split_ss      fp32 rows -> ss rows
 *   prv2_layernorm_ss  prv2_layernorm with an ss output (no activation)
 *   prv2_attention_ss  prv2_attention_bias (bf16x3) with an ss output
 *   prv2_gemm_ss       y = epilogue(A_ss W^T): t = act(acc + bias[n]); t *= gamma[n]; t += res[m, n]; fp32 rows (y) or ss rows
 *                      (y_ss; then no gamma / res).  w_packed: prv2_pack_conv_weight(.., kh = kw = 1, PRV2_PREC_BF16X3).
 * prv2_gemm_ss is bit-identical to prv2_conv2d's 1x1 path on the same values (same split, products, order, epilogue).
 * ------------------------------------------------------------------------------------------ */
int prv2_split_ss(const float* x, int64_t rows, int32_t c, int32_t ldx, void* y_ss, void* stream);
int prv2_layernorm_ss(const float* x, int64_t rows, int32_t c, int32_t ldx, const float* weight, const float* bias, float eps,
                      void* y_ss, void* stream);
int prv2_attention_ss(const float* qkv, int32_t b, int32_t ntok, int32_t heads, int32_t hd, const float* bias, int32_t ld_bias,
                      void* out_ss, void* workspace, int64_t workspace_bytes, void* stream);
int prv2_gemm_ss(const void* a_ss, int64_t m, int32_t k, const void* w_packed, int32_t n, const float* bias, const float* gamma,
                 const float* res, int32_t ld_res, int32_t act, float* y, int32_t ldy, void* y_ss, void* stream);
/* The attention block without a pre-pass (attention.py:49-62; MiDaS beit.py attention_forward): the qkv Linear writes its [q | k | v] rows
 * split-swizzled with the q third (columns [0, q_cols)) multiplied by q_scale = hd^-0.5 log2 e behind the bias, and prv2_attention_qkv_ss reads
 * those rows directly (q / k fragments are 16-byte copies; v is transposed by the LDS read).  Same values as prv2_gemm_ss (fp32 rows) ->
 * prv2_attention_ss, bit for bit; no workspace, no fp32 qkv tensor.  Exactly one of out (fp32 rows [b * ntok, heads * hd]) / out_ss. */
int prv2_gemm_ss_qkv(const void* a_ss, int64_t m, int32_t k, const void* w_packed, int32_t n, const float* bias, int32_t q_cols, float q_scale,
                     void* qkv_ss, void* stream);
int prv2_attention_qkv_ss(const void* qkv_ss, int32_t b, int32_t ntok, int32_t heads, int32_t hd, const float* bias, int32_t ld_bias, float* out,
                          void* out_ss, void* stream);

/* device scratch the split-bf16 attention needs (pre-split q/k rows + transposed v planes); 0 for PRV2_PREC_F32.
 * The workspace must be 256-byte aligned; its contents are dead when the call returns (stream order). */
int64_t prv2_attention_workspace_bytes(int32_t b, int32_t ntok, int32_t heads, int32_t prec);

/* ------------------------------------------------------------------------------------------
 * ZoeDepth metric-bins head, elementwise parts (the 1x1 MLPs go through prv2_conv2d)
 * ------------------------------------------------------------------------------------------ */
/* y = a + b over [rows, c] with row strides (x + prev_b_embedding, external/zoedepth/models/layers/attractor.py:178) */
int prv2_add(const float* a, int32_t lda, const float* b, int32_t ldb, int64_t rows, int32_t c, float* y, int32_t ldy,
             void* stream);

/* Zero the pad channels [c, ld) of every pixel of an NHWC buffer (rows = n*h*w).  Buffers whose channel count is
 * not a multiple of 4 (the [feat | pred1 | pred2] concats of fusion_model.py:91-118: 34, 66, 98 ...) carry pad
 * channels up to ld; the conv loaders read them against zero weights, so they must be finite. */
int prv2_zero_pad_channels(float* y, int64_t rows, int32_t c, int32_t ld, void* stream);
/* AttractorLayerUnnormed, kind='mean', type='inv' (attractor.py:45-57,186-206):
 *   out[r, j] = bins[r, j] + mean_i( dx / (1 + alpha * dx^2) ),  dx = attr[r, i] - bins[r, j]               */
int prv2_zoe_attractor(const float* attr, int32_t ld_attr, int32_t n_attr, const float* bins, int32_t ld_bins,
                       int32_t n_bins, float alpha, int64_t rows, float* out, int32_t ld_out, void* stream);
/* ConditionalLogBinomial tail + expectation (dist_layers.py:29-69,100-116; zoedepth_v1.py:219):
 *   pt[r, 0..3] = softplus MLP output; p = (pt0+eps)/(pt0+pt1+2eps); t = (max-min)*(pt2+eps)/(pt2+pt3+2eps)+min;
 *   depth[r] = sum_k softmax_k( (logC(K-1,k) + k log p + (K-1-k) log(1-p)) / t ) * centers[r, k]                */
int prv2_zoe_logbinom_depth(const float* pt, int32_t ld_pt, const float* centers, int32_t ld_c, int32_t n_bins,
                            float min_temp, float max_temp, int64_t rows, float* depth, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gathers
 * ------------------------------------------------------------------------------------------ */
/* Input stage of the image dataset (estimator/datasets/general_dataset.py:22-62, generic branch): RGB image, HWC, uint8
 * (src_is_u8) or fp32, device memory -> v / 255 (uint8 only) -> F.interpolate(mode='bicubic', align_corners=True) to H x W ->
 * CHW fp32 image_hr.  Evaluated in float64 like the reference (its cv2-image / 255.0 is a float64 array), rounded once. */
int prv2_bicubic_resize(const void* src_hwc, int32_t src_is_u8, int32_t h, int32_t w, float* dst_chw, int32_t H, int32_t W,
                        void* stream);

/* Crop + bilinear(align_corners=True) resize of K tiles of a CHW image into NHWC patches, with the
 * (v - mean[c]) / std[c] input normalisation fused.
 *   baseline_pretrain.py:169-170,274-275 -> external/depth_anything/transform.py:127-129 (ResizeDA)
 *   or external/zoedepth/models/base_models/midas.py:171-174 (ResizeZoe); dpt.py:183; lightweight_refiner.py:293.
 * tiles: device int32 [k][2] = (h_start, w_start); crop size ch x cw; output [k, oh, ow, ldo] channels 0..2. */
int prv2_crop_resize(const float* img_chw, int32_t img_h, int32_t img_w, const int32_t* tiles, int32_t k, int32_t ch,
                     int32_t cw, int32_t oh, int32_t ow, const float* mean3_host, const float* std3_host, float* out,
                     int32_t ldo, void* stream);

/* torchvision.ops.roi_align(feat.repeat(K), boxes, (oh, ow), spatial_scale, sampling_ratio=-1, aligned=True)
 * without materialising the K copies (patchrefinerplus.py:263-276, patchrefiner.py:199-210).
 * feat NHWC [1, h, w, c]; boxes device fp32 [k][4] = (x1, y1, x2, y2) in lr-frame pixels. */
int prv2_roi_align(const float* feat, int32_t h, int32_t w, int32_t c, int32_t ldf, const float* boxes, int32_t k,
                   float spatial_scale, int32_t oh, int32_t ow, float* out, int32_t ldo, void* stream);

/* prv2_roi_align writing the pre-split "X2" format of prv2_conv_desc.fmt (c % 8 == 0): the coarse half of a GatedConvUnit's concat
 * buffer, whose only consumer is the gate kernel.  Same arithmetic; out[...] = X2(roi value). */
int prv2_roi_align_x2(const float* feat, int32_t h, int32_t w, int32_t c, int32_t ldf, const float* boxes, int32_t k,
                      float spatial_scale, int32_t oh, int32_t ow, float* out, int32_t ldo, void* stream);

/* The coarse half of a ``cat([fine, coarse_roi])`` 3x3 convolution, once per frame at coarse resolution (csrc/coarse_taps.hip):
 *   GatedConvUnit.forward        bi_directional_fusion_model.py:70-73    fusion_conv.0(cat([out, c_feat]))    (no activation in front)
 *   BiDirectionalFusion.forward  bi_directional_fusion_model.py:424-426  fusion_layers_1[l](cat([c, f]))
 *   with c_feat = roi_align(feat.repeat(K), boxes, (h, w), h / P) of the per-frame pyramid level (patchrefinerplus.py:263-283).
 * The conv is linear and its coarse input is a bilinear zoom of ``feat``, so
 *     conv3x3(c_feat; W_c)(p) = sum_tap [p + d_tap inside the tile] Bil(G_tap; s(p + d_tap)),   G_tap = W_c[:, :, tap] . feat
 * (s = roi_align's sample position, Bil = its clamped bilinear sample).  G is a 1x1 GEMM at COARSE resolution (prv2_conv2d with the
 * weights [tap * c + co][ci]); the reference spends 9 * cin * cout MACs per output pixel of each of the frame's tiles on it.
 *
 * prv2_coarse_tap_knots: tiles of one frame share their size, i.e. consecutive output pixels are knot_b = tile / frame (per axis,
 *   <= 1/2) apart in coarse coordinates; U(y, x) = sum_tap Bil(G_tap; y + dy knot_bh, x + dx knot_bw) is then piecewise bilinear on
 *   the knot grid {k - b, k, k + b} and this call tabulates it there: g [h, w, ldg] (channel tap * c + co) -> v [3h, 3w, ldv].
 * prv2_coarse_tap_gather: out[k, i, j, :] = U(s(i, j)) - the taps the zero padding hides on the tile's border pixels (sampled from
 *   g): the pre-LayerNorm addend of prv2_conv3x3_ln_gate_pre / the pre-activation addend of the level's fusion conv.  A 4-tap
 *   gather, like the prv2_roi_align of c_feat it replaces.  boxes / spatial_scale as prv2_roi_align; every box must lie inside the
 *   frame and yield one sample per bin (roi extent <= output size).  Exact algebra; rounding differs from the reference's order by
 *   ~1e-7 relative. */
int prv2_coarse_tap_knots(const float* g, int32_t h, int32_t w, int32_t c, int32_t ldg, float knot_bh, float knot_bw, float* v,
                          int32_t ldv, void* stream);
int prv2_coarse_tap_gather(const float* v, const float* g, int32_t h, int32_t w, int32_t c, int32_t ldv, int32_t ldg, float knot_bh,
                           float knot_bw, const float* boxes, int32_t k, float spatial_scale, int32_t oh, int32_t ow, float* out,
                           int32_t ldo, void* stream);

/* F.interpolate(mode='bilinear', align_corners=True) on NHWC (every decoder upsample; Appendix C row 1) */
int prv2_upsample_bilinear(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ldx, int32_t oh,
                           int32_t ow, float* y, int32_t ldy, void* stream);

/* The two depth maps every fusion level appends to its features ([feat | pred1 | pred2], fusion_model.py:91-118,
 * bi_directional_fusion_model.py:424-436): p1, p2 dense [n, h, w], resized bilinear(align_corners=True) to oh x ow and written
 * as y[pixel][0..3] = (p1, p2, 0, 0) -- y points at the first of the buffer's last four channels (the two maps and the two
 * pad channels), 16-byte aligned, pixel stride ldy.  Same arithmetic per map as prv2_upsample_bilinear. */
int prv2_depth_pair_fill(const float* p1, const float* p2, int32_t n, int32_t h, int32_t w, int32_t oh, int32_t ow, float* y,
                         int32_t ldy, void* stream);

/* Border correction of a 3x3 / pad 1 conv whose bias was folded from an upstream constant: GatedFusionBlock's ``out_conv`` (1x1, bias b)
 * followed by the bilinear x2 and ``output_conv1`` (3x3, W) is ONE 3x3 conv with weights W o out_conv and bias + sum_taps W_tap b
 * (bi_directional_fusion_model.py:139-142,201: a 1x1 commutes with the interpolation, whose weights sum to one) -- except that at
 * the image border the zero padding hides some taps from b.  y[n, oy, ox, :c] -= sum of tap_bias[tap][:] over the taps of (oy, ox)
 * that fall outside the image; tap_bias: [9][c] (ky, kx order), c % 4 == 0. */
int prv2_conv_border_bias(float* y, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ldy, const float* tap_bias, void* stream);

/* NCHW <-> NHWC layout changes at the boundary (image_lr in, coarse_prediction out) */
int prv2_nchw_to_nhwc(const float* x, int32_t n, int32_t c, int32_t h, int32_t w, float* y, int32_t ldy, void* stream);
int prv2_nhwc_to_nchw(const float* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t ldx, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Overlap blend = RunningAverageMap kept on the device (estimator/models/utils.py:22-49,
 * paste/update loops baseline_pretrain.py:212-229, 347-373).
 * avg / cnt: dense [H, W] maps.  pred: [k, ph, pw] patch predictions.  mask: [th, tw] blend weights.
 * tiles: device int32 [k][2] = (h_start, w_start) in map coordinates; tile size th x tw.
 * When (ph, pw) != (th, tw) the prediction is upsampled with legacy 'nearest' (baseline_pretrain.py:210).
 * Tiles are applied in order k = 0..K-1 (the running mean is order dependent).
 * ------------------------------------------------------------------------------------------ */
int prv2_blend_paste(float* avg, float* cnt, int32_t map_h, int32_t map_w, const float* pred, int32_t ph, int32_t pw,
                     const float* mask, const int32_t* tiles, int32_t k, int32_t th, int32_t tw, void* stream);
int prv2_blend_update(float* avg, float* cnt, int32_t map_h, int32_t map_w, const float* pred, int32_t ph,
                      int32_t pw, const float* mask, const int32_t* tiles, int32_t k, int32_t th, int32_t tw,
                      void* stream);
/* RunningAverageMap.resize: avg -> nearest, cnt -> bilinear(align_corners=True) (utils.py:38-43) */
int prv2_blend_resize(const float* avg, const float* cnt, int32_t h, int32_t w, float* avg_out, float* cnt_out,
                      int32_t oh, int32_t ow, void* stream);

/* ------------------------------------------------------------------------------------------
 * Frames (ABI 20): B frames per call.  Each entry point below is the B-frame form of the entry point of the same name without
 * ``_frames`` -- the same kernel, same arithmetic per tile, bit-identical to calling the single-frame form on each frame.
 * n_frames = B >= 1.  Per-frame inputs are dense and frame-major: images [B, 3, H, W], feature maps / tap tables [B, h, w, ld].
 * A tile names its frame in its first column: tiles int32 [k][3] = (frame, h_start, w_start), boxes fp32 [k][5] =
 * (frame, x1, y1, x2, y2) (torchvision's roi_align format).  Frame indices live on the device and are clamped to [0, B) there.
 * ------------------------------------------------------------------------------------------ */
int prv2_crop_resize_frames(const float* img_bchw, int32_t n_frames, int32_t img_h, int32_t img_w, const int32_t* tiles, int32_t k,
                            int32_t ch, int32_t cw, int32_t oh, int32_t ow, const float* mean3_host, const float* std3_host, float* out,
                            int32_t ldo, void* stream);
int prv2_roi_align_frames(const float* feat, int32_t n_frames, int32_t h, int32_t w, int32_t c, int32_t ldf, const float* boxes, int32_t k,
                          float spatial_scale, int32_t oh, int32_t ow, float* out, int32_t ldo, void* stream);
int prv2_roi_align_x2_frames(const float* feat, int32_t n_frames, int32_t h, int32_t w, int32_t c, int32_t ldf, const float* boxes, int32_t k,
                             float spatial_scale, int32_t oh, int32_t ow, float* out, int32_t ldo, void* stream);
/* g [B, h, w, ldg] -> v [B, 3h, 3w, ldv] in one launch; the gather reads each box's own frame of v and g */
int prv2_coarse_tap_knots_frames(const float* g, int32_t n_frames, int32_t h, int32_t w, int32_t c, int32_t ldg, float knot_bh, float knot_bw,
                                 float* v, int32_t ldv, void* stream);
int prv2_coarse_tap_gather_frames(const float* v, const float* g, int32_t n_frames, int32_t h, int32_t w, int32_t c, int32_t ldv, int32_t ldg,
                                  float knot_bh, float knot_bw, const float* boxes, int32_t k, float spatial_scale, int32_t oh, int32_t ow,
                                  float* out, int32_t ldo, void* stream);
/* One pass step of the overlap blend for B maps avg / cnt [B, map_h, map_w] in one launch.  Frame f's k tiles are
 * tiles[f * tile_fstride .. + k) (rows of 2: (h_start, w_start)) and its predictions start at pred + f * pred_fstride
 * ([k, ph, pw] each; tile_fstride >= k, pred_fstride >= k * ph * pw: frames do not overlap).  Within a frame the tiles are
 * applied in order, as prv2_blend_paste / prv2_blend_update. */
int prv2_blend_paste_frames(float* avg, float* cnt, int32_t n_frames, int32_t map_h, int32_t map_w, const float* pred, int32_t ph, int32_t pw,
                            int64_t pred_fstride, const float* mask, const int32_t* tiles, int32_t tile_fstride, int32_t k, int32_t th,
                            int32_t tw, void* stream);
int prv2_blend_update_frames(float* avg, float* cnt, int32_t n_frames, int32_t map_h, int32_t map_w, const float* pred, int32_t ph, int32_t pw,
                             int64_t pred_fstride, const float* mask, const int32_t* tiles, int32_t tile_fstride, int32_t k, int32_t th,
                             int32_t tw, void* stream);
/* RunningAverageMap.resize of B maps [B, h, w] -> [B, oh, ow] in one launch */
int prv2_blend_resize_frames(const float* avg, const float* cnt, int32_t n_frames, int32_t h, int32_t w, float* avg_out, float* cnt_out,
                             int32_t oh, int32_t ow, void* stream);

/* ------------------------------------------------------------------------------------------
 * Overlap statistics: the blend of B >= 1 frames (arguments, frame strides and checks as the *_frames entry points; B = 1 is
 * n_frames = 1) with two more maps per frame, m2 / ntiles [B, map_h, map_w]:
 *   m2     weighted sum of squared deviations of the covering tiles' predictions from the running mean;
 *   ntiles number of tiles whose footprint covers the pixel (an exact integer, stored as float).
 * paste: avg = p, cnt = ct, m2 = 0, ntiles = 1.  update, for every covering tile in order: ntiles += 1; when ct > 0,
 * d = p - avg, avg and cnt as prv2_blend_update, m2 += ct * d * (p - avg_new) (computed as its exact equal
 * (cnt ct / (cnt + ct)) d^2, free of cancellation).  avg / cnt are bit-identical to the entry points without statistics.
 * m2 / ntiles are read and written only where a tile of the call lies.
 * The weighted standard deviation of the overlapping predictions is sqrt(max(m2, 0) / cnt) where cnt > 0.
 * ------------------------------------------------------------------------------------------ */
int prv2_blend_paste_stats(float* avg, float* cnt, float* m2, float* ntiles, int32_t n_frames, int32_t map_h, int32_t map_w, const float* pred,
                           int32_t ph, int32_t pw, int64_t pred_fstride, const float* mask, const int32_t* tiles, int32_t tile_fstride,
                           int32_t k, int32_t th, int32_t tw, void* stream);
int prv2_blend_update_stats(float* avg, float* cnt, float* m2, float* ntiles, int32_t n_frames, int32_t map_h, int32_t map_w, const float* pred,
                            int32_t ph, int32_t pw, int64_t pred_fstride, const float* mask, const int32_t* tiles, int32_t tile_fstride,
                            int32_t k, int32_t th, int32_t tw, void* stream);
/* prv2_blend_resize_frames plus: ntiles -> nearest; m2_out = v[nearest] * cnt_out with v = m2 / cnt where cnt > 0 and 0 elsewhere
 * (the variance is kept and rescaled to the resampled weight) */
int prv2_blend_resize_stats(const float* avg, const float* cnt, const float* m2, const float* ntiles, int32_t n_frames, int32_t h, int32_t w,
                            float* avg_out, float* cnt_out, float* m2_out, float* ntiles_out, int32_t oh, int32_t ow, void* stream);


/* ------------------------------------------------------------------------------------------
 * Edge-aware evaluation (csrc/edges.hip): Canny edges of depth maps and the boundary metrics, B >= 1 frames [n, h, w] per call
 * (frame-major, dense; h, w >= 3; n * h * w < 2^31).  Edge / mask maps are uint8 0/1 (a torch bool tensor is one).  Every entry
 * point but prv2_binary_dilate takes a caller workspace of at least prv2_edges_workspace_bytes(n, h, w) bytes (device memory);
 * the launch count of each call is fixed (no host loop, no readback: graph-capture safe).
 * ------------------------------------------------------------------------------------------ */
enum prv2_edge_pre { PRV2_EDGE_PRE_NONE = 0, PRV2_EDGE_PRE_LOG = 1, PRV2_EDGE_PRE_INV = 2 };

/* bytes of workspace the edge entry points need for n frames of h x w (-1 for a bad shape) */
int64_t prv2_edges_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* extract_edges' depth preprocessing (estimator/utils/metric.py:157-207; to_log :155-159, to_inv :161-165), fp32 -> fp32:
 *   PRV2_EDGE_PRE_LOG   (d > 0) * log(max(d, eps_f32))
 *   PRV2_EDGE_PRE_INV   (d > 0) / max(d, eps_f32), then -= min(frame), then /= max(frame) (deterministic device reductions)
 *   PRV2_EDGE_PRE_NONE  log((d > 0) * max(d, eps_f32)) / log(1.5f)
 * NaN propagates as in torch (clamp keeps it, min / max return it). */
int prv2_depth_preprocess(const float* depth, int32_t n, int32_t h, int32_t w, int32_t mode, float* out, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* skimage.feature.canny(image, sigma) as metrics.canny restates it (metric.py:203, tester.py:99-106): bit-identical to it on the
 * same fp32 input.  gauss_w_host: HOST array of radius + 1 float64 Gaussian taps, centre first (scipy's _gaussian_kernel1d,
 * radius = int(4 sigma + 0.5) <= 15); mode='constant' Gaussian with the bleed correction, reflect Sobel, 4-sector non-maximum
 * suppression, hysteresis over 8-connected components.  edges: uint8 [n, h, w]. */
int prv2_canny(const float* image, int32_t n, int32_t h, int32_t w, const double* gauss_w_host, int32_t radius, float low_threshold,
               float high_threshold, uint8_t* edges, void* workspace, int64_t workspace_bytes, void* stream);

/* exact squared Euclidean distance of every pixel to the nearest set pixel of its frame (int32; INT32_MAX in a frame with no set
 * pixel).  sqrt in float64 == scipy.ndimage.distance_transform_edt(~mask) (metric.py:225-229).  w <= 5120, h + w <= 32768. */
int prv2_edt_sq(const uint8_t* mask, int32_t n, int32_t h, int32_t w, int32_t* d2, void* workspace, int64_t workspace_bytes, void* stream);

/* k x k binary dilation with zero padding, k in {3, 5, 7}: kornia.filters.gaussian_blur2d(m, (k, k), sigma, 'reflect') > 0
 * (metric.py:252-263 k = 5; scannet_dataset.py:221-224 k = 7; tester.py:99-106 k = 3) */
int prv2_binary_dilate(const uint8_t* mask, int32_t n, int32_t h, int32_t w, int32_t k, uint8_t* out, void* stream);

/* the statistics of compute_boundary_metrics (metric.py:210-272) per frame, stats: DEVICE float64 [n, 8] =
 *   TP, FP, FN, TN   of the dilated maps gt_ext / pred_ext at the valid pixels,
 *   n_bde            #(pred & valid & sqrt(d2_target) < th_edges_acc),   n_gt    #(gt & valid),
 *   sum_acc          sum of sqrt(d2_target) over the bde set,             sum_comp  sum of sqrt(d2_pred) over gt & valid.
 * d2_* come from prv2_edt_sq of the unmasked maps (INT32_MAX -> scipy's distance to (-1, 0) for an empty frame).  Per-block
 * partials and a fixed-order final sum: bit-identical run to run. */
int prv2_boundary_stats(const uint8_t* gt_edges, const uint8_t* pred_edges, const uint8_t* valid, const int32_t* d2_target,
                        const int32_t* d2_pred, const uint8_t* gt_ext, const uint8_t* pred_ext, int32_t n, int32_t h, int32_t w,
                        double th_edges_acc, double* stats, void* workspace, int64_t workspace_bytes, void* stream);


/* ------------------------------------------------------------------------------------------
 * Output stage (csrc/output.hip): the pixel bytes of the files the tester saves (estimator/tester/tester.py:72-106,132-181;
 * the colour maps of estimator/utils/color.py:95-158), produced on the device from B >= 1 dense frames [n, h, w]
 * (h, w >= 1; n * h * w < 2^29).  Fixed launch counts, no host synchronisation, bit-deterministic (integer atomics only).
 * A "scanline buffer" holds, per frame, the deflate-ready image of a PNG: h rows of 1 + bpp * w bytes, the first byte of each
 * row the filter type 0; frames lie rows_fstride bytes apart (a multiple of 16, at least prv2_rows_bytes(h, w, bpp)), the
 * buffer is 16-byte aligned and the bytes between a frame's image and the next multiple of 16 are written as zeros.
 * ------------------------------------------------------------------------------------------ */

/* bytes of workspace prv2_order_stats needs for n frames (-1 for a bad n) */
int64_t prv2_output_workspace_bytes(int32_t n);

/* h * (1 + bpp * w) rounded up to 16: the smallest frame stride of a scanline buffer (bpp 1 .. 4; -1 for bad arguments) */
int64_t prv2_rows_bytes(int32_t h, int32_t w, int32_t bpp);

/* exact order statistics of the valid pixels of each frame (color.py:118-125: np.percentile(value[mask], p) needs them).
 * valid: mask[i] != 0 when ``mask`` is given, value[i] != invalid_val otherwise (a NaN invalid_val keeps every pixel); with
 * ``gate`` also !((double)gate[i] < gate_thr) (tester.py:164-166: pixels enough tiles cover).  counts: DEVICE int64 [n], the
 * valid pixels of each frame.  ranks_host: HOST int64 [n_ranks <= 8], the same for every frame: k >= 0 the k-th smallest,
 * k < 0 the (count + k)-th (-1: the largest), clamped to [0, count - 1].  out: DEVICE fp32 [n, n_ranks] = np.sort(valid)[k]
 * (np.sort's order: -0.0 before +0.0, every NaN last and returned as the default NaN; NaN for a frame without a valid pixel).
 * Radix select over a monotone 32-bit key, 4 passes of 8 bits; n_ranks == 0 counts only. */
int prv2_order_stats(const float* value, const uint8_t* mask, float invalid_val, const float* gate, double gate_thr, int32_t n, int32_t h,
                     int32_t w, const int64_t* ranks_host, int32_t n_ranks, int64_t* counts, float* out, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* colorize (color.py:95-158) into RGB scanlines (bpp 3): x = (v - vmin) / (vmax - vmin) in correctly rounded fp32, v * 0 when
 * vmin == vmax (norm: DEVICE fp32 [n, 2] = vmin, vmax of each frame); matplotlib's index rule (xa = x * ncolors; xa == ncolors
 * -> ncolors - 1; xa < 0 -> under; xa >= ncolors -> over; NaN -> bad; else truncation) into lut: DEVICE uint8
 * [ncolors + 3, 4] = (cmap._lut * 255).astype(uint8) (rows ncolors .. ncolors + 2: under, over, bad).  Invalid pixels
 * (invalid_mask[i] != 0 when given, v == invalid_val otherwise) get background_rgb = r | g << 8 | b << 16. */
int prv2_colorize_rows(const float* value, const uint8_t* invalid_mask, float invalid_val, int32_t n, int32_t h, int32_t w, const float* norm,
                       const uint8_t* lut, int32_t ncolors, uint32_t background_rgb, uint8_t* rows, int64_t rows_fstride, void* stream);

/* 16-bit big-endian gray scanlines (bpp 2) of value * scale (tester.py:89-91 scale 256): truncation, == numpy's
 * astype(uint16), where 0 <= value * scale < 65536; outside it the result saturates to 0 / 65535 and NaN gives 0 (numpy's
 * cast is platform-defined there) */
int prv2_quantize16_rows(const float* value, int32_t n, int32_t h, int32_t w, float scale, uint8_t* rows, int64_t rows_fstride, void* stream);

/* the pseudo-label uncertainty (tester.py:160-176) in float64: u = (uncertainty - lo) / (hi - lo), 0 when !(hi > lo), then 1
 * where count_map < thr.  params: DEVICE float64 [n, 5] = lo, hi, thr, umin, umax (lo / hi: extrema of the frame's uncertainty,
 * thr = count_thr * tiles, umin / umax: extrema of u).  rows16: clip(floor(u * 256), 0, 65535) as 16-bit scanlines; rows_rgb:
 * u coloured like prv2_colorize_rows between umin and umax (float64 arithmetic, as colorize of a float64 map). */
int prv2_pl_uncertainty_rows(const float* uncertainty, const float* count_map, int32_t n, int32_t h, int32_t w, const double* params,
                             const uint8_t* lut, int32_t ncolors, uint8_t* rows16, int64_t rows16_fstride, uint8_t* rows_rgb,
                             int64_t rows_rgb_fstride, void* stream);

/* a 0/1 mask as 0 / 255 gray scanlines (bpp 1): <name>_edge.png (tester.py:99-106) */
int prv2_mask_rows(const uint8_t* mask, int32_t n, int32_t h, int32_t w, uint8_t* rows, int64_t rows_fstride, void* stream);

/* F.interpolate(mode='bilinear', align_corners=False) of fp32 maps [n, ph, pw] -> [n, oh, ow]: the coarse prediction at the
 * raw resolution (tester.py:93-96) */
int prv2_upsample_bilinear_map(const float* x, int32_t n, int32_t ph, int32_t pw, float* y, int32_t oh, int32_t ow, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device deflate (csrc/deflate.hip): zlib streams (RFC 1950 / 1951) of byte buffers that are already on the device -- the IDAT
 * payload of a scanline buffer, so that only compressed bytes are copied to the host.  Frames convention of the output stage:
 * rows [n, rows_fstride] with len valid bytes per frame (what prv2_*_rows write); every frame becomes one stream.  A frame is cut
 * into independent segments of prv2_deflate_segment() bytes (one workgroup each; no match crosses a segment; every segment but
 * the last ends byte-aligned with an empty stored block); greedy LZ77 in LDS (lengths 3 .. 258, every match verified byte for
 * byte), dynamic Huffman codes per block of 4096 positions, a stored block where that is smaller.  Three launches, no host
 * synchronisation, deterministic: the same bytes give the same stream on every call.  The streams differ from zlib's own
 * (zlib.decompress restores the input; the Adler-32 trailer is that of the len input bytes).
 * ------------------------------------------------------------------------------------------ */

/* input bytes per segment (a compile-time constant >= 32768) */
int32_t prv2_deflate_segment(void);

/* upper bound of a stream's size for any input of len bytes: a multiple of 16, at most len + len / 512 + 64 (-1 for len < 0 or
 * len >= 2^31) */
int64_t prv2_deflate_bound(int64_t len);

/* bytes of workspace prv2_deflate_rows needs for n frames of len bytes (-1 for bad arguments) */
int64_t prv2_deflate_workspace_bytes(int32_t n, int64_t len);

/* rows: DEVICE uint8 [n, rows_fstride], 16-byte aligned, rows_fstride a multiple of 16 and >= len; bytes behind len are not read
 * into the stream.  out: DEVICE uint8 [n, out_fstride], 16-byte aligned, out_fstride a multiple of 16 and >= prv2_deflate_bound(len):
 * frame f's stream is out[f, 0 .. out_bytes[f]).  out_bytes: DEVICE int64 [n].  workspace: 16-byte aligned.  len == 0 gives the
 * stream of an empty input.  Every argument is checked before the first launch. */
int prv2_deflate_rows(const uint8_t* rows, int32_t n, int64_t len, int64_t rows_fstride, uint8_t* out, int64_t out_fstride, int64_t* out_bytes,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ground-truth evaluation (csrc/evalgt.hip): the device half of UnrealStereo4kDataset (estimator/datasets/u4k_dataset.py) and the
 * sums behind compute_metrics (estimator/utils/metric.py:11-149).  Dense maps, h, w >= 1, fewer than 2^31 pixels per call.  Fixed
 * launch counts, no host synchronisation, no floating-point atomics: every output is the same bits on every call.  Added without
 * an ABI bump (additive, as the edge / output / deflate sections).
 * ------------------------------------------------------------------------------------------ */

/* u4k_dataset.py:125-147: image.astype(np.float32)[:, :, ::-1].copy() / 255.0, then to_tensor.  src: uint8 [h, w, 3]; dst: fp32
 * [3, h, w]; dst[c] = float(src[swap_rb ? 2 - c : c]) / 255.0f, a correctly rounded fp32 division (bit-equal to numpy's). */
int prv2_u8_image(const uint8_t* src, int32_t h, int32_t w, int32_t swap_rb, float* dst, void* stream);

/* u4k_dataset.py:128-129,216: depth = factor / disp (fp32 IEEE division: disp == 0 gives inf, as numpy) and, in the same pass,
 * boundary = get_boundaries(disp, th, dilation=0) (metric.py:74-85) as uint8 0/1 [h, w]: a pixel is set when the absolute
 * difference to its upper, lower, left or right neighbour exceeds th; a frame border has no neighbour on that side; a comparison
 * with NaN is false. */
int prv2_disp_gt(const float* disp, int32_t h, int32_t w, float factor, float th, float* depth, uint8_t* boundary, void* stream);

/* bytes of workspace prv2_depth_metrics needs for n frames of h x w (-1 for a bad shape) */
int64_t prv2_depth_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* compute_metrics (metric.py:87-149: clamping and masks; compute_errors :11-50; soft_edge_error(radius=1) :53-72) of n frames as
 * sums.  gt, pred: fp32 [n, h, w]; boundary, region: uint8 [n, h, w] (non-zero = set) or NULL.  pred is cleaned in the reference's
 * order (NaN -> min_depth, clamp to [min_depth, max_depth], inf -> max_depth); a pixel is valid when min_depth < gt < max_depth
 * (fp32 comparisons) inside the crop rows [y0, y1) x columns [x0, x1) (0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w: the garg / kitti /
 * eigen crops of metric.py:108-120, the whole frame for none).  sums: DEVICE float64 [n, S, 12], S = 1 without region, else 3: set
 * 0 all valid pixels, set 1 those inside the region, set 2 those outside (cityscapes_dataset.py / scannet_dataset.py:221-243's
 * three scoring calls from one read).  With g, p the fp32 values as float64, d = g - p, err = log p - log g:
 *   0 valid count   1..3 counts of max(g / p, p / g) < 1.25, 1.25^2, 1.25^3   4 sum |d| / g   5 sum d^2
 *   6 sum |log10 g - log10 p|   7 sum err^2   8 sum err   9 sum d^2 / g
 *   10 count of valid pixels on the boundary   11 sum over them of the fp32 minimum over the 3 x 3 shifts of gt (zero outside the
 *   frame) of |shift(gt) - p| (NaN propagates, as np.minimum).
 * Per-block partials in the workspace, summed in block order by a second launch. */
int prv2_depth_metrics(const float* gt, const float* pred, const uint8_t* boundary, const uint8_t* region, int32_t n, int32_t h,
                       int32_t w, float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, double* sums,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* The ground-truth formats of the general dataset (estimator/datasets/general_dataset.py:75-158, class DepthMap), decoded from the
 * raw samples as the host read them from the file.  Additive as well: the ABI version does not change. */
enum prv2_gt_kind {
  PRV2_GT_ETH3D = 0,      /* :103-111  fp32 depth; non-finite -> 0; edges of the cleaned depth                              */
  PRV2_GT_MIDDLEBURY = 1, /* :113-139 + datasets/utils.py:5-60  fp32 PFM payload (disparity); edges of the disparity with +inf -> 0 */
  PRV2_GT_CITYSCAPES = 2  /* :141-151  uint16 disparity PNG samples; edges of the depth                                      */
};

/* One pass over src [h, w] (fp32 for ETH3D / MIDDLEBURY, uint16 for CITYSCAPES) -> depth fp32 [h, w] and boundary uint8 0/1 [h, w]
 * = get_boundaries(e, th, dilation=0) (metric.py:74-85; the rule of prv2_disp_gt) of the map e the reference takes its edges from.
 * Every fp32 operation is numpy's IEEE operation in numpy's order (divisions are divisions):
 *   ETH3D       d = isfinite(v) ? v : 0                                   depth = d;  e = d
 *   MIDDLEBURY  inv = (v == +inf);  t = (factor / (v + doffs)) / 1000      depth = inv ? 0 : t;  e = inv ? 0 : v
 *   CITYSCAPES  f = float(v);  t = v > 0 ? (f - 1) / 256 : f;  q = factor / t    depth = isfinite(q) ? q : 0;  e = depth
 * (the reference's factor there is float32(0.209313 * 2262.52); doffs is read by MIDDLEBURY only).  flip != 0: the rows of src
 * are bottom-to-top (a PFM payload): output row y reads source row h - 1 - y.  byteswap != 0: the samples are of the other byte
 * order and are swapped as they are read. */
int prv2_gt_decode(const void* src, int32_t kind, int32_t h, int32_t w, float factor, float doffs, float th, int32_t flip,
                   int32_t byteswap, float* depth, uint8_t* boundary, void* stream);

/* prv2_depth_metrics for a prediction of another resolution (compute_metrics' F.interpolate(pred, gt.shape, mode='bilinear',
 * align_corners=False), metric.py:94-95, taken into the scoring kernel: the resized map is never written).  pred: fp32 [n, ph, pw];
 * everything else as prv2_depth_metrics, workspace of prv2_depth_metrics_workspace_bytes(n, h, w) bytes.  The value at (y, x), in
 * fp32 and PyTorch's formulation: sy = max(0, (ph / h) * (y + 0.5) - 0.5) (the scale an fp32 division), y0 = (int)sy,
 * y1 = min(y0 + 1, ph - 1), ly = sy - y0, the same in x, and
 *   p = (1 - ly) * ((1 - lx) * pred[y0, x0] + lx * pred[y0, x1]) + ly * ((1 - lx) * pred[y1, x0] + lx * pred[y1, x1]);
 * NaN -> min_depth and the clamps apply to p.  ph == h and pw == w runs prv2_depth_metrics itself (the same bits). */
int prv2_depth_metrics_lowres(const float* gt, const float* pred, const uint8_t* boundary, const uint8_t* region, int32_t n, int32_t h,
                              int32_t w, int32_t ph, int32_t pw, float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0,
                              int32_t x1, double* sums, void* workspace, int64_t workspace_bytes, void* stream);

/* ETHDataset (estimator/datasets/eth_dataset.py), the parts that run on the device.  Additive as well: the ABI version does not
 * change. */

/* eth_dataset.py:133,150-161: the RGB bytes / 255 (a correctly rounded fp32 division, as prv2_u8_image), then
 * F.interpolate(mode='bilinear', align_corners=True) to transform_cfg.input_size_shallow, as CHW.  src_hwc: uint8 [h, w, 3];
 * dst_chw: fp32 [3, H, W].  The fp32 operations of PyTorch's upsample_bilinear2d, none of them contracted: scale = (in - 1) / (out - 1)
 * (0 for out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, and
 *   dst = ly0 * (lx0 * v[y0, x0] + lx1 * v[y0, x1]) + ly1 * (lx0 * v[y1, x0] + lx1 * v[y1, x1]).
 * H == h and W == w gives prv2_u8_image(swap_rb = 0)'s bits. */
int prv2_u8_image_resize(const uint8_t* src_hwc, int32_t h, int32_t w, float* dst_chw, int32_t H, int32_t W, void* stream);

/* bytes of workspace prv2_image_edge_region needs for an image of h x w (-1 for a bad shape) */
int64_t prv2_image_edge_region_workspace_bytes(int32_t h, int32_t w);

/* eth_dataset.py:261-272: the edge area get_metrics splits its metrics by, from the IMAGE's gradient.  image_chw: fp32 [3, h, w];
 * region: uint8 0/1 [H, W] (the ground truth's shape).  Per channel the Sobel derivatives / 8 with replicate padding
 * (kornia.filters.spatial_gradient's defaults), m_c = sqrt(gx * gx + gy * gy) in fp32 with a correctly rounded sqrt, g = (m_0 + m_1) +
 * m_2, edge = g >= frac * max(g) (a constant image has max(g) == 0: every pixel is an edge).  The two steps after it need no
 * floating point: gaussian_blur2d(3 x 3, sigma 3, reflect) > 0 is the 3 x 3 dilation with the window clipped at the frame (positive
 * weights), and F.interpolate(bilinear, align_corners=True) > 0 at an output pixel is "one of the up to four source taps with a
 * non-zero weight is set", the taps and weights as prv2_u8_image_resize computes them (the upper tap of an axis counts only when
 * l1 > 0).  The maximum is an integer atomic maximum on the bits of non-negative floats: the same bits on every call.  Three
 * launches after a 16-byte memset; workspace 16-byte aligned, of prv2_image_edge_region_workspace_bytes(h, w) bytes; no float map of
 * H x W is made. */
int prv2_image_edge_region(const float* image_chw, int32_t h, int32_t w, float frac, uint8_t* region, int32_t H, int32_t W,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* CityScapesDataset (estimator/datasets/cityscapes_dataset.py), the parts that run on the device.  Additive as well: the ABI version
 * does not change. */

/* cityscapes_dataset.py:153-174 and :300, one pass.  disp: uint16 [h, w] (the disparity PNG's samples); seg_hwc: uint8 [h, w, 3] (the
 * RGB bytes of the gtFine colour map) or NULL; factor: float32(baseline * fx) of the frame's camera file.  Per pixel
 *   d = PRV2_GT_CITYSCAPES' depth (prv2_gt_decode);
 *   d = -1 in the last ceil(h / 4) rows, the first w / 16 and the last ceil(w / 16) columns (Python's -h // 4, w // 16, -w // 16);
 *   d = 0 where the segmentation pixel has R == 70 and G == 130 (the sky class; applied after the bands).
 * depth: fp32 [h, w] = d; boundary: uint8 0/1 [h, w] = get_boundaries(d, th=1, dilation=0) of that FINAL map (metric.py:74-85; the
 * rule of prv2_disp_gt, every neighbour decoded with the bands and the class mask applied); seg_chw: fp32 [3, h, w] holding the bytes
 * as 0 .. 255 (to_tensor(seg / 1.0), :232-233, :258), NULL exactly when seg_hwc is. */
int prv2_cityscapes_gt(const uint16_t* disp, const uint8_t* seg_hwc, int32_t h, int32_t w, float factor, float* depth, uint8_t* boundary,
                       float* seg_chw, void* stream);

/* cityscapes_dataset.py:333-334: kornia.filters.canny(seg)[1] > 0 with kornia's defaults (low 0.1, high 0.2, 5 x 5 Gaussian of
 * sigma 1, hysteresis on), on the colour segmentation map.  seg_chw: fp32 [3, h, w]; edges: uint8 0/1 [h, w]; h, w >= 3 (a reflect pad
 * of 2).  All fp32, each product / sum / difference rounded on its own (nothing contracted), in this order:
 *   grey  = (0.299f R + 0.587f G) + 0.114f B
 *   blur  : gauss_w5_host (five float32 taps, made on the host) along x, then along y; border reflect without the edge pixel
 *           (-1 -> 1, -2 -> 2); the taps summed from -2 to +2
 *   Sobel : unnormalised, border replicate; with u, c, d the rows above, at and below
 *           gx = ((u[x+1] - u[x-1]) + 2 (c[x+1] - c[x-1])) + (d[x+1] - d[x-1]);  gy likewise over the rows
 *   mag   = sqrt((gx gx + gy gy) + 1e-6f), a correctly rounded sqrt
 *   axis  : kornia rounds atan2(gy, gx) to a multiple of 45 degrees and compares with the neighbours in that direction and the
 *           opposite one, so only the axis counts.  a = |gx|, b = |gy|, T = float32(tan(pi / 8)): horizontal if b <= T a (takes
 *           gx = gy = 0), else vertical if a <= T b, else the (+1, +1) diagonal when gx and gy have the same sign, else (+1, -1)
 *   max   : min(mag - n1, mag - n2) > 0 with the two neighbours along the axis, 0 for one outside the frame
 *   hysteresis: strong = max and mag > high_threshold, weak = max and mag > low_threshold; edges = the weak pixels 8-connected to a
 *           strong one through weak pixels (the fixed point of kornia's loop), by prv2_canny's connected-component kernels.
 * workspace of prv2_edges_workspace_bytes(1, h, w) bytes.  Eight launches, the same bits on every call. */
int prv2_seg_canny(const float* seg_chw, int32_t h, int32_t w, const float* gauss_w5_host, float low_threshold, float high_threshold,
                   uint8_t* edges, void* workspace, int64_t workspace_bytes, void* stream);

/* cityscapes_dataset.py:360-365, one pass.  seg_edges (prv2_seg_canny), gt_edges (prv2_canny of the log ground truth), hr_region
 * (prv2_image_edge_region with frac 0.05, :346-352): uint8 [h, w], non-zero = set.  edge_mask = seg_edges and dilate7(gt_edges) --
 * gaussian_blur2d(7 x 7, sigma 5, reflect) > 0 is the 7 x 7 dilation with the window clipped at the frame (positive weights) --;
 * flatten = not edge_mask and not hr_region.  Both uint8 0/1 [h, w].  The valid-depth test of :324-329 stays with the scoring kernel
 * (the bands are -1 in prv2_cityscapes_gt's depth). */
int prv2_cityscapes_masks(const uint8_t* seg_edges, const uint8_t* gt_edges, const uint8_t* hr_region, int32_t h, int32_t w,
                          uint8_t* edge_mask, uint8_t* flatten, void* stream);

/* KittiDataset and ScanNetDataset (estimator/datasets/kitti_dataset.py, scannet_dataset.py), the part that runs on the device.
 * Additive as well: the ABI version does not change. */
enum prv2_depth16_grid {
  PRV2_GRID_WINDOW = 0, /* kitti_dataset.py:123-131  Image.crop: output (y, x) reads source (top + y, left + x)                  */
  PRV2_GRID_NEAREST = 1 /* scannet_dataset.py:112-118  Image.resize(size, NEAREST): output (y, x) reads source
                           ((int)((y + 0.5) * (sh / H)), (int)((x + 0.5) * (sw / W))), float64, one product per index           */
};

/* kitti_dataset.py:123-131, :142, :203 and scannet_dataset.py:112-118, :132, :188, one pass.  src: uint16 [sh, sw], the samples of the
 * depth PNG as the file holds them; the output map is [H, W].  PRV2_GRID_WINDOW: the H x W window whose first sample is (top, left) --
 * the host computes KITTI's kb-crop offsets top = sh - 352, left = int((sw - 1216) / 2); top = left = 0 with H = sh, W = sw is the whole
 * map.  PRV2_GRID_NEAREST: Pillow's NEAREST resize to H x W (top = left = 0): the scale sh / H is ONE float64 division, the index one
 * float64 product truncated (adding the step up instead picks other pixels than Pillow does); equal sizes are the identity.
 * depth: fp32 [H, W] = float32(sample) / divisor, an IEEE fp32 division (numpy's astype(float32) / 256.0 for KITTI, / 1000.0 for
 * ScanNet, bit for bit); boundary: uint8 0/1 [H, W] = get_boundaries(depth, th, dilation=0) of that OUTPUT map (metric.py:74-85; the
 * rule of prv2_disp_gt): a neighbour of an output pixel is the output's neighbour, read through the same grid rule.  The window's
 * first sample need not be aligned (KITTI's left margin is 13): the loads narrow to what its address allows. */
int prv2_depth16_gt(const uint16_t* src, int32_t sh, int32_t sw, int32_t grid, int32_t top, int32_t left, int32_t H, int32_t W,
                    float divisor, float th, float* depth, uint8_t* boundary, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scale-and-shift-invariant evaluation (csrc/ssi_eval.hip): compute_scale_and_shift (estimator/models/losses.py:523-544) and the
 * three modes of ScaleAndShiftInvariantLoss (losses.py:600-700: SSI L1, gradient matching, the 'inverse' gradient-space fit) as
 * scores of n frames, with the sums of compute_errors (metric.py:11-50) on the aligned prediction.  Additive as well: the ABI version
 * does not change.
 * ------------------------------------------------------------------------------------------ */

/* float64 values per frame prv2_ssi_metrics writes */
#define PRV2_SSI_VALUES 41

/* bytes of workspace prv2_ssi_metrics needs for n frames of h x w (-1 for a bad shape) */
int64_t prv2_ssi_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* gt: fp32 [n, h, w]; pred: fp32 [n, ph, pw].  ph == h and pw == w: the prediction is loaded; otherwise it is sampled as
 * prv2_depth_metrics_lowres samples it (bilinear, align_corners=False: the evaluation's resize of metric.py:94-95, not the loss's).
 * The mask m is min_depth < gt < max_depth (fp32 comparisons, a NaN is not valid) inside the crop rows [y0, y1) x columns [x0, x1);
 * the prediction is NOT clamped for the fit and the four scores (losses.py does not), a pixel outside the mask is never looked at.
 * Every term is float64 from the fp32 values p, g; a pair (y, y + 2) or (x, x + 2) counts when both its pixels are in the mask.
 * Two passes over the maps, no host round trip between them.  out: DEVICE float64 [n, PRV2_SSI_VALUES]:
 *    0, 1  scale s and shift t of compute_scale_and_shift(p, g, m) (losses.py:652)
 *    2, 3  s_v, t_v of the vertical differences p[y] - p[y+2] against g[y] - g[y+2] (losses.py:627-635)
 *    4, 5  s_h, t_h of the horizontal differences (losses.py:631-638)
 *    6     N = sum m
 *    7..21 the normal-equation sums a00 = sum p^2, a01 = sum p, a11 = count, b0 = sum p g, b1 = sum g of the three systems in that
 *          order; a system with det = a00 a11 - a01^2 <= 0 (or NaN) has scale = shift = 0 (losses.py:537-542)
 *    22    sum m |s p + t - g|                                                         (ssi=True, losses.py:698)
 *    23, 24  with d = s p + t - g: sum |d[y] - d[y+2]|, sum |d[x] - d[x+2]| over the pairs    (grad_matching=True, :683-696)
 *    25, 26  the same two with s = 1, t = 0                                            (ssi=False, grad_matching=True)
 *    27, 28  sum |s_v (p[y] - p[y+2]) + t_v - (g[y] - g[y+2])|, and the horizontal twin with s_h, t_h   (inverse=True, :623-647)
 *    29..40  the twelve sums of prv2_depth_metrics on the aligned prediction (float)(s p + t) (rounded once to fp32, then cleaned as
 *          there: NaN -> min_depth, clamp); 39 and 40 are 0 (no boundary map).
 * The reference divides every score by N, not by the number of pairs.  Per-block partials in the workspace, summed in block order:
 * the same bits on every call, and for a frame alone or among others. */
int prv2_ssi_metrics(const float* gt, const float* pred, int32_t n, int32_t h, int32_t w, int32_t ph, int32_t pw, float min_depth,
                     float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, double* out, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Boundary F1 evaluation (csrc/boundary_eval.hip): the scale-invariant boundary F1 of Depth Pro (Bochkovskii et al., 2024) of n
 * frames.  Not in the reference; metrics.compute_boundary_f1 is the numpy statement of the definition.  Additive: the ABI version
 * does not change.
 *   mask         a pixel is valid when it lies inside the crop and gt > min_depth && gt < max_depth (fp32 comparisons, a NaN ground
 *                truth is not valid: the test of prv2_ssi_metrics)
 *   prediction   cleaned at a valid pixel as compute_metrics cleans it (NaN -> min_depth, clamp to [min_depth, max_depth]); never read
 *                at an invalid pixel
 *   pairs        a horizontal pair is (x, y), (x + 1, y), a vertical pair (x, y), (x, y + 1); a pair counts only if BOTH pixels are
 *                valid; n_h and n_v are the numbers of such pairs
 *   boundary     for a depth map, a pair (a, b) (a = the left or top value, b = the right or bottom value) and a threshold t, fp32
 *                compare-after-multiply with no division (the product rounded to fp32, not contracted):
 *                horizontal  L: a > t * b (left is farther), R: b > t * a;  vertical  T: a > t * b (top is farther), B: b > t * a
 *                (Depth Pro applies the ratio test to inverse depth, which swaps L <-> R and T <-> B in prediction and ground truth alike:
 *                the same counts up to the rounding of the division)
 *   counts       per threshold i and direction d in the order (L, T, R, B), over the valid pairs: tp = pairs flagged in prediction AND
 *                ground truth, np = flagged in the prediction, ng = flagged in the ground truth
 * The scores (P_i = 1/4 sum_d tp / max(np, 1), R_i likewise with ng, F_i = 2 P_i R_i / (P_i + R_i), weights t_i / sum t) are formed on
 * the host: metrics.boundary_from_values.
 * ------------------------------------------------------------------------------------------ */

#define PRV2_BOUNDARY_MAX_THRESHOLDS 16
/* float64 values per frame prv2_boundary_f1 writes for T thresholds */
#define PRV2_BOUNDARY_VALUES(T) (2 + 12 * (T))

/* bytes of workspace prv2_boundary_f1 needs for n frames of h x w (-1 for a bad shape or frame count); proportional to n */
int64_t prv2_boundary_f1_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* gt: fp32 [n, h, w]; pred: fp32 [n, ph, pw].  ph == h and pw == w: the prediction is loaded; otherwise it is sampled at the valid
 * pixels as prv2_depth_metrics_lowres samples it (bilinear, align_corners=False).  The crop is rows [y0, y1) x columns [x0, x1).
 * thresholds: HOST array of n_thresholds (1 .. PRV2_BOUNDARY_MAX_THRESHOLDS) finite fp32 ratios > 1, in any order (they travel in the
 * kernel's arguments).  out: DEVICE float64 [n, PRV2_BOUNDARY_VALUES(T)], integers below 2^53 (exact):
 *    0, 1                     n_h, n_v
 *    2 + (4 i + d) * 3 + k    threshold i, direction d in (L, T, R, B), k in (tp, np, ng)
 * One pass over the maps writes per-block rows of 64-bit integers into the workspace, a second kernel adds them in block order: no
 * global atomics, the same bits on every call, and for a frame alone or among others. */
int prv2_boundary_f1(const float* gt, const float* pred, int32_t n, int32_t h, int32_t w, int32_t ph, int32_t pw, float min_depth,
                     float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, const float* thresholds, int32_t n_thresholds, double* out,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sparsification (csrc/sparsify.hip): does a per-pixel uncertainty mark the pixels where the depth is wrong?  The sparsification
 * curves behind AUSE / AURG (Ilg et al. 2018; Poggi et al. 2020) of n frames.  Not in the reference (its tester only writes the
 * uncertainty, estimator/tester/tester.py:132-181); the definition below is this project's, chosen so that ties need no tie-break,
 * and metrics.compute_uncertainty_metrics is its numpy statement.  Additive: the ABI version does not change.
 *   valid        min_depth < gt < max_depth (fp32 comparisons, a NaN is not valid; no crop); n = the number of valid pixels
 *   pred         cleaned as metric.py:98-101: NaN -> min_depth, < min_depth -> min_depth, > max_depth (inf too) -> max_depth
 *   key          uncert, +inf where (double)count < min_count (count given); a NaN orders last, as in np.sort
 *   terms        fp32, correctly rounded, no contraction: e_rel = |gt - pred| / gt, e_sq = (gt - pred) * (gt - pred)
 *   level k      k = 0 .. L - 1, for a key set K: n_k = n - floor(n k / L), t_k = the n_k-th smallest key (an exact order statistic),
 *                S_k = {i valid : K_i <= t_k} (ties are kept; every key is <= a NaN t_k)
 *   three orderings: K = the uncertainty key, K = e_rel (the oracle of abs_rel), K = e_sq (the oracle of rmse)
 * ------------------------------------------------------------------------------------------ */

#define PRV2_SPARSIFY_MAX_LEVELS 64
/* float64 values per frame prv2_sparsify writes for L levels */
#define PRV2_SPARSIFY_VALUES(L) (1 + 10 * (L))

/* bytes of workspace prv2_sparsify needs for n frames of h x w and L levels (-1 for a bad shape or L outside [1, 64]): the three key
 * maps and the valid mask (13 bytes per pixel), the selection state of prv2_order_stats and the per-block partials */
int64_t prv2_sparsify_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t levels);

/* gt, pred, uncert: fp32 [n, h, w]; count: fp32 [n, h, w] or NULL (then min_count is not looked at); n * h * w < 2^29.
 * out: DEVICE float64 [n, PRV2_SPARSIFY_VALUES(L)] per frame:
 *    0                 n
 *    1 .. 3L           the thresholds t_k of the uncertainty, the e_rel and the e_sq ordering (fp32 values; NaN for n = 0)
 *    1 + 3L .. 10L     seven rows of L float64 sums over S_k: |S_k|, sum e_rel, sum e_sq (uncertainty ordering); |S_k|, sum e_rel
 *                      (e_rel ordering); |S_k|, sum e_sq (e_sq ordering)
 * One pass makes the key maps and the mask, prv2_order_stats' radix select finds the thresholds (3 ceil(L / 8) selections, the ranks
 * computed from each frame's count on the device), one pass puts every valid pixel into its bucket (t_{k+1}, t_k] of each ordering,
 * a last kernel adds the per-block partials in block order and forms the suffix sums.  No host round trip, no floating-point
 * atomics: the same bits on every call, and for a frame alone or among others. */
int prv2_sparsify(const float* gt, const float* pred, const float* uncert, const float* count, double min_count, int32_t n, int32_t h,
                  int32_t w, float min_depth, float max_depth, int32_t levels, double* out, void* workspace, int64_t workspace_bytes,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Geometry export (csrc/pointcloud.hip): the depth map as geometry -- the vertex records of a binary PLY point cloud and the
 * scanlines of a surface-normal map, made from B >= 1 dense frames [n, h, w] where they are (h, w >= 1; n * h * w < 2^29).  Not in
 * the reference.  Fixed launch counts, no host synchronisation, no atomics: the same input gives the same bytes on every call.
 * Added without an ABI bump (additive).  The host specification is the numpy float32 restatement pointcloud_host /
 * normal_map_host of patchrefinerv2_amd/output.py, which the kernels equal bit for bit: fp32, one rounding per operation in the
 * order written, correctly rounded division and square root.
 *   camera     pinhole, x right, y down, z forward: Z = D[y, x], X = (((float)x + 0.5) - cx) * Z / fx, Y = (((float)y + 0.5) - cy) * Z / fy;
 *              fx, fy, cx, cy in pixels of the [h, w] grid (fx, fy > 0, all finite), the same for every frame of a call
 *   valid      Z finite and lo < Z < hi
 *   flying     edge_thr > 0 and one of the four in-frame neighbours is valid with |Z - Zn| > edge_thr * min(Z, Zn)
 *   kept       valid, not flying, y % stride == 0 and x % stride == 0 (the neighbours are the full-resolution ones)
 *   byte       clamp(rint(v * 255), 0, 255), ties to even, NaN -> 0
 * ------------------------------------------------------------------------------------------ */

/* bytes of workspace prv2_pointcloud_count / _pack need for n frames of h x w: one int32 per run of pixels a block owns (-1 for
 * bad arguments) */
int64_t prv2_pointcloud_workspace_bytes(int32_t n, int32_t h, int32_t w);

/* 15 * ceil(h / stride) * ceil(w / stride): the bytes of a frame's vertex records when every strided pixel is kept (-1 for bad
 * arguments) */
int64_t prv2_pointcloud_bound(int32_t h, int32_t w, int32_t stride);

/* depth: fp32 [n, h, w].  counts: DEVICE int64 [n] = N, the kept pixels of each frame.  workspace: DEVICE, 4-byte aligned,
 * prv2_pointcloud_workspace_bytes(n, h, w); it leaves with the exclusive offsets of every block's run of pixels, in block order
 * (a block counts its run, a one-block scan per frame adds the counts up) -- what prv2_pointcloud_pack reads. */
int prv2_pointcloud_count(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float fy, float cx, float cy, float lo, float hi,
                          float edge_thr, int32_t stride, int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream);

/* the vertex records of the kept pixels in row-major pixel order: float x, y, z (little endian) + uchar red, green, blue, 15 bytes
 * each, frame f's at vertices[f * vertices_fstride + 15 * k], k < N.  Same depth, camera, range, edge_thr and stride as the
 * prv2_pointcloud_count call that filled ``workspace``.  image: fp32 [n, 3, ih, iw] (any size), sampled nearest with integer
 * arithmetic: sy = ((2 y + 1) * ih) / (2 h), sx = ((2 x + 1) * iw) / (2 w); colour = byte(image[c, sy, sx]).  vertices: DEVICE uint8,
 * no alignment asked of the pointer or of vertices_fstride >= prv2_pointcloud_bound(h, w, stride).  Exactly the 15 * N bytes of a
 * frame are written and nothing else is touched: a block stores the ragged ends of its byte range with byte stores and the
 * 16-byte-aligned interior with 16-byte stores; no byte is read back. */
int prv2_pointcloud_pack(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx, float fy,
                         float cx, float cy, float lo, float hi, float edge_thr, int32_t stride, const void* workspace,
                         int64_t workspace_bytes, uint8_t* vertices, int64_t vertices_fstride, void* stream);

/* the surface normals as RGB scanlines (bpp 3; a scanline buffer of the output stage).  P = (X, Y, Z) of a valid pixel;
 * Px = P[y, x + 1] - P[y, x - 1] where both neighbours are valid and in frame, else P[y, x + 1] - P or P - P[y, x - 1] with the one
 * that is, else the pixel has no normal; Py likewise along y.  n = cross(Px, Py) / |cross(Px, Py)| (|v| = sqrt((vx vx + vy vy) + vz vz)),
 * negated where (n.x X + n.y Y) + n.z Z > 0 (it faces the camera); a length that is zero or not finite, or a component that is not
 * finite, gives no normal.  RGB = byte(n * 0.5 + 0.5); (0, 0, 0) for invalid pixels and pixels without a normal.  The flying-pixel
 * filter and the stride do not apply. */
int prv2_normal_rows(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float fy, float cx, float cy, float lo, float hi,
                     uint8_t* rows, int64_t rows_fstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh export (csrc/pointcloud.hip): the faces of a triangle mesh over the point cloud's vertices, from the connectivity the pixel
 * grid already holds.  Not in the reference.  Fixed launch counts, no host synchronisation, no atomics: the same input gives the
 * same bytes on every call.  Added without an ABI bump (additive).  The host specification is mesh_faces_host of
 * patchrefinerv2_amd/output.py, which the kernels equal byte for byte.
 *   vertices   the kept pixels of "Geometry export" in row-major order; a face index is a vertex's rank in that order
 *   grid       node (gy, gx) is pixel (gy * stride, gx * stride), gh = ceil(h / stride), gw = ceil(w / stride)
 *   cell       (gy, gx) with gy + 1 < gh and gx + 1 < gw; corners a = (gy, gx), b = (gy, gx + 1), c = (gy + 1, gx), d = (gy + 1, gx + 1)
 *   joined     two kept corners p, q: edge_thr <= 0, or not (|Zp - Zq| > edge_thr * min(Zp, Zq)) (the fp32 operations of "flying")
 *   diagonal   four corners kept: a-d if |Za - Zd| <= |Zb - Zc|, else b-c; three kept: the diagonal whose two ends are kept;
 *              fewer: the cell has no face
 *   candidates a-d: (a, c, d) then (a, d, b); b-c: (a, c, b) then (b, c, d); a candidate is a face when its three corners are kept
 *              and its three edges are joined
 *   order      cells row-major, inside a cell the first candidate first; with x right, y down, z forward every face looks at the
 *              camera (cross(P1 - P0, P2 - P0) has negative z on a fronto-parallel plane)
 *   record     uchar 3, then the three vertex indices as little-endian int32: 13 bytes
 * ------------------------------------------------------------------------------------------ */

/* bytes of workspace prv2_mesh_index / _count / _pack need for n frames of h x w at a stride: the index map int32 [n, gh, gw], then
 * one int32 per run of cells a block owns (-1 for bad arguments) */
int64_t prv2_mesh_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t stride);

/* 26 * (gh - 1) * (gw - 1): the bytes of a frame's face records when every cell has two faces; 0 for a grid of one row or one
 * column (-1 for bad arguments).  Past 2^31 for the largest frames: every byte offset is an int64. */
int64_t prv2_mesh_bound(int32_t h, int32_t w, int32_t stride);

/* the index map: workspace[f][gy][gx] (int32, at the start of ``workspace``) = the rank of pixel (gy * stride, gx * stride) among
 * frame f's kept pixels in row-major order -- the vertex prv2_pointcloud_pack writes for it -- or -1 where it is not kept.  Same
 * depth, range, edge_thr and stride as the prv2_pointcloud_count call that filled ``cloud_workspace`` (its exclusive offsets are
 * read; the camera is not needed).  workspace: DEVICE, 4-byte aligned, prv2_mesh_workspace_bytes(n, h, w, stride). */
int prv2_mesh_index(const float* depth, int32_t n, int32_t h, int32_t w, float lo, float hi, float edge_thr, int32_t stride,
                    const void* cloud_workspace, int64_t cloud_workspace_bytes, void* workspace, int64_t workspace_bytes, void* stream);

/* counts: DEVICE int64 [n] = M, the faces of each frame, by the rule above.  ``workspace`` holds prv2_mesh_index's map and leaves
 * with the exclusive offsets of every block's run of cells as well, in block order (a block counts its run, the one-block scan of
 * prv2_pointcloud_count adds the counts up) -- what prv2_mesh_pack reads.  Same depth, edge_thr and stride as that call. */
int prv2_mesh_count(const float* depth, int32_t n, int32_t h, int32_t w, float edge_thr, int32_t stride, int64_t* counts, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* the face records in cell order, frame f's at faces[f * faces_fstride + 13 * k], k < M (the offset computed in int64).  Same
 * arguments as the prv2_mesh_count call that filled ``workspace``.  faces: DEVICE uint8, no alignment asked of the pointer or of
 * faces_fstride >= prv2_mesh_bound(h, w, stride).  Exactly the 13 * M bytes of a frame are written and nothing else is touched: a
 * block stores the ragged ends of its byte range with byte stores and the 16-byte-aligned interior with 16-byte stores; no byte is
 * read back. */
int prv2_mesh_pack(const float* depth, int32_t n, int32_t h, int32_t w, float edge_thr, int32_t stride, const void* workspace,
                   int64_t workspace_bytes, uint8_t* faces, int64_t faces_fstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adaptive mesh export (csrc/mesh_adaptive.hip): a triangle mesh of the depth map with large triangles where the surface is flat and
 * pixel-sized ones at its boundaries -- a right-triangulated irregular network, the longest-edge-bisection hierarchy of terrain
 * renderers, with its own vertex list.  Not in the reference.  Fixed launch counts, no host synchronisation, no read-modify-write
 * atomics: the same input gives the same bytes on every call.  Added without an ABI bump (additive).  The host specification is
 * mesh_adaptive_host of patchrefinerv2_amd/output.py, which the kernels equal byte for byte.
 *   parameters tolerance T (fp32, finite, >= 0), block B (a power of two in [2, 64], L = log2 B); depth range and edge_thr as in
 *              "Geometry export"; there is no stride
 *   grid       vertices are pixels, kept as in "Geometry export" at stride 1; the grid is padded to whole blocks of B x B cells,
 *              Hp = B ceil((h - 1) / B) + 1, Wp likewise, with vertices that are neither kept nor smooth; h < 2 or w < 2: no face
 *   smooth     v is kept, and every 8-neighbour inside the frame is kept and joined to v ("Mesh export"'s joined)
 *   hierarchy  block (y0, x0) has the corners A = (y0, x0), B' = (y0, x0 + B), C = (y0 + B, x0), D = (y0 + B, x0 + B) and the root
 *              triangles (D, A, C) then (A, D, B'); (a, b, c) has the hypotenuse a-b, the apex c, the midpoint m = (a + b) / 2 and
 *              the children (c, a, m) then (b, c, m); after 2L bisections the legs are one pixel long (the finest triangles)
 *   vertex     not a block corner, hh = 2^min(tz(y), tz(x)).  y / hh and x / hh odd: a centre; its hypotenuse is the diagonal of
 *              the 2hh-square around it through the centre of the enclosing 4hh-aligned square (the block's A-D for 2hh = B), its
 *              apexes are the square's other corners, its child vertices the axial neighbours at hh.  One of them odd: an edge
 *              midpoint; hypotenuse ends at +-hh along the odd axis, apexes at +-hh along the other, child vertices the diagonal
 *              neighbours at hh / 2.  What lies outside the padded grid does not exist.
 *   required   of a vertex m that is not a block corner: m is not smooth, or a hypotenuse end or an existing apex is not kept, or an
 *              existing child vertex is required, or s = Za + Zb, p = Zm s, q = (Za Zb) 2, |p - q| > T p (one fp32 operation each;
 *              the depth at m against the harmonic mean of the ends, which is what a flat 3-D triangle has there)
 *   faces      blocks row-major, roots and children in the order above; a triangle above the finest is a face iff its midpoint is
 *              not required, else it splits; a finest one is a face iff its corners are kept and its edges joined.  Every face
 *              looks at the camera as "Mesh export"'s do.  T bounds a vertex against its own hypotenuse, not a pixel against the
 *              face finally emitted: no error bound is promised.
 *   vertices   the kept pixels a face references, in row-major pixel order, as the 15-byte records of "Geometry export"
 *   record     of a face: "Mesh export"'s 13 bytes, indices into the frame's vertex list
 * ------------------------------------------------------------------------------------------ */

/* bytes of workspace the two calls below need for n frames of h x w (-1 for bad arguments, among them n * Hp * Wp >= 2^29): per
 * frame the vertex index map int32 [Hp, Wp], one int32 per run of 2048 finest slots (2 B^2 a block) and per run of 2048 padded
 * vertices, and the kept and required maps uint8 [Hp, Wp]; 4 for a frame without a cell */
int64_t prv2_mesh_adaptive_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t block);

/* 15 * h * w and 26 * (h - 1) * (w - 1): the bytes of a frame's vertex and face records at most, those of the stride-1 cloud and
 * mesh (-1 for bad arguments) */
int64_t prv2_mesh_adaptive_vertex_bound(int32_t h, int32_t w);
int64_t prv2_mesh_adaptive_face_bound(int32_t h, int32_t w);

/* vertex_counts, face_counts: DEVICE int64 [n] = N and M of each frame.  Fills ``workspace`` (DEVICE, 4-byte aligned,
 * prv2_mesh_adaptive_workspace_bytes(n, h, w, block)) with what prv2_mesh_adaptive_pack reads: the kept and required maps, a mark
 * on every vertex a face uses (several lanes store the same value: no atomics), and the exclusive offsets of every run of slots and
 * of vertices.  2 L + 5 launches for a frame with cells. */
int prv2_mesh_adaptive_count(const float* depth, int32_t n, int32_t h, int32_t w, float lo, float hi, float edge_thr, float tolerance,
                             int32_t block, int64_t* vertex_counts, int64_t* face_counts, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* the records: frame f's vertices at vertices[f * vertices_fstride + 15 * k], k < N, and its faces at faces[f * faces_fstride + 13 * k],
 * k < M.  Same depth, range, edge_thr, tolerance and block as the prv2_mesh_adaptive_count call that filled ``workspace`` (which
 * leaves with every used vertex's rank in place of its mark); image and intrinsics as in prv2_pointcloud_pack.  vertices, faces: DEVICE
 * uint8, no alignment asked; vertices_fstride >= prv2_mesh_adaptive_vertex_bound(h, w), faces_fstride >=
 * prv2_mesh_adaptive_face_bound(h, w).  Exactly the 15 * N and 13 * M bytes of a frame are written and nothing else is touched. */
int prv2_mesh_adaptive_pack(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx,
                            float fy, float cx, float cy, float lo, float hi, float edge_thr, float tolerance, int32_t block,
                            void* workspace, int64_t workspace_bytes, uint8_t* vertices, int64_t vertices_fstride, uint8_t* faces,
                            int64_t faces_fstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stereo export (csrc/stereo.hip): the frame re-rendered from a second eye a baseline to the right of the camera, from its metric
 * depth map: B >= 1 dense frames [n, h, w] (h, w >= 1; n * h * w < 2^29; w <= prv2_stereo_max_width()).  Not in the reference.  One
 * workgroup per (frame, row) keeps the row in LDS; one launch, no host synchronisation; the depth test is an integer minimum, so the
 * same input gives the same bytes on every call.  Added without an ABI bump (additive).  The host specification is
 * stereo_source_host / stereo_image_host of patchrefinerv2_amd/output.py, which the kernel equals byte for byte.
 *   valid      Z finite and lo < Z < hi ("Geometry export")
 *   target     k = fx * baseline, c = k / convergence (0 for an infinite convergence; both fp32, rounded once), s = k / Z - c,
 *              t(x) = (int)clip((float)x - rint(s), -1, w), ties of rint to even, NaN -> -1
 *   span       a valid pixel x covers the columns [t(x), e]: e = max(t(x), t(x + 1) - 1) when x + 1 is in the frame, valid and joined
 *              to x ("Mesh export": edge_thr <= 0, or not |Z - Zn| > edge_thr * min(Z, Zn)), else e = t(x); cut to [0, w - 1]
 *   depth test a column shows the covering source of the smallest Z, between equal Z the smaller x; no source: a hole (-1)
 *   fill       a hole takes the source of the nearest shown column to its left, l, or right, r, of its row: r's when r's winner has
 *              the larger Z, else l's; the one that exists at a border; -1 in a row that shows nothing
 *   colour     image fp32 [n, 3, ih, iw] sampled as prv2_pointcloud_pack does, at (y, source column); byte = "Geometry export";
 *              (0, 0, 0) for -1
 * ------------------------------------------------------------------------------------------ */
#define PRV2_STEREO_RIGHT 0    /* the right-eye view, w columns */
#define PRV2_STEREO_SBS 1      /* left | right, 2 w columns; left = the image sampled to the [h, w] grid */
#define PRV2_STEREO_ANAGLYPH 2 /* red of the left eye, green and blue of the right eye, w columns */

/* the widest row prv2_stereo_rows / _source take: the columns of depth-test keys a workgroup keeps in LDS (8192) */
int32_t prv2_stereo_max_width(void);

/* src, filled: DEVICE int32 [n, h, w]: the winning source column of every column of the view (-1: hole), and the same with the holes
 * filled by the rule above.  fx > 0 finite, baseline finite (metres, positive: the eye moves right), convergence != 0 (the depth
 * that keeps its column; +/-inf: parallel axes). */
int prv2_stereo_source(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float baseline, float convergence, float lo, float hi,
                       float edge_thr, int32_t* src, int32_t* filled, void* stream);

/* the view as RGB scanlines (bpp 3; a scanline buffer of the output stage: [h][1 + 3 wout] bytes per frame, wout = 2 w for
 * PRV2_STEREO_SBS, else w; rows 16-byte aligned, rows_fstride a multiple of 16 and >= prv2_rows_bytes(h, wout, 3); the tail up to the
 * next multiple of 16 is zero).  A workgroup assembles its scanline in LDS and stores it once: byte stores at the ragged ends,
 * 16-byte stores inside; no byte is read back. */
int prv2_stereo_rows(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx, float baseline,
                     float convergence, float lo, float hi, float edge_thr, int32_t layout, uint8_t* rows, int64_t rows_fstride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Temporal stabilisation (csrc/temporal.hip): the metric maps of consecutive video frames with the frame-to-frame jitter of their
 * global scale and shift taken out.  Not in the reference.  Every frame is aligned to the previous OUTPUT by a gated least-squares
 * scale and shift and blended with it where the image has not changed.  Four launches per frame, chained on the stream: the
 * coefficients go from the fit to the apply pass through device memory, nothing is synchronised, nothing is allocated (graph-capture
 * safe).  Every sum is an int64 sum of integers, so the same input gives the same bits on every call and however a sequence is cut
 * into calls.  Added without an ABI bump (additive).  The host specification is temporal_step_host of
 * patchrefinerv2_amd/temporal.py, which the kernels equal bit for bit.
 *   state      the previous output y (fp32 [h, w]) and the previous luma Lp (uint8 [h, w]), or nothing
 *   valid(v)   v finite and > 0
 *   luma       R, G, B = the bytes prv2_pointcloud_pack gives pixel (r, c) from image fp32 [3, ih, iw] ("Geometry export": its nearest
 *              sample and its byte rule); L = (77 R + 150 G + 29 B + 128) >> 8
 *   gate       g = |L - Lp| <= tau and valid(x) and valid(y); without a state no pixel is gated
 *   fit mask   m = g and 1 <= qx < 2^18 and 1 <= qy < 2^18 and |x - y| <= 0.5 y (float64), qx = rint(x * 256), qy = rint(y * 256) in
 *              fp32, ties to even
 *   sums       over m, int64: n, sum qx, sum qx^2, sum qx qy, sum qy ((2^18)^2 * 2^25 < 2^63: frames of at most 2^25 pixels)
 *   reset      n < max(64, h w / 100) (no state, or a scene cut): out = x
 *   fit        float64 from the sums, one IEEE operation per step: a00 = sum qx^2, a01 = sum qx, a11 = n, b0 = sum qx qy, b1 = sum qy,
 *              det = a00 a11 - a01 a01; det > 0: s = (a11 b0 - a01 b1) / det, b = ((a00 b1 - a01 b0) / det) / 256; det <= 0 or NaN,
 *              s outside [0.5, 2] or b not finite: identity (s = 1, b = 0).  Then s = 1 + anchor (s - 1), b = anchor b
 *   apply      a = fp32(s x + b) where x and that value are valid, else a = x; where g: r = (a - y) / min(a, y),
 *              w = alpha / (1 + (r / rho)(r / rho)), out = fp32(a + w (y - a)); elsewhere out = a (an invalid x leaves as it came)
 *   change     sum over g of rint(65536 min(1, |v - y| / y)), v = x ("before") and v = out ("after"); a NaN ratio counts as 1
 *   then       state = (out, L)
 * ------------------------------------------------------------------------------------------ */
#define PRV2_TEMPORAL_STATS 12 /* 8-byte words per frame of prv2_temporal_step's stats */

/* bytes of workspace prv2_temporal_step needs for frames of h x w, whatever their count: the int64 partials of one frame's blocks
 * (-1 for bad arguments: h, w < 1 or more than 2^25 pixels) */
int64_t prv2_temporal_workspace_bytes(int32_t h, int32_t w);

/* n >= 1 frames in sequence order.  depth: fp32 [n, h, w]; image: fp32 [n, 3, ih, iw] (any size); out: fp32 [n, h, w] (not the
 * input).  alpha in [0, 1), tau in 0 .. 255, rho > 0 finite, anchor in [0, 1].  state_depth: fp32 [h, w], read by the first frame when
 * state_present is 1 and left holding the last frame's output.  luma0, luma1: two distinct uint8 [h, w] buffers; frame f reads the
 * previous luma from luma[f & 1] and writes its own into luma[(f + 1) & 1], so the caller passes the buffer that holds the state
 * first and the state leaves in luma[n & 1].  The maps are read and written with 16-byte accesses when w % 4 == 0 and depth, out
 * and state_depth are 16-byte, the luma buffers 4-byte aligned; element by element otherwise.  stats: DEVICE, 8-byte aligned,
 * [n][PRV2_TEMPORAL_STATS] 8-byte words per frame: int64 0 reset, 1 n, 2 n_gate (pixels of g), 3 sum qx, 4 sum qx^2, 5 sum qx qy,
 * 6 sum qy, 7 change before, 8 change after, 11 fitted (1: the fit was taken, 0: reset or identity); float64 9 s, 10 b (after the
 * anchor).  workspace: DEVICE, 8-byte aligned, prv2_temporal_workspace_bytes(h, w).  Every argument is checked before anything is
 * launched (prv2_last_error). */
int prv2_temporal_step(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, double alpha,
                       int32_t tau, double rho, double anchor, float* state_depth, uint8_t* luma0, uint8_t* luma1, int32_t state_present,
                       float* out, int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Temporal motion (csrc/motion.hip): an optional motion stage in front of the stabiliser's step, so that a moving camera no longer
 * gates the frame out.  Not in the reference.  A dense field of block vectors between the frame's luma L and the previous luma P is
 * found by an integer block-matching search, the state (y, P) is moved by it, and the step above runs on the moved state.  Bytes and
 * integer sums throughout: the same bits on every call and however a sequence is cut into calls; no atomics, no allocation, no host
 * synchronisation.  Added without an ABI bump (additive).  The host specification is temporal_motion_host / temporal_warp_host /
 * temporal_step_host(motion_range=R) of patchrefinerv2_amd/temporal.py, which the kernels equal bit for bit.
 *   clamp      every index that leaves its map is clamped into it: cy(i) = min(max(i, 0), h - 1), cx and cq (quarter map) likewise
 *   vector     m = (my, mx): pixel p of the frame was at p + m in the previous frame
 *   quarter    hq = ceil(h / 4), wq = ceil(w / 4); Q[i, j] = (sum over a, b < 4 of L[cy(4i + a), cx(4j + b)] + 8) >> 4; QP from P
 *   blocks     16 x 16 pixels, nby = ceil(h / 16), nbx = ceil(w / 16)
 *   coarse     block (by, bx) owns the 8 x 8 window of Q at rows 4by - 2 .. 4by + 5, columns 4bx - 2 .. 4bx + 5; for |dy|, |dx| <= R:
 *              S(d) = sum over the window of |Q[cq(i), cq(j)] - QP[cq(i + dy), cq(j + dx)]|; the smallest (S, dy^2 + dx^2, dy, dx) in
 *              lexicographic order wins and is taken if S + 64 < S(0, 0), else the block's coarse vector is (0, 0)
 *   median     v^ = the component-wise median (fifth smallest) of the nine coarse vectors of the 3 x 3 blocks, block indices clamped
 *   fine       c = 4 v^ + e, e in [-3, 3]^2; T(c) = sum over the block's npix pixels inside the frame of |L[y, x] - P[cy(y + c_y),
 *              cx(x + c_x)]|; the smallest (T, ey^2 + ex^2, ey, ex) wins; m = c if T + npix < T(0, 0), else (0, 0).  |m| <= 4R + 3
 *   warp       pixel p takes its block's m; p + m inside the frame: yw[p] = y[p + m], Pw[p] = P[p + m]; elsewhere yw[p] = the quiet NaN
 *              0x7FC00000 (not valid: the pixel is not gated) and Pw[p] = 0
 *   step       "Temporal stabilisation" with (yw, Pw) in place of the state; the new state is (out, L), the un-warped luma.  A frame
 *              without a state runs no motion stage: its motion row and vectors are zero
 * ------------------------------------------------------------------------------------------ */
#define PRV2_TEMPORAL_MOTION_STATS 8 /* 8-byte words per frame of prv2_temporal_motion_step's motion_stats */

/* bytes of workspace prv2_temporal_motion_step needs for frames of h x w, whatever their count: the step's partials, the warped state,
 * the two quarter maps and the blocks' records (-1 for bad arguments, as prv2_temporal_workspace_bytes) */
int64_t prv2_temporal_motion_workspace_bytes(int32_t h, int32_t w);

/* prv2_temporal_step with the motion stage: the same arguments, conventions and stats, and
 *   motion_range  R, an integer in 1 .. 16 (quarter pixels: vectors of up to 4R + 3 pixels a component)
 *   motion_stats  DEVICE, 8-byte aligned, [n][PRV2_TEMPORAL_MOTION_STATS] int64 per frame: 0 blocks, 1 blocks with m != 0, 2 sum my,
 *                 3 sum mx, 4 sum (|my| + |mx|), 5 max(|my|, |mx|) over the blocks, 6 sum T(m) (T(0, 0) for a zeroed block),
 *                 7 sum T(0, 0); all zero for a frame whose stage did not run
 *   vectors       DEVICE int16 [n][nby][nbx][2] (my, mx), or NULL
 *   workspace     DEVICE, 8-byte aligned, prv2_temporal_motion_workspace_bytes(h, w)
 * Per frame with a state six launches (luma and Q, QP, coarse search, median and refinement, warp, stats) come before the step's four; a
 * frame without one has a single launch that zeroes its row and vectors.  Every argument is checked before anything is launched. */
int prv2_temporal_motion_step(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, double alpha,
                              int32_t tau, double rho, double anchor, int32_t motion_range, float* state_depth, uint8_t* luma0, uint8_t* luma1,
                              int32_t state_present, float* out, int64_t* stats, int64_t* motion_stats, int16_t* vectors, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depth-of-field export (csrc/bokeh.hip): the frame re-rendered through a thin lens focused at one distance ("portrait mode"), from
 * its metric depth map: B >= 1 dense frames [n, h, w] (h, w >= 1; n * h * w < 2^29).  Not in the reference.  One launch, no host
 * synchronisation (the focus distance is read from the device map), no atomics on memory: the same input gives the same bits on
 * every call.  Added without an ABI bump (additive).  The host specification is bokeh_render_host / bokeh_image_host of
 * patchrefinerv2_amd/output.py, which the kernel equals bit for bit.  Everything is fp32, round to nearest, no contraction.
 *   valid      Z finite and lo < Z < hi ("Geometry export"); zk = valid ? Z : +inf; iz = valid ? 1 / Z : 0 (invalid: infinitely far)
 *   focus      Zf = focus when focus > 0 (finite), else the map at the focus pixel (min(h - 1, floor(focus_v h)), min(w - 1,
 *              floor(focus_u w))), products in float64; that pixel not valid: r = 0 everywhere (the image itself) and focus_out = NaN
 *   radius     k = (fx * aperture) * 0.5 on the host; r = min(max_radius, k |iz - 1 / Zf|) (a NaN product gives max_radius): the
 *              thin-lens circle of confusion in pixels for Zf much larger than the focal length; m = max(r, 0.5); ia = 1 / (m m)
 *   window     for output p the taps q = p + (dx, dy) inside the frame, dy = -R .. R outer, dx = -R .. R inner, R = ceil(max_radius);
 *              dist = fp32(sqrt(dx dx + dy dy))
 *   disc       own = zk_q <= zk_p or r_q <= r_p; (me, ie) = own ? (m_q, ia_q) : (m_p, ia_p): a source spreads over its own disc
 *              unless it lies behind p with the larger disc -- a defocused background does not bleed over a sharp foreground
 *   weight     cov = clamp((me + 0.5) - dist, 0, 1); wgt = cov ie; where wgt > 0: sw = sw + wgt, sc[ch] = sc[ch] + (wgt c_q[ch])
 *   result     sc[ch] / sw (sw > 0: the centre tap has cov >= 0.5).  A tap of weight 0 changes no bit, so a tile walks only the
 *              offsets the largest m in its reach can cover
 *   colour     image fp32 [n, 3, ih, iw] sampled as prv2_pointcloud_pack does; a non-finite colour counts as 0; byte = "Geometry
 *              export" on result * 255
 * ------------------------------------------------------------------------------------------ */

/* the largest max_radius prv2_bokeh_render / _rows take (32: a window of 65 x 65 taps; it sets the pitch of the LDS band) */
int32_t prv2_bokeh_max_radius(void);

/* measurement only: on = 0 makes every tile walk the full window, on = 1 (the default) bounds the walk per tile, on < 0 changes
 * nothing; returns the previous setting.  Process-wide; the bits of the result do not depend on it. */
int32_t prv2_bokeh_tile_bound(int32_t on);

/* out: DEVICE fp32 [n, 3, h, w]; focus_out: DEVICE fp32 [n], the Zf of every frame (NaN: its focus pixel was not valid).  fx > 0
 * finite; aperture >= 0 finite (metres); focus finite (<= 0 or NaN: use the focus point); focus_u, focus_v in [0, 1]; max_radius
 * in [0, prv2_bokeh_max_radius()]; lo, hi not NaN.  Every argument is checked before anything is launched (prv2_last_error). */
int prv2_bokeh_render(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx, float aperture,
                      float focus, float focus_u, float focus_v, float max_radius, float lo, float hi, float* out, float* focus_out,
                      void* stream);

/* the same frames as RGB scanlines (bpp 3; a scanline buffer of the output stage: [h][1 + 3 w] bytes per frame; rows 16-byte
 * aligned, rows_fstride a multiple of 16 and >= prv2_rows_bytes(h, w, 3); the tail up to the next multiple of 16 is zero): the
 * bytes of prv2_bokeh_render's result.  A workgroup assembles its tile's part of every scanline in LDS and stores it once: byte
 * stores at the ragged ends, 16-byte stores inside; no byte is read back. */
int prv2_bokeh_rows(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx, float aperture,
                    float focus, float focus_u, float focus_v, float max_radius, float lo, float hi, uint8_t* rows, int64_t rows_fstride,
                    float* focus_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Novel-view export (csrc/view.hip): the frame seen from a camera that has moved (a "3D photo", one frame of a parallax clip), from
 * its metric depth map: B >= 1 dense frames [n, h, w] and nv >= 1 poses per call (h, w >= 1; n * nv * h * w < 2^29;
 * w <= prv2_stereo_max_width()).  Not in the reference.  The map's own mesh is rasterised exactly, with a depth test: three kernels
 * (clear, raster, resolve) chained on the caller's stream, no host synchronisation, no allocation.  The depth test is an unsigned
 * 64-bit minimum on memory, which has no order: the same input gives the same bits on every call.  Added without an ABI bump
 * (additive).  The host specification is view_source_host / view_image_host of patchrefinerv2_amd/output.py, which the kernels equal
 * bit for bit.  Everything is fp32, one rounding per operation in the order written, no contraction, correctly rounded division;
 * after "fixed" everything but the interpolation of "depth" is integer arithmetic.
 *   camera     "Geometry export": Z = D[y, x], X = (((float)x + 0.5) - cx) * Z / fx, Y likewise; valid: Z finite and lo < Z < hi
 *   pose       M: fp32 [12], a row-major 3 x 4 matrix [R | t], made on the host in float64 and rounded once:
 *              Xc = ((M0 X + M1 Y) + M2 Z) + M3, Yc and Zc with rows 1 and 2
 *   project    iz = 1 / Zc; fu = fx * (Xc / Zc) + cx; fv = fy * (Yc / Zc) + cy
 *              a vertex is "seen" when valid, Zc finite and > 0, iz finite, |fu| < 65536 and |fv| < 65536
 *              (there is no clipping at a near plane: a face with a vertex that is not seen is dropped)
 *   fixed      ux = (int)rint(fu * 16), uy = (int)rint(fv * 16), ties to even; the centre of view pixel (px, py) is (16 px + 8, 16 py + 8)
 *   points     every seen vertex is a candidate for the view pixel (ux >> 4, uy >> 4) (arithmetic shift = floor), when that lies in
 *              the frame, with q = iz and its own index
 *   faces      "Mesh export" at stride 1 with "kept" read as "valid" (the flying-pixel filter does not apply, as in "Stereo export"):
 *              same diagonal rule, same candidates in the same order, same "joined" rule with edge_thr; all three vertices seen
 *              A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) in fixed units; A = 0: no face; s = sign(A)
 *              (a face seen from behind is drawn: there is no culling)
 *   box        px from ceil((min ux - 8) / 16) to floor((max ux - 8) / 16), py likewise
 *              a face whose box spans more than prv2_view_max_face() = 16 pixel centres in x or in y is dropped (stretched more than
 *              16-fold: it belongs to no surface worth showing); then the box is cut to the frame
 *   cover      w0 = s E12(p), w1 = s E20(p), w2 = s E01(p), Eij(p) = (xj - xi)(py' - yi) - (yj - yi)(px' - xi) at the pixel centre p'
 *              p is covered when all three are >= 0 (edges inclusive: a centre on a shared edge belongs to both faces and the depth
 *              test decides, so a surface has no cracks); w0 + w1 + w2 = |A| < 2^24, so the conversions below are exact
 *   depth      q = (((float)w0 * iz0 + (float)w1 * iz1) + (float)w2 * iz2) / (float)|A|
 *              (1 / Zc is linear in the view, so this is perspective-correct)
 *   source     the vertex with the largest w, the first of (0, 1, 2) between equals: its pixel index y * w + x
 *   test       key = ((0xFFFFFFFF - bits(q)) << 32) | source
 *              a view pixel keeps the smallest key over all its candidates: the largest q, between equal q the smallest source index
 *              No candidate: a hole (src = -1, iz = 0)
 *   fill       "Stereo export"'s rule on every row of the view, with the winners' q for the comparison:
 *              a hole takes the source of the nearest shown column to its left, l, or right, r; r's when q_r < q_l (the farther side),
 *              else l's; the one that exists at a border; -1 in a row that shows nothing
 *   colour     image fp32 [n, 3, ih, iw] sampled as prv2_pointcloud_pack does at the filled source pixel; byte = "Geometry export";
 *              (0, 0, 0) for -1
 * ------------------------------------------------------------------------------------------ */

/* the pixel centres a face's box may span in x and in y (16) */
int32_t prv2_view_max_face(void);

/* measurement only: which of the three kernels prv2_view_source / _rows launch, as a mask (1 clear, 2 raster, 4 resolve; 7 is the
 * default; mask < 0 changes nothing); returns the previous mask.  Process-wide.  With a kernel left out the results are not the
 * specification's. */
int32_t prv2_view_stages(int32_t mask);

/* bytes of workspace prv2_view_source / _rows need for n frames and nv poses of h x w: one 64-bit key per view pixel (-1 for bad
 * arguments, n * nv * h * w >= 2^29 among them) */
int64_t prv2_view_workspace_bytes(int32_t n, int32_t nv, int32_t h, int32_t w);

/* poses: DEVICE fp32 [nv][12].  src, filled: DEVICE int32 [n, nv, h, w]: the source pixel (y * w + x of the frame) every pixel of
 * every view shows (-1: hole), and the same with the holes filled by the rule above.  iz: DEVICE fp32 [n, nv, h, w], the winners' q
 * (0: hole), or null.  workspace: DEVICE, 16-byte aligned, prv2_view_workspace_bytes(n, nv, h, w).  fx, fy > 0, all four finite;
 * lo, hi, edge_thr not NaN.  Every argument is checked before anything is launched (prv2_last_error). */
int prv2_view_source(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float fy, float cx, float cy, const float* poses, int32_t nv,
                     float lo, float hi, float edge_thr, int32_t* src, int32_t* filled, float* iz, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* the views as RGB scanlines (bpp 3; scanline buffers of the output stage, one per (frame, view): [h][1 + 3 w] bytes at
 * rows[(f * nv + v) * rows_vstride]; rows 16-byte aligned, rows_vstride a multiple of 16 and >= prv2_rows_bytes(h, w, 3); the tail
 * up to the next multiple of 16 is zero).  A workgroup assembles its scanline in LDS and stores it once: byte stores at the ragged
 * ends, 16-byte stores inside; no byte is read back. */
int prv2_view_rows(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx, float fy, float cx,
                   float cy, const float* poses, int32_t nv, float lo, float hi, float edge_thr, uint8_t* rows, int64_t rows_vstride,
                   void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRV2_H */
