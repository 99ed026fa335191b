// vso_kernels.h — launch parameter blocks of the ONNX-session kernels
// (vso_kernels.hip), shared with the session planner (vso_model.hip).
// float32 NCHW tensors; plain structs passed by value.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

namespace vso {

constexpr int kMaxDims = 6;

// Activations fused into the producing kernel's epilogue (and the unary kernel).
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_CLIP = 2, ACT_PRELU = 3, ACT_LEAKY = 4, ACT_SIGMOID = 5, ACT_TANH = 6,
                 ACT_F16 = 7 /* Cast to float16: round to the nearest half (ties to even), kept as f32 */,
                 ACT_HSIGMOID = 8 /* HardSigmoid: clamp(a0 * x + a1, 0, 1) */,
                 ACT_HSWISH = 9 /* x * clamp(a0 * x + a1, 0, 1): HardSwish (a0 1/6, a1 0.5), Mul(x, HardSigmoid(x)) */,
                 ACT_GELU = 10 /* Gelu, approximate none: 0.5 x (1 + erf(x / sqrt 2)) */,
                 ACT_GELU_TANH = 11 /* Gelu, approximate tanh: 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) */,
                 ACT_ERF = 12 /* Erf (k_unary only) */ };

struct Epilogue {
  const float* bias;   // [M] or null
  const float* res;    // residual added before the activation (same layout as y) or null
  int act;             // Act
  float a0, a1;        // CLIP lo/hi, LEAKY alpha, HSIGMOID / HSWISH alpha/beta
  const float* slope;  // PRELU: per output channel ([M]) or one value (slope_stride 0)
  int slope_stride;
  // res_mode 1: res is [N][res_c][Ho][Wo], channels >= res_c add 0 (an ONNX Pad
  // of the channel axis, fused); 2: res is [N][res_c][res_h][res_w] and the
  // value added is its 2x2 stride-2 max (a MaxPool, fused, then that Pad)
  int res_mode, res_c, res_h, res_w;
  int out_c, out_hw, out_w;  // the output's M, Ho*Wo, Wo (res_mode != 0)
  int act_c_end;             // > 0: the activation applies to channels < act_c_end only (an IBNorm's BN half)
};

// A depthwise convolution fused in front of a 1x1 one (k_conv_dwpw): `x` is
// the depthwise conv's input; its output — the 1x1's input — exists only in
// LDS.  Same FMA order and epilogue as k_conv_dw: the values k_conv_dw would
// have stored, bit for bit.
struct DwPre {
  const float* w;  // [C][kh][kw]; null: no fused producer
  int H, W;        // the depthwise input's size
  int kh, kw, sh, sw, dh, dw, pt, pl;
  Epilogue ep;     // bias / activation (no residual)
};

struct ConvParams {
  const float* x;  // [N][C][H][W]
  const float* w;  // [M][Cg][kh][kw]
  float* y;        // [N][M][Ho][Wo]
  int N, C, H, W, M, Ho, Wo;
  int G, Cg, Mg;   // groups, input / output channels per group
  int kh, kw, sh, sw, dh, dw, pt, pl;
  Epilogue ep;
  DwPre pre;       // k_conv_dwpw only (x is then the depthwise input)
  // extra output elements per image: y is a channel range of a wider
  // [N][ctot][Ho][Wo] tensor (a Concat input written in place), image n's
  // output at y + n * (M * Ho * Wo + y_nx); 0 = a tensor of its own
  long y_nx;
};

// Operand precision of the dense convolutions (vso_conv.hip; vso_options.conv_precision)
enum ConvPrec : int { PREC_F32 = 0, PREC_BF16 = 1, PREC_F16 = 2 };

// k_conv_tile's plan: tile shape, padding of the packed weights, K split
struct ConvTileShape {
  int prec, ks, s, th, tw, bm;
  int up;              // k_conv_tile_up: channels [up_c0, up_c1) upsampled from ConvTileParams::up
  int tiles_x, tiles;  // pixel tiles per tile row / per image
  int Mp, Cp;          // output channels padded to bm, input channels to 32
  int ksplit, cps;     // workgroups splitting the 32-channel chunks, chunks per split
};

struct ConvTileParams {
  ConvParams c;        // geometry, x, y, epilogue
  const void* wp;      // weights packed [kh*kw][Mp][Cp] in the operand type
  int Mp, Cp, tiles_x, tiles, mtiles, ksplit, cps;
  float* part;         // ksplit > 1: partial tiles [output block][ksplit][bm/16][th*tw/64][256 threads] as f4
  int* counters;       // ksplit > 1: arrivals per output block [N][M tiles][tiles], zero between runs
  // k_conv_tile_up: input channels [up_c0, up_c1) (whole 32-channel chunks)
  // are the 2x linear (half-pixel) upsample of up ([N][up_c1 - up_c0][up_H][up_W])
  const float* up;
  int up_c0, up_c1, up_H, up_W;
  // a Concat's last input read from its own tensor instead of copied into the
  // concatenation: channels [x2_c0, x2_c0 + x2_C) ([N][x2_C][H][W]; x2_c0 a
  // multiple of 32), or x2 = null
  const float* x2;
  int x2_c0, x2_C;
  int items;           // work items (pixel tile x M tile x image x split); set by launch_conv_tile
  int qskip;           // skip the loads of quads past C in a partial last chunk (VSO_CONV_QSKIP=0: off)
  int xcd;             // XCD-contiguous item order (k_conv_tile, ksplit 1; VSO_CONV_XCD=0: off)
};

constexpr int kDwPwMaxC = 256;  // channels a fused depthwise -> 1x1 pair may have

enum BinOp : int { BIN_ADD = 0, BIN_SUB = 1, BIN_MUL = 2, BIN_DIV = 3, BIN_PRELU = 4 };

struct BinParams {  // y = a (op) b with numpy broadcasting (strides 0 on broadcast dims)
  const float* a;
  const float* b;
  float* y;
  long n;
  int nd;
  int dims[kMaxDims];
  long sa[kMaxDims], sb[kMaxDims];
  int op;
};

struct UnaryParams {
  const float* x;
  float* y;
  long n;
  int act;
  float a0, a1;
};

// dst[dst_base + sum_d i_d * dst_stride_d] = src[src_base + sum_d c_d * src_stride_d]
// with c_d = i_d * step_d + start_d, or `fill` when some c_d is outside [0, lim_d):
// Transpose, Slice, Split, Concat (one launch per input), Pad.
struct CopyParams {
  const float* src;
  float* dst;
  long n;
  int nd;
  int size[kMaxDims];
  long dst_stride[kMaxDims], src_stride[kMaxDims];
  int start[kMaxDims], step[kMaxDims], lim[kMaxDims];
  long dst_base, src_base;
  float fill;
};

// dst[dst_base + r * dst_row + i] = src[src_base + r * src_row + i], i < inner,
// r < rows: a Concat / Split / Slice of whole trailing dimensions
struct RowCopyParams {
  const float* src;
  float* dst;
  long inner, rows, src_row, dst_row, src_base, dst_base;
};

struct PoolParams {
  const float* x;
  float* y;
  int N, C, H, W, Ho, Wo, kh, kw, sh, sw, dh, dw, pt, pl;
  int He, We;             // H + bottom pad, W + right pad: where the padded input ends
  int max_mode;           // 1 max, 0 average
  int count_include_pad;  // divide by the window's taps inside the padded input [-pt, He) x [-pl, We)
};

struct RowParams {  // per-row reductions over `inner` contiguous elements (rows = N*C)
  const float* x;
  float* y;
  long rows, inner;
  const float* scale;  // InstanceNormalization gamma [C] (rows % C), beta
  const float* shift;
  int C;
  float eps;
};

// InstanceNormalization of N*C planes of `inner` elements, plane (n, c) at
// x + (n * ctot + c0 + c) * inner (c0 / ctot: an IBNorm's InstanceNorm half
// of a convolution's output, normalised in place), in two parallel passes:
// k_norm_stats writes each `chunk`-element piece's (mean, M2, count), then
// k_norm_apply merges a plane's pieces in order (Chan et al.) and normalises
// its piece, with an optional Relu.
struct NormParams {
  const float* x;
  float* y;  // addressed as x (may be x)
  int N, C, c0, ctot;
  long inner;
  const float* scale;  // [C]
  const float* shift;
  float eps;
  int act;             // ACT_NONE or ACT_RELU
  float* stats;        // [N*C][chunks][3]
  int chunks, chunk;
};

struct AffineParams {  // y = x * scale[c] + shift[c] over NC(HW)
  const float* x;
  float* y;
  long n, inner;
  int C;
  const float* scale;
  const float* shift;
};

// Resize of [N][C][H][W] -> [N][C][Ho][Wo]; ctm: 0 half_pixel, 1 pytorch_half_pixel,
// 2 align_corners, 3 asymmetric; nearest: 0 round_prefer_floor, 1 round_prefer_ceil, 2 floor, 3 ceil
struct ResizeParams {
  const float* x;
  float* y;
  int N, C, H, W, Ho, Wo;
  float sy, sx;  // scales (output / input)
  int linear, ctm, nearest;
  long y_nx;     // as ConvParams::y_nx (C * Ho * Wo + y_nx elements per image)
};

constexpr long kGapWaveMax = 1024;  // k_gap_wave: planes of at most this many elements
struct GemmParams {  // y[b][m][n] = alpha * sum_k A[b][m][k] B[b][k][n] + beta * c
  const float* a;
  const float* b;
  const float* c;     // broadcast over (m, n) with strides cm, cn (0 = broadcast) or null
  float* y;
  int batch, M, N, K;
  long sab, sam, sak;  // A strides (batch, m, k)
  long sbb, sbk, sbn;  // B strides
  long scm, scn;
  float alpha, beta;
  Epilogue ep;         // act only
};

// LayerNormalization of `rows` contiguous rows of D elements (k_layer_norm):
// y = (x - mean) / sqrt(var + eps) * scale[i] + shift[i], the variance taken
// about the mean over the register- or LDS-resident row.  A wave per row up
// to kLnWaveMax elements, a workgroup per row above (the row in LDS up to
// kLnLdsMax elements, re-read from global memory beyond).
constexpr int kLnWaveMax = 1024, kLnLdsMax = 8192;
struct LayerNormParams {
  const float* x;
  float* y;
  long rows;
  int D;
  const float* scale;  // [D] or null (1)
  const float* shift;  // [D] or null (0)
  float eps;
};
const char* layer_norm_name(const LayerNormParams& p);
void launch_layer_norm(const LayerNormParams& p, hipStream_t s);

// Fused attention (vso_attn.hip, k_attn): y[b] = softmax(scale * Q[b] K[b]^T + bias) V[b]
// for b < BH; Q [BH][Nq][d], K [BH][Nk][d], V [BH][Nk][dv], y [BH][Nq][dv], all
// contiguous and 16-byte aligned; d and dv multiples of 4, at most kAttnMaxD.
// bias (or null): [..][Nq][Nk], slice b's plane at bias + sum_k i_k * bstr[k]
// with b unravelled over lead[0 .. nlead) (bstr 0 on a broadcast dim).
constexpr int kAttnMaxD = 128, kAttnMaxLead = kMaxDims - 2;
struct AttnParams {
  const float* q;
  const float* k;
  const float* v;
  const float* bias;
  float* y;
  int BH, Nq, Nk, d, dv;
  float scale;
  int nlead, lead[kAttnMaxLead];
  long bstr[kAttnMaxLead];
};
bool attn_supported(const AttnParams& p);
const char* attn_kernel_name(const AttnParams& p);
void launch_attn(const AttnParams& p, hipStream_t s);

// A class head (vso_head.hip, k_class_head): a reduction of [N][C][Ho][Wo]
// logits over the channel axis, a thread per output pixel (four of a row where
// Wo is a multiple of 4).  The logits are x itself (rz.linear 0: plain form,
// rz.H x rz.W == Ho x Wo), or the linear Resize `rz` of x [N][C][rz.H][rz.W]
// (upsampled form: each logit interpolated on the fly with k_resize's own
// arithmetic, vso_resize.h; the full-size logits are never written).
//   HEAD_SOFTMAX / HEAD_LOGSOFTMAX: classes [c0, c0 + n) of the (log-)softmax
//     over all C -> y [N][n][Ho][Wo] (c0 0, n C: the whole operator);
//   HEAD_ARGMAX: the first (last: select_last_index) index of the maximum, as a
//     float holding the exact integer (C < 2^24) -> y [N][1][Ho][Wo];
//   HEAD_ARGMAX_EQ: 1.0 where that index equals k, else 0.0;
//   HEAD_MAX: the maximum (ReduceMax).
enum HeadOp : int { HEAD_SOFTMAX = 0, HEAD_LOGSOFTMAX = 1, HEAD_ARGMAX = 2, HEAD_ARGMAX_EQ = 3, HEAD_MAX = 4 };
struct HeadParams {
  ResizeParams rz;  // x, N, C, H, W (the source planes), Ho, Wo; sy, sx, ctm and linear 1 in the upsampled form
  float* y;
  int op;           // HeadOp
  int c0, n;        // softmax forms: the classes written
  int last;         // arg forms: select_last_index
  float k;          // HEAD_ARGMAX_EQ: the class compared with
};
const char* head_kernel_name(const HeadParams& p);
void launch_head(const HeadParams& p, hipStream_t s);

// A MobileNetV2 inverted residual block — 1x1 expand + Clip -> 3x3 depthwise
// (stride 1 / 2) + Clip -> 1x1 project (+ the block input) — in one launch
// (vso_ir.hip, k_ir): output tiles of kIrTH x 16 pixels, all output channels,
// a slice of the hidden channels per workgroup (ks slices of cps 16-channel
// chunks, the partial tiles summed in slice order by the last to arrive).
constexpr int kIrTH = 4;
struct IrParams {
  const float* x;     // [N][CIN][H][W]
  const float* w1;    // [HID][CIN], b1 [HID]: expand, then clip to [lo1, hi1]
  const float* b1;
  const float* wdw;   // [9][HID] (tap-major), bdw [HID]: depthwise, then clip to [lo2, hi2]
  const float* bdw;
  const float* w2;    // [COUT][HID], b2 [COUT]: project
  const float* b2;
  // b16 (k_ir_b16, bf16 / f16 sessions): each hidden-channel slice's weights
  // as one contiguous block of sl_bytes (ir_slab_build: the 1x1 weights split
  // into bf16 hi / lo planes in the MFMA operand order, rows padded for
  // conflict-free LDS reads, then the depthwise taps and biases in f32),
  // copied into LDS by the workgroup's prologue; o_*: byte offsets of the
  // parts, s1 / s2: 16-byte slots per W1 / W2 row, o_hid: the hidden planes
  const unsigned char* slab;
  int b16, sl_bytes, o_w1l, o_w2h, o_w2l, o_wd, o_bd, o_b1, o_hid, s1, s2;
  int wv;     // b16 with CIN <= 64: the wave-private form (k_ir_b16w; opt-in, VSO_IR_WAVE=1)
  int probe;  // timing probes (VSO_IR_PROBE, results invalid): 1 no slab DMA, 2 no x loads,
              // 4 no expand MFMAs, 8 no project MFMAs, 16 no split-K exchange
  float* y;           // [N][COUT][Ho][Wo], image n at y + n * (COUT * Ho * Wo + y_nx)
  long y_nx;
  int N, CIN, H, W, HID, COUT, Ho, Wo, stride, res;  // res: + x (stride 1, CIN == COUT)
  float lo1, hi1, lo2, hi2;
  int pstr;           // floats between the staged input channels' rows in LDS (ir_pstr)
  int tiles_x, tiles; // output tiles per tile row / per image (ir_tiles)
  int ks, cps;        // hidden-channel slices per tile, 16-channel chunks per slice
  float* part;        // ks > 1: the slices' partial sums [ks][N][COUT][Ho][Wo] (k_ir_reduce adds them)
};
bool ir_supported(const IrParams& p);
int ir_pstr(int stride);
size_t ir_lds_bytes(const IrParams& p);
// b16: choose the slices (p->cps / ks, LDS budget and ~wgs workgroups) and the
// slab's layout (p->sl_bytes, offsets); then ir_slab_build writes every
// slice's block: w1 [HID][CIN], b1 [HID], wdt [9][HID] (tap-major), bd [HID],
// w2 [COUT][HID]
bool ir_slab_plan(IrParams* p, long wgs, int cps_target);
void ir_slab_build(const IrParams& p, const float* w1, const float* b1, const float* wdt, const float* bd,
                   const float* w2, std::vector<unsigned char>* out);
void ir_tiles(int Ho, int Wo, int* tiles_x, int* tiles);
const char* ir_kernel_name(const IrParams& p);
void launch_ir(const IrParams& p, hipStream_t s);
void launch_ir_reduce(const IrParams& p, hipStream_t s);  // ks > 1: the launch after launch_ir

// ConvTranspose at stride > 1 (vso_deconv.hip).  A transposed convolution of
// stride s is sh * sw stride-1 correlations, one per output phase: with
// t = oy + pt, py = t mod sh and q = t div sh, the taps of phase py are the ky
// with (ky * dh) mod sh == py, and tap ky reads input row q - (ky * dh) div sh;
// likewise in x.  Every phase runs over the same grid of q: rows qy0 ..
// qy0 + Qh - 1, columns qx0 .. qx0 + Qw - 1 (outputs outside [0, Ho) x [0, Wo)
// are not written).  Two kernels:
//  * k_deconv_tile — group 1, dilation 1, at most kDeconvMaxTaps taps per
//    phase and axis: an implicit GEMM per phase on v_mfma_f32_16x16x4_f32
//    (exact f32 products).  A workgroup owns one image, one phase, a
//    kDeconvTH x 16 tile of the phase's pixels (a wave per row) and
//    kDeconvBM output channels; the input channels go in chunks of 16, each
//    chunk's region (tile + taps - 1 rows and columns, zero outside the image)
//    staged in LDS.  At sw == 2 the workgroup computes both x phases from one
//    region (k_deconv_tile<2>: a lane holds two neighbouring outputs, rows go
//    out contiguous); otherwise one phase (k_deconv_tile<1>).  w: packed [phase][tap jy * tmx + jx][Mp][Cp], tap (jy, jx)
//    of phase (py, px) being W[c][m][py + jy * sh][px + jx * sw], zero padded.
//  * k_deconv_direct — any group, dilation and channel count: a VALU gather,
//    kDeconvPx consecutive pixels of one phase row per thread, over the
//    phase's taps (`taps`, enumerated by the planner) x the group's channels.
//    w: the node's [C][Mg][kh][kw].
constexpr int kDeconvTH = 4, kDeconvBM = 64, kDeconvMaxTaps = 4, kDeconvPx = 4;
struct DeconvParams {
  const float* x;  // [N][C][H][W]
  const float* w;
  float* y;        // [N][M][Ho][Wo], image n at y + n * (M * Ho * Wo + y_nx)
  long y_nx;
  int N, C, H, W, M, Ho, Wo;
  int G, Cg, Mg;
  int kh, kw, sh, sw, dh, dw, pt, pl;
  int qy0, qx0, Qh, Qw;
  Epilogue ep;
  // direct: ints [sh + 1] first tap of each y phase, [kh][2] (ky, rows back) by
  // phase, [sw + 1], [kw][2] likewise in x; o_*: where each part starts
  const int* taps;
  int o_yt, o_xs, o_xt;
  // tile: padded channels, the most taps of a phase per axis, pixel tiles per
  // row of tiles / per image, floats between the staged region's rows / channels
  int Mp, Cp, tmy, tmx, tiles_x, tiles, pitch, plane;
  int sx;  // x phases per workgroup: 2 (sw == 2: both, rows stored contiguous) or 1
};
const char* deconv_tile_name(const DeconvParams& p);
void launch_deconv_tile(const DeconvParams& p, hipStream_t s);
void launch_deconv_direct(const DeconvParams& p, hipStream_t s);
size_t deconv_tile_lds(const DeconvParams& p);

// Statically quantised (QDQ) graphs (vso_quant.hip).  A quantised runtime
// tensor is 8 bits per element in HBM — the model's own uint8 / int8 values,
// NCHW, one byte each — and exists between QuantizeLinear and DequantizeLinear
// only; `sgn` says which of the two types the bytes are.
//  * k_quantize: y = saturate(rne(x / scale) + zp) of f32 x; k_dequantize:
//    y = (x - zp) * scale in f32 (scale 1, zp 0: a quantised graph output as
//    the exact integers in float32).
//  * the fused forms end in the same requantisation (Requant): the float value
//    v -> activation (ACT_NONE / ACT_RELU / ACT_CLIP to [lo, hi]) -> v / sy ->
//    round half to even -> + zy -> saturate to [qmin, qmax].
struct QuantParams {
  const float* x;
  unsigned char* y;
  long n;
  float scale;
  int zp, qmin, qmax;
};
struct DequantParams {
  const unsigned char* x;
  float* y;
  long n;
  float scale;
  int zp, sgn;
};
struct Requant {
  float sy;
  int zy, qmin, qmax;
  int act;
  float lo, hi;
};
// k_qconv_tile: DequantizeLinear -> Conv (group 1) [-> Relu / Clip] ->
// QuantizeLinear as an implicit GEMM on v_mfma_i32_16x16x64_i8, K = C * kh * kw
// in the weights' own (c, ky, kx) order, padded with zero weights to Kp (a
// multiple of kQK); w: int8 (Wq - zw) packed [Mp][Kp], Mp = M rounded up to
// kQBM.  The MFMA multiplies signed bytes: a uint8 activation is read as
// xq ^ 0x80 = xq - 128 (xflip 0x80) and carries zx - 128 as its zero point;
// xpad is that zero point as a byte, what a tap outside the image contributes.
// corr[m] = zero point * sum_k w[m][k], so acc - corr[m] = sum (x - zx) w.
// k_qconv_dw: the same pattern of a depthwise Conv (group = C = M) on the VALU,
// w: int8 (Wq - zw) [C][kh * kw]; a tap outside the image is x - zx = 0.
constexpr int kQK = 64, kQBM = 64, kQPix = 64;
struct QConvParams {
  const unsigned char* x;  // [N][C][H][W]
  unsigned char* y;        // [N][M][Ho][Wo]
  const signed char* w;
  const int* corr;         // [M] (k_qconv_tile)
  const float* mult;       // [M]: sx * sw[m]
  const float* bias;       // [M] or null
  int N, C, H, W, M, Ho, Wo;
  int kh, kw, sh, sw, dh, dw, pt, pl;
  int K, Kp, Mp;
  int xflip, xpad;         // k_qconv_tile
  int zx, xsgn;            // k_qconv_dw: the activations' zero point and type
  Requant rq;
};
// k_qadd: Add(DequantizeLinear(a), DequantizeLinear(b)) [-> Relu] -> QuantizeLinear, equal shapes
struct QAddParams {
  const unsigned char* a;
  const unsigned char* b;
  unsigned char* y;
  long n;
  float sa, sb;
  int za, zb, asgn, bsgn;
  Requant rq;
};
void launch_quantize(const QuantParams& p, hipStream_t s);
void launch_dequantize(const DequantParams& p, hipStream_t s);
void launch_qconv_tile(const QConvParams& p, hipStream_t s);
void launch_qconv_dw(const QConvParams& p, hipStream_t s);
void launch_qadd(const QAddParams& p, hipStream_t s);

// Dynamically quantised graphs (vso_dynq.hip): DynamicQuantizeLinear,
// ConvInteger, MatMulInteger.  The byte tensors are the QDQ graphs' (above); an
// int32 runtime tensor (a ConvInteger / MatMulInteger output nothing fused) is
// four bytes per element.
//  * k_dyn_minmax + k_dyn_quantize: DynamicQuantizeLinear of the whole tensor
//    (uint8): `blocks` (min, max) pairs in `part`, reduced again by every
//    workgroup of the second launch; y_scale and y_zero_point stay in HBM.
constexpr int kDynParts = 256;  // (min, max) pairs at the most: one per thread of the second launch
struct DynQParams {
  const float* x;
  unsigned char* y;
  float* scale;        // y_scale, one float
  unsigned char* zp;   // y_zero_point, one byte
  float* part;         // [blocks][2]
  long n;
  int blocks;          // workgroups of k_dyn_minmax, <= kDynParts
};
//  * k_iconv_tile (group 1, K < 2^15) and k_iconv_direct (any group): the exact
//    sum_k (x - zx) (w - zw[m]) of ConvInteger, and of MatMulInteger as the 1x1
//    convolution of N = rows, C = K, H = W = 1.  zx is one byte in HBM, read by
//    the kernel (null: 0).  w holds signed bytes w' = Wq - 128 (uint8 weights)
//    or Wq (int8), zw[m] their zero point moved alike (null: all 0), wsum[m] =
//    sum_k w'[m][k].  k_iconv_tile: w packed [Mp][Kp] as k_qconv_tile's, the
//    activations read as x ^ xflip; k_iconv_direct: w [M][Cg * kh * kw].
//    Epilogue: yi (int32) — or, yi null, yf = act(float(v) * (xscale[0] *
//    wscale[m]) + bias[m]), every step rounded once: the roundings of the
//    launches Cast, Mul, Mul, Add, Relu | Clip it stands for.
struct IConvParams {
  const unsigned char* x;   // [N][C][H][W]
  const unsigned char* zx;  // the activations' zero point (their type), or null
  const signed char* w;
  const int* wsum;          // [M] (k_iconv_tile)
  const int* zw;            // [M] or null
  int* yi;                  // [N][M][Ho][Wo], or null: the float epilogue
  float* yf;
  const float* xscale;      // one float in HBM
  const float* wscale;      // [M]
  const float* bias;        // [M] or null
  int act;                  // ACT_NONE / ACT_RELU / ACT_CLIP
  float lo, hi;
  int N, C, H, W, M, Ho, Wo;
  int G, Cg, Mg;
  int kh, kw, sh, sw, dh, dw, pt, pl;
  int K, Kp, Mp;
  int xflip;                // 0x80: uint8 activations, 0: int8
  int rows;                 // k_iconv_tile: H = W = 1, 1x1, no pads — a pixel's K bytes are contiguous (MatMulInteger)
};
void launch_dyn_minmax(const DynQParams& p, hipStream_t s);
void launch_dyn_quantize(const DynQParams& p, hipStream_t s);
void launch_iconv_tile(const IConvParams& p, hipStream_t s);
void launch_iconv_direct(const IConvParams& p, hipStream_t s);
int dyn_blocks(long n);  // k_dyn_minmax's workgroups for n elements
// Cast of an int32 runtime tensor to float32 (vso_kernels.hip)
struct CastI32Params {
  const int* x;
  float* y;
  long n;
};
void launch_cast_i32(const CastI32Params& p, hipStream_t s);

const char* conv_kernel_name(const ConvParams& p);
// a depthwise -> 1x1 pair of N images of P pixels into M channels runs fused
// on k_conv_pw (vso_kernels.hip: where that measured faster)
bool pw_fused_pays(int N, long P, int M);
// the same decision with pw_kernel's 32-bit offset limits: a C-channel depthwise
// over pre_hw input pixels per image into P output pixels, then 1x1 to M
// channels — what the planner must ask before deferring a depthwise whose
// channels exceed k_conv_dwpw's LDS tile (kDwPwMaxC)
bool pw_pair_fits(int N, long C, long pre_hw, long P, int M);
// false: not a k_conv_tile convolution (grouped, dilated, other kernel sizes)
bool conv_tile_shape(const ConvParams& p, int prec, ConvTileShape* sh);
const char* conv_tile_name(const ConvTileShape& t);
void launch_conv_tile(const ConvTileParams& p, const ConvTileShape& t, hipStream_t s);

void launch_conv(const ConvParams& p, hipStream_t s, const char** name);

// k_conv_thin: a 1x1 convolution to at most kThinMaxM output channels (a
// matte / logit head) — a per-pixel dot product over the input channels on
// the VALU, 4 pixels per thread — optionally normalising input channels
// [norm.c0, norm.c0 + norm.C) on the way in: an InstanceNorm (+ Relu) whose
// statistics k_norm_stats computed (NormParams, its apply step not launched:
// the IBNorm in front of MODNet's matte head)
constexpr int kThinMaxM = 4;
bool thin_conv_fits(const ConvParams& p);
void launch_conv_thin(const ConvParams& p, const NormParams* norm, hipStream_t s);
const char* conv_thin_name(int M);
void launch_binary(const BinParams& p, hipStream_t s);
void launch_unary(const UnaryParams& p, hipStream_t s);
void launch_copy(const CopyParams& p, hipStream_t s);
void launch_copy_rows(const RowCopyParams& p, hipStream_t s);
const char* row_copy_name(const RowCopyParams& p);
void launch_pool(const PoolParams& p, hipStream_t s);
void launch_gap(const RowParams& p, hipStream_t s);
void launch_norm_stats(const NormParams& p, hipStream_t s);
void launch_norm_apply(const NormParams& p, hipStream_t s);
// k_norm_plane: statistics and apply of planes up to kNormPlaneMax elements in one launch
constexpr long kNormPlaneMax = 36864;
bool norm_plane_fits(long inner);
const char* norm_plane_name(long inner);
void launch_norm_plane(const NormParams& p, hipStream_t s);
constexpr int kNormChunk = 4096;  // elements per k_norm_stats / k_norm_apply workgroup
void launch_softmax(const RowParams& p, hipStream_t s);
void launch_affine(const AffineParams& p, hipStream_t s);
const char* resize_kernel_name(const ResizeParams& p);  // the kernel launch_resize picks (profiles)
void launch_resize(const ResizeParams& p, hipStream_t s);
void launch_gemm(const GemmParams& p, hipStream_t s);
bool gemm_vec(const GemmParams& p);
const char* binary_kernel_name(const BinParams& p);
const char* gap_kernel_name(const RowParams& p);
const char* gemm_kernel_name(const GemmParams& p);

}  // namespace vso
