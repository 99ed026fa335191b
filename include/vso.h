/*
 * vso.h — ONNX model sessions on gfx950: the part of onnxruntime-web the
 * reference uses to run its models, behind the same kind of C ABI as
 * ORT-web's own wasm exports (client/public/ort-wasm-simd-threaded.mjs:50-53).
 *
 * The reference creates ORT sessions for MODNet (initializeModnet,
 * client/src/core/model.ts:12-29; the weights file model_q4f16.onnx is absent
 * here), the MediaPipe face detector (initializeFaceDetector, model.ts:36-53,
 * client/src/assets/MediaPipeFaceDetector.onnx) and the landmark model
 * (initializeLandmarks, model.ts:58-67), and calls session.run on them
 * (frameProcessorTest.ts:91, :406, :478).  A vso_session parses an ONNX
 * ModelProto with its own protobuf reader, infers every shape for the
 * session's input shape, folds the shape arithmetic, and runs the graph as a
 * fixed list of HIP kernels (dense convolutions as implicit GEMMs on MFMA —
 * f32, or bf16 / f16 operands by option — depthwise convolutions direct, activations and
 * residual adds fused into the convolution epilogues), replayed from a
 * hipGraph.  Tensors are float32 NCHW.
 *
 * Supported operators: Conv, ConvTranspose, Relu, PRelu, LeakyRelu, Clip,
 * Sigmoid, Tanh, HardSigmoid, HardSwish, Gelu, Erf, Add, Sub, Mul, Div (numpy
 * broadcasting), MaxPool, AveragePool, GlobalAveragePool, ReduceMean (over H
 * and W; over the last axis inside a decomposed LayerNorm), Pad (constant),
 * Concat, Split, Slice, Transpose,
 * Reshape, Flatten, Squeeze, Unsqueeze, Identity, Dropout, Cast (float; of
 * an index tensor also INT64, INT32, UINT8),
 * Resize/Upsample (nearest, linear; half_pixel, pytorch_half_pixel,
 * align_corners, asymmetric), InstanceNormalization, BatchNormalization,
 * LayerNormalization, MatMul, Gemm, Softmax, LogSoftmax, ArgMax, ReduceMax
 * (the last three over the channel axis), Gather (one constant index), Equal
 * (inside ArgMax -> Equal -> Cast), Pow and Sqrt (inside a
 * decomposed LayerNorm), and Shape, Gather, Constant, ConstantOfShape,
 * Floor, Ceil, Cast, Sqrt, Erf, Pow on constants; QuantizeLinear and
 * DequantizeLinear of runtime tensors (statically quantised models in the QDQ
 * format, below); DynamicQuantizeLinear, ConvInteger and MatMulInteger
 * (dynamically quantised models, what quantize_dynamic writes, below).  For q4f16 exports (model_q4f16.onnx's
 * form): float16 initializers, Cast to FLOAT16 (values rounded to halves and
 * kept as f32; later ops compute in f32), DequantizeLinear of int8 / uint8 /
 * int4 / uint4 weights (per tensor, per axis, opset-21 blocks; folded at
 * create) and com.microsoft MatMulNBits (4-bit blocks, packed uint8 zero
 * points, bias; dequantised once at create).  Anything else fails vso_create
 * with VSO_E_UNSUPPORTED naming the node.
 *
 * Attributes (tests/op_cases.py, tests/op_cases_deconv.py and
 * tests/op_cases_attn.py, tests/op_cases_head.py, tests/op_cases_quant.py and
 * tests/op_cases_dynq.py are the tables the sessions are held to):
 *   opset_import          read; it selects Softmax's form and Split's default.
 *   Conv                  2-D, constant weights and bias; group, strides,
 *                         dilations (0 or 2 values each), pads (0 or 4 values),
 *                         auto_pad (it wins over pads); kernel_shape is taken
 *                         from the weights.  Refused: any other list length,
 *                         channels that do not match the weights and group, an
 *                         empty output.
 *   ConvTranspose         2-D: X [N,C,H,W], constant W [C, M/group, kh, kw] and
 *                         optional constant B [M]; group, strides, dilations,
 *                         output_padding (0 or 2 values each), pads (0 or 4
 *                         values), auto_pad, output_shape (2 values);
 *                         kernel_shape is taken from the weights.  Per axis
 *                         Ho = s (H - 1) + output_padding + (k - 1) d + 1 -
 *                         pad_begin - pad_end, and Y[n, g Mg + m, oy, ox] = B +
 *                         the sum over the group's c and ky, kx of X[n, c, iy,
 *                         ix] W[c, m, ky, kx] with oy = iy s + ky d - pad_begin.
 *                         With output_shape (it wins over pads) or auto_pad
 *                         SAME_UPPER / SAME_LOWER (the output is H s) the total
 *                         padding is derived from the size and split as the
 *                         ONNX operator text says — SAME_UPPER: total / 2 at the
 *                         beginning, otherwise total - total / 2 — which matters
 *                         for an odd total only; PyTorch has no such attribute
 *                         to compare with: the operator text is the authority.
 *                         VALID: zero pads.  Refused: runtime weights, channels
 *                         that do not match the weights and group, an
 *                         output_padding not below max(stride, dilation) on its
 *                         axis, negative pads (given or derived), any other
 *                         list length, an empty output, tensors of 2^31
 *                         elements or more, a stride, dilation or kernel side
 *                         above 1024.  Computed on f32 operands in every
 *                         session: conv_precision does not round it (as the
 *                         1x1, grouped and inverted-residual convolutions).
 *                         It absorbs a following BatchNormalization, residual
 *                         Add and activation as Conv does.  Stride 1 runs as
 *                         the Conv it equals (flipped weights, pads d (k - 1) -
 *                         pads); other strides as one stride-1 correlation per
 *                         output phase (vso_deconv.hip), see below.
 *   HardSigmoid           alpha (0.2), beta (0.5): max(0, min(1, alpha x + beta)).
 *   HardSwish             x max(0, min(1, x / 6 + 0.5)).  Both run in the
 *                         epilogue of a producing Conv, ConvTranspose, Gemm or
 *                         MatMul; so does Mul(x, HardSigmoid(x)), the
 *                         hard-swish of exports before opset 14, for any alpha
 *                         and beta, when that Mul is the HardSigmoid's only
 *                         consumer (one activation, x clamp(alpha x + beta)).
 *   LayerNormalization    opset 17; input of rank >= 2; axis (default -1,
 *                         negative forms accepted): the normalised extent D is
 *                         the product of the dims from axis on, the rest are
 *                         rows; epsilon (1e-5); constant Scale of D elements
 *                         and optional constant B.  y = (x - mean) / sqrt(var +
 *                         epsilon) * Scale + B, the variance taken about the
 *                         mean over the resident row (never E[x^2] - mean^2),
 *                         one k_layer_norm launch: a wave per row up to D =
 *                         1024, a workgroup per row above.  The form PyTorch
 *                         exports below opset 17 — ReduceMean(x, axes [-1],
 *                         keepdims 1) -> Sub -> Pow(., 2) or Mul(d, d) ->
 *                         ReduceMean -> Add(eps) -> Sqrt -> Div [-> Mul(gamma)]
 *                         [-> Add(beta)], eps a scalar, gamma / beta constants
 *                         of 1 or D elements, every interior value read inside
 *                         the pattern only — is the same one launch.  Refused:
 *                         a runtime Scale or B, a used Mean / InvStdDev
 *                         output, stash_type other than 1; outside the pattern
 *                         (the difference read a third time, keepdims 0,
 *                         another axis) a ReduceMean over a non-spatial axis
 *                         set, Pow and Sqrt of runtime tensors stay refused.
 *   Gelu, Erf             Gelu (opset 20): approximate none (0.5 x (1 + erf(x /
 *                         sqrt 2))) or tanh.  Erf: elementwise.  The erf form
 *                         of older exports, x * 0.5 * (1 + Erf(x / sqrt 2)) —
 *                         either association of the product, Div by sqrt 2 or
 *                         Mul by 1 / sqrt 2, the constants matched to 1e-6
 *                         relative — is the same one activation.  All three
 *                         run in the epilogue of a producing Conv,
 *                         ConvTranspose, Gemm or MatMul when they are all that
 *                         reads it, else as one elementwise launch.  A
 *                         constant that misses (0.7 for 0.70710678) leaves the
 *                         nodes as they are: five launches, the same values.
 *                         Refused: any other approximate.
 *   ReduceMean            rank-4 input; axes (attribute, or constant input from
 *                         opset 18) exactly the two spatial axes, negative
 *                         forms accepted; keepdims 0 or 1;
 *                         noop_with_empty_axes.  Runs on GlobalAveragePool's
 *                         kernels.  Refused: every other axis set or rank.
 *   MaxPool, AveragePool  kernel_shape, strides, dilations, pads (0 or 4
 *                         values), auto_pad, ceil_mode, count_include_pad: the
 *                         divisor is the window's taps inside the padded input
 *                         (a ceil_mode window reaching past the padding is cut
 *                         there first, as ONNX's reference implementation and
 *                         PyTorch do).  Refused: storage_order 1, MaxPool's
 *                         Indices output, any other pads length.
 *   Resize                mode nearest / linear, the four coordinate
 *                         transformations above, nearest_mode
 *                         round_prefer_floor / round_prefer_ceil / floor /
 *                         ceil, constant scales or sizes on H and W.  Upsample:
 *                         asymmetric, floor.  Refused: cubic, antialias, axes,
 *                         keep_aspect_ratio_policy other than stretch, any
 *                         other nearest_mode or transformation.
 *   PRelu                 the slope broadcasts to the input as ONNX says (a
 *                         1-D slope aligns with W); [C,1,1], [1,C,1,1] or one
 *                         value after a Conv run in its epilogue.  Refused: a
 *                         slope that does not broadcast to the input.
 *   Clip                  min / max as attributes or constant inputs, either
 *                         or both absent.
 *   Pad                   constant mode; constant pads (negative: crop), value
 *                         and axes.  Refused: reflect, edge, wrap.
 *   Slice                 constant starts / ends / axes / steps (inputs, or
 *                         attributes before opset 10), negative steps and
 *                         indices, ends clamped.
 *   Split                 sizes by input or attribute; else equal parts, from
 *                         opset 18 on ceil-sized with a smaller last part.
 *                         Refused: an uneven default split below opset 18.
 *   Gemm                  transA, transB, alpha, beta, C broadcast to [M, N].
 *   MatMul                B of rank 2, of batch 1, or batched like A.  By a
 *                         constant B, a following Add of a constant [N] (or
 *                         [1, .., N]) that is all that reads the product is the
 *                         launch's bias (a Linear layer), and an activation
 *                         behind it is still absorbed.
 *   attention             MatMul(Q, Transpose(K: the last two axes swapped)) [->
 *                         Mul or Div by a constant scalar] [-> Add(bias)] ->
 *                         Softmax(last axis) -> MatMul(., V) is one k_attn
 *                         launch that never writes the scores (vso_attn_count,
 *                         below): Q [.., Nq, d], K [.., Nk, d], V [.., Nk, dv]
 *                         runtime tensors with equal leading dims; every
 *                         interior value read by the next node only; the bias
 *                         constant or runtime, its last two dims [Nq, Nk], its
 *                         leading ones 1 or Q's; a Mul by a constant scalar on
 *                         Q or on K in front of the first MatMul, read by it
 *                         only, is taken too; d and dv multiples of 4 up to
 *                         128.  The K Transpose launches nothing when the
 *                         pattern is all that reads it.  Anything else — the
 *                         Softmax read elsewhere, other axes transposed, d = 6
 *                         or 132, a constant K — keeps the five launches.
 *   Softmax               the last axis; below opset 13 the input flattened to
 *                         2-D at axis (default 1), every row normalised.  From
 *                         opset 13 on also the channel axis (1 or -3) of rank-4
 *                         input: a class head, below.  Refused: any other axis
 *                         from opset 13 on.
 *   LogSoftmax            opset 13 on, the channel axis (1 or -3) of rank-4
 *                         input: x - max - log(sum exp(x - max)).  Refused: any
 *                         other axis, rank or opset.
 *   ArgMax                rank-4 input, axis 1 or -3; keepdims 0 or 1;
 *                         select_last_index 0 (the first index of the maximum)
 *                         or 1 (the last); fewer than 2^24 classes.  The result
 *                         is an index tensor: float32 in HBM holding the exact
 *                         integer (vso_output_type).  Refused: any other axis or
 *                         rank.
 *   ReduceMax             rank-4 input; axes (attribute, or constant input from
 *                         opset 18) exactly [1] or [-3]; keepdims 0 or 1.
 *                         Refused: every other axis set or rank.
 *   class heads           each of the four above is one k_class_head launch
 *                         (vso_head.hip: a thread per pixel, the classes reduced
 *                         in registers).  Fused into that launch, every interior
 *                         value read by the next node only (vso_head_count):
 *                         a linear Resize (any of the four transformations,
 *                         constant scales or sizes) in front of it — each logit
 *                         interpolated on the fly with k_resize's arithmetic, the
 *                         full-size logits never written; behind a Softmax, a
 *                         Slice (axis 1, step 1), a Split with one used output
 *                         or a Gather (axis 1, one constant index) — only those
 *                         channels are written; behind an ArgMax, Equal(constant
 *                         scalar, int64 or float) -> Cast(to FLOAT) — 1.0 where
 *                         the label is that class.  A near miss (the Resize or
 *                         the Softmax read twice, a nearest Resize, a Slice with
 *                         step 2) keeps separate launches with the same values.
 *   Equal                 inside ArgMax -> Equal -> Cast only.  Refused elsewhere.
 *   Gather                of a runtime tensor: a constant scalar or one-element
 *                         index (negative accepted), any axis; a strided copy,
 *                         the axis dropped for a scalar index.  Refused: any
 *                         other index shape, a runtime index.
 *   Cast                  to FLOAT: an alias; to FLOAT16: rounded to halves;
 *                         of an index tensor (an ArgMax result or a view of it)
 *                         to INT64, INT32 or UINT8: an alias; of an int32
 *                         tensor (ConvInteger, MatMulInteger) to FLOAT: one
 *                         conversion per element (k_cast_i32).  Refused: any
 *                         other runtime tensor to a non-float type.
 *   QuantizeLinear        opset 10 to 21, of a runtime float32 tensor: y =
 *                         saturate(round_half_even(x / y_scale) + y_zero_point),
 *                         a quantised tensor of the zero point's type — uint8
 *                         [0, 255] (also when it is absent) or int8 [-128,
 *                         127] — one byte per element in HBM.  Scale and zero
 *                         point: constants of one element.  One k_quantize
 *                         launch.  Refused: a runtime scale or zero point,
 *                         per-axis or blocked quantisation, a zero point (or
 *                         output_dtype) of any other type — 16-bit, 4-bit,
 *                         float8 —, saturate 0.
 *   DequantizeLinear      of a runtime quantised tensor: (x - zero_point) *
 *                         scale in float32, the same restrictions, one
 *                         k_dequantize launch; of constants (weights, int32
 *                         biases): folded at create, as before.  Refused: a
 *                         runtime input that is not a quantised tensor.  Only
 *                         DequantizeLinear may read a quantised tensor: any
 *                         other operator on one is refused.  A quantised graph
 *                         output follows the index tensors' convention: the
 *                         buffer holds the exact integers in float32 and
 *                         vso_output_type reports 2 (UINT8) or 3 (INT8).
 *   quantised patterns    between a DequantizeLinear and a QuantizeLinear, three
 *                         patterns run on the integers, one launch each
 *                         (vso_qconv_count), every interior value read by the
 *                         next node only: DequantizeLinear(xq) -> Conv(.,
 *                         DequantizeLinear(Wq), [B]) [-> Relu | Clip(constant
 *                         bounds)] -> QuantizeLinear with group 1 (k_qconv_tile,
 *                         v_mfma_i32_16x16x64_i8, any kernel, stride, dilation
 *                         and pads) or depthwise (k_qconv_dw: group = C, kernel
 *                         up to 7x7, stride 1 or 2) — Wq a constant int8 /
 *                         uint8 tensor, scale and zero point per tensor or per
 *                         output channel (axis 0), Wq - zero point within int8;
 *                         B a float constant or DequantizeLinear of an int32
 *                         one — and Add(DequantizeLinear(a), DequantizeLinear(b))
 *                         [-> Relu] -> QuantizeLinear of equal shapes (k_qadd).
 *                         A near miss (a DequantizeLinear or the Conv read
 *                         twice, weights that leave int8) keeps k_dequantize,
 *                         the float kernel and k_quantize: the same values
 *                         wherever float32 is exact.  Everything else between
 *                         Q / DQ pairs (Resize, pools, Concat, Gemm, MatMul,
 *                         ConvTranspose) runs that way too.  QLinearConv,
 *                         QLinearMatMul and QLinearAdd (the QOperator format)
 *                         are refused.
 *   DynamicQuantizeLinear opset 11, of a runtime float32 tensor, the whole
 *                         tensor (batch included), uint8.  The operator text
 *                         in float32, each step rounded once: mn = min(0, min
 *                         x), mx = max(0, max x), y_scale = (mx - mn) / 255,
 *                         y_zero_point = saturate(rne((0 - mn) / y_scale)), y =
 *                         saturate(rne(x / y_scale) + y_zero_point); mx == mn
 *                         (all zero; left open by the text) gives scale 1, zero
 *                         point 0, y 0, as onnxruntime does.  Two launches
 *                         (k_dyn_minmax, k_dyn_quantize); nothing goes back to
 *                         the host: y is a quantised uint8 tensor, y_scale a
 *                         float32 runtime tensor of rank 0, y_zero_point a
 *                         one-element quantised tensor, each a legal graph
 *                         output (y and the zero point as UINT8).  y is read by
 *                         ConvInteger / MatMulInteger (input 0) or
 *                         DequantizeLinear only, the zero point as their input 2
 *                         only; y_scale is a float like any other.
 *   ConvInteger /         input 0 a quantised runtime tensor (uint8 / int8),
 *   MatMulInteger         its zero point (input 2) one value of that type —
 *                         a DynamicQuantizeLinear's, or a constant —; the
 *                         weights (W; B of rank 2) a constant uint8 / int8
 *                         tensor, their zero point (input 3) a constant of the
 *                         same type, one value or one per output channel /
 *                         column.  ConvInteger: auto_pad, dilations, group,
 *                         kernel_shape, pads, strides as Conv (the same list
 *                         lengths and refusals).  The exact int32 sum of
 *                         (x - x_zero_point)(w - w_zero_point): group 1 and
 *                         C kh kw < 2^15 on k_iconv_tile
 *                         (v_mfma_i32_16x16x64_i8; MatMulInteger as its 1x1
 *                         case, rows as pixels), anything else on
 *                         k_iconv_direct.  The int32 tensor is read by Cast to
 *                         FLOAT only (k_cast_i32) and is no graph output.
 *                         Refused: runtime weights, an input 0 that is not a
 *                         quantised tensor, a runtime weight zero point, a zero
 *                         point of the wrong size or type, a B of rank other
 *                         than 2.
 *   dynamic patterns      ConvInteger | MatMulInteger -> Cast(FLOAT) -> Mul(., s)
 *                         [-> Add(constant bias)] [-> Relu | Clip(constant
 *                         bounds)] with s = Mul(x_scale, w_scale) in either
 *                         operand order — x_scale the y_scale of the
 *                         DynamicQuantizeLinear that made input 0, w_scale and
 *                         the bias constants of one value (w_scale) or one per
 *                         output channel lying along the channel axis ([M,1,1],
 *                         [1,M,1,1] behind a ConvInteger, [N] behind a
 *                         MatMulInteger), every interior value and s read by
 *                         the next node only — is one launch (vso_dynq_count)
 *                         storing float32 act(float(acc) * (x_scale *
 *                         w_scale[m]) + bias[m]), each step rounded once: bit
 *                         for bit what the separate launches store.  The
 *                         DynamicQuantizeLinear is not part of the pattern: it
 *                         may feed several layers.  A near miss (the Cast or s
 *                         read twice, a runtime bias, a w_scale of another size
 *                         or along another axis) keeps every node's own launch.
 *   BatchNormalization    constant parameters, rank >= 2 (inference form).
 *   InstanceNormalization constant scale and B, rank >= 3.
 *
 * Errors: int returns are 0 or a negative code, message in vso_last_error
 * (thread-local when the session is NULL), like _OrtGetLastError (:50).
 * One call in flight per session.
 */
#ifndef VSO_H_
#define VSO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  VSO_OK = 0,
  VSO_E_INVALID_ARG = -1,
  VSO_E_HIP = -2,
  VSO_E_PARSE = -3,
  VSO_E_UNSUPPORTED = -4,
  VSO_E_OOM = -5
};

typedef struct vso_session vso_session;

/* Session options (the part of ORT's SessionOptions this runtime has).
 * conv_precision: operands of the dense k x k convolutions (k_conv_tile,
 * vso_conv.hip) — VSO_PRECISION_F32: exact f32 products
 * (v_mfma_f32_16x16x4_f32), the default; _BF16 / _F16: activations and weights
 * rounded to bfloat16 / float16 (nearest even) on
 * v_mfma_f32_16x16x32_{bf16,f16}, f32 accumulation.  _F16 keeps every
 * float16-typed weight of a q4f16 export exact. */
enum { VSO_PRECISION_F32 = 0, VSO_PRECISION_BF16 = 1, VSO_PRECISION_F16 = 2 };
typedef struct vso_options {
  int conv_precision;
  int reserved[7];
} vso_options;

void vso_options_default(vso_options* o);

/* Replaces InferenceSession.create(url) (model.ts:14) / _OrtCreateSession(modelPtr,
 * len, opts) (ort-wasm-simd-threaded.mjs:51): model = the ONNX file's bytes.
 * input_dims/input_ndim: the shape of input 0 when the model leaves dims
 * symbolic (NULL/0 = the model's own static shape).  device_id: HIP ordinal. */
int vso_create(const void* model, size_t bytes, const int64_t* input_dims, int input_ndim, int device_id,
               vso_session** out);

/* vso_create with options (NULL = vso_options_default): InferenceSession.create(url, options). */
int vso_create_ex(const void* model, size_t bytes, const int64_t* input_dims, int input_ndim, int device_id,
                  const vso_options* opts, vso_session** out);

/* Replaces InferenceSession.release / _OrtReleaseSession (:51). */
void vso_destroy(vso_session* s);

/* Replaces _OrtGetLastError (:50). */
const char* vso_last_error(const vso_session* s);

/* Replaces _OrtGetInputOutputCount (:51). */
int vso_io_count(const vso_session* s, int* n_inputs, int* n_outputs);

/* Names (session.inputNames / outputNames) and shapes of inputs / outputs:
 * return the string length / the rank, or a negative code. */
int vso_input_name(const vso_session* s, int i, char* buf, int cap);
int vso_output_name(const vso_session* s, int i, char* buf, int cap);
int vso_input_shape(const vso_session* s, int i, int64_t* dims, int cap);
int vso_output_shape(const vso_session* s, int i, int64_t* dims, int cap);
/* Output i's element type as the model declares it, an ONNX TensorProto code:
 * 1 FLOAT, 7 INT64, 6 INT32, 2 UINT8 (1 when the model states none); a quantised
 * output reports its own type, 2 UINT8 or 3 INT8, whatever the model declares.
 * The buffers vso_run and vso_run_device fill are float32 whatever it returns —
 * an integer-typed output (ArgMax labels, a quantised tensor) holds exact
 * integers in float32, as a float16-typed value holds exact halves; the hosts
 * convert (ort.py, segment.ts). */
int vso_output_type(const vso_session* s, int i);

/* Replaces session.run(feeds) (frameProcessorTest.ts:91) / _OrtRun (:53) for
 * host buffers: inputs[i] = float32 data of input i (its shape as above),
 * outputs[i] = room for output i.  Synchronous. */
int vso_run(vso_session* s, const float* const* inputs, float* const* outputs);

/* Device-resident variant: HBM pointers, enqueued on `stream` (hipStream_t;
 * NULL = the session's stream), not waited for. */
int vso_run_device(vso_session* s, const float* const* d_inputs, float* const* d_outputs, void* stream);

/* Introspection: the number of kernel launches per run, and launch k's
 * kernel name as rocprofv3 reports it (returns the string length). */
int vso_launch_count(const vso_session* s);
int vso_launch_name(const vso_session* s, int k, char* buf, int cap);
/* Convolutions planned on the LDS-tiled MFMA kernel (k_conv_tile). */
int vso_tile_conv_count(const vso_session* s);
/* Inverted residual blocks (1x1 expand -> Clip -> 3x3 depthwise -> Clip -> 1x1
 * project [-> + input]) the session runs as one fused launch each (MODNet's
 * MobileNetV2 backbone): k_ir in f32 sessions, k_ir_b16 (bf16 hi / lo splits
 * of both 1x1 operands, ~f32 precision) in bf16 / f16 ones, plus a
 * k_ir_reduce launch when the hidden channels are split over workgroups.
 * A block fuses when its input channels are a multiple of 4, its hidden ones
 * of 16, its depthwise is 3x3 / pads 1 / stride 1 or 2, and (CIN, COUT,
 * stride) has a kernel instance.  f32, by (ceil(CIN / 16), ceil(COUT / 16),
 * stride): (1,2,2) (2,2,1) (2,2,2) (2,4,2) (4,4,1) (4,6,1) (6,6,1) (6,10,2)
 * (10,10,1) (10,20,1) (4,4,2) (6,6,2) — MobileNetV2's 16->24 s2, 24->24,
 * 24->32 s2, 32->64 s2, 64->64, 64->96, 96->96, 96->160 s2, 160->160,
 * 160->320, 64->64 s2, 96->96 s2 and every pair that rounds to the same
 * steps (20->20, 28->49 s2, 148->305 ...).  bf16 / f16, by (ceil(CIN / 32),
 * ceil(COUT / 16), stride): (1,2,2) (1,2,1) (1,4,2) (2,4,1) (2,6,1) (3,6,1)
 * (3,10,2) (5,10,1) (5,20,1) (2,4,2) (3,6,2) — the same blocks, and 16->24
 * and 48->64 at stride 1, which have no f32 instance (there the block runs as
 * two or three generic launches).  A block whose project feeds the Add of a
 * strided residual (MaxPool 2x2 [+ channel Pad] of the block's input:
 * BlazeFace) is left to the generic plan, whose epilogue reads the pool's input.
 * Planning knobs, read once per process: VSO_IR=0 plans them as three
 * launches; VSO_IR_B16=0 keeps the f32 form in 16-bit sessions; VSO_IR_CPS
 * (default 6) hidden 16-channel chunks per slice of a 16-bit block. */
int vso_ir_block_count(const vso_session* s);
/* Attention patterns (see "attention" above) the session runs as one fused
 * launch each (vso_attn.hip, k_attn): a 256-thread workgroup owns one slice of
 * the leading dims and 64 query rows, walks the keys in blocks of 32 staged in
 * LDS, keeps the running row maximum and sum in registers (exp only of the
 * difference from the maximum) and writes the output once; both products on
 * v_mfma_f32_16x16x4_f32 (exact f32 products) in every session precision, so
 * bf16 / f16 sessions are bitwise the f32 one on these nodes.  Planning knob,
 * read once per process: VSO_ATTN=0 keeps the Transpose, MatMul, scale, bias,
 * Softmax and MatMul launches; its outputs meet the same 1e-4 bar against the
 * float64 reference but are not bitwise the fused ones (another order of the
 * same sums). */
int vso_attn_count(const vso_session* s);
/* Class heads (see "class heads" above) whose launch stands for more than its
 * own node: a Resize in front, a channel selection or Equal -> Cast behind.
 * The head computes on f32 operands in every session precision.  Planning
 * knob, read once per process: VSO_HEAD=0 keeps the Resize (k_resize), the
 * plain head and the selection's copy as launches of their own — the same
 * device functions in the same order, so its outputs are bitwise the fused
 * plan's (ArgMax -> Equal -> Cast stays one launch: Equal has no kernel). */
int vso_head_count(const vso_session* s);
/* Quantised patterns (see "quantised patterns" above) the session runs on the
 * integers, one launch each: k_qconv_tile + k_qconv_dw + k_qadd (vso_quant.hip).
 * k_qconv_tile: an implicit GEMM over K = C kh kw on v_mfma_i32_16x16x64_i8 —
 * 8-bit activations read (uint8 with the top bit flipped, the zero point folded
 * as sum x w - zx sum w, spatial padding contributing zx), int32 accumulation,
 * the requantisation acc (sx sw[m]) + bias[m] -> activation -> / sy -> round
 * half to even -> + zy -> saturate in the epilogue, 8-bit activations written.
 * They compute in integers in every session precision: bf16 / f16 sessions are
 * bitwise the f32 one on them.  Planning knob, read once per process:
 * VSO_QDQ=0 plans every pattern as k_dequantize, the float kernel, k_quantize. */
int vso_qconv_count(const vso_session* s);
/* Dynamic patterns (see "dynamic patterns" above) the session runs as one
 * launch each: k_iconv_tile + k_iconv_direct with the float epilogue
 * (vso_dynq.hip).  k_iconv_tile is k_qconv_tile's implicit GEMM with the
 * activations' zero point read from HBM and the weights' zero point kept out
 * of the bytes: with signed bytes x' = x - 128, w' = w - 128 (uint8; int8 as
 * they are) and zero points moved alike, sum (x - zx)(w - zw[m]) = acc - zx'
 * sum_k w'[m] - zw'[m] sum_k x'[pixel] + K zx' zw'[m] in wrapping 32-bit
 * arithmetic, the window sum of x' taken by the threads that stage it.  They
 * compute in integers in every session precision: bf16 / f16 sessions are
 * bitwise the f32 one on them.  Planning knob, read once per process:
 * VSO_DYNQ=0 plans every pattern as the integer launch, k_cast_i32 and the
 * Mul / Add / Relu / Clip launches — the same bits. */
int vso_dynq_count(const vso_session* s);
/* ConvTranspose at a stride above 1 (vso_deconv.hip): per output phase
 * ((oy + pad) mod stride, per axis) one stride-1 correlation over the taps
 * ky = phase + j stride, 1 / (sh sw) of the zero-stuffed form's multiply-adds.
 * k_deconv_tile — group 1, dilation 1, at least 16 input and 16 output
 * channels, at most 4 taps per phase and axis: an implicit GEMM per phase on
 * v_mfma_f32_16x16x4_f32 (exact f32 products); at stride 2 in x with 1024
 * workgroups or more both x phases come from one workgroup and rows are stored
 * contiguous (k_deconv_tile<2>, else <1>).  k_deconv_direct — groups
 * (depthwise), dilations, thin channel counts (a one-channel matte head), and
 * stride 1 with pads beyond d (k - 1): a gather on the VALU.  Planning knobs,
 * read once per process: VSO_DECONV_TILE=0 plans every one on k_deconv_direct;
 * VSO_DECONV_PAIR=0 / 1 forces k_deconv_tile<1> / <2> at stride 2 in x. */
/* Lanes of the captured graph (0 before the first run): launches that share no
 * activation buffer run on two capture streams, so independent branches of
 * the model (MODNet's HR branch beside its backbone) execute concurrently —
 * for sessions whose input 0 holds >= 2^21 elements; smaller ones capture one
 * stream (the cross-lane event edges cost more than the overlap there).
 * VSO_LANES=1 / 2 (read once per process) forces either. */
int vso_lane_count(const vso_session* s);

#ifdef __cplusplus
}
#endif

#endif /* VSO_H_ */
