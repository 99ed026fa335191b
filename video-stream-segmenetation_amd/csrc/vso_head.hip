// vso_head.hip — the ONNX sessions' class heads (the planner's find_heads):
// Softmax, LogSoftmax, ArgMax and ReduceMax over the channel axis of
// [N][C][Ho][Wo] logits, in one launch — with the linear Resize in front of
// them computed on the fly, so the full-size logits are never written.
//
// Work.  A thread owns one output pixel, or four consecutive pixels of a row
// where Wo is a multiple of 4 (QUAD: one index split per four pixels, one
// 16-byte store per class; k_resize's idea).  It walks the classes with stride
// H * W: at any class, a wave's loads are contiguous in the plain form (64
// floats, or 64 float4s) and fall on a few rows of one small plane in the
// upsampled form.  No LDS, no atomics, no cross-lane operation: a pixel's
// reduction lives in its thread's registers.
//
// Sources.  Plain (UP false): x is [N][C][Ho][Wo].  Upsampled (UP true): x is
// [N][C][H][W] and the logit of class c at (oy, ox) is resize_lerp over the
// four taps resize_row / resize_col_taps give — the functions k_resize is
// built from (vso_resize.h), in its order, so the value is the one k_resize
// would have stored.  A pixel's tap offsets and weights do not depend on the
// class: they are worked out once, in front of the class loops.
//
// Reductions (RED).
//   0, the softmax forms: three passes over the classes — the maximum, the
//      sum of expf(x - max), then expf(x - max) / sum (or x - max - logf(sum))
//      for the classes written, [c0, c0 + n).  The upsampled form interpolates
//      again in each pass: the same function of the same operands, so class c
//      of a pixel is one value in all three.
//   1, the arg forms: one pass keeping the maximum and its index — the first
//      (v > best) or the last (v >= best) — written as the index, as
//      (index == k), or as the maximum.
//
// Bounds.  Pixels: o < N * Ho * Wo, and a QUAD thread's four lie in one row.
// Plain reads are at (n, c, pixel) for c < C.  Upsampled taps are clamped into
// [0, H) x [0, W) by resize_row / resize_col_taps.  Stores go to channel
// < n (softmax forms) or 0 of pixel o.  All indices are 32-bit: the planner
// checks N * C * Ho * Wo and N * C * H * W < 2^31.
//
// Resources (gfx950, hipcc -O3, this unit's resource usage remarks): no
// scratch, no LDS; VGPRs by <RED, UP, QUAD>: the upsampled quad forms 122 and
// 116 (four waves per SIMD: two classes x four pixels x four taps in flight),
// the plain quad forms 86 and 42, the one-pixel forms 20 to 62.  The class
// loops are unrolled by hand-set counts and not interleaved: the vectoriser's
// interleaving of the maximum took the one-pixel upsampled form to 200 VGPRs.
#include <hip/hip_runtime.h>

#include "vso_device.h"
#include "vso_kernels.h"
#include "vso_resize.h"

namespace vso {

namespace {

// A thread's pixels' view of the logits: value(c, e) is class c at its pixel e.
template <bool UP, int PX>
struct HeadSrc {
  const float* xn;  // image n's class 0 plane
  int plane;        // floats between class planes
  // plain: the first pixel's offset in a plane.  upsampled: the rows' offsets,
  // each pixel's columns and the weights
  int o0, o1;
  int x0[PX], x1[PX];
  float ly, lx[PX];

  __device__ __forceinline__ void load(int c, float (&v)[PX]) const {
    const float* xc = xn + c * plane;
    if constexpr (UP) {
#pragma unroll
      for (int e = 0; e < PX; ++e)
        v[e] = resize_lerp(ly, lx[e], xc[o0 + x0[e]], xc[o0 + x1[e]], xc[o1 + x0[e]], xc[o1 + x1[e]]);
    } else if constexpr (PX == 4) {
      const f4 q = *reinterpret_cast<const f4*>(xc + o0);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = q[e];
    } else {
      v[0] = xc[o0];
    }
  }
};

template <int PX>
__device__ __forceinline__ void head_store(float* y, const float (&v)[PX]) {
  if constexpr (PX == 4) {
    f4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = v[e];
    *reinterpret_cast<f4*>(y) = q;
  } else {
    y[0] = v[0];
  }
}

}  // namespace

template <int RED, bool UP, bool QUAD>
__global__ __launch_bounds__(256) void k_class_head(HeadParams p) {
  // No contraction in this body either (resize_lerp pins its own roundings):
  // x - max - log(sum) and the like are the operations as written, the same in
  // every instance.
#pragma clang fp contract(off)
  constexpr int PX = QUAD ? 4 : 1;
  constexpr int UNR = UP && QUAD ? 2 : 4;  // classes in flight per thread (register budget: see the header)
  const ResizeParams& r = p.rz;
  const int C = r.C, Ho = r.Ho, Wo = r.Wo, hw = Ho * Wo, total = r.N * hw;
  const float iy = 1.f / r.sy, ix = 1.f / r.sx;
  const bool py = pow2f(r.sy), px = pow2f(r.sx);
  for (long ol = (blockIdx.x * 256L + threadIdx.x) * PX; ol < total; ol += gridDim.x * 256L * PX) {
    const int o = (int)ol, ox = o % Wo, t = o / Wo, oy = t % Ho, n = t / Ho, pix = o - n * hw;
    HeadSrc<UP, PX> src;
    if constexpr (UP) {
      src.plane = r.H * r.W;
      src.xn = r.x + n * C * src.plane;
      const ResizeRow rw = resize_row(r, src.xn, oy, iy, py);
      src.o0 = (int)(rw.r0 - src.xn);
      src.o1 = (int)(rw.r1 - src.xn);
      src.ly = rw.ly;
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const ResizeCol cl = resize_col_taps(r, resize_src_fast(ox + e, r.sx, ix, px, r.W, Wo, r.ctm));
        src.x0[e] = cl.x0;
        src.x1[e] = cl.x1;
        src.lx[e] = cl.lx;
      }
    } else {
      src.plane = hw;
      src.xn = r.x + n * C * hw;
      src.o0 = pix;
    }
    float v[PX], m[PX];
    if constexpr (RED == 0) {
      float s[PX];
#pragma unroll
      for (int e = 0; e < PX; ++e) { m[e] = -INFINITY; s[e] = 0.f; }
#pragma clang loop unroll_count(UNR) vectorize(disable) interleave(disable)
      for (int c = 0; c < C; ++c) {
        src.load(c, v);
#pragma unroll
        for (int e = 0; e < PX; ++e) m[e] = fmaxf(m[e], v[e]);
      }
#pragma clang loop unroll_count(UNR) vectorize(disable) interleave(disable)
      for (int c = 0; c < C; ++c) {
        src.load(c, v);
#pragma unroll
        for (int e = 0; e < PX; ++e) s[e] += expf(v[e] - m[e]);
      }
      const bool lg = p.op == HEAD_LOGSOFTMAX;
      if (lg) {
#pragma unroll
        for (int e = 0; e < PX; ++e) s[e] = logf(s[e]);
      }
      float* y = p.y + n * p.n * hw + pix;
#pragma clang loop unroll_count(2) vectorize(disable) interleave(disable)
      for (int c = 0; c < p.n; ++c) {
        src.load(p.c0 + c, v);
#pragma unroll
        for (int e = 0; e < PX; ++e) v[e] = lg ? v[e] - m[e] - s[e] : expf(v[e] - m[e]) / s[e];
        head_store<PX>(y + c * hw, v);
      }
    } else {
      int idx[PX];
      src.load(0, m);
#pragma unroll
      for (int e = 0; e < PX; ++e) idx[e] = 0;
      const bool last = p.last != 0;
#pragma clang loop unroll_count(UNR) vectorize(disable) interleave(disable)
      for (int c = 1; c < C; ++c) {
        src.load(c, v);
#pragma unroll
        for (int e = 0; e < PX; ++e) {
          const bool take = last ? v[e] >= m[e] : v[e] > m[e];
          m[e] = take ? v[e] : m[e];
          idx[e] = take ? c : idx[e];
        }
      }
#pragma unroll
      for (int e = 0; e < PX; ++e)
        v[e] = p.op == HEAD_MAX ? m[e] : p.op == HEAD_ARGMAX_EQ ? ((float)idx[e] == p.k ? 1.f : 0.f) : (float)idx[e];
      head_store<PX>(p.y + o, v);
    }
  }
}

static int grid_for(long n) { return (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536); }

static bool head_quad(const HeadParams& p) {
  return (p.rz.Wo & 3) == 0 && (reinterpret_cast<uintptr_t>(p.y) & 15) == 0 &&
         (p.rz.linear || (reinterpret_cast<uintptr_t>(p.rz.x) & 15) == 0);
}

const char* head_kernel_name(const HeadParams& p) {
  static const char* names[] = {"void vso::k_class_head<0, false, false>(vso::HeadParams)",
                                "void vso::k_class_head<0, false, true>(vso::HeadParams)",
                                "void vso::k_class_head<0, true, false>(vso::HeadParams)",
                                "void vso::k_class_head<0, true, true>(vso::HeadParams)",
                                "void vso::k_class_head<1, false, false>(vso::HeadParams)",
                                "void vso::k_class_head<1, false, true>(vso::HeadParams)",
                                "void vso::k_class_head<1, true, false>(vso::HeadParams)",
                                "void vso::k_class_head<1, true, true>(vso::HeadParams)"};
  const int red = p.op == HEAD_SOFTMAX || p.op == HEAD_LOGSOFTMAX ? 0 : 1;
  return names[red * 4 + (p.rz.linear ? 2 : 0) + (head_quad(p) ? 1 : 0)];
}

template <int RED>
static void launch_red(const HeadParams& p, hipStream_t s) {
  const long pixels = (long)p.rz.N * p.rz.Ho * p.rz.Wo;
  const bool quad = head_quad(p);
  const dim3 grid(grid_for(quad ? pixels / 4 : pixels));
  if (p.rz.linear) {
    if (quad) hipLaunchKernelGGL((k_class_head<RED, true, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_class_head<RED, true, false>), grid, dim3(256), 0, s, p);
  } else {
    if (quad) hipLaunchKernelGGL((k_class_head<RED, false, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_class_head<RED, false, false>), grid, dim3(256), 0, s, p);
  }
}

void launch_head(const HeadParams& p, hipStream_t s) {
  if (p.rz.N <= 0 || p.rz.C <= 0 || p.rz.Ho <= 0 || p.rz.Wo <= 0) return;
  if (p.op == HEAD_SOFTMAX || p.op == HEAD_LOGSOFTMAX) launch_red<0>(p, s);
  else launch_red<1>(p, s);
}

}  // namespace vso
