// vso_resize.h — the Resize arithmetic, shared by k_resize (vso_kernels.hip)
// and the class head's upsampled form (vso_head.hip, k_class_head): the source
// coordinate of an output index, a row's and a column's taps and weight, the
// four-tap interpolation.  One definition, so that a head computing a logit on
// the fly gets the value k_resize would have stored, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "vso_kernels.h"

namespace vso {

__device__ __forceinline__ float resize_src(int o, float scale, int in, int out, int ctm) {
  switch (ctm) {
    case 0: return ((float)o + 0.5f) / scale - 0.5f;
    case 1: return out > 1 ? ((float)o + 0.5f) / scale - 0.5f : 0.f;
    case 2: return out > 1 ? (float)o * (float)(in - 1) / (float)(out - 1) : 0.f;
    default: return (float)o / scale;
  }
}

__device__ __forceinline__ int nearest_idx(float v, int mode, int in) {
  float r;
  if (mode == 0) r = (v == floorf(v) + 0.5f) ? floorf(v) : rintf(v);        // round_prefer_floor
  else if (mode == 1) r = floorf(v + 0.5f);                                   // round_prefer_ceil
  else if (mode == 2) r = floorf(v);
  else r = ceilf(v);
  const int i = (int)r;
  return i < 0 ? 0 : (i > in - 1 ? in - 1 : i);
}

// The source coordinate with the division by the scale as a multiplication
// when the scale is a power of two (2, 0.5, ...: the reciprocal is exact, so
// the value is the division's bit for bit); other scales divide.
__device__ __forceinline__ float resize_src_fast(int o, float scale, float inv, bool pow2, int in, int out, int ctm) {
  if ((ctm == 0 || (ctm == 1 && out > 1)) && pow2) return ((float)o + 0.5f) * inv - 0.5f;
  return resize_src(o, scale, in, out, ctm);
}

// One output row's source rows (linear) or row (nearest), worked out once
// for all the outputs of a thread (they share oy).
struct ResizeRow {
  const float* r0;
  const float* r1;
  float ly;
};

__device__ __forceinline__ ResizeRow resize_row(const ResizeParams& p, const float* __restrict__ xc, int oy, float inv,
                                                bool pow2) {
  const float fy = resize_src_fast(oy, p.sy, inv, pow2, p.H, p.Ho, p.ctm);
  if (!p.linear) {
    const float* r = xc + nearest_idx(fy, p.nearest, p.H) * p.W;
    return {r, r, 0.f};
  }
  const float sy = fminf(fmaxf(fy, 0.f), (float)(p.H - 1));
  const int y0 = (int)sy, y1 = min(y0 + 1, p.H - 1);
  return {xc + y0 * p.W, xc + y1 * p.W, sy - (float)y0};
}

// A linear output column's two source columns (inside [0, W)) and its weight
struct ResizeCol {
  int x0, x1;
  float lx;
};

__device__ __forceinline__ ResizeCol resize_col_taps(const ResizeParams& p, float fx) {
  const float sx = fminf(fmaxf(fx, 0.f), (float)(p.W - 1));
  const int x0 = (int)sx, x1 = min(x0 + 1, p.W - 1);
  return {x0, x1, sx - (float)x0};
}

// The four taps' interpolation: along x in each row, then along y —
//   (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11)
// with its roundings written out.  Left to the compiler, which product of a
// sum is contracted into an fma depends on the code around it, and a second
// kernel would get other bits.  These are the operations hipcc chose for both
// instances of k_resize (read from their ISA: v_pk_mul, v_pk_fma with the
// addends swapped, v_pk_mul, v_add), so k_resize computes what it did, and
// k_class_head computes the same.
__device__ __forceinline__ float resize_lerp(float ly, float lx, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
  const float top = __builtin_fmaf(lx, v01, (1.f - lx) * v00);
  const float bot = __builtin_fmaf(1.f - lx, v10, lx * v11);
  return (1.f - ly) * top + ly * bot;
}

__device__ __forceinline__ float resize_col(const ResizeParams& p, const ResizeRow& rw, int ox, float inv, bool pow2) {
  const float fx = resize_src_fast(ox, p.sx, inv, pow2, p.W, p.Wo, p.ctm);
  if (!p.linear) return rw.r0[nearest_idx(fx, p.nearest, p.W)];
  const ResizeCol cl = resize_col_taps(p, fx);
  return resize_lerp(rw.ly, cl.lx, rw.r0[cl.x0], rw.r0[cl.x1], rw.r1[cl.x0], rw.r1[cl.x1]);
}

__device__ __forceinline__ bool pow2f(float v) { return v > 0.f && (__float_as_uint(v) & 0x7FFFFFu) == 0; }

}  // namespace vso
