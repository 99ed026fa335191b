// vss_video.hip — NV12 <-> packed RGBA, the colour conversion at the two ends of
// a decoder -> library -> encoder pipeline.  The definition (frame layout, the
// coefficient table, the integer formulas) is in include/vss_video.h;
// tests/video_ref.py restates it in numpy and the kernels match it bit for bit.
//
//   k_nv12_unpack : one thread = 8 pixels x 2 rows (four 2x2 chroma blocks):
//                   two 8-B Y loads and one 8-B UV load, four 16-B RGBA stores.
//   k_nv12_pack   : the same footprint: four 16-B RGBA loads, two 8-B Y stores
//                   and one 8-B UV store.
// Both are streaming kernels (no LDS, no reuse beyond the thread's registers).
// Pitches and base pointers need no alignment, so every vector access tests
// its own address and falls back to bytes (Y, UV) or dwords (RGBA); the tail of
// a width that is no multiple of 8 takes the same per-pixel path and writes
// nothing past column fw - 1.
#include <hip/hip_runtime.h>

#include "vss_kernels.h"

namespace vss {

namespace {

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// One unpacked pixel from c = cy*(Y - y0) and the block's chroma terms (each with
// the rounding 128 added).  clip(v >> 8) is taken as clip16(v) >> 8, clip16 the
// clamp to 0..65535: the same value for every v (the shift is monotone, and
// 65535 >> 8 = 255), and the bytes then sit where the pixel wants them.
__device__ __forceinline__ uint32_t rgba_px(int c, int cr, int cg, int cb) {
  const uint32_t r = (uint32_t)min(max(c + cr, 0), 65535), g = (uint32_t)min(max(c + cg, 0), 65535),
                 b = (uint32_t)min(max(c + cb, 0), 65535);
  return (r >> 8) | (g & 0xFF00u) | ((b & 0xFF00u) << 8) | 0xFF000000u;
}

// 8 bytes at q (cnt < 8: only the first cnt, the rest 0) -> b[8]
__device__ __forceinline__ void load8(const uint8_t* q, int cnt, int (&b)[8]) {
  if (cnt == 8 && (reinterpret_cast<uintptr_t>(q) & 7) == 0) {
    const uint2 v = *reinterpret_cast<const uint2*>(q);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[k] = (v.x >> (8 * k)) & 255u;
      b[4 + k] = (v.y >> (8 * k)) & 255u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = k < cnt ? q[k] : 0;
  }
}

__device__ __forceinline__ void store8(uint8_t* q, int cnt, const int (&b)[8]) {
  if (cnt == 8 && (reinterpret_cast<uintptr_t>(q) & 7) == 0) {
    uint2 v = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v.x |= (uint32_t)b[k] << (8 * k);
      v.y |= (uint32_t)b[4 + k] << (8 * k);
    }
    *reinterpret_cast<uint2*>(q) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < cnt) q[k] = (uint8_t)b[k];
  }
}

// 8 RGBA pixels at q (4-byte aligned; cnt < 8: only the first cnt)
__device__ __forceinline__ void load_px8(const uint8_t* q, int cnt, uint32_t (&px)[8]) {
  if (cnt == 8 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
    const uint4 a = reinterpret_cast<const uint4*>(q)[0], b = reinterpret_cast<const uint4*>(q)[1];
    px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w;
    px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) px[k] = k < cnt ? reinterpret_cast<const uint32_t*>(q)[k] : 0u;
  }
}

__device__ __forceinline__ void store_px8(uint8_t* q, int cnt, const uint32_t (&px)[8]) {
  if (cnt == 8 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
    reinterpret_cast<uint4*>(q)[0] = make_uint4(px[0], px[1], px[2], px[3]);
    reinterpret_cast<uint4*>(q)[1] = make_uint4(px[4], px[5], px[6], px[7]);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < cnt) reinterpret_cast<uint32_t*>(q)[k] = px[k];
  }
}

// the thread's footprint: frame t, rows 2*yp and 2*yp + 1, columns x0 .. x0 + cnt - 1 (cnt even, <= 8)
struct Foot {
  int t, yp, x0, cnt;
};
__device__ __forceinline__ bool footprint(int fh, int fw, Foot& f) {
  f.t = blockIdx.z;
  f.yp = blockIdx.y * 4 + (threadIdx.x >> 6);
  f.x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
  f.cnt = min(8, fw - f.x0);
  return 2 * f.yp < fh && f.x0 < fw;
}

}  // namespace

__global__ __launch_bounds__(256) void k_nv12_unpack(Nv12Params p) {
  Foot f;
  if (!footprint(p.fh, p.fw, f)) return;
  const CscCoef& k = p.k;
  const uint8_t* yr = p.y + (long)f.t * p.y_frame_stride + (long)(2 * f.yp) * p.y_pitch + f.x0;
  int y0[8], y1[8], uv[8];
  load8(yr, f.cnt, y0);
  load8(yr + p.y_pitch, f.cnt, y1);
  load8(p.uv + (long)f.t * p.uv_frame_stride + (long)f.yp * p.uv_pitch + f.x0, f.cnt, uv);
  uint32_t o0[8], o1[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // one 2x2 block per (U, V) pair
    const int d = uv[2 * j] - 128, e = uv[2 * j + 1] - 128;
    const int cr = k.rv * e + 128, cg = k.gu * d + k.gv * e + 128, cb = k.bu * d + 128;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      o0[2 * j + i] = rgba_px(k.cy * (y0[2 * j + i] - k.y0), cr, cg, cb);
      o1[2 * j + i] = rgba_px(k.cy * (y1[2 * j + i] - k.y0), cr, cg, cb);
    }
  }
  uint8_t* o = p.rgba + (long)f.t * p.frame_stride + (long)(2 * f.yp) * p.row_stride + (long)f.x0 * 4;
  store_px8(o, f.cnt, o0);
  store_px8(o + p.row_stride, f.cnt, o1);
}

__global__ __launch_bounds__(256) void k_nv12_pack(Nv12Params p) {
  Foot f;
  if (!footprint(p.fh, p.fw, f)) return;
  const CscCoef& k = p.k;
  const uint8_t* q = p.rgba + (long)f.t * p.frame_stride + (long)(2 * f.yp) * p.row_stride + (long)f.x0 * 4;
  uint32_t r0[8], r1[8];
  load_px8(q, f.cnt, r0);
  load_px8(q + p.row_stride, f.cnt, r1);
  int y0[8], y1[8], uv[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int m[3] = {2, 2, 2};  // the block's rounded mean per channel: (p00 + p01 + p10 + p11 + 2) >> 2
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t a = r0[2 * j + i], b = r1[2 * j + i];
      const int ar = a & 255u, ag = (a >> 8) & 255u, ab = (a >> 16) & 255u;
      const int br = b & 255u, bgn = (b >> 8) & 255u, bb = (b >> 16) & 255u;
      y0[2 * j + i] = clip255(((k.yr * ar + k.yg * ag + k.yb * ab + 128) >> 8) + k.y0);
      y1[2 * j + i] = clip255(((k.yr * br + k.yg * bgn + k.yb * bb + 128) >> 8) + k.y0);
      m[0] += ar + br;
      m[1] += ag + bgn;
      m[2] += ab + bb;
    }
    const int mr = m[0] >> 2, mg = m[1] >> 2, mb = m[2] >> 2;
    uv[2 * j] = clip255(((k.ur * mr + k.ug * mg + k.ub * mb + 128) >> 8) + 128);
    uv[2 * j + 1] = clip255(((k.vr * mr + k.vg * mg + k.vb * mb + 128) >> 8) + 128);
  }
  uint8_t* yr = p.y + (long)f.t * p.y_frame_stride + (long)(2 * f.yp) * p.y_pitch + f.x0;
  store8(yr, f.cnt, y0);
  store8(yr + p.y_pitch, f.cnt, y1);
  store8(p.uv + (long)f.t * p.uv_frame_stride + (long)f.yp * p.uv_pitch + f.x0, f.cnt, uv);
}

// 64 footprints (512 pixels) x 4 row pairs per workgroup
static dim3 nv12_grid(const Nv12Params& p, int n) { return dim3((p.fw + 511) / 512, (p.fh / 2 + 3) / 4, n); }

void launch_nv12_unpack(const Nv12Params& p, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_nv12_unpack, nv12_grid(p, n), dim3(256), 0, s, p);
}

void launch_nv12_pack(const Nv12Params& p, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_nv12_pack, nv12_grid(p, n), dim3(256), 0, s, p);
}

}  // namespace vss
