// vss_layers.hip — branding layers of the virtual backgrounds: the overlay
// plate O that goes between the background and the person (the definition:
// include/vss_layers.h; the reference: updateCanvas, client/customization.ts:
// 44-77).  None of this runs per frame: the plate is rebuilt when the layers,
// the privacy level or the frame size change, one launch per layer step.
//
//   k_layer_draw    : one layer's premultiplied sample (the rounded rectangle's
//                     4 x 4 coverage, or the sprite scaled with k_bg_resize's
//                     recipe) source-over into O, over the clipped rectangle.
//   k_shadow_alpha  : the layer's alpha at the shifted rectangle, a u8 plane.
//   k_shadow_h      : the horizontal Gaussian pass in k_blur_h's shape (256
//                     pixels of a row and their halo in LDS), zero padding.
//   k_shadow_over   : the vertical pass, the shadow's colour and source-over.
//   k_bg_bake       : bg' = O over the colour or the scaled image, into the RGB
//                     plate that k_bg_composite<IMAGE> reads.
// The shadow kernels cover the shifted rectangle grown by the radius and
// clipped to the frame; outside it P is 0 by definition, so reads are bounded
// by the region and nothing outside it is touched.
#include <hip/hip_runtime.h>

#include "vss_kernels.h"

namespace vss {

namespace {

// up_coord for a 64-bit output index (the unclipped rectangle may be far larger than the frame)
__device__ __forceinline__ void up_coord_l(long o, float scale, int in, int& i0, int& i1, float& l) {
#pragma clang fp contract(off)
  float s = ((float)o + 0.5f) * scale - 0.5f;
  s = fmaxf(s, 0.f);
  const int a = (int)fminf(s, (float)(in - 1));
  i0 = a;
  i1 = a < in - 1 ? a + 1 : a;
  l = s - (float)a;
}

__device__ __forceinline__ uint32_t div255(uint32_t v) { return (v + 127u) / 255u; }

// the layer's premultiplied sample at frame pixel (x, y) inside its rectangle
__device__ __forceinline__ uint32_t layer_sample(const LayerGeom& g, long x, long y) {
#pragma clang fp contract(off)
  if (g.type == kLayerRect) {
    const long R8 = 8 * g.R, lx = 8 * g.X0 + R8, hx = 8 * g.X1 - R8, ly = 8 * g.Y0 + R8, hy = 8 * g.Y1 - R8;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long sy = 8 * y + 2 * j + 1;
      const long dy = sy < ly ? ly - sy : (sy > hy ? sy - hy : -1);  // -1: not in a corner row
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long sx = 8 * x + 2 * i + 1;
        const long dx = sx < lx ? lx - sx : (sx > hx ? sx - hx : -1);
        n += (dx < 0 || dy < 0 || dx * dx + dy * dy <= R8 * R8) ? 1u : 0u;
      }
    }
    const uint32_t a = ((g.color >> 24) * n + 8u) >> 4;
    uint32_t s = a << 24;
#pragma unroll
    for (int c = 0; c < 3; ++c) s |= div255(((g.color >> (8 * c)) & 255u) * a) << (8 * c);
    return s;
  }
  int ya, yb, xa, xb;
  float fy, fx;
  up_coord_l(y - g.Y0, g.sy, g.sh, ya, yb, fy);
  up_coord_l(x - g.X0, g.sx, g.sw, xa, xb, fx);
  const uint8_t* ra = g.sprite + (long)ya * g.sw * 4;
  const uint8_t* rb = g.sprite + (long)yb * g.sw * 4;
  uint32_t v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float a00 = ra[xa * 4 + c], a01 = ra[xb * 4 + c], a10 = rb[xa * 4 + c], a11 = rb[xb * 4 + c];
    const float top = __builtin_fmaf(a01 - a00, fx, a00), bot = __builtin_fmaf(a11 - a10, fx, a10);
    v[c] = (uint32_t)floorf(__builtin_fmaf(bot - top, fy, top) + 0.5f);
  }
  return min(v[0], v[3]) | (min(v[1], v[3]) << 8) | (min(v[2], v[3]) << 16) | (v[3] << 24);
}

// O' = min(255, S + (O*(255 - S.a) + 127) / 255) per channel, alpha included
__device__ __forceinline__ uint32_t source_over(uint32_t o, uint32_t s) {
  const uint32_t ia = 255u - (s >> 24);
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t v = ((s >> (8 * c)) & 255u) + div255(((o >> (8 * c)) & 255u) * ia);
    out |= min(v, 255u) << (8 * c);
  }
  return out;
}

}  // namespace

__global__ __launch_bounds__(256) void k_layer_draw(LayerDrawParams p) {
  const int y = p.y0 + blockIdx.y * 4 + (threadIdx.x >> 6), x = p.x0 + blockIdx.x * 64 + (threadIdx.x & 63);
  if (y >= p.y1 || x >= p.x1) return;
  uint32_t* o = p.plate + (long)y * p.pitch + x;
  *o = source_over(*o, layer_sample(p.g, x, y));
}

__global__ __launch_bounds__(256) void k_shadow_alpha(ShadowParams p) {
  const int y = p.y0 + blockIdx.y * 4 + (threadIdx.x >> 6), x = p.x0 + blockIdx.x * 64 + (threadIdx.x & 63);
  if (y >= p.y1 || x >= p.x1) return;
  const long lx = x - p.dx, ly = y - p.dy;
  const bool in = lx >= p.g.X0 && lx < p.g.X1 && ly >= p.g.Y0 && ly < p.g.Y1;
  p.P[(long)y * p.pitch + x] = in ? (uint8_t)(layer_sample(p.g, lx, ly) >> 24) : (uint8_t)0;
}

// One workgroup = 256 consecutive pixels of one row of the region and their halo (0 outside the region)
__global__ __launch_bounds__(256) void k_shadow_h(ShadowParams p) {
  __shared__ uint32_t row[256 + 2 * kBlurMaxRadius];
  __shared__ uint32_t wl[kBlurMaxRadius + 1];
  const int tid = threadIdx.x, r = p.radius;
  const int X0 = p.x0 + blockIdx.x * 256, y = p.y0 + blockIdx.y;
  const uint8_t* src = p.P + (long)y * p.pitch;
  for (int i = tid; i < 256 + 2 * r; i += 256) {
    const int xx = X0 - r + i;
    row[i] = (xx >= p.x0 && xx < p.x1) ? src[xx] : 0u;
  }
  if (tid <= r) wl[tid] = p.w[tid];
  __syncthreads();
  const int x = X0 + tid;
  if (x >= p.x1) return;
  uint32_t acc = 32768u;
  for (int d = 0; d <= 2 * r; ++d) acc += wl[d < r ? r - d : d - r] * row[tid + d];
  p.Hb[(long)y * p.pitch + x] = (uint8_t)(acc >> 16);
}

__global__ __launch_bounds__(256) void k_shadow_over(ShadowParams p) {
  const int y = p.y0 + blockIdx.y * 4 + (threadIdx.x >> 6), x = p.x0 + blockIdx.x * 64 + (threadIdx.x & 63);
  if (y >= p.y1 || x >= p.x1) return;
  const int r = p.radius;
  uint32_t B;
  if (r == 0) {
    B = p.P[(long)y * p.pitch + x];
  } else {
    uint32_t acc = 32768u;
    for (int d = -r; d <= r; ++d) {
      const int yy = y + d;
      if (yy >= p.y0 && yy < p.y1) acc += (uint32_t)p.w[d < 0 ? -d : d] * p.Hb[(long)yy * p.pitch + x];
    }
    B = acc >> 16;
  }
  const uint32_t a = div255((p.color >> 24) * B);
  uint32_t s = a << 24;
#pragma unroll
  for (int c = 0; c < 3; ++c) s |= div255(((p.color >> (8 * c)) & 255u) * a) << (8 * c);
  uint32_t* o = p.plate + (long)y * p.pitch + x;
  *o = source_over(*o, s);
}

__global__ __launch_bounds__(256) void k_bg_bake(BgBakeParams p) {
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6), x = blockIdx.x * 64 + (threadIdx.x & 63);
  if (y >= p.fh || x >= p.fw) return;
  uint8_t* q = p.image + (long)y * bg_image_stride(p.fw) + (long)x * 3;
  const uint32_t bg = p.from_color ? p.color : ((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16));
  const uint32_t v = under_overlay(bg, p.overlay[(long)y * layer_pitch(p.fw) + x]);
  q[0] = (uint8_t)v;
  q[1] = (uint8_t)(v >> 8);
  q[2] = (uint8_t)(v >> 16);
}

namespace {
dim3 region_grid(int x0, int y0, int x1, int y1) { return dim3((x1 - x0 + 63) / 64, (y1 - y0 + 3) / 4); }
}  // namespace

void launch_layer_draw(const LayerDrawParams& p, hipStream_t s) {
  if (p.x1 <= p.x0 || p.y1 <= p.y0) return;
  hipLaunchKernelGGL(k_layer_draw, region_grid(p.x0, p.y0, p.x1, p.y1), dim3(256), 0, s, p);
}

void launch_layer_shadow(const ShadowParams& p, hipStream_t s) {
  if (p.x1 <= p.x0 || p.y1 <= p.y0) return;
  const dim3 grid = region_grid(p.x0, p.y0, p.x1, p.y1);
  hipLaunchKernelGGL(k_shadow_alpha, grid, dim3(256), 0, s, p);
  if (p.radius)
    hipLaunchKernelGGL(k_shadow_h, dim3((p.x1 - p.x0 + 255) / 256, p.y1 - p.y0), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_shadow_over, grid, dim3(256), 0, s, p);
}

void launch_bg_bake(const BgBakeParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_bake, dim3((p.fw + 63) / 64, (p.fh + 3) / 4), dim3(256), 0, s, p);
}

}  // namespace vss
