// vss_background.hip — virtual backgrounds: the person over a solid colour, a
// user image or the blurred frame, as one opaque RGBA frame.
//
// The reference shows the person over a colour (composeMatteOnCanvas,
// client/src/core/u2FrameProc.ts:78-148) or over a background image drawn to
// the canvas size (client/customization.ts:41).  Here, per colour channel,
//   out = (fg*A + bg*(255-A) + 127) / 255        (integer division)
// with A = k_composite's alpha (the half-pixel bilinear of the mask's u8 alpha,
// rounded half up) and the output alpha byte 255; for a = A/255 this equals
// composeMatteOnCanvas's Math.round((a*s/255 + (1-a)*b/255)*255) for all 256^3
// (A, fg, bg) (tests/test_background_ref.py).
//
//   k_bg_resize          : the user image scaled to the frame size with the
//                          alpha's half-pixel bilinear, per channel (once per
//                          image and frame geometry).
//   k_bg_composite<mode> : COLOR / IMAGE: k_composite's thread shape (4
//                          consecutive pixels, one 16-B store) plus the blend.
//   k_blur_h             : BLUR's horizontal pass, 16-bit fixed-point weights,
//                          h = (sum w*p + 32768) >> 16, packed RGBX u8.
//   k_bg_composite<BLUR> : the vertical pass over an LDS tile of k_blur_h's
//                          output (radius halo rows above and below), fused
//                          with the alpha upscale and the blend: the blurred
//                          frame never goes to HBM.
// Edges replicate.  The sums stay below 2^32 (65536 * 255 + 32768).
// Every k_bg_composite also has a REFINE form (the edge-aware matte,
// vss_matte.hip): only where A comes from changes — two bilinear fetches of the
// (abar, bbar) plane applied to the luma of the frame bytes the thread loads
// anyway, in place of the one of the alpha bytes.
#include <hip/hip_runtime.h>

#include "vss_kernels.h"

namespace vss {

namespace {

// 4 consecutive pixels x0.. of row y of frame t over bg[4] (r | g<<8 | b<<16);
// REFINE: the alpha from frame t's (abar, bbar) taps m (pixel_alpha, vss_kernels.h)
template <bool REFINE>
__device__ __forceinline__ void blend_quad(const CompositeParams& p, const MatteTaps& m, int t, int y, int x0,
                                           const uint32_t (&bg)[4]) {
#pragma clang fp contract(off)
  int ya, yb;
  float ly;
  up_coord(y, p.sy, p.H, ya, yb, ly);
  const uint8_t* a = p.alpha + (long)t * p.H * p.W;
  const uint8_t* ra = a + (long)ya * p.W;
  const uint8_t* rb = a + (long)yb * p.W;
  const float2* ma = nullptr;
  const float2* mb = nullptr;
  if constexpr (REFINE) {
    ma = m.p + (ya - m.row0) * m.pitch;
    mb = m.p + (yb - m.row0) * m.pitch;
  }
  const uint8_t* f = p.frames + (long)t * p.frame_stride + (long)y * p.row_stride;
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = min(x0 + k, p.fw - 1);
    int xa, xb;
    float lx;
    up_coord(x, p.sx, p.W, xa, xb, lx);
    const uint8_t* q = f + (long)x * p.fc;
    const uint32_t A = pixel_alpha<REFINE>(ra, rb, ma, mb, xa, xb, m.col0, lx, ly, q);
    uint32_t o = 0xFF000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t b = (bg[k] >> (8 * c)) & 255u;
      o |= (((uint32_t)q[c] * A + b * (255u - A) + 127u) / 255u) << (8 * c);
    }
    px[k] = o;
  }
  uint8_t* o = p.out + (long)t * p.out_frame_stride + (long)y * p.out_row_stride + (long)x0 * 4;
  if (x0 + 4 <= p.fw && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
    *reinterpret_cast<uint4*>(o) = make_uint4(px[0], px[1], px[2], px[3]);
  } else {
    for (int k = 0; k < 4 && x0 + k < p.fw; ++k) reinterpret_cast<uint32_t*>(o)[k] = px[k];
  }
}

constexpr int kBlurTW = 64, kBlurTH = 32;  // k_bg_composite<BLUR>'s tile: 16 x 16 threads, 4 x 2 pixels each

// The flat form's workgroup: 4 rows of 256 pixels of frame t over a colour
// (image null) or the plate `image`.  MODE = kBgColor / kBgImage fixes which at
// compile time (k_bg_composite), kBgAny leaves it to the pointer (the pooled
// form).  taps: the workgroup's LDS window of frame t's (abar, bbar) plane ab.
constexpr int kBgAny = -1;
template <int MODE, bool REFINE>
__device__ __forceinline__ void flat_tile(const CompositeParams& c, int t, const float2* ab, const uint8_t* image,
                                          uint32_t color, float2* taps) {
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  MatteTaps m{};
  if constexpr (REFINE) m = stage_matte_taps(c, ab, blockIdx.y * 4, blockIdx.x * 256, taps);
  if (y >= c.fh || x0 >= c.fw) return;
  uint32_t bg[4];
  if (MODE == kBgColor || (MODE == kBgAny && !image)) {
    bg[0] = bg[1] = bg[2] = bg[3] = color;
  } else {
    // 4 RGB pixels = 3 dwords (rows padded to whole quads, bg_image_stride)
    const uint32_t* q = reinterpret_cast<const uint32_t*>(image + (long)y * bg_image_stride(c.fw) + (long)x0 * 3);
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
    bg[0] = d0 & 0xFFFFFFu;
    bg[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
    bg[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
    bg[3] = d2 >> 8;
  }
  blend_quad<REFINE>(c, m, t, y, x0, bg);
}

// The blur form's workgroup: a 64 x 32 tile of frame t.  h: the frame's
// horizontal pass [fh][fw]; tile: [kBlurTH + 2r][kBlurTW] RGBX, then the r + 1
// weights, which the caller has stored (this function's barrier covers them).
// LAYERS: the overlay plate O goes between the blurred frame and the person,
// bg' = O over bg (under_overlay, vss_kernels.h), one 16-B load of O's 4 pixels
// per thread row.  REFINE: the taps straight from the plane ab (a 64 x 32 tile's
// window is up to 34 x 66 taps on top of the blur's tile).
template <bool REFINE, bool LAYERS>
__device__ __forceinline__ void blur_tile(const CompositeParams& c, int t, const uint32_t* h, const float2* ab,
                                          const uint32_t* overlay, int r, uint32_t* tile) {
  const int rows = kBlurTH + 2 * r;
  const uint32_t* wl = tile + rows * kBlurTW;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int X0 = blockIdx.x * kBlurTW, Y0 = blockIdx.y * kBlurTH;
  const MatteTaps m = {REFINE ? ab : nullptr, c.W, 0, 0};
  for (int i = tid; i < rows * kBlurTW; i += 256) {
    const int yy = min(max(Y0 - r + i / kBlurTW, 0), c.fh - 1), xx = min(X0 + i % kBlurTW, c.fw - 1);
    tile[i] = h[(long)yy * c.fw + xx];
  }
  __syncthreads();
  const int x0 = X0 + tx * 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ly = ty + 16 * j, y = Y0 + ly;
    if (y >= c.fh || x0 >= c.fw) continue;
    uint32_t acc[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 32768u;
    for (int d = 0; d <= 2 * r; ++d) {
      const uint4 v = *reinterpret_cast<const uint4*>(tile + (ly + d) * kBlurTW + tx * 4);
      const uint32_t w = wl[d < r ? r - d : d - r];
      const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[k][0] += w * (q[k] & 255u);
        acc[k][1] += w * ((q[k] >> 8) & 255u);
        acc[k][2] += w * ((q[k] >> 16) & 255u);
      }
    }
    uint32_t bg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bg[k] = (acc[k][0] >> 16) | ((acc[k][1] >> 16) << 8) | ((acc[k][2] >> 16) << 16);
    if constexpr (LAYERS) {
      // x0 is a multiple of 4 below fw, the plate's rows are whole quads: in bounds and 16-B aligned
      const uint4 o = *reinterpret_cast<const uint4*>(overlay + (long)y * layer_pitch(c.fw) + x0);
      bg[0] = under_overlay(bg[0], o.x);
      bg[1] = under_overlay(bg[1], o.y);
      bg[2] = under_overlay(bg[2], o.z);
      bg[3] = under_overlay(bg[3], o.w);
    }
    blend_quad<REFINE>(c, m, t, y, x0, bg);
  }
}

// k_blur_h's workgroup: 256 consecutive pixels of row f (frame bytes) into out
// (the same row of the horizontal pass); the row segment and its radius halo
// (replicated at the frame's edges) packed RGBX in LDS.  wl: the r + 1 weights,
// stored by the caller (this function's barrier covers them).
__device__ __forceinline__ void blur_h_segment(const uint8_t* f, int fw, int fc, int r, uint32_t* row,
                                               const uint32_t* wl, uint32_t* out) {
  const int tid = threadIdx.x, X0 = blockIdx.x * 256;
  for (int i = tid; i < 256 + 2 * r; i += 256) {
    const uint8_t* q = f + (long)min(max(X0 - r + i, 0), fw - 1) * fc;
    row[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
  }
  __syncthreads();
  const int x = X0 + tid;
  if (x >= fw) return;
  uint32_t a0 = 32768u, a1 = 32768u, a2 = 32768u;
  for (int d = 0; d <= 2 * r; ++d) {
    const uint32_t v = row[tid + d], w = wl[d < r ? r - d : d - r];
    a0 += w * (v & 255u);
    a1 += w * ((v >> 8) & 255u);
    a2 += w * ((v >> 16) & 255u);
  }
  out[x] = (a0 >> 16) | ((a1 >> 16) << 8) | ((a2 >> 16) << 16);
}

}  // namespace

// COLOR / IMAGE with layers run the IMAGE form over a plate that holds bg'
// already (k_bg_bake, vss_layers.hip); LAYERS is BLUR's alone.
template <int MODE, bool REFINE, bool LAYERS = false>
__global__ __launch_bounds__(256) void k_bg_composite(BgCompositeParams p) {
  const CompositeParams& c = p.c;
  const int t = blockIdx.z;
  const float2* ab = REFINE ? p.ab + (long)t * c.H * c.W : nullptr;
  if constexpr (MODE != kBgBlur) {
    if constexpr (REFINE) {
      __shared__ float2 taps[kMatteTapRows * kMatteTapCols];
      flat_tile<MODE, true>(c, t, ab, p.image, p.color, taps);
    } else {
      flat_tile<MODE, false>(c, t, nullptr, p.image, p.color, nullptr);
    }
  } else {
    extern __shared__ __align__(16) uint32_t tile[];
    const int r = p.radius;
    if (threadIdx.x <= r) tile[(kBlurTH + 2 * r) * kBlurTW + threadIdx.x] = p.w[threadIdx.x];
    blur_tile<REFINE, LAYERS>(c, t, p.hblur + (long)t * c.fh * c.fw, ab, p.overlay, r, tile);
  }
}

// One workgroup = 256 consecutive pixels of one row.
__global__ __launch_bounds__(256) void k_blur_h(BlurHParams p) {
  __shared__ uint32_t row[256 + 2 * kBlurMaxRadius];
  __shared__ uint32_t wl[kBlurMaxRadius + 1];
  const int y = blockIdx.y, t = blockIdx.z;
  if (threadIdx.x <= p.radius) wl[threadIdx.x] = p.w[threadIdx.x];
  blur_h_segment(p.frames + (long)t * p.frame_stride + (long)y * p.row_stride, p.fw, p.fc, p.radius, row, wl,
                 p.out + ((long)t * p.fh + y) * p.fw);
}

// ---- many streams: frame t over its own background (BgStreamsParams, vss_kernels.h) ----
// Refinement and layers are workgroup-uniform branches on the frame's
// descriptor; the pixel arithmetic is flat_tile / blur_tile / blur_h_segment.
__global__ __launch_bounds__(256) void k_bg_streams_flat(BgStreamsParams p) {
  __shared__ float2 taps[kMatteTapRows * kMatteTapCols];
  const int t = stream_list_at(p.flat, blockIdx.z);
  const float2* ab = p.entry[t].ab;
  const uint8_t* image = p.entry[t].image;
  const uint32_t color = p.entry[t].color;
  if (ab)
    flat_tile<kBgAny, true>(p.c, t, ab, image, color, taps);
  else
    flat_tile<kBgAny, false>(p.c, t, nullptr, image, color, taps);
}

// The dynamic LDS holds the tile of the launch's largest radius; a workgroup
// uses the rows and taps of its own frame's.
__global__ __launch_bounds__(256) void k_bg_streams_blur(BgStreamsParams p) {
  extern __shared__ __align__(16) uint32_t tile[];
  const int t = stream_list_at(p.blur, blockIdx.z);
  const float2* ab = p.entry[t].ab;
  const uint32_t* h = p.entry[t].hblur;
  const uint32_t* overlay = p.entry[t].overlay;
  const uint16_t* taps = p.entry[t].taps;
  const int r = p.entry[t].radius;
  if (threadIdx.x <= r) tile[(kBlurTH + 2 * r) * kBlurTW + threadIdx.x] = taps[threadIdx.x];
  if (ab) {
    if (overlay) blur_tile<true, true>(p.c, t, h, ab, overlay, r, tile);
    else blur_tile<true, false>(p.c, t, h, ab, nullptr, r, tile);
  } else {
    if (overlay) blur_tile<false, true>(p.c, t, h, nullptr, overlay, r, tile);
    else blur_tile<false, false>(p.c, t, h, nullptr, nullptr, r, tile);
  }
}

__global__ __launch_bounds__(256) void k_blur_h_streams(BgStreamsParams p) {
  __shared__ uint32_t row[256 + 2 * kBlurMaxRadius];
  __shared__ uint32_t wl[kBlurMaxRadius + 1];
  const CompositeParams& c = p.c;
  const int y = blockIdx.y, t = stream_list_at(p.blur, blockIdx.z);
  const uint16_t* taps = p.entry[t].taps;
  uint32_t* out = p.entry[t].hblur;
  const int r = p.entry[t].radius;
  if (threadIdx.x <= r) wl[threadIdx.x] = taps[threadIdx.x];
  blur_h_segment(c.frames + (long)t * c.frame_stride + (long)y * c.row_stride, c.fw, c.fc, r, row, wl,
                 out + (long)y * c.fw);
}

// One thread per pixel of the scaled image (runs once per image and geometry).
__global__ __launch_bounds__(256) void k_bg_resize(BgResizeParams p) {
#pragma clang fp contract(off)
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6), x = blockIdx.x * 64 + (threadIdx.x & 63);
  if (y >= p.fh || x >= p.fw) return;
  int ya, yb, xa, xb;
  float ly, lx;
  up_coord(y, p.sy, p.sh, ya, yb, ly);
  up_coord(x, p.sx, p.sw, xa, xb, lx);
  const uint8_t* ra = p.src + (long)ya * p.sw * p.sc;
  const uint8_t* rb = p.src + (long)yb * p.sw * p.sc;
  uint8_t* o = p.out + (long)y * bg_image_stride(p.fw) + (long)x * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a00 = ra[xa * p.sc + c], a01 = ra[xb * p.sc + c], a10 = rb[xa * p.sc + c], a11 = rb[xb * p.sc + c];
    const float top = __builtin_fmaf(a01 - a00, lx, a00), bot = __builtin_fmaf(a11 - a10, lx, a10);
    o[c] = (uint8_t)floorf(__builtin_fmaf(bot - top, ly, top) + 0.5f);
  }
}

void launch_bg_resize(const BgResizeParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_resize, dim3((p.fw + 63) / 64, (p.fh + 3) / 4), dim3(256), 0, s, p);
}

void launch_blur_h(const BlurHParams& p, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_blur_h, dim3((p.fw + 255) / 256, p.fh, n), dim3(256), 0, s, p);
}

void launch_bg_composite(const BgCompositeParams& p, int mode, int n, hipStream_t s) {
  const dim3 grid((p.c.fw + 255) / 256, (p.c.fh + 3) / 4, n);
  const bool refine = p.ab != nullptr;
  if (mode == kBgColor) {
    if (refine)
      hipLaunchKernelGGL((k_bg_composite<kBgColor, true>), grid, dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((k_bg_composite<kBgColor, false>), grid, dim3(256), 0, s, p);
  } else if (mode == kBgImage) {
    if (refine)
      hipLaunchKernelGGL((k_bg_composite<kBgImage, true>), grid, dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((k_bg_composite<kBgImage, false>), grid, dim3(256), 0, s, p);
  } else {
    const size_t lds = ((size_t)(kBlurTH + 2 * p.radius) * kBlurTW + p.radius + 1) * 4;
    const dim3 bgrid((p.c.fw + kBlurTW - 1) / kBlurTW, (p.c.fh + kBlurTH - 1) / kBlurTH, n);
    if (p.overlay) {
      if (refine)
        hipLaunchKernelGGL((k_bg_composite<kBgBlur, true, true>), bgrid, dim3(256), lds, s, p);
      else
        hipLaunchKernelGGL((k_bg_composite<kBgBlur, false, true>), bgrid, dim3(256), lds, s, p);
    } else if (refine)
      hipLaunchKernelGGL((k_bg_composite<kBgBlur, true>), bgrid, dim3(256), lds, s, p);
    else
      hipLaunchKernelGGL((k_bg_composite<kBgBlur, false>), bgrid, dim3(256), lds, s, p);
  }
}

void launch_bg_streams(const BgStreamsParams& p, int nflat, int nblur, int max_radius, hipStream_t s) {
  const CompositeParams& c = p.c;
  if (nblur > 0) {
    hipLaunchKernelGGL(k_blur_h_streams, dim3((c.fw + 255) / 256, c.fh, nblur), dim3(256), 0, s, p);
    const size_t lds = ((size_t)(kBlurTH + 2 * max_radius) * kBlurTW + max_radius + 1) * 4;
    const dim3 bgrid((c.fw + kBlurTW - 1) / kBlurTW, (c.fh + kBlurTH - 1) / kBlurTH, nblur);
    hipLaunchKernelGGL(k_bg_streams_blur, bgrid, dim3(256), lds, s, p);
  }
  if (nflat > 0)
    hipLaunchKernelGGL(k_bg_streams_flat, dim3((c.fw + 255) / 256, (c.fh + 3) / 4, nflat), dim3(256), 0, s, p);
}

}  // namespace vss
