// vss_matte.hip — the edge-aware matte: a fast guided filter (He & Sun) of the
// post chain's alpha bytes by the frame's luma.  The definition, step by step,
// is in include/vss.h (and DESIGN.md 7.2); every step is integer arithmetic,
// doubles in one prescribed order or the upscale's f32 recipe, so the kernels
// match tests/matte_ref.py bit for bit.
//
//   k_matte_guide : L[n][H][W] u8, the area mean of the luma over each mask
//                   pixel's footprint.  One workgroup = one mask row: its
//                   threads walk the frame rows of the footprint side by side
//                   (consecutive lanes, consecutive pixels; 4 RGB pixels as 3
//                   dwords where the rows allow), each sums its columns in
//                   registers and adds them to the mask columns' LDS
//                   accumulators.
//   k_matte_coeff : 16 x 16 mask pixels per workgroup over an LDS tile of
//                   (L, p) with a radius halo (zeros outside the mask, N counts
//                   the clipped window): the four sums, the f64 fit, (a_q, b_q).
//   k_matte_mean  : the same tile shape over (a_q, b_q): the box mean as f32
//                   (abar, bbar), interleaved — one 8-B load per bilinear tap.
//   k_matte_alpha : the frame-resolution alpha plane alone (pixel_alpha and
//                   stage_matte_taps, vss_kernels.h: the code k_bg_composite
//                   blends with).
#include <hip/hip_runtime.h>

#include "vss_kernels.h"

namespace vss {

namespace {

constexpr int kMatteT = 16;  // mask pixels per tile side; with the halo of radius R, R + 1 makes the row pitch odd
__host__ __device__ constexpr int matte_side(int R) { return kMatteT + 2 * R; }
__host__ __device__ constexpr int matte_ld(int R) { return matte_side(R) + 1; }

// pixels of [i - r, i + r] inside [0, n)
__device__ __forceinline__ int clipped(int i, int r, int n) { return min(i + r, n - 1) - max(i - r, 0) + 1; }

// k_matte_guide's workgroup: mask row i of one frame (`frame`: its bytes, Lp:
// its guide plane); p gives the geometry.  acc: [W] luma sums of the row's footprints.
__device__ __forceinline__ void matte_guide_row(const MatteParams& p, const uint8_t* frame, uint8_t* Lp, int i,
                                                uint32_t* acc) {
  const int tid = threadIdx.x;
  const int r0 = (int)((long)i * p.fh / p.H), r1 = (int)((long)(i + 1) * p.fh / p.H);
  for (int j = tid; j < p.W; j += 256) acc[j] = 0;
  __syncthreads();
  const uint8_t* f = frame + (long)r0 * p.row_stride;
  // the mask column whose footprint [j*fw/W, (j+1)*fw/W) holds x: the largest j with j*fw/W <= x
  const auto column = [&](int x) { return (int)((((long)x + 1) * p.W - 1) / p.fw); };
  // RGB rows that start on dwords: 4 pixels = 3 dwords per thread and row; the
  // quad's sums go to LDS once per mask column it touches
  const bool quads = p.fc == 3 && ((reinterpret_cast<uintptr_t>(p.frames) | p.row_stride | p.frame_stride) & 3) == 0;
  const int fwq = quads ? p.fw & ~3 : 0;
  for (int x0 = tid * 4; x0 < fwq; x0 += 1024) {
    const uint8_t* q = f + (long)x0 * 3;
    uint32_t s[4] = {0, 0, 0, 0};
    for (int y = r0; y < r1; ++y, q += p.row_stride) {
      const uint32_t* d = reinterpret_cast<const uint32_t*>(q);
      const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
      s[0] += (77u * (d0 & 255u) + 150u * ((d0 >> 8) & 255u) + 29u * ((d0 >> 16) & 255u) + 128u) >> 8;
      s[1] += (77u * (d0 >> 24) + 150u * (d1 & 255u) + 29u * ((d1 >> 8) & 255u) + 128u) >> 8;
      s[2] += (77u * ((d1 >> 16) & 255u) + 150u * (d1 >> 24) + 29u * (d2 & 255u) + 128u) >> 8;
      s[3] += (77u * ((d2 >> 8) & 255u) + 150u * ((d2 >> 16) & 255u) + 29u * (d2 >> 24) + 128u) >> 8;
    }
    int cur = column(x0);
    uint32_t sum = s[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const int j = column(x0 + k);
      if (j != cur) {
        atomicAdd(&acc[cur], sum);
        cur = j;
        sum = 0;
      }
      sum += s[k];
    }
    atomicAdd(&acc[cur], sum);
  }
  for (int x = fwq + tid; x < p.fw; x += 256) {  // RGBA, unaligned rows, and the last fw % 4 pixels
    const uint8_t* q = f + (long)x * p.fc;
    uint32_t s = 0;
    for (int y = r0; y < r1; ++y, q += p.row_stride) s += matte_luma(q);
    atomicAdd(&acc[column(x)], s);
  }
  __syncthreads();
  uint8_t* L = Lp + (long)i * p.W;
  for (int j = tid; j < p.W; j += 256) {
    const int c0 = (int)((long)j * p.fw / p.W), c1 = (int)((long)(j + 1) * p.fw / p.W);
    const uint32_t cnt = (uint32_t)(r1 - r0) * (uint32_t)(c1 - c0);
    L[j] = (uint8_t)((acc[j] + cnt / 2) / cnt);
  }
}

// k_matte_coeff's workgroup on one frame's planes (Lp, ap: guide and alpha
// bytes, qp: out).  The radius is a template argument: the window loops have
// constant bounds, so the compiler unrolls the rows and keeps their LDS reads
// in flight instead of waiting for one at a time.  tile: side * matte_ld(R) dwords.
template <int R>
__device__ __forceinline__ void matte_coeff_tile(int H, int W, const uint8_t* Lp, const uint8_t* ap, int2* qp,
                                                 double eps, uint32_t* tile) {
#pragma clang fp contract(off)
  constexpr int r = R, side = matte_side(R), kMatteLd = matte_ld(R);
  const int tid = threadIdx.x;
  const int X0 = blockIdx.x * kMatteT, Y0 = blockIdx.y * kMatteT;
  for (int k = tid; k < side * side; k += 256) {
    const int ly = k / side, lx = k - ly * side, yy = Y0 - r + ly, xx = X0 - r + lx;
    uint32_t v = 0;  // L | p << 8, 0 outside the mask
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const long o = (long)yy * W + xx;
      v = (uint32_t)Lp[o] | ((uint32_t)ap[o] << 8);
    }
    tile[ly * kMatteLd + lx] = v;
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4, j = X0 + tx, i = Y0 + ty;
  if (i >= H || j >= W) return;
  uint32_t sL = 0, sp = 0, sLp = 0, sLL = 0;  // 289 * 65025 < 2^25
  for (int dy = 0; dy <= 2 * r; ++dy)
#pragma unroll
    for (int dx = 0; dx <= 2 * r; ++dx) {
      const uint32_t v = tile[(ty + dy) * kMatteLd + tx + dx], l = v & 255u, a = v >> 8;
      sL += l;
      sp += a;
      sLp += l * a;
      sLL += l * l;
    }
  const long N = (long)clipped(i, r, H) * clipped(j, r, W);
  const long cov = N * (long)sLp - (long)sL * (long)sp;
  const long var = N * (long)sLL - (long)sL * (long)sL;
  const double a = (double)cov / ((double)var + eps * (double)(N * N));
  const double prod = a * (double)sL;
  const double b = ((double)sp - prod) / (double)N;
  qp[(long)i * W + j] = make_int2((int)floor(a * 65536.0 + 0.5), (int)floor(b * 256.0 + 0.5));
}

// k_matte_mean's workgroup on one frame's planes.  tile: side * matte_ld(R) int2, (a_q, b_q), 0 outside the mask.
template <int R>
__device__ __forceinline__ void matte_mean_tile(int H, int W, const int2* qp, float2* abp, int2* tile) {
  constexpr int r = R, side = matte_side(R), kMatteLd = matte_ld(R);
  const int tid = threadIdx.x;
  const int X0 = blockIdx.x * kMatteT, Y0 = blockIdx.y * kMatteT;
  for (int k = tid; k < side * side; k += 256) {
    const int ly = k / side, lx = k - ly * side, yy = Y0 - r + ly, xx = X0 - r + lx;
    int2 v = make_int2(0, 0);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = qp[(long)yy * W + xx];
    tile[ly * kMatteLd + lx] = v;
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4, j = X0 + tx, i = Y0 + ty;
  if (i >= H || j >= W) return;
  int sa = 0, sb = 0;  // |a_q| <= 2^22, |b_q| <= 2^23: 289 terms fit int32
  for (int dy = 0; dy <= 2 * r; ++dy)
#pragma unroll
    for (int dx = 0; dx <= 2 * r; ++dx) {
      const int2 v = tile[(ty + dy) * kMatteLd + tx + dx];
      sa += v.x;
      sb += v.y;
    }
  const long N = (long)clipped(i, r, H) * clipped(j, r, W);
  abp[(long)i * W + j] =
      make_float2((float)((double)sa / (double)(N * 65536)), (float)((double)sb / (double)(N * 256)));
}

// the pooled forms' per-frame radius: one instantiation of `body` per radius, the branch workgroup-uniform
#define VSS_MATTE_RADIUS_SWITCH(radius, body) \
  switch (radius) {                           \
    case 1: body(1); break;                   \
    case 2: body(2); break;                   \
    case 3: body(3); break;                   \
    case 4: body(4); break;                   \
    case 5: body(5); break;                   \
    case 6: body(6); break;                   \
    case 7: body(7); break;                   \
    default: body(8); break;                  \
  }

}  // namespace

__global__ __launch_bounds__(256) void k_matte_guide(MatteParams p) {
  extern __shared__ __align__(16) uint32_t acc[];
  const int t = blockIdx.y;
  matte_guide_row(p, p.frames + (long)t * p.frame_stride, p.L + (long)t * p.H * p.W, blockIdx.x, acc);
}

template <int R>
__global__ __launch_bounds__(256) void k_matte_coeff(MatteParams p) {
  __shared__ uint32_t tile[matte_side(R) * matte_ld(R)];
  const long base = (long)blockIdx.z * p.H * p.W;
  matte_coeff_tile<R>(p.H, p.W, p.L + base, p.alpha + base, p.q + base, p.eps, tile);
}

template <int R>
__global__ __launch_bounds__(256) void k_matte_mean(MatteParams p) {
  __shared__ int2 tile[matte_side(R) * matte_ld(R)];
  const long base = (long)blockIdx.z * p.H * p.W;
  matte_mean_tile<R>(p.H, p.W, p.q + base, p.ab + base, tile);
}

// ---- many streams: frame list[z] with its own radius, eps and planes (MatteStreamsParams) ----
__global__ __launch_bounds__(256) void k_matte_guide_streams(MatteStreamsParams p) {
  extern __shared__ __align__(16) uint32_t acc[];
  const int t = stream_list_at(p.list, blockIdx.y);
  matte_guide_row(p.m, p.m.frames + (long)t * p.m.frame_stride, p.entry[t].L, blockIdx.x, acc);
}

__global__ __launch_bounds__(256) void k_matte_coeff_streams(MatteStreamsParams p) {
  __shared__ uint32_t tile[matte_side(kMatteMaxRadius) * matte_ld(kMatteMaxRadius)];
  const int t = stream_list_at(p.list, blockIdx.z), H = p.m.H, W = p.m.W;
  const uint8_t* Lp = p.entry[t].L;
  const uint8_t* ap = p.m.alpha + (long)t * H * W;
  int2* qp = p.entry[t].q;
  const double eps = p.entry[t].eps;
#define VSS_BODY(R) matte_coeff_tile<R>(H, W, Lp, ap, qp, eps, tile)
  VSS_MATTE_RADIUS_SWITCH(p.entry[t].radius, VSS_BODY)
#undef VSS_BODY
}

__global__ __launch_bounds__(256) void k_matte_mean_streams(MatteStreamsParams p) {
  __shared__ int2 tile[matte_side(kMatteMaxRadius) * matte_ld(kMatteMaxRadius)];
  const int t = stream_list_at(p.list, blockIdx.z), H = p.m.H, W = p.m.W;
  const int2* qp = p.entry[t].q;
  float2* abp = p.entry[t].ab;
#define VSS_BODY(R) matte_mean_tile<R>(H, W, qp, abp, tile)
  VSS_MATTE_RADIUS_SWITCH(p.entry[t].radius, VSS_BODY)
#undef VSS_BODY
}

// k_composite's thread shape: 4 consecutive pixels of one row, one 4-B store.
template <bool REFINE>
__global__ __launch_bounds__(256) void k_matte_alpha(MatteAlphaParams p) {
  const CompositeParams& c = p.c;
  const int t = blockIdx.z;
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const long plane = (long)t * c.H * c.W;
  MatteTaps m{};
  if constexpr (REFINE) {
    __shared__ float2 taps[kMatteTapRows * kMatteTapCols];
    m = stage_matte_taps(c, p.ab + plane, blockIdx.y * 4, blockIdx.x * 256, taps);
  }
  if (y >= c.fh || x0 >= c.fw) return;
  int ya, yb;
  float ly;
  up_coord(y, c.sy, c.H, ya, yb, ly);
  const uint8_t* ra = c.alpha + plane + (long)ya * c.W;
  const uint8_t* rb = c.alpha + plane + (long)yb * c.W;
  const float2* ma = nullptr;
  const float2* mb = nullptr;
  if constexpr (REFINE) {
    ma = m.p + (ya - m.row0) * m.pitch;
    mb = m.p + (yb - m.row0) * m.pitch;
  }
  const uint8_t* f = c.frames + (long)t * c.frame_stride + (long)y * c.row_stride;
  uint32_t A[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = min(x0 + k, c.fw - 1);
    int xa, xb;
    float lx;
    up_coord(x, c.sx, c.W, xa, xb, lx);
    A[k] = pixel_alpha<REFINE>(ra, rb, ma, mb, xa, xb, m.col0, lx, ly, f + (long)x * c.fc);
  }
  uint8_t* o = c.out + (long)t * c.out_frame_stride + (long)y * c.out_row_stride + x0;
  if (x0 + 4 <= c.fw && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(o) = A[0] | (A[1] << 8) | (A[2] << 16) | (A[3] << 24);
  } else {
    for (int k = 0; k < 4 && x0 + k < c.fw; ++k) o[k] = (uint8_t)A[k];
  }
}

template <int R>
static void launch_matte_fit(const MatteParams& p, int n, hipStream_t s) {
  const dim3 grid((p.W + kMatteT - 1) / kMatteT, (p.H + kMatteT - 1) / kMatteT, n);
  hipLaunchKernelGGL(k_matte_coeff<R>, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_matte_mean<R>, grid, dim3(256), 0, s, p);
}

void launch_matte_stage(const MatteParams& p, int n, hipStream_t s) {
  static_assert(kMatteMaxRadius == 8, "one case per radius below");
  hipLaunchKernelGGL(k_matte_guide, dim3(p.H, n), dim3(256), (size_t)p.W * 4, s, p);
  switch (p.radius) {  // 1 .. 8 (vss_background_set_refine)
    case 1: launch_matte_fit<1>(p, n, s); break;
    case 2: launch_matte_fit<2>(p, n, s); break;
    case 3: launch_matte_fit<3>(p, n, s); break;
    case 4: launch_matte_fit<4>(p, n, s); break;
    case 5: launch_matte_fit<5>(p, n, s); break;
    case 6: launch_matte_fit<6>(p, n, s); break;
    case 7: launch_matte_fit<7>(p, n, s); break;
    default: launch_matte_fit<8>(p, n, s); break;
  }
}

void launch_matte_streams(const MatteStreamsParams& p, int n, hipStream_t s) {
  const MatteParams& m = p.m;
  const dim3 grid((m.W + kMatteT - 1) / kMatteT, (m.H + kMatteT - 1) / kMatteT, n);
  hipLaunchKernelGGL(k_matte_guide_streams, dim3(m.H, n), dim3(256), (size_t)m.W * 4, s, p);
  hipLaunchKernelGGL(k_matte_coeff_streams, grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_matte_mean_streams, grid, dim3(256), 0, s, p);
}

void launch_matte_alpha(const MatteAlphaParams& p, int n, hipStream_t s) {
  const dim3 grid((p.c.fw + 255) / 256, (p.c.fh + 3) / 4, n);
  if (p.ab)
    hipLaunchKernelGGL(k_matte_alpha<true>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(k_matte_alpha<false>, grid, dim3(256), 0, s, p);
}

}  // namespace vss
