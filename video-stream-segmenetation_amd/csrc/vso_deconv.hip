// vso_deconv.hip — the ONNX sessions' transposed convolution at stride > 1
// (ConvTranspose; a stride-1 one is planned as the Conv it equals): the phase
// decomposition of vso_kernels.h (DeconvParams) as an implicit GEMM per phase
// on v_mfma_f32_16x16x4_f32, k_deconv_tile, and as a VALU gather,
// k_deconv_direct.  Every operand is f32 in every session precision.
//
// Bounds.  Both kernels read x only at (iy, ix) tested against [0, H) x [0, W)
// and write y only at (oy, ox) tested against [0, Ho) x [0, Wo), m < M.
// k_deconv_tile reads its packed weights at rows < Mp (a multiple of
// kDeconvBM) and columns < Cp (a multiple of 16), both zero padded by the
// planner, and the LDS region at rows wave + nty - 1 - jy in [0, 3 + nty - 1],
// columns r + ntx0 - 1 - jx in [0, 15 + ntx0 - 1] (jx < ntx <= ntx0), of
// channels < 16: inside the 16 x plane floats staged (plane >=
// (kDeconvTH + tmy - 1) * pitch, pitch = 16 + tmx - 1, nty <= tmy, ntx0 <= tmx).  k_deconv_direct reads the node's
// weights at (c < C, mg < Mg, ky < kh, kx < kw) from the tap tables.
#include <hip/hip_runtime.h>

#include "vso_device.h"
#include "vso_kernels.h"

namespace vso {

// MFMA operand maps (lane = 16 g + r), as k_ir's: A[row r][k g], B[k g][col r],
// D[row 4 g + v][col r].  Here rows are output channels, columns the 16 pixels
// of the wave's tile row, k four input channels: a lane's 16-byte weight load
// holds channels c0 + 4 g .. + 3 of output channel r, so MFMA step j multiplies
// channel c0 + 4 g + j on both sides (any order of a chunk's 16 channels over
// the 4 steps x 4 k is one sum).
//
// SX: the x phases a workgroup computes.  1: one phase (blockIdx.y counts
// sh * sw of them); a row's stores are sw floats apart.  2 (sw == 2): both x
// phases of a y phase from one staged region (phase 0's, the wider), so lane r
// holds outputs 2 (q0x + r) - pl and the one after it of every channel and a
// row goes out as one contiguous run.
template <int SX>
__global__ __launch_bounds__(256) void k_deconv_tile(DeconvParams p) {
  extern __shared__ float xs[];  // [16 channels][plane]: rows `pitch` apart
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
  const int mblocks = p.Mp / kDeconvBM;
  const int ph = blockIdx.y / mblocks, mb = blockIdx.y - ph * mblocks;
  const int py = SX == 1 ? ph / p.sw : ph, px0 = SX == 1 ? ph - py * p.sw : 0;
  const int n = blockIdx.z;
  // a phase's taps per axis: k = phase + j * stride < kernel
  const int nty = py < p.kh ? (p.kh - py + p.sh - 1) / p.sh : 0;
  const int ntx0 = px0 < p.kw ? (p.kw - px0 + p.sw - 1) / p.sw : 0;  // (SX 2: phase 0 has the most)
  const int q0y = p.qy0 + tile_y * kDeconvTH, q0x = p.qx0 + tile_x * 16;
  const int ncb = min(4, (p.M - mb * kDeconvBM + 15) / 16);  // 16-channel blocks holding an output channel
  const int HW = p.H * p.W;
  f4 acc[SX][4];
#pragma unroll
  for (int sx = 0; sx < SX; ++sx)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[sx][cb] = f4{0.f, 0.f, 0.f, 0.f};

  if (nty > 0 && ntx0 > 0) {
    const int RH = kDeconvTH + nty - 1, RW = 16 + ntx0 - 1, RP = RH * RW;
    const int iy0 = q0y - (nty - 1), ix0 = q0x - (ntx0 - 1);
    const float* xn = p.x + (long)n * p.C * HW;
    for (int c0 = 0; c0 < p.C; c0 += 16) {
      __syncthreads();  // (the chunk before has been read)
      for (int e = tid; e < 16 * RP; e += 256) {
        const int cc = e / RP, rem = e - cc * RP, ry = rem / RW, rx = rem - ry * RW;
        const int c = c0 + cc, iy = iy0 + ry, ix = ix0 + rx;
        float v = 0.f;
        if (c < p.C && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) v = xn[(long)c * HW + iy * p.W + ix];
        xs[cc * p.plane + ry * p.pitch + rx] = v;
      }
      __syncthreads();
#pragma unroll
      for (int sx = 0; sx < SX; ++sx) {
        const int px = px0 + sx;
        const int ntx = px < p.kw ? (p.kw - px + p.sw - 1) / p.sw : 0;
        for (int jy = 0; jy < nty; ++jy)
          for (int jx = 0; jx < ntx; ++jx) {
            const float* wt = p.w + ((long)(((py * p.sw + px) * p.tmy + jy) * p.tmx + jx) * p.Mp + mb * kDeconvBM + r) * p.Cp +
                              c0 + 4 * g;
            const float* xb = xs + 4 * g * p.plane + (wave + nty - 1 - jy) * p.pitch + (r + ntx0 - 1 - jx);
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = xb[j * p.plane];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
              if (cb < ncb) {
                const f4 a = *reinterpret_cast<const f4*>(wt + (long)cb * 16 * p.Cp);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  acc[sx][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[sx][cb], 0, 0, 0);
              }
          }
      }
    }
  }

  // ---- epilogue: lane (r, g) holds pixel r of row `wave`, channels 16 cb + 4 g + v ----
  const int oy = (q0y + wave) * p.sh + py - p.pt;
  if ((unsigned)oy >= (unsigned)p.Ho) return;
  const int m0 = mb * kDeconvBM + 4 * g;
  const long P = (long)p.Ho * p.Wo;
  auto ch_of = [&](int k) { return m0 + (k >> 2) * 16 + (k & 3); };
  float* yn = p.y + (long)n * ((long)p.M * P + p.y_nx);
  float o[SX][16];
#pragma unroll
  for (int sx = 0; sx < SX; ++sx) {
    const int ox = (q0x + r) * p.sw + px0 + sx - p.pl;
    const bool in = (unsigned)ox < (unsigned)p.Wo;
    const int pix = oy * p.Wo + ox;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int m = ch_of(k);
      o[sx][k] = acc[sx][k >> 2][k & 3];
      if (in && m < p.M) {
        if (p.ep.bias) o[sx][k] += p.ep.bias[m];
        if (p.ep.res) o[sx][k] += residual(p.ep, m, ((long)n * p.M + m) * P + pix, n, pix);
      }
    }
    act_block(o[sx], ch_of, p.ep);
  }
  const int ox0 = (q0x + r) * p.sw + px0 - p.pl;
  if constexpr (SX == 2) {
    // both outputs inside the row and their pair 8-byte aligned in every plane: one store
    const bool both = ox0 >= 0 && ox0 + 1 < p.Wo;
    if (both && ((P | (long)(oy * p.Wo + ox0)) & 1) == 0 && (reinterpret_cast<uintptr_t>(yn) & 7) == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int m = ch_of(k);
        if (m < p.M) *reinterpret_cast<float2*>(yn + (long)m * P + oy * p.Wo + ox0) = float2{o[0][k], o[1][k]};
      }
      return;
    }
  }
#pragma unroll
  for (int sx = 0; sx < SX; ++sx) {
    const int ox = ox0 + sx;
    if ((unsigned)ox >= (unsigned)p.Wo) continue;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int m = ch_of(k);
      if (m < p.M) yn[(long)m * P + oy * p.Wo + ox] = o[sx][k];
    }
  }
}

__global__ __launch_bounds__(256) void k_deconv_direct(DeconvParams p) {
  const int quads = (p.Qw + kDeconvPx - 1) / kDeconvPx;
  const long total = (long)p.N * p.M * p.sh * p.sw * p.Qh * quads;
  const int* ys = p.taps;
  const int* yt = p.taps + p.o_yt;
  const int* xst = p.taps + p.o_xs;
  const int* xt = p.taps + p.o_xt;
  const long HW = (long)p.H * p.W, P = (long)p.Ho * p.Wo;
  const long wstep = (long)p.Mg * p.kh * p.kw;  // weights of the next input channel
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
    long t = it;
    const int qd = (int)(t % quads); t /= quads;
    const int qr = (int)(t % p.Qh); t /= p.Qh;
    const int px = (int)(t % p.sw); t /= p.sw;
    const int py = (int)(t % p.sh); t /= p.sh;
    const int m = (int)(t % p.M);
    const int n = (int)(t / p.M);
    const int qy = p.qy0 + qr, qx = p.qx0 + qd * kDeconvPx;
    const int oy = qy * p.sh + py - p.pt;
    if ((unsigned)oy >= (unsigned)p.Ho) continue;
    const int grp = m / p.Mg, mg = m - grp * p.Mg;
    const float* xg = p.x + ((long)n * p.C + (long)grp * p.Cg) * HW;
    const float* wg = p.w + ((long)grp * p.Cg * p.Mg + mg) * p.kh * p.kw;
    float acc[kDeconvPx];
#pragma unroll
    for (int j = 0; j < kDeconvPx; ++j) acc[j] = 0.f;
    for (int a = ys[py]; a < ys[py + 1]; ++a) {
      const int ky = yt[2 * a], iy = qy - yt[2 * a + 1];
      if ((unsigned)iy >= (unsigned)p.H) continue;
      for (int b = xst[px]; b < xst[px + 1]; ++b) {
        const int kx = xt[2 * b], ix = qx - xt[2 * b + 1];
        if (ix + kDeconvPx <= 0 || ix >= p.W) continue;
        const float* xc = xg + (long)iy * p.W;
        const float* wc = wg + ky * p.kw + kx;
        for (int c = 0; c < p.Cg; ++c, xc += HW, wc += wstep) {
          const float wv = *wc;
#pragma unroll
          for (int j = 0; j < kDeconvPx; ++j)
            if ((unsigned)(ix + j) < (unsigned)p.W) acc[j] = __builtin_fmaf(xc[ix + j], wv, acc[j]);
        }
      }
    }
    const long o0 = ((long)n * p.M + m) * P + (long)oy * p.Wo;
#pragma unroll
    for (int j = 0; j < kDeconvPx; ++j) {
      const int ox = (qx + j) * p.sw + px - p.pl;
      if (qd * kDeconvPx + j < p.Qw && (unsigned)ox < (unsigned)p.Wo)
        p.y[o0 + ox + n * p.y_nx] = epilogue(p.ep, acc[j], m, o0 + ox, n, oy * p.Wo + ox);
    }
  }
}

size_t deconv_tile_lds(const DeconvParams& p) { return (size_t)16 * p.plane * sizeof(float); }

const char* deconv_tile_name(const DeconvParams& p) {
  return p.sx == 2 ? "void vso::k_deconv_tile<2>(vso::DeconvParams)" : "void vso::k_deconv_tile<1>(vso::DeconvParams)";
}

void launch_deconv_tile(const DeconvParams& p, hipStream_t s) {
  const dim3 grid((unsigned)p.tiles, (unsigned)(p.sh * (p.sx == 2 ? 1 : p.sw) * (p.Mp / kDeconvBM)), (unsigned)p.N);
  if (p.sx == 2) hipLaunchKernelGGL(k_deconv_tile<2>, grid, dim3(256), deconv_tile_lds(p), s, p);
  else hipLaunchKernelGGL(k_deconv_tile<1>, grid, dim3(256), deconv_tile_lds(p), s, p);
}

void launch_deconv_direct(const DeconvParams& p, hipStream_t s) {
  const long total = (long)p.N * p.M * p.sh * p.sw * p.Qh * ((p.Qw + kDeconvPx - 1) / kDeconvPx);
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_deconv_direct, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, p);
}

}  // namespace vso
