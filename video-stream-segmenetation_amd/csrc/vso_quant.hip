// vso_quant.hip — the ONNX sessions' statically quantised (QDQ) graphs (the
// planner's find_qdq): QuantizeLinear / DequantizeLinear of runtime tensors,
// and the three patterns between a DequantizeLinear and a QuantizeLinear that
// run on the integers themselves: a dense Conv on the int8 MFMA (k_qconv_tile),
// a depthwise Conv (k_qconv_dw) and the quantised residual Add (k_qadd).
//
// Storage.  A quantised tensor is one byte per element, NCHW, the model's own
// uint8 / int8 values (vso_kernels.h); every kernel here reads and writes that
// one layout, so a fused launch, a fallback k_dequantize and a graph output
// read the same bytes.
//
// k_qconv_tile.  An implicit GEMM D[m][pixel] = sum_k W[m][k] X[k][pixel] on
// v_mfma_i32_16x16x64_i8 with K = C * kh * kw in the weights' (c, ky, kx)
// order.  A 256-thread workgroup owns kQPix = 64 consecutive output pixels (of
// the flattened N * Ho * Wo) and kQBM = 64 output channels; wave w owns pixels
// 16 w .. 16 w + 15 and all four 16-channel row blocks (16 accumulator
// registers).  Per step of kQK = 64 of K the workgroup stages, in LDS,
//   Ws[64 rows][64 bytes]: one 16-byte load per thread from the packed weights
//     [Mp][Kp] (zero rows past M, zero columns past K: padding K adds nothing);
//   Xs[64 pixels][64 bytes]: thread t gathers the 16 consecutive k of segment
//     t / 64 for pixel t % 64 — a wave's 64 threads read 64 neighbouring pixels
//     of one tap at a time, so the byte loads of a tap coalesce — xor xflip
//     (uint8 -> signed), or xpad where the tap lies outside the image: spatial
//     padding contributes the zero point, not 0.
// Rows are kQLd = 80 bytes apart: 16-byte aligned, and the 16 rows a quarter
// wave reads start 20 banks apart.  Lane l then reads A = Ws[row block + l %
// 16][16 (l / 16) ..] and B = Xs[16 w + l % 16][16 (l / 16) ..]: both operands
// hold the same 16 k per lane, so the sum over k does not depend on the
// instruction's k order; the result's lane map is the dtype-independent one,
// column (pixel) l % 16, rows 4 (l / 16) + r — the matrix tests hold it to an
// asymmetric integer matrix.  Epilogue: acc - corr[m] (the zero point's share,
// exact in int32), * mult[m] + bias[m], Requant, one byte per (m, pixel).
//
// Bounds.  All indices 32-bit: the planner (try_plan_q, make_q_out) fuses only
// below 2^30 elements per tensor — N * C * H * W and N * M * Ho * Wo, leaving a
// grid stride's room under 2^31 — and below K = 2^16: a term |x| |w| is at most
// 2^14, so the int32 accumulator and corr[m] cannot overflow.  Weight loads: rows < Mp, columns < Kp of the packed image.
// Activation loads: only at (c < C, 0 <= iy < H, 0 <= ix < W) of image n < N
// (pixels >= N * Ho * Wo gather nothing).  Stores: pixel < N * Ho * Wo, m < M.
// The elementwise kernels: index < n.
#include <hip/hip_runtime.h>

#include "vso_device.h"
#include "vso_kernels.h"

namespace vso {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kQLd = 80;  // bytes between the staged rows

__device__ __forceinline__ float q_round(float v, float scale, int zp, int qmin, int qmax) {
  float r = rintf(v / scale) + (float)zp;  // (v_rndne: ties to even)
  return fminf(fmaxf(r, (float)qmin), (float)qmax);
}

__device__ __forceinline__ unsigned char requant(float v, const Requant& q) {
  if (q.act == ACT_RELU) v = fmaxf(v, 0.f);
  else if (q.act == ACT_CLIP) v = fminf(fmaxf(v, q.lo), q.hi);
  return (unsigned char)(int)q_round(v, q.sy, q.zy, q.qmin, q.qmax);
}

__device__ __forceinline__ int q_load(const unsigned char* p, int sgn) {
  return sgn ? (int)(signed char)*p : (int)*p;
}

}  // namespace

__global__ __launch_bounds__(256) void k_quantize(QuantParams p) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)gridDim.x * 256)
    p.y[i] = (unsigned char)(int)q_round(p.x[i], p.scale, p.zp, p.qmin, p.qmax);
}

__global__ __launch_bounds__(256) void k_dequantize(DequantParams p) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)gridDim.x * 256)
    p.y[i] = (float)(q_load(p.x + i, p.sgn) - p.zp) * p.scale;
}

__global__ __launch_bounds__(256) void k_qadd(QAddParams p) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)gridDim.x * 256) {
    const float a = (float)(q_load(p.a + i, p.asgn) - p.za) * p.sa;
    const float b = (float)(q_load(p.b + i, p.bsgn) - p.zb) * p.sb;
    p.y[i] = requant(a + b, p.rq);
  }
}

__global__ __launch_bounds__(256) void k_qconv_dw(QConvParams p) {
  const int total = p.N * p.C * p.Ho * p.Wo;
  const int khw = p.kh * p.kw;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
    const int ox = o % p.Wo, oy = (o / p.Wo) % p.Ho, nc = o / (p.Wo * p.Ho), c = nc % p.C;
    const unsigned char* xp = p.x + (long)nc * p.H * p.W;
    const signed char* w = p.w + c * khw;
    int acc = 0;
    for (int ky = 0; ky < p.kh; ++ky) {
      const int iy = oy * p.sh - p.pt + ky * p.dh;
      if (iy < 0 || iy >= p.H) continue;
      for (int kx = 0; kx < p.kw; ++kx) {
        const int ix = ox * p.sw - p.pl + kx * p.dw;
        if (ix < 0 || ix >= p.W) continue;
        acc += (q_load(xp + iy * p.W + ix, p.xsgn) - p.zx) * (int)w[ky * p.kw + kx];
      }
    }
    float v = (float)acc * p.mult[c];
    if (p.bias) v += p.bias[c];
    p.y[o] = requant(v, p.rq);
  }
}

__global__ __launch_bounds__(256) void k_qconv_tile(QConvParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char Ws[kQBM * kQLd];
  __shared__ __attribute__((aligned(16))) unsigned char Xs[kQPix * kQLd];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int HoWo = p.Ho * p.Wo, P = p.N * HoWo;
  const int pix0 = blockIdx.x * kQPix, m0 = blockIdx.y * kQBM;

  // this thread's part of the staging: a pixel and a 16-byte segment of K; a weight row and segment
  const int gp = pix0 + lane;
  const bool pv = gp < P;
  int n = 0, oy = 0, ox = 0;
  if (pv) {
    n = gp / HoWo;
    const int r = gp - n * HoWo;
    oy = r / p.Wo;
    ox = r - oy * p.Wo;
  }
  const int iy0 = oy * p.sh - p.pt, ix0 = ox * p.sw - p.pl;
  const unsigned char* xn = p.x + (long)n * p.C * p.H * p.W;
  const signed char* wrow = p.w + (long)(m0 + (t >> 2)) * p.Kp + (t & 3) * 16;
  const int khw = p.kh * p.kw;

  i32x4 acc[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = i32x4{0, 0, 0, 0};

  for (int k0 = 0; k0 < p.Kp; k0 += kQK) {
    *reinterpret_cast<uint4*>(Ws + (t >> 2) * kQLd + (t & 3) * 16) = *reinterpret_cast<const uint4*>(wrow + k0);
    unsigned int q[4] = {0u, 0u, 0u, 0u};
    const int k = k0 + wave * 16;
    if (pv && k < p.K) {
      int c = k / khw;
      const int r = k - c * khw;
      int ky = r / p.kw, kx = r - ky * p.kw;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        unsigned int b = 0u;
        if (k + j < p.K) {
          const int iy = iy0 + ky * p.dh, ix = ix0 + kx * p.dw;
          b = (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                  ? ((unsigned int)xn[((long)c * p.H + iy) * p.W + ix] ^ (unsigned int)p.xflip)
                  : (unsigned int)p.xpad;
        }
        q[j >> 2] |= b << ((j & 3) * 8);
        if (++kx == p.kw) {
          kx = 0;
          if (++ky == p.kh) {
            ky = 0;
            ++c;
          }
        }
      }
    }
    *reinterpret_cast<uint4*>(Xs + lane * kQLd + wave * 16) = uint4{q[0], q[1], q[2], q[3]};
    __syncthreads();
    const i32x4 bf = *reinterpret_cast<const i32x4*>(Xs + (wave * 16 + (lane & 15)) * kQLd + (lane >> 4) * 16);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const i32x4 af = *reinterpret_cast<const i32x4*>(Ws + (mt * 16 + (lane & 15)) * kQLd + (lane >> 4) * 16);
      acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, acc[mt], 0, 0, 0);
    }
    __syncthreads();
  }

  // D: column (pixel) lane % 16, rows (channels) 4 (lane / 16) + r of each 16-row block
  const int e = pix0 + wave * 16 + (lane & 15);
  if (e >= P) return;
  const int en = e / HoWo;
  unsigned char* yo = p.y + (long)en * p.M * HoWo + (e - en * HoWo);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + mt * 16 + (lane >> 4) * 4 + r;
      if (m >= p.M) continue;
      float v = (float)(acc[mt][r] - p.corr[m]) * p.mult[m];
      if (p.bias) v += p.bias[m];
      yo[(long)m * HoWo] = requant(v, p.rq);
    }
}

static int grid_for(long n) { return (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536); }

void launch_quantize(const QuantParams& p, hipStream_t s) {
  if (p.n > 0) hipLaunchKernelGGL(k_quantize, dim3(grid_for(p.n)), dim3(256), 0, s, p);
}

void launch_dequantize(const DequantParams& p, hipStream_t s) {
  if (p.n > 0) hipLaunchKernelGGL(k_dequantize, dim3(grid_for(p.n)), dim3(256), 0, s, p);
}

void launch_qadd(const QAddParams& p, hipStream_t s) {
  if (p.n > 0) hipLaunchKernelGGL(k_qadd, dim3(grid_for(p.n)), dim3(256), 0, s, p);
}

void launch_qconv_dw(const QConvParams& p, hipStream_t s) {
  const long total = (long)p.N * p.C * p.Ho * p.Wo;
  if (total > 0) hipLaunchKernelGGL(k_qconv_dw, dim3(grid_for(total)), dim3(256), 0, s, p);
}

void launch_qconv_tile(const QConvParams& p, hipStream_t s) {
  const long P = (long)p.N * p.Ho * p.Wo;
  if (P <= 0 || p.M <= 0) return;
  hipLaunchKernelGGL(k_qconv_tile, dim3((unsigned)((P + kQPix - 1) / kQPix), (unsigned)(p.Mp / kQBM)), dim3(256), 0, s, p);
}

}  // namespace vso
