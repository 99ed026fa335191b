// vso_dynq.hip — the ONNX sessions' dynamically quantised graphs (what
// onnxruntime's quantize_dynamic writes; the planner's find_dynq):
// DynamicQuantizeLinear of a runtime tensor (k_dyn_minmax + k_dyn_quantize),
// and ConvInteger / MatMulInteger on the integers: a dense one on the int8 MFMA
// (k_iconv_tile), any other on the VALU (k_iconv_direct).  Either ends in the
// int32 values, or — the chain Cast -> Mul by x_scale * w_scale [-> Add bias]
// [-> Relu | Clip] fused — in float32.
//
// Storage.  The byte tensors of vso_quant.hip: one byte per element, NCHW, the
// model's own uint8 / int8 values.  y_scale is one float32 and y_zero_point one
// byte in HBM; every kernel that needs them reads them there, so nothing of a
// DynamicQuantizeLinear goes back to the host and its launches replay in the
// captured graph like any other.  An int32 tensor is four bytes per element.
//
// DynamicQuantizeLinear.  The operator text in float32, each step rounded once
// (no reciprocal, nothing contracted: `fp contract(off)` below):
//   mn = min(0, min x), mx = max(0, max x), scale = (mx - mn) / 255,
//   zp = saturate(rne((0 - mn) / scale)), y = saturate(rne(x / scale) + zp).
// mx == mn (an all-zero tensor), which the text leaves open, gives scale 1,
// zero point 0 and y 0: onnxruntime's choice.  k_dyn_minmax: a grid-stride
// loop, a wave reduction by lane shuffles, the four waves through LDS, one
// (min, max) pair per workgroup.  k_dyn_quantize: every workgroup reduces the
// <= kDynParts pairs again (thread t takes pair t), derives scale and zero
// point, quantises its share; workgroup 0 stores the two.  No atomics.
//
// k_iconv_tile.  k_qconv_tile's implicit GEMM (vso_quant.hip: the 64-pixel x
// 64-channel tile, the 80-byte LDS pitch, the operand and result lane maps),
// with what the dynamic form changes: the activations' zero point is a byte in
// HBM; the weights are w' = Wq - 128 (uint8) or Wq (int8) with the zero point
// zw'[m] moved alike, so w' - zw' is the model's w - zw though that difference
// does not fit int8; the activations x' = x ^ xflip carry zx' alike, a tap
// outside the image is staged as zx' and K padding as 0 (zero weights).  Then
//   sum_k (x - zx)(w - zw[m]) = acc - zx' Sw[m] - zw'[m] Sx[pixel] + K zx' zw'[m]
// in wrapping 32-bit arithmetic, Sw[m] = sum_k w' made at create, Sx[pixel] =
// sum_k x' over the K real taps summed by the staging threads from the bytes
// they stage (each thread its 16-byte segments; the four segments of a pixel
// meet in LDS after the loop) — only when some zw'[m] != 0.  The loop is a copy
// of k_qconv_tile's, not shared with it: the gather differs in each of these
// points, and k_qconv_tile's code stays as it was measured.  A MatMulInteger
// row (rows = 1: H = W = 1, 1x1) has its K bytes contiguous: one 16-byte load
// per thread where the segment's 16 k lie below K and the address is 16-byte
// aligned, byte loads at the ragged end.
//
// k_iconv_direct.  One thread per output element, the loop over the group's
// input channels and the kernel window, sum (x - zx)(w - zw[m]) as written (a
// tap outside the image adds 0).  Any group, kernel, stride, dilation, pads,
// any K: the plan that always works.
//
// The float epilogue: float(v) * (x_scale * w_scale[m]) + bias[m], then Relu /
// Clip — convert, multiply, multiply, add, each rounded once and none
// contracted: bit for bit what k_cast_i32, k_binary (Mul, Mul, Add) and k_unary
// store when the chain is not fused.
//
// Bounds.  All indices 32-bit: the planner (plan_iconv, make_q_out) takes
// tensors below 2^30 elements only — N * C * H * W and N * M * Ho * Wo, leaving
// a grid stride's room under 2^31.  k_dyn_minmax / k_dyn_quantize: x and y at
// index < n; part at pair < blocks <= kDynParts; scale and zp one element each.
// k_iconv_tile: weight loads at rows < Mp, columns < Kp of the packed image;
// activation loads only at (c < C, 0 <= iy < H, 0 <= ix < W) of image n < N
// (pixels >= N * Ho * Wo gather nothing), the 16-byte row load only where
// k + 16 <= K = C; wsum, zw, wscale, bias at m < M; stores at pixel < N * Ho *
// Wo, m < M.  k_iconv_direct: the same conditions per tap, weights at m < M,
// k < Cg * kh * kw.  K < 2^15 on k_iconv_tile: |x'| |w'| <= 2^14 per term, so
// the int32 accumulator holds.
#include <hip/hip_runtime.h>

#include "vso_device.h"
#include "vso_kernels.h"

#pragma clang fp contract(off)

namespace vso {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kILd = 80;  // bytes between the staged rows (k_qconv_tile's pitch)

// (min, max) over the workgroup's 256 threads, in every thread
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float (*red)[2]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = mn;
    red[wave][1] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
  mx = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
}

__device__ __forceinline__ int sum_bytes(unsigned int v) {  // of four signed bytes
  return (int)(signed char)(v & 0xff) + (int)(signed char)((v >> 8) & 0xff) + (int)(signed char)((v >> 16) & 0xff) +
         (int)(signed char)(v >> 24);
}

// the epilogue of both ConvInteger kernels: v = sum (x - zx)(w - zw[m]) to element `idx` of channel m
__device__ __forceinline__ void iconv_store(const IConvParams& p, unsigned int v, int m, long idx) {
  if (p.yi) {
    p.yi[idx] = (int)v;
    return;
  }
  const float s = __fmul_rn(p.xscale[0], p.wscale[m]);
  float y = __fmul_rn((float)(int)v, s);
  if (p.bias) y = __fadd_rn(y, p.bias[m]);
  if (p.act == ACT_RELU) y = fmaxf(y, 0.f);
  else if (p.act == ACT_CLIP) y = fminf(fmaxf(y, p.lo), p.hi);
  p.yf[idx] = y;
}

}  // namespace

__global__ __launch_bounds__(256) void k_dyn_minmax(DynQParams p) {
  __shared__ float red[4][2];
  float mn = 0.f, mx = 0.f;  // (the range always holds 0)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)gridDim.x * 256) {
    const float v = p.x[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, red);
  if (threadIdx.x == 0) {
    p.part[2 * blockIdx.x] = mn;
    p.part[2 * blockIdx.x + 1] = mx;
  }
}

__global__ __launch_bounds__(256) void k_dyn_quantize(DynQParams p) {
  __shared__ float red[4][2];
  float mn = 0.f, mx = 0.f;
  if ((int)threadIdx.x < p.blocks) {
    mn = p.part[2 * threadIdx.x];
    mx = p.part[2 * threadIdx.x + 1];
  }
  block_minmax(mn, mx, red);
  float scale = 1.f, zp = 0.f;
  if (mx != mn) {
    scale = __fdiv_rn(__fsub_rn(mx, mn), 255.f);
    zp = fminf(fmaxf(rintf(__fdiv_rn(__fsub_rn(0.f, mn), scale)), 0.f), 255.f);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    p.scale[0] = scale;
    p.zp[0] = (unsigned char)(int)zp;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)gridDim.x * 256) {
    const float r = __fadd_rn(rintf(__fdiv_rn(p.x[i], scale)), zp);
    p.y[i] = (unsigned char)(int)fminf(fmaxf(r, 0.f), 255.f);
  }
}

__global__ __launch_bounds__(256) void k_iconv_direct(IConvParams p) {
  const int total = p.N * p.M * p.Ho * p.Wo;
  const int khw = p.kh * p.kw;
  const int zxs = (int)(signed char)(((p.zx ? (int)p.zx[0] : 0) ^ p.xflip) & 0xff);
  for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
    const int ox = o % p.Wo, oy = (o / p.Wo) % p.Ho, nm = o / (p.Wo * p.Ho), m = nm % p.M, n = nm / p.M;
    const unsigned char* xg = p.x + ((long)n * p.C + (long)(m / p.Mg) * p.Cg) * p.H * p.W;
    const signed char* w = p.w + (long)m * p.Cg * khw;
    const int zwm = p.zw ? p.zw[m] : 0;
    unsigned int acc = 0u;
    for (int c = 0; c < p.Cg; ++c)
      for (int ky = 0; ky < p.kh; ++ky) {
        const int iy = oy * p.sh - p.pt + ky * p.dh;
        if (iy < 0 || iy >= p.H) continue;
        for (int kx = 0; kx < p.kw; ++kx) {
          const int ix = ox * p.sw - p.pl + kx * p.dw;
          if (ix < 0 || ix >= p.W) continue;
          const int xv = (int)(signed char)(xg[((long)c * p.H + iy) * p.W + ix] ^ (unsigned char)p.xflip);
          acc += (unsigned int)((xv - zxs) * ((int)w[c * khw + ky * p.kw + kx] - zwm));
        }
      }
    iconv_store(p, acc, m, o);
  }
}

__global__ __launch_bounds__(256) void k_iconv_tile(IConvParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char Ws[kQBM * kILd];
  __shared__ __attribute__((aligned(16))) unsigned char Xs[kQPix * kILd];
  __shared__ int Sxs[4][kQPix];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int HoWo = p.Ho * p.Wo, P = p.N * HoWo;
  const int pix0 = blockIdx.x * kQPix, m0 = blockIdx.y * kQBM;
  // the activations' zero point as the signed byte the MFMA multiplies: what a tap outside the image holds
  const unsigned int xpad = (unsigned int)(((p.zx ? (int)p.zx[0] : 0) ^ p.xflip) & 0xff);
  const int zxs = (int)(signed char)xpad;
  const unsigned int flip4 = (unsigned int)p.xflip * 0x01010101u;

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
  int sxp = 0;  // this thread's share of Sx[its pixel]

  i32x4 acc[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = i32x4{0, 0, 0, 0};

  for (int k0 = 0; k0 < p.Kp; k0 += kQK) {
    *reinterpret_cast<uint4*>(Ws + (t >> 2) * kILd + (t & 3) * 16) = *reinterpret_cast<const uint4*>(wrow + k0);
    unsigned int q[4] = {0u, 0u, 0u, 0u};
    const int k = k0 + wave * 16;
    if (pv && k < p.K) {
      if (p.rows && k + 16 <= p.K && ((reinterpret_cast<uintptr_t>(xn + k) & 15) == 0)) {
        const uint4 v = *reinterpret_cast<const uint4*>(xn + k);
        q[0] = v.x ^ flip4; q[1] = v.y ^ flip4; q[2] = v.z ^ flip4; q[3] = v.w ^ flip4;
      } else {
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
                    : xpad;
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
      if (p.zw) sxp += sum_bytes(q[0]) + sum_bytes(q[1]) + sum_bytes(q[2]) + sum_bytes(q[3]);
    }
    *reinterpret_cast<uint4*>(Xs + lane * kILd + wave * 16) = uint4{q[0], q[1], q[2], q[3]};
    __syncthreads();
    const i32x4 bf = *reinterpret_cast<const i32x4*>(Xs + (wave * 16 + (lane & 15)) * kILd + (lane >> 4) * 16);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const i32x4 af = *reinterpret_cast<const i32x4*>(Ws + (mt * 16 + (lane & 15)) * kILd + (lane >> 4) * 16);
      acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, acc[mt], 0, 0, 0);
    }
    __syncthreads();
  }
  Sxs[wave][lane] = sxp;
  __syncthreads();

  // D: column (pixel) lane % 16, rows (channels) 4 (lane / 16) + r of each 16-row block
  const int col = wave * 16 + (lane & 15);
  const int e = pix0 + col;
  if (e >= P) return;
  const unsigned int sx = (unsigned int)(Sxs[0][col] + Sxs[1][col] + Sxs[2][col] + Sxs[3][col]);
  const int en = e / HoWo;
  const long base = (long)en * p.M * HoWo + (e - en * HoWo);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + mt * 16 + (lane >> 4) * 4 + r;
      if (m >= p.M) continue;
      unsigned int v = (unsigned int)acc[mt][r] - (unsigned int)zxs * (unsigned int)p.wsum[m];
      if (p.zw) {
        const unsigned int zwm = (unsigned int)p.zw[m];
        v = v - zwm * sx + (unsigned int)p.K * (unsigned int)zxs * zwm;
      }
      iconv_store(p, v, m, base + (long)m * HoWo);
    }
}

static int grid_for(long n) { return (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536); }

int dyn_blocks(long n) {
  const long b = (n + 1023) / 1024;
  return (int)(b < 1 ? 1 : b > kDynParts ? kDynParts : b);
}

void launch_dyn_minmax(const DynQParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_dyn_minmax, dim3(p.blocks), dim3(256), 0, s, p);
}

void launch_dyn_quantize(const DynQParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_dyn_quantize, dim3(grid_for(p.n > 0 ? p.n : 1)), dim3(256), 0, s, p);
}

void launch_iconv_direct(const IConvParams& p, hipStream_t s) {
  const long total = (long)p.N * p.M * p.Ho * p.Wo;
  if (total > 0) hipLaunchKernelGGL(k_iconv_direct, dim3(grid_for(total)), dim3(256), 0, s, p);
}

void launch_iconv_tile(const IConvParams& p, hipStream_t s) {
  const long P = (long)p.N * p.Ho * p.Wo;
  if (P <= 0 || p.M <= 0) return;
  hipLaunchKernelGGL(k_iconv_tile, dim3((unsigned)((P + kQPix - 1) / kQPix), (unsigned)(p.Mp / kQBM)), dim3(256), 0, s, p);
}

}  // namespace vso
