// vso_attn.hip — the ONNX sessions' fused attention (the planner's
// find_attention): y = softmax(scale * Q K^T + bias) V per slice of the leading
// dims, in one launch that never writes the [Nq][Nk] score matrix.  Every
// product runs on v_mfma_f32_16x16x4_f32 — exact f32 products, f32
// accumulation — in every session precision, as k_gemm's.
//
// Work.  A 256-thread workgroup owns one slice b and 64 query rows, 16 per
// wave.  It walks the keys in blocks of 32 (two 16-key halves; the second is
// skipped when the block's tail has no key in it): the block's K and V rows
// are staged once in LDS for the four waves, each wave computes its 16 x 32
// scores, folds them into the running maximum m and running sum l of its
// queries (the flash recurrence: l and the output accumulators are scaled by
// exp(m_old - m_new) when the maximum moves, exp is only ever taken of a
// difference from the maximum) and adds P V to its accumulators.  The output
// is written once, divided by l.
//
// MFMA operand maps (lane = 16 g + r): A[row r][k g], B[k g][col r],
// D[row 4 g + v][col r].  Both products are computed transposed, so that a
// query is a COLUMN of either result and all of its state sits in the four
// lanes (r, 0 .. 3):
//   S^T = K Q^T   A = K[key r][e], B = Q[query r][e] with e = 8 j + 2 g + {0, 1}
//                 for the step pair j (an 8-byte fragment per lane and pair: any
//                 order of d's elements over steps x k is one sum);
//                 D = S^T[key 4 g + v][query r]: lane (r, g) holds keys
//                 4 g .. 4 g + 3 of query r.  The row maximum / sum is four
//                 in-lane values, then lanes r, r + 16, r + 32, r + 48.
//   O^T = V^T P^T A = V[key 4 g + e][column 16 t + r], B = P[query r][key 4 g + e]
//                 — the register S^T left it in, no transpose through LDS;
//                 D = O^T[column 16 t + 4 g + v][query r]: a lane's four values
//                 are consecutive in the output row (one 16-byte store).
// U = ceil(max(d, dv) / 16) rounded up to 1, 2, 4 or 8 is the template
// parameter; fragment lanes past d / dv are zero.
//
// LDS.  K and V blocks: [32 keys][16 U + 4] floats each.  The pitch 16 U + 4:
//  * K fragments are ds_read_b64 (banks (a / 4) mod 64, conflicts per 32-lane
//    half): lane (r, g) of a half reads 8-byte slot r (8 U + 2) + 4 j + g,
//    and 8 U + 2 = 2 (4 U + 1) with 4 U + 1 odd sends r = 0 .. 15 to the 16
//    distinct even slots mod 32, g & 1 picks the odd one beside: 32 lanes on
//    32 distinct slots, conflict-free.  (ds_read_b128 fragments cannot be
//    made conflict-free by a pitch: its 16-lane groups mix lanes g and g + 1
//    of rows whose differences cover every residue.)
//  * V operands are ds_read_b32 (banks (a / 4) mod 32, per 32-lane half):
//    lane (r, g) reads word (4 g + e)(16 U + 4) + 16 t + r; 4 (16 U + 4) = 16
//    mod 32, so g = 0, 1 take banks r and 16 + r: conflict-free.
//
// Bounds.  Q rows are read at min(query, Nq - 1), K / V rows at
// min(key, Nk - 1), columns at min(column, d - 2 | d - 4 | dv - 4), the bias at
// the same clamped (query, key): every address formed lies inside its tensor,
// on taken and untaken lanes alike; what a clamp duplicated is replaced by 0
// (operands) or -inf (scores of keys >= Nk, before the maximum: Nk >= 1, so a
// row always keeps a key).  Rows >= Nq and columns >= dv are not stored.  LDS
// is read at rows < 32 and floats < 16 U of a row.
//
// Resources (gfx950, hipcc -O3, the resource usage remarks of this unit; no
// instance uses scratch):
//   U (d, dv up to)   VGPRs   LDS / workgroup   workgroups per CU (one wave per SIMD each)
//   1 (16)              50       5 120 B           8 (the SIMD's 8 wave slots)
//   2 (32)              58       9 216 B           8
//   4 (64)              72      17 408 B           7 (512 / 72 VGPRs; LDS would allow 9)
//   8 (128)            108      33 792 B           4 (512 / 108 VGPRs, and 160 KB / 33 KB of LDS)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vso_device.h"
#include "vso_kernels.h"

namespace vso {

typedef float f2 __attribute__((ext_vector_type(2)));

template <int U>
__global__ __launch_bounds__(256) void k_attn(AttnParams p) {
  constexpr int P = 16 * U + 4;  // floats between the staged rows
  __shared__ __attribute__((aligned(16))) float sk[32 * P];
  __shared__ __attribute__((aligned(16))) float sv[32 * P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int tiles_q = (p.Nq + 63) >> 6;
  const int b = blockIdx.x / tiles_q, qt = blockIdx.x - b * tiles_q;
  const int Nq = p.Nq, Nk = p.Nk, d = p.d, dv = p.dv;
  const int q = qt * 64 + wave * 16 + r, qc = min(q, Nq - 1);

  // this lane's Q fragments: elements 8 j + 2 g, + 1 of its query
  f2 qf[2 * U];
  {
    const float* qrow = p.q + ((long)b * Nq + qc) * d;
#pragma unroll
    for (int j = 0; j < 2 * U; ++j) {
      const int c = 8 * j + 2 * g;
      const f2 t = *reinterpret_cast<const f2*>(qrow + min(c, d - 2));
      qf[j] = c < d ? t : f2{0.f, 0.f};
    }
  }
  const float* brow = nullptr;
  if (p.bias) {
    long off = 0;
    int rem = b;
    for (int k = p.nlead - 1; k >= 0; --k) {
      off += (long)(rem % p.lead[k]) * p.bstr[k];
      rem /= p.lead[k];
    }
    brow = p.bias + off + (long)qc * Nk;
  }
  const float* kb = p.k + (long)b * Nk * d;
  const float* vb = p.v + (long)b * Nk * dv;

  f4 o[U];
#pragma unroll
  for (int t = 0; t < U; ++t) o[t] = f4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;  // l_run: this lane's keys only; summed over g at the end

  for (int j0 = 0; j0 < Nk; j0 += 32) {
    __syncthreads();  // the block before is read
    for (int idx = tid; idx < 32 * 4 * U; idx += 256) {
      const int row = idx / (4 * U), c = 4 * (idx - row * 4 * U);
      const int key = j0 + row, kc = min(key, Nk - 1);
      const f4 kv = *reinterpret_cast<const f4*>(kb + (long)kc * d + min(c, d - 4));
      const f4 vv = *reinterpret_cast<const f4*>(vb + (long)kc * dv + min(c, dv - 4));
      const f4 z = f4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f4*>(&sk[row * P + c]) = (key < Nk && c < d) ? kv : z;
      *reinterpret_cast<f4*>(&sv[row * P + c]) = (key < Nk && c < dv) ? vv : z;
    }
    __syncthreads();
    const bool two = Nk - j0 > 16;  // the second half holds a key (uniform)

    float pr[2][4];
    float mb = -INFINITY;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f4 s = f4{0.f, 0.f, 0.f, 0.f};
      if (h == 0 || two) {
#pragma unroll
        for (int j = 0; j < 2 * U; ++j) {
          const f2 kf = *reinterpret_cast<const f2*>(&sk[(16 * h + r) * P + 8 * j + 2 * g]);
          s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[0], qf[j][0], s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[1], qf[j][1], s, 0, 0, 0);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int key = j0 + 16 * h + 4 * g + v;
        float t = s[v] * p.scale;
        if (brow) t += brow[min(key, Nk - 1)];
        t = key < Nk ? t : -INFINITY;
        pr[h][v] = t;
        mb = fmaxf(mb, t);
      }
    }
    mb = fmaxf(mb, __shfl_xor(mb, 16));
    mb = fmaxf(mb, __shfl_xor(mb, 32));
    const float m_new = fmaxf(m_run, mb);
    const float alpha = expf(m_run - m_new);  // 0 on the first block (m_run = -inf)
    m_run = m_new;
    float ls = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        pr[h][v] = expf(pr[h][v] - m_new);
        ls += pr[h][v];
      }
    l_run = l_run * alpha + ls;
#pragma unroll
    for (int t = 0; t < U; ++t) {
      o[t] *= alpha;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 1 && !two) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[(16 * h + 4 * g + e) * P + 16 * t + r], pr[h][e], o[t], 0, 0, 0);
      }
    }
  }
  float l = l_run + __shfl_xor(l_run, 16);
  l += __shfl_xor(l, 32);
  if (q >= Nq) return;
  float* yrow = p.y + ((long)b * Nq + q) * dv;
#pragma unroll
  for (int t = 0; t < U; ++t) {
    const int c = 16 * t + 4 * g;
    if (c < dv) *reinterpret_cast<f4*>(yrow + c) = f4{o[t][0] / l, o[t][1] / l, o[t][2] / l, o[t][3] / l};
  }
}

static int attn_u(const AttnParams& p) {
  const int c = (std::max(p.d, p.dv) + 15) / 16;
  return c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8;
}

bool attn_supported(const AttnParams& p) {
  const auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  return p.BH >= 1 && p.Nq >= 1 && p.Nk >= 1 && p.d >= 4 && p.dv >= 4 && p.d % 4 == 0 && p.dv % 4 == 0 &&
         p.d <= kAttnMaxD && p.dv <= kAttnMaxD && p.nlead <= kAttnMaxLead && al(p.q) && al(p.k) && al(p.v) && al(p.y) &&
         (long)p.BH * ((p.Nq + 63) / 64) < (1L << 31);
}

const char* attn_kernel_name(const AttnParams& p) {
  switch (attn_u(p)) {
    case 1: return "void vso::k_attn<1>(vso::AttnParams)";
    case 2: return "void vso::k_attn<2>(vso::AttnParams)";
    case 4: return "void vso::k_attn<4>(vso::AttnParams)";
    default: return "void vso::k_attn<8>(vso::AttnParams)";
  }
}

void launch_attn(const AttnParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(p.BH * ((p.Nq + 63) / 64)));
  switch (attn_u(p)) {
    case 1: hipLaunchKernelGGL(k_attn<1>, grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL(k_attn<2>, grid, dim3(256), 0, s, p); break;
    case 4: hipLaunchKernelGGL(k_attn<4>, grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL(k_attn<8>, grid, dim3(256), 0, s, p); break;
  }
}

}  // namespace vso
