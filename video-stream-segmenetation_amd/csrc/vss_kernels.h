// vss_kernels.h — launch parameter blocks shared by the HIP kernels
// (vss_kernels.hip) and the host planner (vss_capi.hip).  Plain structs
// passed by value as kernel arguments; no torch types anywhere.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace vss {

// Arithmetic used for the pointwise (1x1) GEMMs.
//   PREC_F32    : v_mfma_f32_16x16x4_f32 (exact f32 fma chain)
//   PREC_BF16X2 : v_mfma_f32_16x16x32_bf16 on a hi+lo bf16 split of the f32
//                 activation against bf16-exact weights (K=16 per MFMA)
//   PREC_BF16   : same MFMA, activations rounded to bf16 (lo dropped) — the
//                 lossy "pure bf16" mode; parity only vs the bf16-emulating oracle
enum Prec : int { PREC_F32 = 0, PREC_BF16X2 = 1, PREC_BF16 = 2 };

enum BlockMode : int { MODE_IR_EXPAND = 0, MODE_IR_DIRECT = 1, MODE_DEC = 2 };

// k_block FLAGS: bit 0 the decoder's src needs instance norm + ReLU, bit 1
// residual add, bits 2-3 XP-1, bits 4-5 SP-1, bits 6-7 KS-1, bit 8 STEM_IN where
//   STEM_IN = the block's input is the stem's output, computed in the block's
//        prologue from the frame (stem fused into its only consumer: one launch
//        and one HBM round trip fewer); the block still writes the stem
//        activation's tile so every layer stays readable;
//   KS = hidden-channel split of this (expand) layer: KS workgroups per tile,
//        slice s owns hidden channels [s*chid/KS, (s+1)*chid/KS) and writes
//        its partial project sum to part s of the output (bias and residual
//        in part 0): deep low-res layers get KS x the workgroups and 1/KS of
//        the weights per workgroup;
//   XP / SP = parts of the x / skip input, summed in part order (fixed, so
//        results never depend on the tiling) as the prologue loads them.
__host__ __device__ constexpr int block_flags(int norm_in, int residual, int xp, int sp, int ks, int stem_in = 0) {
  return (norm_in ? 1 : 0) | (residual ? 2 : 0) | ((xp - 1) << 2) | ((sp - 1) << 4) | ((ks - 1) << 6) |
         (stem_in ? 256 : 0);
}
__host__ __device__ constexpr bool flags_stem_in(int f) { return (f & 256) != 0; }
__host__ __device__ constexpr int flags_xp(int f) { return ((f >> 2) & 3) + 1; }
__host__ __device__ constexpr int flags_sp(int f) { return ((f >> 4) & 3) + 1; }
__host__ __device__ constexpr int flags_ks(int f) { return ((f >> 6) & 3) + 1; }

constexpr int kThreads = 256;       // 4 wave64 per workgroup
// gfx950 allocates LDS to workgroups in 2 KiB granules, 80 per CU (measured:
// tools/micro/lds_resident.cpp; hipOccupancyMaxActiveBlocksPerMultiprocessor
// assumes a finer granule and reports 3 per CU up to 54,613 B where only
// 53,248 B fit three)
constexpr int kLdsGranule = 2048, kLdsGranulesPerCu = 80;
__host__ __device__ constexpr int lds_wg_per_cu(int bytes) {
  return kLdsGranulesPerCu / ((bytes + kLdsGranule - 1) / kLdsGranule);
}
constexpr int kMaxAcc = 16;         // 16x16 project accumulators per wave
// LDS layout of the input tile and the expand waves' hidden chunks.  Measured
// (round 2, tools/lds_model.py + tools/micro/lds_taps.cpp + tools/ab_pinned.sh):
// gfx950's ds_read_b128 serves lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}
// (and +32), so a 16-pixel block read with a pixel stride of 5 or 13 bank quads
// (the padding below) is 2-way conflicted.  A layout that is conflict-free for
// every depthwise tap (VSS_PERM=1: lanes {0-3,12-15} take pixels 0-7, lanes
// {4-11} pixels 8-15; VSS_XS_PAD=8 and VSS_HS1=24: 2 mod 4 quads per pixel)
// has 4.5x fewer conflict cycles (model; SQ_LDS_BANK_CONFLICT agreed within
// 5 %) and makes the tap reads alone 1.6x faster, but its extra LDS costs
// occupancy (LDS is allocated in 2 KiB granules, 80 per CU — d3's 6x16 tile
// went from 3 to 2 workgroups per CU at 53,952 B) and the whole layers
// measured equal or slower except d2 (-5 %): the default stays the tight one.
#ifndef VSS_PERM
#define VSS_PERM 0
#endif
#ifndef VSS_XS_PAD
#define VSS_XS_PAD 4
#endif
#ifndef VSS_HS1
#define VSS_HS1 20
#endif
// decoders with even tiles upsample by 2x2 quads (VSS_QUADS=0: per pixel,
// from tap records, as odd tiles always do — an A/B knob)
#ifndef VSS_QUADS
#define VSS_QUADS 1
#endif
__host__ __device__ constexpr int block_pix(int r) { return VSS_PERM ? (r < 4 ? r : (r < 12 ? r + 4 : r - 8)) : r; }
// floats per pixel of an expand wave's hidden chunk in LDS (16 channels + pad)
// (the padded layout, VSS_SWZ=0)
__host__ __device__ constexpr int hid_stride(int stride) { return stride == 2 ? 20 : VSS_HS1; }

// Bank-conflict-free LDS layouts (round 5, VSS_SWZ=1; tools/lds_sites.py models
// every access site lane by lane against gfx950's bank rules).  The access
// pattern that sets them: a ds_read_b128 of a 16-pixel block, lane (r, g) =
// pixel r, channel quad g, is served in lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31} (+32) over 64 banks (16 bank quads); a pixel stride of
// 5 or 13 quads — the +4 float pads — is 2-way conflicted, and a plain 16-B
// write (8 contiguous lanes, 32 banks) wants the opposite of what the reads
// want from a pad.  Three layouts, no padding:
//  * quad-major planes ("QM"): quad q of pixel p at q * PLANE + 4 p floats.  A
//    lane group's 16 pixels are consecutive quads of one or two planes; with
//    PLANE a multiple of 16 quads the two channel quads of a group fall on
//    complementary pixel sets, so a run of 16 consecutive pixels is
//    conflict-free, and so is a write of 8 consecutive pixels of one plane —
//    at any pixel offset, so the taps keep immediate offsets (no VALU).
//    Stride-2 taps read every other pixel: their planes are PLANE + 1 quads
//    apart.  For b1's input tile and every expand layer's hidden chunk;
//  * XOR-swizzled pixel-major ("SW"): quad q of pixel p at p * CX + 4 (q ^
//    gray(p) % M), M = the largest power of two dividing the pixel's quads
//    (<= 16).  For the expand layers' input tile (the MFMA B reads take
//    pixel cb * 16 + r, whose swizzle is the lane's own for M <= 8), the
//    epilogue slabs and the residual centre;
//  * the decoders with 16-wide tiles keep pixel-major rows padded to 8 mod 16
//    floats (2 mod 4 quads: conflict-free for runs of 16 pixels).
#ifndef VSS_SWZ
#define VSS_SWZ 1
#endif
__host__ __device__ constexpr int pow2div16(int q) {
  return q % 16 == 0 ? 16 : (q % 8 == 0 ? 8 : (q % 4 == 0 ? 4 : (q % 2 == 0 ? 2 : 1)));
}
__host__ __device__ constexpr int gray_swz(int pix, int m) { return (pix ^ (pix >> 1)) & (m - 1); }
constexpr int kAccSlots = 4;        // instance-norm accumulator slots per frame and layer
                                    // (spreads the producers' atomics over 16x the cache lines)

__host__ __device__ constexpr int r4(int v) { return (v + 3) & ~3; }
__host__ __device__ constexpr int cmax(int a, int b) { return a > b ? a : b; }

// dw pixel runs: the output pixels of XR consecutive pixel blocks are dealt
// to lanes in horizontal runs — lane r of a "super-block" evaluates the XR
// adjacent pixels (row, c0 .. c0 + XR - 1) — so the 3 x 3 taps those pixels
// share are read from LDS once: per tap row STRIDE * (XR - 1) + 3 reads for
// XR pixels instead of 3 * XR (stride 1, XR = 4: 18 reads per 4 pixels, not
// 36).  Element j of the run is pixel block sb * XR + j's column r, so the
// MFMAs still take one 16-pixel block per call, and every output pixel's
// arithmetic is unchanged (bitwise the same activations for any XR / tile).
// XR = the largest of 4, 2, 1 that tiles the TW-wide rows and deals evenly
// to the PW pixel-block groups of waves.
__host__ __device__ constexpr int dw_run(int TW, int NPB, int PW) {
  return (TW % 4 == 0 && 16 % (TW / 4) == 0 && NPB % 4 == 0 && (NPB / 4) % PW == 0)   ? 4
         : (TW % 2 == 0 && 16 % (TW / 2) == 0 && NPB % 2 == 0 && (NPB / 2) % PW == 0) ? 2
                                                                                      : 1;
}

// Geometry + LDS carve (floats) of one k_block instantiation.  Evaluated at
// compile time in the kernel and at run time by the host planner, so the two
// can never disagree.  Every region is a multiple of 4 floats (16-B aligned).
struct BlockLds {
  int IH, IW, P_in, P_in_pad, P_out, CX, XS, LD2, SR, SC;
  // layouts (VSS_SWZ): XQM = xt quad-major (plane XPL floats; XS = 4 then),
  // XSW / RSW / XRW = the xt / slab / residual-centre swizzle modulus (1 = none),
  // HPL = the hidden chunk's plane (floats; 0 = the padded pixel-major chunk)
  bool XQM;
  int XPL, XSW, HPL, RS, RSW, XRW;
  int NCB, NPB, NCHUNK, PW, CS, NPBW, NACC;  // CS = chunk groups, PW = pixel-block groups
  int xt, xr, w1, w2, wdw, bdw, b2, wimg_end, lr, nrm, uc, work, stt, total;  // [w1, wimg_end): the weight image
  int slab_stride;  // floats per wave slab = P_out * (cout + 4)
  int slab;         // the epilogue's accumulator slabs: the work region, or (decoder) the input tile
};

// Row pitch (floats) of the fused stem's resized region x0 [3][2*IH+1][XWP]:
// its XW = 2*IW+1 columns are written two per thread, columns lx and lx + HW2
// (HW2 = (XW+1)/2) of row ly by thread ly*HW2 + lx, so a pitch = HW2 mod 32
// makes consecutive threads hit consecutive banks (ds_write_b32: 32 banks);
// being odd it also puts the stem MFMA's paired taps on opposite bank parities
// (tools/lds_sites.py: 125 -> 19 conflict cycles per b1 wave with the rest of
// the round-5 layouts).  VSS_SWZ=0: XW + 1.
__host__ __device__ constexpr int stem_xwp(int IW) {
  if (!VSS_SWZ) return 2 * IW + 2;
  const int xw = 2 * IW + 1, hw2 = IW + 1;
  int x = xw;
  while ((x - hw2) % 32 != 0) ++x;
  return x;
}
// LDS the fused stem needs (x0 region [3][2*IH+1][stem_xwp(IW)] + stem weights), in the work region
__host__ __device__ constexpr int stem_in_lds(int IH, int IW) {
  return r4(3 * (2 * IH + 1) * stem_xwp(IW)) + 27 * 16 + 16;
}

__host__ __device__ constexpr BlockLds block_lds(int mode, int stride, int TH, int TW, int cin, int cskip, int chid,
                                                 int cout, int stem_in = 0) {
  BlockLds L{};
  L.IH = stride == 2 ? 2 * TH + 1 : TH + 2;
  L.IW = stride == 2 ? 2 * TW + 1 : TW + 2;
  L.P_in = L.IH * L.IW;
  L.P_in_pad = (L.P_in + 15) & ~15;
  L.P_out = TH * TW;
  L.CX = mode == 2 /*MODE_DEC*/ ? cin + cskip : cin;
  L.XQM = VSS_SWZ && mode == 1;
  L.XS = !VSS_SWZ ? L.CX + VSS_XS_PAD : (L.XQM ? 4 : (mode == 2 ? L.CX + (TW == 16 ? 8 : VSS_XS_PAD) : L.CX));
  L.XPL = L.XQM ? 4 * L.P_in_pad : 0;
  L.XSW = VSS_SWZ && mode == 0 ? pow2div16(L.CX / 4) : 1;

  L.RS = VSS_SWZ ? cout : cout + 4;
  L.RSW = VSS_SWZ ? pow2div16(cout / 4) : 1;
  L.XRW = VSS_SWZ ? pow2div16(cin / 4) : 1;
  L.LD2 = chid + 8;  // bf16 elements per W2 row in LDS (16-B aligned rows)
  L.SR = (TH + 1) / 2 + 3;
  L.SC = (TW + 1) / 2 + 3;
  L.NCB = cout / 16;
  L.NPB = L.P_out / 16;
  L.NCHUNK = chid / 16;
  // work split: the 16-channel chunks are dealt to CS = GC groups of waves,
  // GC in {1, 2, 4} fixed by the channel count alone (so the order in which a
  // pixel's partial sums are added never depends on the tile: results are
  // bitwise identical for every tile the planner may pick); the remaining
  // PW = 4 / GC waves of a group split the pixel blocks.  EXPAND has GC = 4.
  L.CS = L.NCHUNK >= 4 ? 4 : (L.NCHUNK >= 2 ? 2 : 1);
  L.PW = 4 / L.CS;
  L.NPBW = L.NPB / L.PW;
  L.NACC = L.NPBW * L.NCB;
  // the hidden chunk quad-major where the dw reads runs of 16 pixels (XR = 1);
  // the 2- and 4-pixel runs of XR > 1 meet its planes 4-way: they keep HSD
  L.HPL = VSS_SWZ && mode == 0 && dw_run(TW, L.NPB, 1) == 1 ? 4 * (L.P_in_pad + (stride == 2 ? 1 : 0)) : 0;
  L.slab_stride = L.P_out * L.RS;
  const int xt_floats = L.XQM ? L.P_in_pad * L.CX : r4(L.P_in_pad * L.XS);
  int o = 0;
  L.xt = o;  o += xt_floats;
  // expand blocks keep xt as MFMA operands (bf16 hi/lo pairs in the split
  // mode); the residual-capable shape keeps the exact f32 centre here
  L.xr = o;  o += (mode == 0 && stride == 1 && cin == cout) ? r4(L.P_out * cin) : 0;
  // The LDS weight image.  Direct and decoder blocks: W2 rows, dw taps and
  // biases, which several waves share.  Expand blocks keep only the project
  // bias b2 here (the epilogue reads it from every thread): each of their
  // 16-channel chunks belongs to one wave, which takes the chunk's W1 / W2
  // fragments, taps and biases straight from global memory (expand_frag below).
  L.w1 = o;
  L.w2 = o;  o += mode == 0 ? 0 : r4(cout * L.LD2 / 2);
  L.wdw = o; o += mode == 0 ? 0 : r4(9 * chid);
  L.bdw = o; o += mode == 0 ? 0 : r4(chid);
  L.b2 = o;  o += r4(cout);
  L.wimg_end = o;
  // per-wave scratch during the main loop (expand: each wave's hidden chunk
  // over the input tile), reused as the accumulator slabs after it.  The
  // decoder's main loop needs no scratch: its slabs go into the input tile
  // xt (dead once the main loop is done) when they fit, and the work region
  // is then the epilogue's stats scratch (int64 pairs, 1024 floats); the
  // decoder stages the src's norm slots in xt before the input tile is
  // committed.  (Slabs in xt: d2 50 -> 39 KB of LDS, four workgroups per CU
  // instead of three.)  Decoder tiles with an odd side also keep their
  // low-res src region (read only in the prologue) in the work region; even
  // tiles upsample from registers (dec_quads) and have none: d3's 6x16 tile
  // 44,736 -> 40,384 B (3 -> 4 workgroups per CU), d1's 4x8 55,360 -> 50,496 B
  // (2 -> 3).
  const bool slab_in_xt = mode == 2 && L.CS * L.slab_stride <= xt_floats;
  const bool dec_quads = mode == 2 && VSS_QUADS && TH % 2 == 0 && TW % 2 == 0;
  L.work = o;
  L.lr = o;
  const int hid_floats = L.HPL ? 4 * 4 * L.HPL : 4 * L.P_in_pad * hid_stride(stride);  // 4 waves
  o += cmax(cmax(cmax(mode == 0 ? hid_floats : 1024, slab_in_xt ? 0 : L.CS * L.slab_stride),
                 mode == 2 && !dec_quads ? r4(L.SR * L.SC * cin) : 0),
            stem_in ? stem_in_lds(L.IH, L.IW) : 0);
  L.nrm = o; o += mode == 2 ? r4(2 * cin) : 0;
  // decoder: per input-tile pixel, its 2x-upsample taps (four lr offsets as
  // u16 pairs, ly1, lx1), built while the prologue loads are in flight — only
  // for tiles with an odd side; even tiles upsample by 2x2 quads (dec_quads)
  L.uc = o;  o += (mode == 2 && !dec_quads) ? 4 * L.P_in_pad : 0;
  L.slab = slab_in_xt ? L.xt : L.work;
  L.stt = slab_in_xt ? L.work : L.xt;
  L.total = o;
  return L;
}

// Fragment-ordered weights of an expand block (built once by the host:
// expand_frag_image in vss_capi.hip).  One record per 16-channel hidden chunk,
// holding what the chunk's wave needs in the order it needs it; with lane
// l = 16 g + r, c0 = the chunk's first hidden channel:
//   aw  : fragment s < NK = cin / 16 : W1[c0 + r][16 s + 4 g .. + 3], 4 bf16 (8 B)
//   f4s : 11 float4 per lane group g (the 16 lanes of a group share them):
//         k = 0: b1[c0 + 4 g ..], k = 1 .. 9: wdw[tap k - 1][c0 + 4 g ..],
//         k = 10: bdw[c0 + 4 g ..]; float4 k of group g at f4s + (4 k + g) * 16
//   a2  : fragment cb < NCB = cout / 16 : W2[16 cb + r][c0 + 4 g .. + 3], 8 B
// A section of N 8-B fragments is stored as N / 2 pairs — lane l's fragments
// 2 j, 2 j + 1 side by side at j * 1024 + l * 16, one 16-B load per lane, 1 KiB
// contiguous per wave — followed, for odd N, by the last one at (N / 2) * 1024
// + l * 8.  Records are 64-B multiples, chunk ck of a slice at ck * bytes.
struct ExpandFrag {
  int NK, NCB, aw, f4s, a2, bytes;
};
constexpr int kFragF4 = 11;
__host__ __device__ constexpr ExpandFrag expand_frag(int cin, int cout) {
  ExpandFrag F{};
  F.NK = cin / 16;
  F.NCB = cout / 16;
  F.aw = 0;
  F.f4s = F.aw + 512 * F.NK;
  F.a2 = F.f4s + kFragF4 * 64;
  F.bytes = F.a2 + 512 * F.NCB;
  return F;
}
// byte offset of lane l's 8-B fragment i within a section of n fragments
__host__ __device__ constexpr int frag_off(int n, int i, int l) {
  return (n % 2 == 1 && i == n - 1) ? (n / 2) * 1024 + l * 8 : (i / 2) * 1024 + l * 16 + (i % 2) * 8;
}

// Fused block: [prologue: stage X tile (or upsample+concat)] ->
//   for each 16-channel chunk c0 of the hidden/concat dim:
//     (expand pw on MFMA) -> dw3x3 (VALU) -> project pw accumulate (MFMA)
//   -> epilogue (bias, residual, store, instance-norm partial stats)
// Opt-in phase trace (make trace -> libvss_trace.so; never in the product
// build): thread 0 of every workgroup stamps s_memrealtime (100 MHz, one
// clock for the whole device) at: 0 start, 1 prologue committed, 2 main
// done, 3 end, 4 every prologue load landed, 5 decoder src norm ready, 6
// every prologue load issued; slots 8-15 the same points in shader clocks
// (s_memtime), so the trace also gives the core clock.
// (Layer launches only: the persistent forward, COH = true, stamps nothing.)
#ifdef VSS_TRACE
#define VSS_TRACE_FIELD unsigned long long* trace;
#define VSS_STAMP(k)                                                                                  \
  do {                                                                                                \
    if constexpr (!COH) {                                                                             \
      if (threadIdx.x == 0 && p.trace) {                                                              \
        unsigned long long* t_ = p.trace + (((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 16; \
        t_[(k)] = __builtin_amdgcn_s_memrealtime();                                                   \
        t_[8 + (k)] = __builtin_amdgcn_s_memtime();                                                   \
        if ((k) == 0) {                                                                               \
          /* where the workgroup runs: HW_ID (cu, sh, se, ...) and XCC_ID */                          \
          t_[7] = __builtin_amdgcn_s_getreg((31 << 11) | 4);                                          \
          t_[15] = __builtin_amdgcn_s_getreg((15 << 11) | 20);                                        \
        }                                                                                             \
      }                                                                                               \
    }                                                                                                 \
  } while (0)
#else
#define VSS_TRACE_FIELD
#define VSS_STAMP(k) \
  do {               \
  } while (0)
#endif

// Workgroup -> tile of the layer launches and the head, computed by the host
// for the launch's grid (tile_map() / xcd_tile() at the end of this file)
struct TileMap {
  unsigned gx, gy;   // the launch's grid x, y (tiles per row, rows of tiles)
  unsigned rx, ry;   // min(floor(2^32 / gx), 2^32 - 1), the same of gy
  unsigned per;      // workgroups per XCD's eighth: (gx * gy * gz) >> 3
  unsigned full;     // per << 3: indices from here on keep their place
};

struct StemParams {
  const uint8_t* frames; // [N] frames, row_stride / frame_stride bytes
  long row_stride, frame_stride;
  int fh, fw, fc;        // frame geometry, fc = 3 or 4
  int Hm, Wm;            // model input resolution
  float ry, rx;          // (float)((double)fh/Hm), (float)((double)fw/Wm)
  const float* w;        // [cout][3][3][3]
  const float* b;
  float* y;              // [N][Ho][Wo][cout]
  int Ho, Wo, cout;
  unsigned long long* acc_zero;  // all decoder norm accumulators [N][acc_stride]: zeroed here
  int acc_stride;
  VSS_TRACE_FIELD
};

struct BlockParams {
  TileMap tm;            // workgroup -> tile of this launch's grid (tiles_x, tiles_y, N * KS)
  const float* wimg;     // the layer's LDS weight image (block_lds regions w1..b2), built by the host;
                         // with KS > 1 one image per hidden slice, wimg_stride floats apart
  long wimg_stride;
  const char* wfrag;     // expand blocks: the chunks' fragment records (expand_frag), slice after slice
  long wfrag_stride;     // bytes between the slices' records
  long x_part_stride;    // floats between the parts of x / skip / y (see block_flags)
  long skip_part_stride;
  long y_part_stride;
  const float* x;        // IR input [N][H][W][cin]   | DEC low-res src [N][h][w][cin]
  const float* skip;     // DEC skip [N][Ho][Wo][cskip]
  float* y;              // output [N][Ho][Wo][cout]
  // Instance norm, exact and order-free: every decoder workgroup adds the
  // fixed-point sums of its tile's outputs (sum v*2^32, sum v^2*2^24, int64)
  // to its frame's accumulator with device-scope atomics; the consumer (the
  // next kernel) turns the totals into scale/shift.  The stem kernel zeroes
  // the accumulators of every frame at the start of each forward.
  const unsigned long long* in_acc;  // DEC with norm_in: src accumulator [N][acc_stride] + src offset,
                                     // kAccSlots slots of [2][cin] (sum, sum of squares)
  const float* in_gamma;             // src layer's norm affine [cin]
  const float* in_beta;
  int in_hw;                         // pixels per frame of the src
  double in_inv_hw;                  // 1 / in_hw
  unsigned long long* out_acc;       // DEC: this layer's accumulator [N][acc_stride] + offset
                                     // (kAccSlots slots of [2][cout]; workgroup -> slot tile % kAccSlots)
  int acc_stride;                    // int64 elements per frame over all decoder layers
  float eps;
  int N, H, W;           // input spatial (IR: x dims; DEC: skip/output dims)
  int Ho, Wo;            // output spatial
  int cin, cskip, chid, cout;   // chid = hidden (IR expand) or channels fed to dw
  int stride;
  int relu6_dw;          // IR: relu6 after dw; DEC: none
  int residual;
  int TH, TW;            // output tile
  int tiles_x, tiles_y;
  int norm_in;           // DEC: src needs norm+relu
  StemParams stem;       // STEM_IN: the fused stem (frames of this call, stem weights, its output y)
  VSS_TRACE_FIELD
};

using BlockFn = void (*)(BlockParams);

// One compiled k_block shape (tools/gen_registry.py -> vss_registry.inc).
// flags: block_flags().
struct BlockEntry {
  int mode, stride, TH, TW, cin, cskip, chid, cout, flags;
  BlockFn fn[2];  // [PREC_F32, PREC_BF16X2]
  int threads = kThreads;  // workgroup size
  int variant = 0;         // BlockVariant: k_block or k_stem_b1 (wide)
};

// b1 with the stem fused on a wide workgroup (k_stem_b1, 16 waves): LDS
// carve in floats — the resized region x0 [3][2*IH+1][2*IW+2], the stem
// weights [27][16] + bias, the stem output tile xt [P_IN_PAD][16 + pad] and the
// block's weight image (block_lds regions w1..b2 of the same shape).
constexpr int kWideThreads = 1024;
struct StemB1Lds {
  int IH, IW, P_IN, P_IN_PAD, XS, XH, XW, XWP, x0, sw, sb, xt, wim, total;
};
__host__ __device__ constexpr StemB1Lds stem_b1_lds(int TH, int TW) {
  StemB1Lds L{};
  L.IH = TH + 2;
  L.IW = TW + 2;
  L.P_IN = L.IH * L.IW;
  L.P_IN_PAD = (L.P_IN + 15) & ~15;
  L.XS = 16 + VSS_XS_PAD;
  L.XH = 2 * L.IH + 1;
  L.XW = 2 * L.IW + 1;
  L.XWP = L.XW + 1;
  int o = 0;
  L.x0 = o;  o += r4(3 * L.XH * L.XWP);
  L.sw = o;  o += 27 * 16;
  L.sb = o;  o += 16;
  L.xt = o;  o += r4(L.P_IN_PAD * L.XS);
  const BlockLds B = block_lds(1 /*MODE_IR_DIRECT*/, 1, TH, TW, 16, 0, 16, 16, 1);
  L.wim = o; o += B.wimg_end - B.w1;
  L.total = o;
  return L;
}
// BlockEntry::variant
enum BlockVariant : int { VAR_BLOCK = 0, VAR_STEM_B1_WIDE = 1 };

const BlockEntry* block_registry(int* count);


struct HeadParams {
  TileMap tm;            // workgroup -> tile of the launch's grid
  const float* x;        // pre-norm dec output [N][h][w][cin]
  const unsigned long long* in_acc;  // its norm accumulator (see BlockParams), frame stride acc_stride
  int acc_stride;
  const float* gamma;    // its norm affine [cin]
  const float* beta;
  float eps;
  double inv_hw;         // 1 / (h * w_)
  const float* w;        // [cin]
  float b;
  float* mask;           // [N][Hm][Wm] f32
  int N, h, w_, cin;
  int Hm, Wm;
  VSS_TRACE_FIELD
};

// Fixed LDS of the stem and head bodies (floats; dynamic shared memory, so the
// persistent forward can run them from its own carve).
constexpr int kStemTH = 8, kStemTW = 32, kStemIH = 2 * kStemTH + 1, kStemIWP = 2 * kStemTW + 2;
constexpr int kStemLds = r4(3 * kStemIH * kStemIWP) + 27 * 16 + 16;
constexpr int kHeadTH = 16, kHeadTW = 64, kHeadZR = 10, kHeadZC = 34, kHeadZCP = 35;
constexpr int kHeadLds = kAccSlots * 2 * 16 * 2 + r4(kHeadZR * kHeadZCP) + 3 * 16;

// Instance-norm scale/shift of one channel from the exact fixed-point totals.
// inv_hw = 1 / (pixels per frame), computed by the host: the mean and E[x^2]
// take one f64 multiply each instead of an f64 division, and 1/sqrt(var + eps)
// is v_rsq_f64 refined by two Newton steps (~2^-50 relative; rounded to f32
// after) instead of an f64 sqrt and division — the norm's setup runs on the
// prologue's critical path of every decoder workgroup and the head.
__host__ __device__ inline void norm_affine(unsigned long long s_fx, unsigned long long q_fx, double inv_hw,
                                            float eps, float gamma, float beta, float* scale, float* shift) {
  const double mean = (double)(long long)s_fx * (0x1p-32 * inv_hw);
  const double ex2 = (double)(long long)q_fx * (0x1p-24 * inv_hw);
  const double var = ex2 - mean * mean > 0.0 ? ex2 - mean * mean : 0.0;
  const double x = var + (double)eps;
#ifdef __HIP_DEVICE_COMPILE__
  double r = __builtin_amdgcn_rsq(x);
  r = r * __builtin_fma(-0.5 * x * r, r, 1.5);
  r = r * __builtin_fma(-0.5 * x * r, r, 1.5);
#else
  const double r = 1.0 / __builtin_sqrt(x);
#endif
  const float rstd = (float)r;
  const float sc = rstd * gamma;
  *scale = sc;
  *shift = beta - (float)mean * sc;
}

struct PrepParams {      // standalone preprocess: frames -> [N][3][Hm][Wm] f32
  const uint8_t* frames;
  long row_stride, frame_stride;
  int fh, fw, fc;
  int Hm, Wm;
  float ry, rx;
  float* out;
  int N;
};

// Post-processing chain (vss_post.hip)
struct PostEmaParams {
  const float* masks;  // [n][P] raw seam masks
  float* ema;          // [n][P] EMA outputs
  float* state;        // [P] prevAlpha
  const int* valid;    // 0 before the stream's first frame
  int n;
  long P;
  double a;            // config.EMA
};

// Per-frame face inputs of the post chain (the same layout as vss_face_frame, include/vss.h)
struct FaceFrame {
  int has_affine;
  double affine[6];
  int has_box;
  double box[4];
  int video_w, video_h;
};

// One frame of the stabilised EMA: base = mask (+ 0.3 * warp(prevAlpha) when the
// frame has an affine), then the EMA; prevAlpha double-buffered (the warp reads
// other pixels' prevAlpha).
struct PostFaceEmaParams {
  const float* mask;     // [P] this frame's raw mask
  const float* prev;     // [P] prevAlpha
  float* next;           // [P] the new prevAlpha (= this frame's EMA)
  float* ema;            // [P] this frame's EMA output
  const int* valid;      // 0 before the stream's first frame
  int first;             // this is the call's first frame
  const FaceFrame* face; // this frame's face inputs (device)
  int H, W;
  double a;
};
void launch_post_face_ema(const PostFaceEmaParams& p, hipStream_t s);

struct PostFilterParams {
  const FaceFrame* faces;  // [n] per-frame face inputs (device) or null: no prior
  const float* ema;      // [n][H][W]
  const uint8_t* frames; // the n source frames (guide)
  long row_stride, frame_stride;
  int fh, fw, fc;
  float ry, rx;
  int H, W;
  const double* rtab;    // exp(-r / (2 sigma_r^2)), r = 0 .. 3*255^2
  double sw[3];          // exp(-s / (2 sigma_s^2)), s = 0, 1, 2
  double lo, hi, denom, gamma;
  int use_bilateral;
  float* alpha;          // [n][H][W] refined (may be null)
  uint8_t* alpha_u8;     // [n][H][W] (may be null)
};

// The post chain over many streams (k_post_pool): frame t of the launch is the
// next frame of one stream; its EMA is computed in the filter's tile load from
// the raw mask and the stream's prevAlpha plane, and stored to the stream's
// other plane.  The per-frame table travels by value: no device flag, no host
// wait, nothing read from the caller's memory after the launch.
constexpr int kPoolFrames = 64;  // frames per launch
struct PostPoolParams {
  PostFilterParams f;    // ema unused; faces, frames, alpha, alpha_u8 point at the launch's first frame
  const float* masks;    // [n][H][W] raw seam masks
  float* planes;         // [capacity][2][H][W] prevAlpha, double-buffered per stream
  double a;              // config.EMA
  unsigned entry[kPoolFrames];  // per frame: stream id << 2 | current plane << 1 | the stream has seen a frame
};
void launch_post_pool(const PostPoolParams& p, int n, hipStream_t s);

// Source taps of output index o of the half-pixel bilinear (scale = in / out):
// shared by the compositing alpha, the frame-resolution masks and the
// background image's scaling (vss_post.hip, vss_background.hip).
__device__ __forceinline__ void up_coord(int o, float scale, int in, int& i0, int& i1, float& l) {
#pragma clang fp contract(off)
  float s = ((float)o + 0.5f) * scale - 0.5f;
  s = fmaxf(s, 0.f);
  const int a = min((int)s, in - 1);
  i0 = a;
  i1 = a < in - 1 ? a + 1 : a;
  l = s - (float)a;
}

// §8(f) row 3: destination-in compositing of the frame by the upscaled mask alpha
struct CompositeParams {
  const uint8_t* frames;  // [n] frames, row_stride / frame_stride bytes, fc = 3 or 4
  long row_stride, frame_stride;
  int fh, fw, fc;
  const uint8_t* alpha;   // [n][H][W] u8 (the post chain's alpha bytes)
  int H, W;
  float sy, sx;           // (float)H / fh, (float)W / fw
  uint8_t* out;           // [n] RGBA frames, out_row_stride / out_frame_stride bytes
  long out_row_stride, out_frame_stride;
};
void launch_composite(const CompositeParams& p, int n, hipStream_t s);

// VSS_OUT_FRAME: the f32 model-res masks upsampled to frame resolution with
// the same half-pixel bilinear as the compositing alpha (k_composite).
struct UpmaskParams {
  const float* masks;  // [n][H][W]
  int H, W;
  float sy, sx;        // (float)H / fh, (float)W / fw
  float* out;          // [n][fh][fw]
  int fh, fw;
};
void launch_upmask(const UpmaskParams& p, int n, hipStream_t s);

// Virtual backgrounds (vss_background.hip): the frame over a background by the
// upscaled mask alpha, out = (fg*A + bg*(255-A) + 127) / 255 per channel, alpha
// byte 255.  mode = VSS_BG_COLOR / _IMAGE / _BLUR (include/vss.h).
constexpr int kBgColor = 0, kBgImage = 1, kBgBlur = 2;
constexpr int kBlurMaxRadius = 32;
// the cached scaled image: RGB, 3 B per pixel, rows padded so that every
// thread's 4 pixels are 3 whole dwords
__host__ __device__ constexpr long bg_image_stride(int fw) { return (long)((fw + 3) / 4) * 12; }
// One pixel's alpha at frame resolution.  REFINE = false: k_composite's, the
// half-pixel bilinear of the mask's alpha bytes (rows ra / rb of the u8 plane).
// REFINE = true (the edge-aware matte, include/vss.h): the same bilinear of the
// two coefficient planes (rows ma / mb of the interleaved (abar, bbar) plane),
// applied to the pixel's luma, A = floor(clamp(abar * Y + bbar, 0, 255) + 0.5),
// the product rounded before the sum.  rgb = the pixel's frame bytes.
__device__ __forceinline__ uint32_t matte_luma(const uint8_t* rgb) {
  return (77u * rgb[0] + 150u * rgb[1] + 29u * rgb[2] + 128u) >> 8;
}
template <bool REFINE>
__device__ __forceinline__ uint32_t pixel_alpha(const uint8_t* ra, const uint8_t* rb, const float2* ma,
                                                const float2* mb, int xa, int xb, int col0, float lx, float ly,
                                                const uint8_t* rgb) {
#pragma clang fp contract(off)
  if constexpr (REFINE) {
    const float2 v00 = ma[xa - col0], v01 = ma[xb - col0], v10 = mb[xa - col0], v11 = mb[xb - col0];
    const float ta = __builtin_fmaf(v01.x - v00.x, lx, v00.x), ba = __builtin_fmaf(v11.x - v10.x, lx, v10.x);
    const float tb = __builtin_fmaf(v01.y - v00.y, lx, v00.y), bb = __builtin_fmaf(v11.y - v10.y, lx, v10.y);
    const float au = __builtin_fmaf(ba - ta, ly, ta), bu = __builtin_fmaf(bb - tb, ly, tb);
    const float prod = au * (float)matte_luma(rgb);
    const float q = prod + bu;
    return (uint32_t)floorf(fminf(fmaxf(q, 0.f), 255.f) + 0.5f);
  } else {
    const float a00 = ra[xa], a01 = ra[xb], a10 = rb[xa], a11 = rb[xb];
    const float top = __builtin_fmaf(a01 - a00, lx, a00), bot = __builtin_fmaf(a11 - a10, lx, a10);
    return (uint32_t)floorf(__builtin_fmaf(bot - top, ly, top) + 0.5f);
  }
}

// Where a kernel reads one frame's (abar, bbar) taps: element (row, col) of the
// mask plane is p[(row - row0) * pitch + col - col0].  The plane itself in HBM
// (row0 = col0 = 0, pitch = W), or a workgroup's window of it staged in LDS.
struct MatteTaps {
  const float2* p;
  int pitch, row0, col0;
};
// A workgroup of k_composite's shape (frame rows Y0 .. Y0 + 3, pixels X0 .. X0 +
// 255) reads mask rows ya(Y0) .. yb(Y0 + 3) and columns xa(X0) .. xb(X0 + 255):
// with a frame no smaller than the mask, at most 5 rows and 257 columns.  They
// are staged in LDS once, so that the four 8-B taps of every pixel are LDS
// reads (most lanes of a wave share them) instead of global gathers.  Every
// thread of the workgroup calls it (one barrier).
constexpr int kMatteTapRows = 6, kMatteTapCols = 260;
__device__ __forceinline__ MatteTaps stage_matte_taps(const CompositeParams& c, const float2* plane, int Y0, int X0,
                                                      float2* tile) {
  int r0, r1, c0, c1, unused;
  float l;
  up_coord(Y0, c.sy, c.H, r0, unused, l);
  up_coord(min(Y0 + 3, c.fh - 1), c.sy, c.H, unused, r1, l);
  up_coord(X0, c.sx, c.W, c0, unused, l);
  up_coord(min(X0 + 255, c.fw - 1), c.sx, c.W, unused, c1, l);
  // fh >= H and fw >= W (the host's check): the clamps never bind; they keep the loop inside the tile
  const int R = min(r1 - r0 + 1, kMatteTapRows), C = min(c1 - c0 + 1, kMatteTapCols);
  for (int k = threadIdx.x; k < R * C; k += 256) {
    const int r = k / C, col = k - r * C;
    tile[r * kMatteTapCols + col] = plane[(long)(r0 + r) * c.W + c0 + col];
  }
  __syncthreads();
  return {tile, kMatteTapCols, r0, c0};
}

struct BgCompositeParams {
  CompositeParams c;       // frames, alpha, output: as k_composite
  const float2* ab;        // refinement on: [n][H][W] (abar, bbar), k_matte_mean's output; else null
  uint32_t color;          // COLOR: r | g << 8 | b << 16
  const uint8_t* image;    // IMAGE: [fh][bg_image_stride(fw)] RGB at frame size
  const uint32_t* hblur;   // BLUR: [n][fh][fw] RGBX, the horizontal pass
  int radius;              // BLUR
  uint16_t w[kBlurMaxRadius + 1];  // BLUR: taps 0 (centre) .. radius, 16-bit fixed point
  const uint32_t* overlay; // BLUR with visible layers: the plate O [fh][layer_pitch(fw)] premultiplied RGBA; else null
};
void launch_bg_composite(const BgCompositeParams& p, int mode, int n, hipStream_t s);

// Backgrounds over many streams (include/vss_streams.h): frame t
// of a launch is composited over its own background.  The per-frame table
// travels by value and is indexed by a blockIdx expression, so its loads are
// scalar and nothing of the caller's arrays is read after the launch.  The flat
// form (colour, scaled image, baked plate) runs over the frames of `flat`, the
// blur form and the pooled k_blur_h over those of `blur`: blockIdx.z -> frame.
constexpr int kBgStreamFrames = 32;  // frames per launch
struct BgStreamEntry {
  const uint8_t* image;    // flat form: the scaled image or baked plate; null = the colour
  uint32_t* hblur;         // blur form: this frame's [fh][fw] slot of its object's horizontal pass
  const uint32_t* overlay; // blur form with visible layers: the object's plate O; else null
  const float2* ab;        // refinement on: this frame's [H][W] (abar, bbar) slot; else null
  const uint16_t* taps;    // blur form: the object's device taps 0 (centre) .. radius
  uint32_t color;
  int radius;              // blur form
};
struct BgStreamsParams {
  CompositeParams c;       // frames, alpha and output point at the launch's first frame
  BgStreamEntry entry[kBgStreamFrames];
  unsigned flat[kBgStreamFrames / 4], blur[kBgStreamFrames / 4];  // frame indices, one byte each
};
__host__ __device__ __forceinline__ int stream_list_at(const unsigned* list, int z) {
  return (int)((list[z >> 2] >> (8 * (z & 3))) & 255u);
}
inline void stream_list_set(unsigned* list, int z, int t) { list[z >> 2] |= (unsigned)t << (8 * (z & 3)); }
// nflat / nblur frames in the lists (either may be 0: that form is not launched); max_radius over the blur frames
void launch_bg_streams(const BgStreamsParams& p, int nflat, int nblur, int max_radius, hipStream_t s);

struct BlurHParams {
  const uint8_t* frames;   // [n] frames, row_stride / frame_stride bytes, fc = 3 or 4
  long row_stride, frame_stride;
  int fh, fw, fc;
  uint32_t* out;           // [n][fh][fw] RGBX
  int radius;
  uint16_t w[kBlurMaxRadius + 1];
};
void launch_blur_h(const BlurHParams& p, int n, hipStream_t s);

struct BgResizeParams {
  const uint8_t* src;      // [sh][sw][sc] u8, tight rows, sc = 3 or 4 (alpha dropped)
  int sh, sw, sc;
  float sy, sx;            // (float)sh / fh, (float)sw / fw
  uint8_t* out;            // [fh][bg_image_stride(fw)] RGB
  int fh, fw;
};
void launch_bg_resize(const BgResizeParams& p, hipStream_t s);

// Branding layers (vss_layers.hip; the definition: include/vss_layers.h).  The
// overlay plate O is premultiplied RGBA, one dword per pixel (r | g << 8 |
// b << 16 | a << 24), rows padded to whole quads so that k_bg_composite's
// threads load their 4 pixels as one 16-B word.
constexpr int kLayerImage = 0, kLayerRect = 1;
__host__ __device__ constexpr int layer_pitch(int fw) { return (fw + 3) / 4 * 4; }
// bg' = min(255, O.c + (bg.c*(255 - O.a) + 127) / 255) on a packed r | g << 8 | b << 16
__device__ __forceinline__ uint32_t under_overlay(uint32_t bg, uint32_t o) {
  const uint32_t ia = 255u - (o >> 24);
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t v = ((o >> (8 * c)) & 255u) + ((((bg >> (8 * c)) & 255u) * ia + 127u) / 255u);
    out |= min(v, 255u) << (8 * c);
  }
  return out;
}

// One layer at one frame size: its unclipped destination rectangle in frame
// pixels (64-bit: x, y and the sizes are free on the canvas).
struct LayerGeom {
  int type;                // kLayerImage / kLayerRect
  long X0, Y0, X1, Y1;
  long R;                  // ROUNDED_RECT: the clamped corner radius, frame pixels
  uint32_t color;          // ROUNDED_RECT: r | g << 8 | b << 16 | a << 24, not premultiplied
  const uint8_t* sprite;   // IMAGE: [sh][sw][4] premultiplied RGBA, tight rows
  int sh, sw;
  float sy, sx;            // (float)sh / (Y1 - Y0), (float)sw / (X1 - X0)
};
// the layer's sample source-over into O, over the clipped rectangle [x0, x1) x [y0, y1)
struct LayerDrawParams {
  LayerGeom g;
  int x0, y0, x1, y1;
  uint32_t* plate;         // [fh][pitch]
  int pitch;
};
void launch_layer_draw(const LayerDrawParams& p, hipStream_t s);
// The drop shadow over the region [x0, x1) x [y0, y1): the shifted rectangle
// grown by the radius and clipped to the frame.  P and Hb are u8 planes
// [fh][pitch], written and read inside the region only (0 outside it).
struct ShadowParams {
  LayerGeom g;
  long dx, dy;             // the shift, frame pixels
  int x0, y0, x1, y1;
  uint8_t* P;              // the shifted alpha
  uint8_t* Hb;             // its horizontal pass
  int pitch;
  int radius;              // 0: B = P, no passes
  uint16_t w[kBlurMaxRadius + 1];
  uint32_t color;          // r | g << 8 | b << 16 | a << 24, not premultiplied
  uint32_t* plate;         // [fh][pitch]
};
void launch_layer_shadow(const ShadowParams& p, hipStream_t s);
// colour and image modes: bg' baked into the RGB plate k_bg_composite<IMAGE> reads
struct BgBakeParams {
  uint8_t* image;          // [fh][bg_image_stride(fw)] RGB, in place (from_color: written only)
  const uint32_t* overlay; // [fh][layer_pitch(fw)]
  int fh, fw;
  int from_color;          // bg = color everywhere instead of the image's pixels
  uint32_t color;
};
void launch_bg_bake(const BgBakeParams& p, hipStream_t s);

// Edge-aware matte (vss_matte.hip; the definition: include/vss.h): a guided
// filter of the alpha bytes by the frame's luma.  The mask-resolution stage —
// k_matte_guide (L = the area mean of the luma per mask pixel), k_matte_coeff
// (the window sums and the f64 fit, quantised) and k_matte_mean (their box
// mean) — leaves the (abar, bbar) plane that k_bg_composite<.., REFINE> and
// k_matte_alpha apply at frame resolution.
constexpr int kMatteMaxRadius = 8;
struct MatteParams {
  const uint8_t* frames;   // [n] frames, row_stride / frame_stride bytes, fc = 3 or 4
  long row_stride, frame_stride;
  int fh, fw, fc;          // fh >= H, fw >= W
  const uint8_t* alpha;    // [n][H][W] u8 (the post chain's alpha bytes)
  int H, W;
  int radius;              // 1 .. kMatteMaxRadius, mask pixels
  double eps;              // [1, 65025]
  uint8_t* L;              // [n][H][W] scratch: the low-resolution guide
  int2* q;                 // [n][H][W] scratch: (a_q, b_q)
  float2* ab;              // [n][H][W] out: (abar, bbar)
};
void launch_matte_stage(const MatteParams& p, int n, hipStream_t s);

// The mask-resolution stage over many streams: frame list[z] of the launch with
// its own radius, eps and plane slot (the three kernels, one launch each).
struct MatteStreamEntry {
  float2* ab;
  int2* q;
  uint8_t* L;
  double eps;
  int radius;
};
struct MatteStreamsParams {
  MatteParams m;           // frames, alpha and geometry (first frame of the launch); radius, eps and planes unused
  MatteStreamEntry entry[kBgStreamFrames];
  unsigned list[kBgStreamFrames / 4];
};
void launch_matte_streams(const MatteStreamsParams& p, int n, hipStream_t s);

// The frame-resolution alpha plane alone: ab != null the refined alpha, else k_composite's.
struct MatteAlphaParams {
  CompositeParams c;       // frames, alpha, geometry; out = [n] u8 planes, out_row_stride / out_frame_stride bytes
  const float2* ab;
};
void launch_matte_alpha(const MatteAlphaParams& p, int n, hipStream_t s);

// NV12 video I/O (vss_video.hip; the definition: include/vss_video.h).  One
// row of the table there: the four standards are values of this struct, a
// kernel argument, not template instances.
struct CscCoef {
  int y0, cy, rv, gu, gv, bu;   // unpack
  int yr, yg, yb, ur, ug, ub, vr, vg, vb;   // pack
};
struct Nv12Params {      // both directions: unpack reads y / uv and writes rgba, pack the reverse
  uint8_t* y;            // [n] Y planes [fh][y_pitch]
  uint8_t* uv;           // [n] UV planes [fh/2][uv_pitch]
  long y_pitch, y_frame_stride, uv_pitch, uv_frame_stride;
  uint8_t* rgba;         // [n] RGBA frames, 4-byte aligned rows
  long row_stride, frame_stride;
  int fh, fw;            // even, >= 2
  CscCoef k;
};
void launch_nv12_unpack(const Nv12Params& p, int n, hipStream_t s);
void launch_nv12_pack(const Nv12Params& p, int n, hipStream_t s);

// Queued host path: only the frame rows the resize reads, pinned host -> HBM
// (vss_stage.hip).  rows: device list of the row indices; src / dst = frame 0.
struct FetchRowsParams {
  const uint8_t* src;    // pinned host staging (device-accessible)
  uint8_t* dst;          // the slot's HBM frame buffer (same layout)
  const int* rows;       // [nrows] rows to move
  long row_stride, frame_stride;
  int row_bytes;         // width * channels
  int vec16;             // 1: every row start and row_bytes are multiples of 16 B
};
void launch_fetch_rows(const FetchRowsParams& p, int nrows, int nframes, hipStream_t s);

void launch_post_ema(const PostEmaParams& p, hipStream_t s);
void launch_post_filter(const PostFilterParams& p, int n, hipStream_t s);

// XCD-aware tile order of the layer launches and the head.  Workgroups are
// dealt round-robin over the 8 XCDs (block b shares an XCD, and its L2, with
// b + 8; MI355X_MICROARCH.md, workgroup dispatch), so with the grid's natural
// order horizontally adjacent tiles — which read the same halo columns of the
// input and, in the decoders, the same low-res src columns — sit on different
// XCDs and each XCD fetches the shared lines again.  Remap: the workgroups of
// one XCD (b % 8) take one contiguous eighth of the logical (x, y, z) tile
// order, i.e. whole rows of tiles of one frame (with 8 frames, one frame per
// XCD), so neighbours share an L2.  A bijection on the grid (any remainder
// past the last full eighth keeps its own index); results do not depend on
// which workgroup computes which tile (tile-invariant, order-free norm sums).
// Measured: the post filter and the frame-resolution kernels gain nothing
// from it (profiles/NOTES.md), so they keep the natural order.
#ifndef VSS_XCD_REMAP
#define VSS_XCD_REMAP 1
#endif
// The remap runs at the head of every workgroup, before its first load, and
// its two divisions by the grid's sizes cost ~25 instructions each as run-time
// integer divisions (v_rcp_iflag_f32 sequences).  The host knows the grid: it
// passes the sizes, their reciprocals and `per` in the kernel's parameter block
// (TileMap, tile_map() below), and a division becomes a multiply-high plus one
// correction step.  With m = min(floor(2^32 / d), 2^32 - 1) the estimate
// q' = (T * m) >> 32 is q or q - 1 for EVERY 32-bit T and every d >= 1
// (T / d - T * m / 2^32 < T / 2^32 < 1; d = 1: q' = T - 1), so one compare of
// the remainder makes it exact: no bound on the grid's size.
struct TileIdx {
  int x, y, z;
};
__host__ __device__ inline unsigned tile_recip(unsigned d) {
  const unsigned long long m = 0x100000000ull / d;
  return m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)m;
}
__host__ __device__ inline TileMap tile_map(unsigned gx, unsigned gy, unsigned gz) {
  const unsigned per = (gx * gy * gz) >> 3;
  return {gx, gy, tile_recip(gx), tile_recip(gy), per, per << 3};
}
// T / d and T % d from d's reciprocal m = tile_recip(d)
__host__ __device__ __forceinline__ void tile_divmod(unsigned T, unsigned d, unsigned m, unsigned& q, unsigned& r) {
  q = (unsigned)(((unsigned long long)T * m) >> 32);
  r = T - q * d;
  if (r >= d) {
    ++q;
    r -= d;
  }
}
// the tile (x, y, z) of workgroup (bx, by, bz)
__host__ __device__ __forceinline__ TileIdx tile_of(const TileMap& m, unsigned bx, unsigned by, unsigned bz) {
  if constexpr (VSS_XCD_REMAP) {
    const unsigned L = bx + m.gx * (by + m.gy * bz);
    const unsigned T = L < m.full ? (L & 7) * m.per + (L >> 3) : L;
    unsigned zy, x, z, y;
    tile_divmod(T, m.gx, m.rx, zy, x);
    tile_divmod(zy, m.gy, m.ry, z, y);
    return {(int)x, (int)y, (int)z};
  } else {
    return {(int)bx, (int)by, (int)bz};
  }
}
__device__ __forceinline__ TileIdx xcd_tile(const TileMap& m) { return tile_of(m, blockIdx.x, blockIdx.y, blockIdx.z); }

}  // namespace vss
