// What the DPT convolution kernels share (conv.hip: conv_f32_kernel, conv_bf16x3_kernel, conv_pre_kernel;
// conv_up.hip: conv_up_kernel): the pieces of a 128-pixel x BN-column x 32-deep split-bf16 tile, one
// definition each, and the host-side resolver's interface.  The K-loop schedules (order of loads, waits
// and barriers) stay in the kernels.
#pragma once
#include "common.h"

constexpr int TILE_M = 128, TILE_K = 32;  // pixels per tile, K per step (one tap's 32-channel slice)

// ---- LDS layout and DMA
// 64-B rows (32 bf16), swizzle chunk ^ h((row >> 2) & 3), h = {0, 3, 2, 1}: conflict-free ds_read_b128
// fragment reads for any 16 consecutive rows (as the GEMM ring)
__device__ __forceinline__ int swz64(int row, int chunk) { return chunk ^ ((4 - ((row >> 2) & 3)) & 3); }

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Raw buffer resource over `num_records` bytes at p (wave-uniform).  Offsets at or past num_records read
// as zeros: the gathers rely on it for out-of-image taps.  The weight descriptors are unbounded
// (0xffffffff): rows up to the N tile's edge must exist (vggt_conv_form's w_rows).
__device__ __forceinline__ i32x4 make_rsrc(const void* p, uint32_t num_records) {
  i32x4 r;
  const uint64_t b = (uint64_t)p;
  r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
  r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) & 0xffff;
  r[2] = (int)num_records;
  r[3] = 0x00020000;
  return r;
}

// 16 B per lane from (rsrc, voff + soff) into LDS at the wave-uniform address `lds` (+ lane * 16):
// buffer_load ... lds (LDS-DMA).  In asm so the compiler does not drain vmcnt around it; completion
// is waited for explicitly before the barrier that publishes the stage.
__device__ __forceinline__ void dma16(i32x4 rsrc, uint32_t voff, uint32_t soff, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds)
               : "memory");
}

// ---- tile origin and pixel rows of the implicit GEMM (M = output pixels, N = GEMM columns, K = taps x ci)
struct ConvTile {
  int M, m0, n0, K, nk, ntap, ci;
  // K-step order of the split-bf16 forms: channel slice outer, tap inner.  Step s covers tap s % ntap and
  // channels (s / ntap)*32 .. +32, i.e. weight columns tap*ci + slice*32 (the (ky, kx, ci) weight layout is
  // unchanged).  The ntap steps of one slice gather overlapping input windows (3x3 shifts of the same pixels
  // and channels), so the gather hits L2 instead of re-streaming the activation from HBM once per tap.
  __device__ __forceinline__ int kcol(int s) const { return (s % ntap) * ci + (s / ntap) * TILE_K; }
};
template <int BNX>
__device__ __forceinline__ ConvTile conv_tile(int nimg, int ho, int wo, int ncols, int kh, int kw, int ci) {
  ConvTile t;
  t.M = nimg * ho * wo;
  const int tiles_n = (ncols + BNX - 1) / BNX;
  const int tiles_m = (t.M + TILE_M - 1) / TILE_M;
  const int b = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  t.m0 = (b / tiles_n) * TILE_M;
  t.n0 = (b % tiles_n) * BNX;
  t.K = kh * kw * ci;
  t.nk = t.K / TILE_K;
  t.ntap = kh * kw;
  t.ci = ci;
  return t;
}

// Output pixel m -> its image and the input coordinate of tap (0, 0); rows past M decompose pixel 0 (ok = false)
struct PixRow { int img, y, x; bool ok; };
__device__ __forceinline__ PixRow pix_row(int m, int M, int ho, int wo, int stride, int pad) {
  const bool ok = m < M;
  const int mm = ok ? m : 0, rem = mm % (ho * wo);
  return PixRow{mm / (ho * wo), (rem / wo) * stride - pad, (rem % wo) * stride - pad, ok};
}

// ---- fragments and the product: waves 2 (M) x 2 (N); lane r16 = row within a 16-row fragment, q = its
// 16-B chunk of the 32 channels, roff = r16 * 64 + (swz64(r16, q) << 4)
template <int NTN>
__device__ __forceinline__ void acc_zero(f32x4 (&acc)[4][NTN]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NTN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// B fragments of wave column wn out of one weight tile's hi / lo halves
template <int NTN>
__device__ __forceinline__ void b_frags(const char* whi, const char* wlo, int wn, int roff, bf16x8 (&bh)[NTN],
                                        bf16x8 (&bl)[NTN]) {
#pragma unroll
  for (int nt = 0; nt < NTN; ++nt) {
    const int o = (wn * NTN * 16 + nt * 16) * 64 + roff;
    bh[nt] = *(const bf16x8*)(whi + o);
    bl[nt] = *(const bf16x8*)(wlo + o);
  }
}

// acc += a . b of split operands as three bf16 MFMAs per fragment pair, in the order lo.hi, hi.lo, hi.hi
// (smallest terms first; lo.lo is dropped).  Every split-bf16 kernel takes the product from here, which
// is what makes the forms bitwise equal to each other.
template <int NTN>
__device__ __forceinline__ void mfma3(f32x4 (&acc)[4][NTN], const bf16x8 (&ah)[4], const bf16x8 (&al)[4],
                                      const bf16x8 (&bh)[NTN], const bf16x8 (&bl)[NTN]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) {
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
      acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
    }
}

// One output element: y (f32, may be null), then the optional split of relu?(v) into yh / yl.
// A: ConvArgs or UpConvArgs (y, ldy, yh, yl, ldys, split_relu)
template <class A>
__device__ __forceinline__ void store_out(const A& a, int64_t opix, int co, float v) {
  if (a.y) a.y[opix * a.ldy + co] = v;
  if (a.yh) {
    const float sv = a.split_relu ? fmaxf(v, 0.f) : v;
    const float hv = round_bf(sv);
    a.yh[opix * a.ldys + co] = f2bf(hv);
    a.yl[opix * a.ldys + co] = f2bf(sv - hv);
  }
}

// ---- host side: the one resolver of the four convolution entry points (defined in conv.hip)
struct ConvIn {
  int entry;                                                // VGGT_CONV_ENTRY_*
  int nimg, hi, wi, ci, co, kh, kw, stride, pad, shuffle;  // fused upsample: hi x wi the source map, 3x3 / 1 / 1 / 0
  int ho, wo;                                               // fused upsample only: the resize target
  int64_t ldx, ldy, ldys;
  int has;           // VGGT_CONV_HAS_*: which of y / y_hi / y_lo / res1 / res2 / pos are given
  bool x_unaligned;  // x (f32: or w; pre: x_hi; fused upsample: or pos_sep) is not 16-byte aligned
  bool w_unaligned;  // w_hi or w_lo (pre: or x_lo) is not 16-byte aligned
  int pf2;           // VGGT_TUNE_CONV_PF2 at the time of the call
};
// conv_up_kernel: output tile rows x columns of pixels, N tile, LDS bytes (asserted there)
constexpr int CONV_UP_R = 4, CONV_UP_C = 32, CONV_UP_BN = 32, CONV_UP_LDS = 62976;
vggt_conv_form_t conv_resolve(const ConvIn& in);
