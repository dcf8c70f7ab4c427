// DPT head convolutions and their element-wise kernels (include/vggt_mi355x.h):
//   vggt_conv2d_f32, vggt_conv2d_bf16x3, vggt_conv2d_bf16x3_pre   the implicit GEMM in three forms
//   vggt_conv_form                             which kernel the four convolution entries launch (host only)
//   vggt_split_act_bf16x2, vggt_split_bf16x2   the hi / lo split of activations / weights
//   vggt_upsample_bilinear_f32, vggt_upsample_bilinear_split, vggt_upsample_bilinear_split_sep
//   vggt_dpt_activate
// (vggt_conv2d_upsample_bf16x3 and its kernel are in conv_up.hip; it resolves through conv_resolve here.)
//
// The reference runs the DPT heads with autocast disabled
// (featureAligned_vggt.py:104), i.e. in fp32.  Two forms of one implicit GEMM
// over NHWC activations: exact-f32 MFMA (v_mfma_f32_16x16x4_f32,
// conv_f32_kernel) and split-bf16 (conv_bf16x3_kernel, below: fp32 operands
// as bf16 hi + lo pairs on the bf16 matrix path, ~2^-16 per product).
//   out[pixel, co] = sum_{ky,kx,ci} act(x[pixel@(ky,kx), ci]) * W[co, ky, kx, ci]
// K is ordered (ky, kx, ci) with Ci % 32 == 0, so every 32-wide K slice is one
// tap and a contiguous channel run (16-B loads, zero for padding taps).
// Block tile 128 pixels x 64 channels x 32 K, 4 waves (2x2), register-staged
// double buffer through XOR-swizzled LDS.  Fused epilogue: bias, ReLU,
// up to two residual adds (one optionally ReLU'd: the in-place-ReLU skip of
// DPT's ResidualConvUnit), a per-pixel positional table, and the
// pixel-shuffle store of a stride == kernel ConvTranspose2d.
#include <math.h>

#include "conv_tile.h"
#include "tune.h"

namespace {

constexpr int BM = TILE_M, BN = 64, BK = TILE_K, NT = 256;

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  const float* res1;
  const float* res2;
  const float* pos;
  int64_t ldx, ldy, ldr1, ldr2;
  int nimg, hi, wi, ci, ho, wo, co, kh, kw, stride, pad;
  int relu_in, relu_out, res1_relu;
  int shuffle;  // >0: ConvT pixel shuffle factor s; co is then the per-tap output channels
  int ncols;    // GEMM N (= co, or s*s*co for the shuffle)
  // optional split output (the next conv's pre-split input): yh / yl = split(relu?(y))
  bf16_t* yh;
  bf16_t* yl;
  int64_t ldys;
  int split_relu;
};

// ---- shared epilogue: lane holds C[m = 4q + i][n = r16] of each 16x16 tile;
// bias, ReLU, positional table, residual adds, pixel-shuffle store
template <int NTN>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, const f32x4 (&acc)[4][NTN], int M, int m0, int n0,
                                              int wm, int wn, int r16, int q) {
#pragma unroll
  for (int nt = 0; nt < NTN; ++nt) {
    const int n = n0 + wn * NTN * 16 + nt * 16 + r16;
    if (n >= a.ncols) continue;
    int co = n, dy = 0, dx = 0;
    if (a.shuffle) {
      const int tap = n / a.co;
      co = n % a.co;
      dy = tap / a.shuffle;
      dx = tap % a.shuffle;
    }
    const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + mt * 16 + 4 * q + i;
        if (m >= M) continue;
        float v = acc[mt][nt][i] + bv;
        if (a.relu_out) v = fmaxf(v, 0.f);
        int64_t opix;
        if (a.shuffle) {
          const int img = m / (a.ho * a.wo), rem = m % (a.ho * a.wo);
          const int oy = (rem / a.wo) * a.shuffle + dy, ox = (rem % a.wo) * a.shuffle + dx;
          opix = ((int64_t)img * a.ho * a.shuffle + oy) * (a.wo * a.shuffle) + ox;
        } else {
          opix = m;
          if (a.pos) v += a.pos[(int64_t)(m % (a.ho * a.wo)) * a.co + co];
          if (a.res1) {
            const float r = a.res1[(int64_t)m * a.ldr1 + co];
            v += a.res1_relu ? fmaxf(r, 0.f) : r;
          }
          if (a.res2) v += a.res2[(int64_t)m * a.ldr2 + co];
        }
        store_out(a, opix, co, v);
      }
  }
}

__global__ __launch_bounds__(NT, 2) void conv_f32_kernel(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float As[2][BM * BK];
  __shared__ __attribute__((aligned(16))) float Ws[2][BN * BK];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const ConvTile t = conv_tile<BN>(a.nimg, a.ho, a.wo, a.ncols, a.kh, a.kw, a.ci);
  const int M = t.M, m0 = t.m0, n0 = t.n0, K = t.K, nk = t.nk;

  // per-thread A rows: r = tid/8 + 32*i, channel quad c4 = tid%8
  const int c4 = tid & 7;
  PixRow p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = pix_row(m0 + (tid >> 3) + 32 * i, M, a.ho, a.wo, a.stride, a.pad);
  // per-thread W rows: r = tid/8 + 32*i (i < 2)
  f32x4 ra[4], rw[2];

  auto load = [&](int kt) {
    const int k0 = kt * BK;
    const int tap = k0 / a.ci;
    const int ci0 = k0 % a.ci + c4 * 4;
    const int ky = tap / a.kw, kx = tap % a.kw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int iy = p[i].y + ky, ix = p[i].x + kx;
      if (p[i].ok && iy >= 0 && iy < a.hi && ix >= 0 && ix < a.wi) {
        f32x4 v = *(const f32x4*)(a.x + (((int64_t)p[i].img * a.hi + iy) * a.wi + ix) * a.ldx + ci0);
        if (a.relu_in) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        ra[i] = v;
      } else {
        ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + (tid >> 3) + 32 * i;  // weights are padded to a multiple of BN rows
      rw[i] = *(const f32x4*)(a.w + (int64_t)n * K + k0 + c4 * 4);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (tid >> 3) + 32 * i;
      *(f32x4*)(&As[buf][r * BK + ((c4 ^ (r & 7)) << 2)]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (tid >> 3) + 32 * i;
      *(f32x4*)(&Ws[buf][r * BK + ((c4 ^ (r & 7)) << 2)]) = rw[i];
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, q = lane >> 4;
  f32x4 acc[4][2];
  acc_zero(acc);

  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const int ch = kc * 4 + q;
      f32x4 af[4], wf[2];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int r = wm * 64 + mt * 16 + r16;
        af[mt] = *(const f32x4*)(&As[cur][r * BK + ((ch ^ (r & 7)) << 2)]);
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int r = wn * 32 + nt * 16 + r16;
        wf[nt] = *(const f32x4*)(&Ws[cur][r * BK + ((ch ^ (r & 7)) << 2)]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[mt][j], wf[nt][j], acc[mt][nt], 0, 0, 0);
    }
    if (kt + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }

  conv_epilogue(a, acc, M, m0, n0, wm, wn, r16, q);
}

// ===========================================================================
// Split-bf16 ("bf16x3") form of the same implicit GEMM: every fp32 operand is
// split as x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (16 significant
// bits), and the product is accumulated in fp32 as hi.hi + hi.lo + lo.hi on
// v_mfma_f32_16x16x32_bf16 (the dropped lo.lo term and the split residue are
// ~2^-16 relative).  Three bf16 MFMAs replace eight f32 ones per 32-deep K
// slice, so the conv runs on the 2.5 PF bf16 matrix path instead of the
// 157 TF f32 one.  Weights come pre-split (vggt_split_bf16x2); activations
// are split on the fly after the (optional) input ReLU.
// LDS layout, DMA, fragments and the three-MFMA product: conv_tile.h.
// ===========================================================================
// The split-bf16 tile of BNX columns: bytes of one bf16 A / W tile half, of a stage (Ahi, Alo, Whi, Wlo),
// the W DMA pieces (1 KiB) per wave per half (BNX 32: waves 0-1 only), and the kernel's LDS (two stages)
template <int BNX>
struct SplitTile {
  static constexpr int NTN = BNX / 32;  // 16-col fragments per wave (2 waves along N)
  static constexpr int AT = BM * BK * 2, WT = BNX * BK * 2;
  static constexpr int STG = 2 * AT + 2 * WT;
  static constexpr int WPW = WT / 1024 / 4 > 0 ? WT / 1024 / 4 : 1;
  static constexpr int LDS = 2 * STG;
};

// Per-lane byte offsets of a wave's W DMA pieces (pre-split bf16 weights, rows padded to the N tile):
// piece p (1 KiB) of a half = rows 16p..16p+15 (64-B rows); lane -> row 16p + lane/4, LDS chunk lane%4,
// which must hold global chunk (lane%4) ^ h(row) -- the swz64 swizzle applied on the source address
// (the DMA image is lane-linear).
template <int WPW>
__device__ __forceinline__ void w_offsets(uint32_t (&woff)[WPW], int wave, int lane, int K) {
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int row = (wave * WPW + i) * 16 + (lane >> 2);
    woff[i] = (uint32_t)(row * K + swz64(row, lane & 3) * 8) * 2u;
  }
}

// A and B fragments of wave (wm, wn) out of one stage
template <int BNX>
__device__ __forceinline__ void stage_frags(const char* base, int wm, int wn, int roff, bf16x8 (&ah)[4], bf16x8 (&al)[4],
                                            bf16x8 (&bh)[BNX / 32], bf16x8 (&bl)[BNX / 32]) {
  typedef SplitTile<BNX> T;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int o = (wm * 64 + mt * 16) * 64 + roff;
    ah[mt] = *(const bf16x8*)(base + o);
    al[mt] = *(const bf16x8*)(base + T::AT + o);
  }
  b_frags<T::NTN>(base + 2 * T::AT, base + 2 * T::AT + T::WT, wn, roff, bh, bl);
}

template <int BNX, bool PF2>
__global__ __launch_bounds__(NT, 2) void conv_bf16x3_kernel(ConvArgs a, const bf16_t* __restrict__ whi,
                                                            const bf16_t* __restrict__ wlo, uint32_t xbytes) {
  typedef SplitTile<BNX> T;
  constexpr int NTN = T::NTN, AT = T::AT, WT = T::WT, STG = T::STG, WPW = T::WPW;
  __shared__ __attribute__((aligned(16))) char smem[T::LDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ConvTile t = conv_tile<BNX>(a.nimg, a.ho, a.wo, a.ncols, a.kh, a.kw, a.ci);
  const int M = t.M, m0 = t.m0, n0 = t.n0, K = t.K, nk = t.nk, ntap = t.ntap;

  // A: rows r = tid/8 + 32*i, fp32 channel quad c4 = tid%8 (4 K values)
  const int c4 = tid & 7;
  PixRow p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = pix_row(m0 + (tid >> 3) + 32 * i, M, a.ho, a.wo, a.stride, a.pad);
  const bool wdma = wave * WPW * 1024 < WT;
  uint32_t woff[WPW];
  w_offsets(woff, wave, lane, K);
  const i32x4 rwh = make_rsrc(whi + (int64_t)n0 * K, 0xffffffffu), rwl = make_rsrc(wlo + (int64_t)n0 * K, 0xffffffffu);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)LDS_PTR(smem));
  auto wstage = [&](int buf, int kt) {
    if (!wdma) return;
    const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)(t.kcol(kt) * 2));
    const uint32_t b = lds0 + buf * STG + 2 * AT + wave * WPW * 1024;
#pragma unroll
    for (int i = 0; i < WPW; ++i) {
      dma16(rwh, woff[i], soff, b + i * 1024);
      dma16(rwl, woff[i], soff, b + WT + i * 1024);
    }
  };
  // A gather staged through registers, one K-step ahead: issued at the start
  // of step kt, split and stored at its end (no use of the loaded values in
  // between -- the input ReLU is applied at the store -- so the loads stay in
  // flight during the MFMAs)
  struct Stage {
    f32x4 ra[4];
  };
  Stage s0;

  auto load = [&](Stage& st, int kt) {
    f32x4 (&ra)[4] = st.ra;
    const int tap = kt % ntap;
    const int ci0 = (kt / ntap) * BK + c4 * 4;
    const int ky = tap / a.kw, kx = tap % a.kw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int iy = p[i].y + ky, ix = p[i].x + kx;
      // no use of the loaded value here (the input ReLU is applied at the
      // store): the gather stays in flight for two MFMA steps
      ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p[i].ok && iy >= 0 && iy < a.hi && ix >= 0 && ix < a.wi)
        ra[i] = *(const f32x4*)(a.x + (((int64_t)p[i].img * a.hi + iy) * a.wi + ix) * a.ldx + ci0);
    }
  };
  // PF2: the gather as raw buffer loads -- every lane issues exactly its 4
  // loads (taps outside the image get an offset past num_records and read
  // zeros), so the K-loop can wait with a COUNTED vmcnt and keep the next
  // step's gather in flight across a barrier (two register stages)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)xbytes, 0x00020000);
  auto load2 = [&](Stage& st, int kt) {
    const int tap = kt % ntap;
    const int ci0 = (kt / ntap) * BK + c4 * 4;
    const int ky = tap / a.kw, kx = tap % a.kw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int iy = p[i].y + ky, ix = p[i].x + kx;
      const bool ok = p[i].ok && iy >= 0 && iy < a.hi && ix >= 0 && ix < a.wi;
      const uint32_t off = ok ? (uint32_t)((((p[i].img * a.hi + iy) * a.wi + ix) * (uint32_t)a.ldx + ci0) * 4u)
                              : 0xfffffff0u;
      st.ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)off, 0, 0));
    }
  };
  auto store = [&](const Stage& st, int buf) {
    char* base = smem + buf * STG;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (tid >> 3) + 32 * i;
      uint2 h, l;
      float xv[4], hv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xv[j] = a.relu_in ? fmaxf(st.ra[i][j], 0.f) : st.ra[i][j];
        hv[j] = round_bf(xv[j]);
      }
      h.x = pack_bf2(hv[0], hv[1]);
      h.y = pack_bf2(hv[2], hv[3]);
      l.x = pack_bf2(xv[0] - hv[0], xv[1] - hv[1]);
      l.y = pack_bf2(xv[2] - hv[2], xv[3] - hv[3]);
      const int off = r * 64 + (swz64(r, c4 >> 1) << 4) + (c4 & 1) * 8;
      *(uint2*)(base + off) = h;
      *(uint2*)(base + AT + off) = l;
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, q = lane >> 4;
  const int roff = r16 * 64 + (swz64(r16, q) << 4);  // fragment read offset (row & 15 == r16)
  f32x4 acc[4][NTN];
  acc_zero(acc);

  auto compute = [&](int cur) {
    bf16x8 ah[4], al[4], bh[NTN], bl[NTN];
    stage_frags<BNX>(smem + cur * STG, wm, wn, roff, ah, al, bh, bl);
    mfma3(acc, ah, al, bh, bl);
  };

  // Per step kt (LDS buffer kt & 1): W DMA of tile kt+1 into the other
  // buffer, the A gather of tile kt+1 into registers, the MFMAs of tile kt,
  // the split + store of A tile kt+1, then every wave's DMA retired
  // (vmcnt(0)) before the barrier that publishes the next buffer.
  if constexpr (PF2) {
    // Two register stages, loop unrolled by two (s0 <-> buffer 0, s1 <->
    // buffer 1, no loop-carried copies): in step kt the gather of tile kt+2
    // is issued before the MFMAs of tile kt and stays in flight across the
    // step's barrier (vmcnt(4) = only this step's 4 gather loads may remain;
    // the W DMA and the previous gather are older).
    Stage s1;
    wstage(0, 0);
    load2(s0, 0);
    store(s0, 0);
    if (nk > 1) {
      load2(s1, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // steady state: every operation unconditional, so the compiler's own
    // waitcnt tracking sees the same pending loads on both loop entries
    int kt = 0;
    for (; kt + 3 < nk; kt += 2) {
      wstage(1, kt + 1);
      load2(s0, kt + 2);
      compute(0);
      store(s1, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __syncthreads();
      wstage(0, kt + 2);
      load2(s1, kt + 3);
      compute(1);
      store(s0, 0);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __syncthreads();
    }
    // the last 1-3 steps (no gather beyond tile kt+2)
    const bool h1 = kt + 1 < nk, h2 = kt + 2 < nk;
    if (h1) wstage(1, kt + 1);
    if (h2) load2(s0, kt + 2);
    compute(0);
    if (h1) {
      store(s1, 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (h2) wstage(0, kt + 2);
      compute(1);
      if (h2) {
        store(s0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        compute(0);
      }
    }
  } else {
  wstage(0, 0);
  load(s0, 0);
  store(s0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      wstage(cur ^ 1, kt + 1);
      load(s0, kt + 1);
    }
    compute(cur);
    if (kt + 1 < nk) store(s0, cur ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  }

  conv_epilogue<NTN>(a, acc, M, m0, n0, wm, wn, r16, q);
}

// ===========================================================================
// Pre-split form (vggt_conv2d_bf16x3_pre): the activation arrives already
// split into bf16 hi / lo maps (vggt_split_act_bf16x2, input ReLU applied
// there), so the im2col gather is LDS-DMA like the weights -- per lane one
// 16-B piece of a 64-B (32-channel) pixel row, out-of-image taps get an offset
// past num_records and land as zeros.  The register-staged form above spends
// ~230 VALU instructions per wave per K-step on the gather addressing, the
// split and the LDS stores (4.75 per MFMA, VALU-issue-bound at 34% MFMA busy,
// 148^2 x 256 -> 256: profiles r3c); here the K-step is 8 DMA pieces and two
// address selects per wave.  Same K order, same MFMA sequence (conv_tile.h
// mfma3): bitwise equal to conv_bf16x3_kernel.
// ===========================================================================
template <int BNX>
__global__ __launch_bounds__(NT, 2) void conv_pre_kernel(ConvArgs a, const bf16_t* __restrict__ xhi,
                                                         const bf16_t* __restrict__ xlo, uint32_t xbytes,
                                                         const bf16_t* __restrict__ whi, const bf16_t* __restrict__ wlo) {
  typedef SplitTile<BNX> T;
  constexpr int NTN = T::NTN, AT = T::AT, WT = T::WT, STG = T::STG, WPW = T::WPW;
  constexpr int APW = AT / 1024 / 4;  // A pieces per wave per half (2)
  __shared__ __attribute__((aligned(16))) char smem[T::LDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const ConvTile t = conv_tile<BNX>(a.nimg, a.ho, a.wo, a.ncols, a.kh, a.kw, a.ci);
  const int M = t.M, m0 = t.m0, n0 = t.n0, K = t.K, nk = t.nk, ntap = t.ntap;

  // A pieces: rows (wave*APW + j)*16 + lane/4, LDS chunk lane%4 <- global chunk swz64(row, lane%4)
  int pb[APW], py[APW], px[APW];
#pragma unroll
  for (int j = 0; j < APW; ++j) {
    const int row = (wave * APW + j) * 16 + (lane >> 2);
    const PixRow p = pix_row(m0 + row, M, a.ho, a.wo, a.stride, a.pad);
    py[j] = p.ok ? p.y : -(1 << 20);  // rows past M: never inside the image (read as zeros)
    px[j] = p.x;
    pb[j] = ((p.img * a.hi + p.y) * a.wi + p.x) * (int)a.ldx + swz64(row, lane & 3) * 8;
  }
  uint32_t woff[WPW];
  w_offsets(woff, wave, lane, K);
  const bool wdma = wave * WPW * 1024 < WT;
  const i32x4 rwh = make_rsrc(whi + (int64_t)n0 * K, 0xffffffffu), rwl = make_rsrc(wlo + (int64_t)n0 * K, 0xffffffffu);
  const i32x4 rxh = make_rsrc(xhi, xbytes), rxl = make_rsrc(xlo, xbytes);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)LDS_PTR(smem));
  auto stage = [&](int buf, int kt) {
    const uint32_t b = lds0 + buf * STG;
    const int tap = kt % ntap, ky = tap / a.kw, kx = tap % a.kw;
    const int sh = (ky * a.wi + kx) * (int)a.ldx + (kt / ntap) * BK;  // wave-uniform element shift
#pragma unroll
    for (int j = 0; j < APW; ++j) {
      const int iy = py[j] + ky, ix = px[j] + kx;
      const bool ok = (unsigned)iy < (unsigned)a.hi && (unsigned)ix < (unsigned)a.wi;
      const uint32_t off = ok ? (uint32_t)(pb[j] + sh) * 2u : 0xfffffff0u;
      dma16(rxh, off, 0, b + (wave * APW + j) * 1024);
      dma16(rxl, off, 0, b + AT + (wave * APW + j) * 1024);
    }
    if (wdma) {
      const uint32_t soff = __builtin_amdgcn_readfirstlane((uint32_t)(t.kcol(kt) * 2));
#pragma unroll
      for (int i = 0; i < WPW; ++i) {
        dma16(rwh, woff[i], soff, b + 2 * AT + (wave * WPW + i) * 1024);
        dma16(rwl, woff[i], soff, b + 2 * AT + WT + (wave * WPW + i) * 1024);
      }
    }
  };

  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, q = lane >> 4;
  const int roff = r16 * 64 + (swz64(r16, q) << 4);
  f32x4 acc[4][NTN];
  acc_zero(acc);
  bf16x8 ah[4], al[4], bh[NTN], bl[NTN];

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
    stage_frags<BNX>(smem + cur * STG, wm, wn, roff, ah, al, bh, bl);
    mfma3(acc, ah, al, bh, bl);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  conv_epilogue<NTN>(a, acc, M, m0, n0, wm, wn, r16, q);
}

// hi / lo = split(relu?(x)) of a [rows, cols] f32 map with row stride ldx
// (cols % 4 == 0) into contiguous [rows, cols] bf16 maps
__global__ __launch_bounds__(256) void split_act_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int cols,
                                                        int relu, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
  const int c4n = cols / 4;
  const int64_t total = rows * c4n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / c4n;
    const int c = (int)(i - r * c4n) * 4;
    f32x4 v = *(const f32x4*)(x + r * ldx + c);
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    uint2 ph, pl;
    bl_split(v, ph, pl);
    *(uint2*)(hi + r * cols + c) = ph;
    *(uint2*)(lo + r * cols + c) = pl;
  }
}

__global__ __launch_bounds__(256) void split_bf16x2_kernel(const float* __restrict__ x, int64_t n, bf16_t* __restrict__ hi,
                                                           bf16_t* __restrict__ lo) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    const float h = round_bf(v);
    hi[i] = f2bf(h);
    lo[i] = f2bf(v - h);
  }
}

// Bilinear resize, align_corners=True, NHWC f32 (F.interpolate semantics),
// optional positional table added to the result: [ho*wo, C] (pos_sep 0), or
// separable (pos_sep 1: DPT's UV sin/cos embedding, whose first C/2 channels
// depend on x only and the last C/2 on y only) as [wo + ho, C/2] = U rows
// then V rows -- 1/ho of the full table's bytes, which the full form re-reads
// for every frame (16 x 137 MB per 16-frame 518^2 chunk, profiles/r5c).
__global__ __launch_bounds__(256) void upsample_kernel(const float* __restrict__ x, int nimg, int hi, int wi, int C,
                                                       float* __restrict__ y, int ho, int wo,
                                                       const float* __restrict__ pos, bf16_t* __restrict__ yh,
                                                       bf16_t* __restrict__ yl, int split_relu, int pos_sep) {
  const int c4n = C / 4;
  const int64_t total = (int64_t)nimg * ho * wo * c4n;
  const float sh = ho > 1 ? (float)(hi - 1) / (float)(ho - 1) : 0.f;
  const float sw = wo > 1 ? (float)(wi - 1) / (float)(wo - 1) : 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    const int64_t p = i / c4n;
    const int img = (int)(p / ((int64_t)ho * wo));
    const int rem = (int)(p % ((int64_t)ho * wo));
    const int oy = rem / wo, ox = rem % wo;
    // coordinates, lerp and split: common.h bl_* (one evaluation order with conv_up_kernel)
    int y0, x0;
    float ly, hy, lx, hx;
    bl_coord(sh, oy, y0, ly, hy);
    bl_coord(sw, ox, x0, lx, hx);
    const int y1 = min(y0 + 1, hi - 1), x1 = min(x0 + 1, wi - 1);
    const float* b = x + (int64_t)img * hi * wi * C;
    const f32x4 v00 = *(const f32x4*)(b + ((int64_t)y0 * wi + x0) * C + c);
    const f32x4 v01 = *(const f32x4*)(b + ((int64_t)y0 * wi + x1) * C + c);
    const f32x4 v10 = *(const f32x4*)(b + ((int64_t)y1 * wi + x0) * C + c);
    const f32x4 v11 = *(const f32x4*)(b + ((int64_t)y1 * wi + x1) * C + c);
    f32x4 o = bl_lerp(hy, ly, hx, lx, v00, v01, v10, v11);
    if (pos) {
      if (pos_sep) {
        const int hc = C / 2;
        o += c < hc ? *(const f32x4*)(pos + (int64_t)ox * hc + c) : *(const f32x4*)(pos + (int64_t)(wo + oy) * hc + c - hc);
      } else {
        o += *(const f32x4*)(pos + (int64_t)rem * C + c);
      }
    }
    if (y) *(f32x4*)(y + p * C + c) = o;
    if (yh) {
      if (split_relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
      }
      uint2 ph, pl;
      bl_split(o, ph, pl);
      *(uint2*)(yh + p * C + c) = ph;
      *(uint2*)(yl + p * C + c) = pl;
    }
  }
}

// DPT activate_head: x [P, ncl] NHWC (last channel = confidence).
//   act 0: exp, 1: inv_log (sign(x)*expm1(|x|)); conf: 1 + exp(c) (expp1).
//   pts[p, j] = act(x[p, j]) * scale[img]   (j < ncl-1),  conf[p] = 1 + exp(x[p, ncl-1])
__global__ __launch_bounds__(256) void dpt_act_kernel(const float* __restrict__ x, int64_t ldx, int64_t npix,
                                                      int ppi, int ncl, int act, const float* __restrict__ scale,
                                                      float* __restrict__ pts, float* __restrict__ conf) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
    const float s = scale ? scale[p / ppi] : 1.f;
    for (int j = 0; j < ncl - 1; ++j) {
      const float v = x[p * ldx + j];
      const float a = act == 0 ? expf(v) : copysignf(expm1f(fabsf(v)), v) * (v == 0.f ? 0.f : 1.f);
      pts[p * (ncl - 1) + j] = a * s;
    }
    conf[p] = 1.f + expf(x[p * ldx + ncl - 1]);
  }
}

constexpr int kMaxBlocks = 16384;  // of the elementwise kernels below

}  // namespace

// ===========================================================================
// Dispatch.  conv_resolve maps what a call gives (ConvIn, conv_tile.h) to the error the entry returns or
// the kernel it launches; VGGT_CONV_KERNELS lists the implicit-GEMM kernels; conv_entry runs a form.
// vggt_conv_form exposes the resolver; tests/test_conv_form.py pins it to the checks this code replaced.
// ===========================================================================
enum { C_F32 = VGGT_CONV_FAMILY_F32, C_SPLIT = VGGT_CONV_FAMILY_SPLIT, C_PRE = VGGT_CONV_FAMILY_PRE };
typedef vggt_conv_form_t ConvForm;

// The checks the three implicit-GEMM entries share, in the order that fixes which code two faults at once return
static int conv_check(const ConvIn& in) {
  if (in.nimg <= 0 || in.hi <= 0 || in.wi <= 0 || in.ci <= 0 || in.co <= 0 || in.kh <= 0 || in.kw <= 0 ||
      in.stride <= 0 || in.pad < 0 || in.ci % BK)
    return VGGT_ERR_SHAPE;
  // rows must not overlap: a pixel stride below ci (on a map of more than one pixel), an output stride below co
  if ((in.ldx < in.ci && (int64_t)in.nimg * in.hi * in.wi > 1) || ((in.has & VGGT_CONV_HAS_Y) && in.ldy < in.co))
    return VGGT_ERR_SHAPE;
  if (in.shuffle && (in.kh != 1 || in.kw != 1 || in.stride != 1 || in.pad != 0 ||
                     (in.has & (VGGT_CONV_HAS_RES1 | VGGT_CONV_HAS_RES2 | VGGT_CONV_HAS_POS))))
    return VGGT_ERR_UNSUPPORTED;
  if ((in.ldx % 4) || in.x_unaligned) return VGGT_ERR_ALIGN;
  return VGGT_OK;
}

// Output size and GEMM columns of an implicit-GEMM call (after conv_check: stride > 0)
static void conv_dims(const ConvIn& in, int& ho, int& wo, int& ncols) {
  ho = (in.hi + 2 * in.pad - in.kh) / in.stride + 1;
  wo = (in.wi + 2 * in.pad - in.kw) / in.stride + 1;
  ncols = in.shuffle ? in.shuffle * in.shuffle * in.co : in.co;
}

// The one place that picks a convolution kernel.  Host arithmetic on `in` alone.
vggt_conv_form_t conv_resolve(const ConvIn& in) {
  ConvForm f{};
  const bool has_y = in.has & VGGT_CONV_HAS_Y, has_hi = in.has & VGGT_CONV_HAS_Y_HI, has_lo = in.has & VGGT_CONV_HAS_Y_LO;
  auto fail = [](int rc) { ConvForm e{}; return e.rc = rc, e; };
  if (in.entry == VGGT_CONV_ENTRY_UPSAMPLE) {  // conv_up_kernel: tiles of 4 x 32 output pixels x all co (<= 32)
    if (in.nimg <= 0 || in.hi <= 0 || in.wi <= 0 || in.ho <= 0 || in.wo <= 0 || in.ci <= 0 || in.ci % TILE_K ||
        in.co <= 0 || in.co > CONV_UP_BN || (!has_y && !has_hi))
      return fail(VGGT_ERR_SHAPE);
    if (has_hi != has_lo || (has_y && in.ldy < in.co) || (has_hi && in.ldys < in.co)) return fail(VGGT_ERR_SHAPE);
    if ((int64_t)31 * 9 * in.ci + 9 * in.ci > 0x3fffffff) return fail(VGGT_ERR_SHAPE);  // 32-bit weight DMA offsets
    if (in.x_unaligned || in.w_unaligned) return fail(VGGT_ERR_ALIGN);
    const int64_t nwg = (int64_t)in.nimg * ((in.ho + CONV_UP_R - 1) / CONV_UP_R) * ((in.wo + CONV_UP_C - 1) / CONV_UP_C);
    if (nwg > 0x7fffffff) return fail(VGGT_ERR_SHAPE);
    f.family = VGGT_CONV_FAMILY_UPSAMPLE, f.bn = f.w_rows = CONV_UP_BN, f.grid = (int)nwg, f.lds = CONV_UP_LDS;
    return f;
  }
  if (const int rc = conv_check(in)) return fail(rc);
  int ho, wo, ncols;
  conv_dims(in, ho, wo, ncols);
  const int64_t tiles_m = ((int64_t)in.nimg * ho * wo + BM - 1) / BM;
  // the grid guard is judged on the 64-wide tile count, whichever width runs
  if (tiles_m * ((ncols + BN - 1) / BN) > 0x7fffffff) return fail(VGGT_ERR_SHAPE);
  const int64_t last = (int64_t)in.nimg * in.hi * in.wi - 1;  // the last pixel
  // split forms: 128-wide N tiles from 128 GEMM columns (more MFMA work per split of the activation
  // tile), 64 above 32, else (output_conv2, 128 -> 32) 32: no padded MFMA columns
  f.bn = in.entry == VGGT_CONV_ENTRY_F32 ? BN : ncols >= 128 ? 128 : ncols > 32 ? 64 : 32;
  f.lds = f.bn == 128 ? SplitTile<128>::LDS : f.bn == 32 ? SplitTile<32>::LDS : SplitTile<64>::LDS;
  if (in.entry == VGGT_CONV_ENTRY_F32) {
    f.family = C_F32, f.lds = 2 * (BM + BN) * BK * 4;
  } else if (in.entry == VGGT_CONV_ENTRY_BF16X3) {
    if (in.w_unaligned) return fail(VGGT_ERR_ALIGN);
    // two-deep gather (buffer loads with 32-bit byte offsets) when the input spans < 4 GiB
    const int64_t xb = last * in.ldx * 4 + (int64_t)in.ci * 4;
    f.family = C_SPLIT, f.pf2 = xb < (int64_t)0xffffff00ll && in.pf2, f.xbytes = f.pf2 ? (uint32_t)xb : 0u;
  } else {
    if ((!has_y && !has_hi) || has_hi != has_lo || (has_hi && in.ldys < in.co)) return fail(VGGT_ERR_SHAPE);
    if (in.w_unaligned || (in.ldx % 8)) return fail(VGGT_ERR_ALIGN);
    // 32-bit byte offsets: the whole map (plus the widest tap shift) below 4 GiB
    const int64_t xb = last * in.ldx * 2 + (int64_t)in.ci * 2;
    if (xb >= (int64_t)0x7fffff00ll) return fail(VGGT_ERR_SHAPE);
    f.family = C_PRE, f.xbytes = (uint32_t)xb;
  }
  const int tiles_n = (ncols + f.bn - 1) / f.bn;
  f.grid = (int)(tiles_m * tiles_n), f.w_rows = tiles_n * f.bn;
  return f;
}

namespace {
// Every implicit-GEMM kernel the library holds, as X(family, BN, PF2)
#define VGGT_CONV_K_C_F32(B, P) conv_f32_kernel
#define VGGT_CONV_K_C_SPLIT(B, P) conv_bf16x3_kernel<B, P>
#define VGGT_CONV_K_C_PRE(B, P) conv_pre_kernel<B>
#define VGGT_CONV_KERNELS(X)                                                                           \
  X(C_F32, 64, false) X(C_SPLIT, 32, true) X(C_SPLIT, 64, true) X(C_SPLIT, 128, true) X(C_SPLIT, 32, false) \
  X(C_SPLIT, 64, false) X(C_SPLIT, 128, false) X(C_PRE, 32, false) X(C_PRE, 64, false) X(C_PRE, 128, false)

template <int FAM, auto KERNEL>
void conv_start(const ConvForm& f, const ConvArgs& a, const bf16_t* xl, const bf16_t* wh, const bf16_t* wl, hipStream_t s) {
  if constexpr (FAM == C_F32) KERNEL<<<f.grid, NT, 0, s>>>(a);
  else if constexpr (FAM == C_SPLIT) KERNEL<<<f.grid, NT, 0, s>>>(a, wh, wl, f.xbytes);
  else KERNEL<<<f.grid, NT, 0, s>>>(a, (const bf16_t*)a.x, xl, f.xbytes, wh, wl);
}

ConvIn conv_in(int entry, int64_t ldx, int nimg, int hi, int wi, int ci, int co, int kh, int kw, int stride, int pad,
               int shuffle, int64_t ldy, int64_t ldys, int has) {
  ConvIn in{};
  in.entry = entry, in.nimg = nimg, in.hi = hi, in.wi = wi, in.ci = ci, in.co = co, in.kh = kh, in.kw = kw;
  in.stride = stride, in.pad = pad, in.shuffle = shuffle, in.ldx = ldx, in.ldy = ldy, in.ldys = ldys, in.has = has;
  in.pf2 = g_vggt_conv_pf2;  // read per call: vggt_tune may change it
  return in;
}

// The three implicit-GEMM entries: x is x_hi for the pre form, which also gives x_lo; w the f32 entry's
// weights, w_hi / w_lo the split ones.  Resolve, fill the kernel's arguments, launch.
int conv_entry(int entry, const void* x, const void* x_lo, int64_t ldx, int nimg, int hi, int wi, int ci, const float* w,
               const void* w_hi, const void* w_lo, const float* bias, int co, int kh, int kw, int stride, int pad,
               float* y, int64_t ldy, int relu_in, int relu_out, const float* res1, int64_t ldr1, int res1_relu,
               const float* res2, int64_t ldr2, const float* pos, int shuffle, void* y_hi, void* y_lo, int64_t ldys,
               int split_relu, void* stream) {
  ConvIn in = conv_in(entry, ldx, nimg, hi, wi, ci, co, kh, kw, stride, pad, shuffle, ldy, ldys,
                      (y ? VGGT_CONV_HAS_Y : 0) | (y_hi ? VGGT_CONV_HAS_Y_HI : 0) | (y_lo ? VGGT_CONV_HAS_Y_LO : 0) |
                          (res1 ? VGGT_CONV_HAS_RES1 : 0) | (res2 ? VGGT_CONV_HAS_RES2 : 0) | (pos ? VGGT_CONV_HAS_POS : 0));
  in.x_unaligned = (((uintptr_t)x | (uintptr_t)w) % 16) != 0;
  in.w_unaligned = (((uintptr_t)x_lo | (uintptr_t)w_hi | (uintptr_t)w_lo) % 16) != 0;
  const ConvForm f = conv_resolve(in);
  if (f.rc != VGGT_OK) return f.rc;
  ConvArgs a{(const float*)x, w, bias, y, res1, res2, pos, ldx, ldy, ldr1, ldr2, nimg, hi, wi, ci, 0, 0, co, kh, kw, stride,
             pad, relu_in, relu_out, res1_relu, shuffle, 0, (bf16_t*)y_hi, (bf16_t*)y_lo, ldys, split_relu};
  conv_dims(in, a.ho, a.wo, a.ncols);
#define VGGT_CONV_TRY(FAM, B, P)                         \
  if (f.family == FAM && f.bn == B && (f.pf2 != 0) == P) \
    conv_start<FAM, VGGT_CONV_K_##FAM(B, P)>(f, a, (const bf16_t*)x_lo, (const bf16_t*)w_hi, (const bf16_t*)w_lo, (hipStream_t)stream);
  VGGT_CONV_KERNELS(VGGT_CONV_TRY)
#undef VGGT_CONV_TRY
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}
}  // namespace

extern "C" int vggt_conv2d_f32(const float* x, int64_t ldx, int nimg, int hi, int wi, int ci, const float* w,
                               const float* bias, int co, int kh, int kw, int stride, int pad, float* y, int64_t ldy,
                               int relu_in, int relu_out, const float* res1, int64_t ldr1, int res1_relu,
                               const float* res2, int64_t ldr2, const float* pos, int shuffle, void* stream) {
  return conv_entry(VGGT_CONV_ENTRY_F32, x, nullptr, ldx, nimg, hi, wi, ci, w, nullptr, nullptr, bias, co, kh, kw, stride,
                    pad, y, ldy, relu_in, relu_out, res1, ldr1, res1_relu, res2, ldr2, pos, shuffle, nullptr, nullptr, 0, 0,
                    stream);
}

extern "C" int vggt_conv2d_bf16x3(const float* x, int64_t ldx, int nimg, int hi, int wi, int ci, const void* w_hi,
                                  const void* w_lo, const float* bias, int co, int kh, int kw, int stride, int pad,
                                  float* y, int64_t ldy, int relu_in, int relu_out, const float* res1, int64_t ldr1,
                                  int res1_relu, const float* res2, int64_t ldr2, const float* pos, int shuffle,
                                  void* stream) {
  return conv_entry(VGGT_CONV_ENTRY_BF16X3, x, nullptr, ldx, nimg, hi, wi, ci, nullptr, w_hi, w_lo, bias, co, kh, kw,
                    stride, pad, y, ldy, relu_in, relu_out, res1, ldr1, res1_relu, res2, ldr2, pos, shuffle, nullptr,
                    nullptr, 0, 0, stream);
}

extern "C" int vggt_conv2d_bf16x3_pre(const void* x_hi, const void* x_lo, int64_t ldx, int nimg, int hi, int wi,
                                      int ci, const void* w_hi, const void* w_lo, const float* bias, int co, int kh,
                                      int kw, int stride, int pad, float* y, int64_t ldy, int relu_out,
                                      const float* res1, int64_t ldr1, int res1_relu, const float* res2, int64_t ldr2,
                                      const float* pos, int shuffle, void* y_hi, void* y_lo, int64_t ldys,
                                      int split_relu, void* stream) {
  return conv_entry(VGGT_CONV_ENTRY_PRE, x_hi, x_lo, ldx, nimg, hi, wi, ci, nullptr, w_hi, w_lo, bias, co, kh, kw, stride,
                    pad, y, ldy, 0, relu_out, res1, ldr1, res1_relu, res2, ldr2, pos, shuffle, y_hi, y_lo, ldys,
                    split_relu, stream);
}

// Which kernel the four convolution entries launch (include/vggt_mi355x.h): conv_resolve under the
// process's gather knob, every pointer taken as aligned.  No device call.
extern "C" int vggt_conv_form(int entry, int nimg, int hi, int wi, int ci, int co, int kh, int kw, int stride, int pad,
                              int shuffle, int ho, int wo, int64_t ldx, int64_t ldy, int64_t ldys, int present,
                              vggt_conv_form_t* form) {
  if (!form || entry < VGGT_CONV_ENTRY_F32 || entry > VGGT_CONV_ENTRY_UPSAMPLE) return VGGT_ERR_UNSUPPORTED;
  ConvIn in = conv_in(entry, ldx, nimg, hi, wi, ci, co, kh, kw, stride, pad, shuffle, ldy, ldys, present);
  in.ho = ho, in.wo = wo;
  *form = conv_resolve(in);
  return form->rc;
}


extern "C" int vggt_split_act_bf16x2(const float* x, int64_t ldx, int64_t rows, int cols, int relu, void* hi, void* lo,
                                     void* stream) {
  if (rows < 0 || cols <= 0 || cols % 4 || ldx < cols) return VGGT_ERR_SHAPE;
  if ((ldx % 4) || ((uintptr_t)x % 16) || ((uintptr_t)hi % 8) || ((uintptr_t)lo % 8)) return VGGT_ERR_ALIGN;
  if (rows == 0) return VGGT_OK;
  split_act_kernel<<<grid_for(rows * (cols / 4), kMaxBlocks), 256, 0, (hipStream_t)stream>>>(x, ldx, rows, cols, relu,
                                                                              (bf16_t*)hi, (bf16_t*)lo);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_split_bf16x2(const float* x, int64_t n, void* hi, void* lo, void* stream) {
  if (n < 0) return VGGT_ERR_SHAPE;
  if (n == 0) return VGGT_OK;
  split_bf16x2_kernel<<<grid_for(n, kMaxBlocks), 256, 0, (hipStream_t)stream>>>(x, n, (bf16_t*)hi, (bf16_t*)lo);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

// The three bilinear entries' launch.  cmod: what C must be a multiple of; shape_ok: the entry's own
// pointer-presence rules; a16: the entry's pointers that must be 16-byte aligned, OR'd
static int upsample_launch(const float* x, int nimg, int hi, int wi, int C, int cmod, float* y, int ho, int wo,
                           const float* pos, int pos_sep, void* y_hi, void* y_lo, int split_relu, bool shape_ok,
                           uintptr_t a16, void* stream) {
  if (nimg <= 0 || hi <= 0 || wi <= 0 || ho <= 0 || wo <= 0 || C % cmod || !shape_ok) return VGGT_ERR_SHAPE;
  if (a16 % 16 || ((uintptr_t)y_hi | (uintptr_t)y_lo) % 8) return VGGT_ERR_ALIGN;
  upsample_kernel<<<grid_for((int64_t)nimg * ho * wo * (C / 4), kMaxBlocks), 256, 0, (hipStream_t)stream>>>(
      x, nimg, hi, wi, C, y, ho, wo, pos, (bf16_t*)y_hi, (bf16_t*)y_lo, split_relu, pos_sep);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_upsample_bilinear_f32(const float* x, int nimg, int hi, int wi, int C, float* y, int ho, int wo,
                                          const float* pos, void* stream) {
  return upsample_launch(x, nimg, hi, wi, C, 4, y, ho, wo, pos, 0, nullptr, nullptr, 0, true,
                         (uintptr_t)x | (uintptr_t)y, stream);
}

extern "C" int vggt_upsample_bilinear_split(const float* x, int nimg, int hi, int wi, int C, float* y, int ho, int wo,
                                            const float* pos, void* y_hi, void* y_lo, int split_relu, void* stream) {
  return upsample_launch(x, nimg, hi, wi, C, 4, y, ho, wo, pos, 0, y_hi, y_lo, split_relu,
                         (y || y_hi) && !y_hi == !y_lo, (uintptr_t)x | (uintptr_t)y, stream);
}

extern "C" int vggt_upsample_bilinear_split_sep(const float* x, int nimg, int hi, int wi, int C, float* y, int ho,
                                                int wo, const float* pos_sep, void* y_hi, void* y_lo, int split_relu,
                                                void* stream) {
  return upsample_launch(x, nimg, hi, wi, C, 8, y, ho, wo, pos_sep, 1, y_hi, y_lo, split_relu,
                         (y || y_hi) && !y_hi == !y_lo && pos_sep, (uintptr_t)x | (uintptr_t)y | (uintptr_t)pos_sep,
                         stream);
}

extern "C" int vggt_dpt_activate(const float* x, int64_t ldx, int64_t npix, int pix_per_img, int ncl, int act,
                                 const float* scale, float* pts, float* conf, void* stream) {
  if (npix <= 0 || ncl < 2 || pix_per_img <= 0 || (act != 0 && act != 1)) return VGGT_ERR_SHAPE;
  dpt_act_kernel<<<grid_for(npix, kMaxBlocks), 256, 0, (hipStream_t)stream>>>(x, ldx, npix, pix_per_img, ncl, act, scale, pts,
                                                                  conf);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}
