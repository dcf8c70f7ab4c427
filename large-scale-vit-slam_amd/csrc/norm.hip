// Row LayerNorm and per-head QK-norm + RoPE (include/vggt_mi355x.h:
// vggt_layernorm, vggt_headnorm_rope).  HBM-bound: one wave per row, 16-B
// vectorised loads/stores, fp32 two-pass statistics in registers.
#include "norm_row.h"

namespace {

__device__ __forceinline__ void unpack_bf4(uint2 u, float (&f)[4]) {
  f[0] = bf2f(u.x & 0xffff);
  f[1] = bf2f(u.x >> 16);
  f[2] = bf2f(u.y & 0xffff);
  f[3] = bf2f(u.y >> 16);
}

// ---------------------------------------------------------------- LayerNorm
// NV = C / 256 float4 per lane (C = 256 * NV); rows through a RowMap.
// x and y carry no __restrict__: the model normalises in place (y == x with equal
// dtypes and strides; a wave reads its whole row before it stores any of it).
// fp32 outputs (the fp32 heads: a few hundred rows) take their statistics and the
// affine step in fp64 with one rounding per stored value: in fp32, 4 NV serial additions
// per lane and rsqrtf left a row up to 5 x as far from fp64 as a plain fp32 evaluation
// (C = 4096, mean 1000: 3.3e-7 against 6.4e-8 of the row norm), which only a bf16
// rounding hides.  bf16 outputs keep the fp32 statistics (and their bits).
template <int NV, bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(256) void layernorm_kernel(const void* x, int64_t ldx, const float* __restrict__ w,
                                                        const float* __restrict__ b, float eps, int M, void* y,
                                                        int64_t ldy, RowMap rm) {
  constexpr int C = NV * 256;
  const int lane = threadIdx.x & 63;
  const int lrow = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (lrow >= M) return;
  const int gi = lrow / rm.G, ii = lrow % rm.G;
  const int64_t row = (int64_t)gi * rm.xgs + rm.xoff + ii;
  const int64_t orow = (int64_t)gi * rm.ygs + rm.yoff + ii;
  float v[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 256 + lane * 4;
    if constexpr (IN_BF16) {
      unpack_bf4(*(const uint2*)((const bf16_t*)x + row * ldx + c), v[i]);
    } else {
      const f32x4 u = *(const f32x4*)((const float*)x + row * ldx + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = u[j];
    }
  }
  if constexpr (OUT_BF16) {
    float mean, rstd;
    row_stats_f32<NV>(v, eps, mean, rstd);
    row_affine_store_bf16<NV>(v, mean, rstd, w, b, (bf16_t*)y + orow * ldy, lane);
  } else {
    double sd = 0.;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) sd += (double)v[i][j];
    const double mean = wave_sum(sd) / C;  // a quotient: the mean of a constant row is exact for every C
    double qd = 0.;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)v[i][j] - mean;
        qd = fma(d, d, qd);
      }
    const double rstd = 1.0 / sqrt(wave_sum(qd) / C + (double)eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 256 + lane * 4;
      f32x4 o;
      if (w) {
        const f32x4 wv = *(const f32x4*)(w + c);
        const f32x4 bv = b ? *(const f32x4*)(b + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)(((double)v[i][j] - mean) * rstd * (double)wv[j] + (double)bv[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)(((double)v[i][j] - mean) * rstd);
      }
      *(f32x4*)((float*)y + orow * ldy + c) = o;
    }
  }
}

template <int NV>
int launch_ln(const void* x, int in_bf, int64_t ldx, const float* w, const float* b, float eps, int M, void* y,
              int out_bf, int64_t ldy, RowMap rm, hipStream_t s) {
  const int grid = (M + 3) / 4;
  if (in_bf && out_bf) layernorm_kernel<NV, true, true><<<grid, 256, 0, s>>>(x, ldx, w, b, eps, M, y, ldy, rm);
  else if (in_bf) layernorm_kernel<NV, true, false><<<grid, 256, 0, s>>>(x, ldx, w, b, eps, M, y, ldy, rm);
  else if (out_bf) layernorm_kernel<NV, false, true><<<grid, 256, 0, s>>>(x, ldx, w, b, eps, M, y, ldy, rm);
  else layernorm_kernel<NV, false, false><<<grid, 256, 0, s>>>(x, ldx, w, b, eps, M, y, ldy, rm);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

// ------------------------------------ LayerScale residual add + LayerNorm
// x[m] += gamma * y[m] (fp32 residual, bf16 branch output -- the arithmetic
// of the GEMM's EPI_RESID_F32 epilogue), optionally mirrored into out2, then
// (LN) xn[m] = LayerNorm(x[m]) in bf16, affine when w is given.  One wave per
// row, NV float4 per lane, like layernorm_kernel.
// The LayerScale residual step of every form below, one fp32 expression (the
// compiler contracts it to a fused multiply-add in each of them), so the
// deferred two-pass forms give the bits of the two stored passes.
__device__ __forceinline__ float resid_step(float u, float g, float y) { return u + g * y; }

// <TWO, STORE> = <0, 1> is the stored form.  The other two are the same two row
// passes of a block with the first one's store of x deferred:
//  <0, 0> (after proj): xn[m] = LayerNorm(x[m] + gamma * y[m]); x is only
//    read -- x' lives in registers for the statistics.
//  <1, 1> (after fc2): x[m] = (x[m] + gamma * y[m]) + gamma2 * y2[m] with the
//    first pass's y and gamma again (resid_step twice: the bits of the two stored
//    passes), the kept-layer mirror, and (LN) xn[m] = LayerNorm(x[m]).
// Per block 180 + 315 MB instead of 270 + 270 MB at 21,984 x 1024.
template <int NV, bool TWO, bool STORE, bool LN>
__global__ __launch_bounds__(256) void resid_add_ln_kernel(
    float* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ y, int64_t ldy, const float* __restrict__ gamma,
    const bf16_t* __restrict__ y2, int64_t ldy2, const float* __restrict__ gamma2, float* __restrict__ out2,
    int64_t ldo2, const float* __restrict__ w, const float* __restrict__ b, float eps, int M,
    bf16_t* __restrict__ xn, int64_t ldn) {
  static_assert(STORE || LN, "a form that stores nothing");
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float v[NV][4];
  uint2 yu[NV], yu2[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    yu[i] = *(const uint2*)(y + (int64_t)row * ldy + i * 256 + lane * 4);
    if constexpr (TWO) yu2[i] = *(const uint2*)(y2 + (int64_t)row * ldy2 + i * 256 + lane * 4);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 256 + lane * 4;
    const f32x4 u = *(const f32x4*)(x + (int64_t)row * ldx + c);
    const f32x4 g = *(const f32x4*)(gamma + c);
    float yv[4];
    unpack_bf4(yu[i], yv);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = resid_step(u[j], g[j], yv[j]);
    if constexpr (TWO) {
      const f32x4 g2 = *(const f32x4*)(gamma2 + c);
      unpack_bf4(yu2[i], yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = resid_step(v[i][j], g2[j], yv[j]);
    }
    if constexpr (STORE) {
      *(f32x4*)(x + (int64_t)row * ldx + c) = f32x4{v[i][0], v[i][1], v[i][2], v[i][3]};
      if (out2) *(f32x4*)(out2 + (int64_t)row * ldo2 + c) = f32x4{v[i][0], v[i][1], v[i][2], v[i][3]};
    }
  }
  if constexpr (LN) {
    float mean, rstd;
    row_stats_f32<NV>(v, eps, mean, rstd);
    row_affine_store_bf16<NV>(v, mean, rstd, w, b, xn + (int64_t)row * ldn, lane);
  }
}

using raln_kernel_t = decltype(&resid_add_ln_kernel<1, false, true, true>);

template <int NV>
raln_kernel_t raln_kernel(bool two, bool store, bool ln) {
  if (two) return ln ? resid_add_ln_kernel<NV, true, true, true> : resid_add_ln_kernel<NV, true, true, false>;
  if (!store) return resid_add_ln_kernel<NV, false, false, true>;
  return ln ? resid_add_ln_kernel<NV, false, true, true> : resid_add_ln_kernel<NV, false, true, false>;
}

// The three residual entry points: two = vggt_resid_add2_layernorm (y2 and gamma2 required), !store =
// vggt_resid_add_layernorm_nostore (xn required).
int raln(bool two, bool store, float* x, int64_t ldx, const void* y, int64_t ldy, const float* gamma, const void* y2,
         int64_t ldy2, const float* gamma2, float* out2, int64_t ldo2, const float* w, const float* b, float eps, int M,
         int C, void* xn, int64_t ldn, void* stream) {
  if (two && !y2) return VGGT_ERR_SHAPE;
  if (M <= 0) return M == 0 ? VGGT_OK : VGGT_ERR_SHAPE;
  if (C % 256 || C > 4096 || C <= 0 || !x || !y || !gamma || (y2 && !gamma2) || (!store && !xn))
    return VGGT_ERR_SHAPE;
  if ((ldx % 4) || (ldy % 4) || (y2 && (ldy2 % 4)) || (out2 && (ldo2 % 4)) || (xn && (ldn % 4)))
    return VGGT_ERR_ALIGN;
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)gamma2 | (uintptr_t)out2 | (uintptr_t)w | (uintptr_t)b) % 16 ||
      ((uintptr_t)y | (uintptr_t)y2 | (uintptr_t)xn) % 8)
    return VGGT_ERR_ALIGN;
  raln_kernel_t k;
  switch (C / 256) {
    case 1: k = raln_kernel<1>(two, store, xn); break;
    case 2: k = raln_kernel<2>(two, store, xn); break;
    case 4: k = raln_kernel<4>(two, store, xn); break;
    case 8: k = raln_kernel<8>(two, store, xn); break;
    default: return VGGT_ERR_SHAPE;
  }
  k<<<(M + 3) / 4, 256, 0, (hipStream_t)stream>>>(x, ldx, (const bf16_t*)y, ldy, gamma, (const bf16_t*)y2, ldy2, gamma2,
                                                  out2, ldo2, w, b, eps, M, (bf16_t*)xn, ldn);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

// ------------------------------------------------- per-head norm + RoPE
// One wave per row; each lane owns 8 consecutive values (one 16-B chunk) of
// a head; LPH = D/8 lanes per head, heads processed 64/LPH at a time.
// Heads [0, hsplit) use (w, b), heads [hsplit, H) use (w2, b2): one launch
// normalises q and k of a fused qkv row (different q_norm / k_norm weights).
// Rows are read from src (row stride lds; == buf for the in-place form) and
// written to buf, at the same column offset.
template <int D, int MODE>
__global__ __launch_bounds__(256) void headnorm_rope_kernel(const bf16_t* src, int64_t lds, bf16_t* buf, int64_t ld,
                                                            int col_off, int M,
                                                            int H, const float* __restrict__ w,
                                                            const float* __restrict__ b, float eps,
                                                            const int32_t* __restrict__ pos, int period,
                                                            const float* __restrict__ cs, const float* __restrict__ sn,
                                                            int tab_len, int hsplit, const float* __restrict__ w2,
                                                            const float* __restrict__ b2) {
  constexpr int LPH = D / 8;
  constexpr int HPP = 64 / LPH;  // heads per pass
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int sub = lane % LPH;  // chunk index within the head
  const int e0 = sub * 8;      // first element within the head
  int p0 = 0, p1 = 0;
  if constexpr (MODE == VGGT_ROPE_2D) {
    const int pr = row % period;
    p0 = min(max(pos[2 * pr], 0), tab_len - 1);
    p1 = min(max(pos[2 * pr + 1], 0), tab_len - 1);
  } else if constexpr (MODE == VGGT_ROPE_1D) {
    p0 = min(max(pos[row % period], 0), tab_len - 1);
  }
  // both weight sets preloaded (heads < hsplit use w/b, the rest w2/b2)
  float wa[8], ba[8], wb[8], bb2[8];
  if (w) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wa[j] = w[e0 + j];
      ba[j] = b ? b[e0 + j] : 0.f;
      wb[j] = w2[e0 + j];
      bb2[j] = b2 ? b2[e0 + j] : 0.f;
    }
  }
  for (int h0 = 0; h0 < H; h0 += HPP) {
    const int h = h0 + lane / LPH;
    const bool act = h < H;
    const bool first_set = h < hsplit;
    float wv[8], bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wv[j] = first_set ? wa[j] : wb[j];
      bv[j] = first_set ? ba[j] : bb2[j];
    }
    bf16_t* p = buf + (int64_t)row * ld + col_off + (act ? h : 0) * D + e0;
    float x[8];
    {
      const uint4 u = *(const uint4*)(src + (int64_t)row * lds + col_off + (act ? h : 0) * D + e0);
      const uint32_t uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[2 * j] = bf2f(uu[j] & 0xffff);
        x[2 * j + 1] = bf2f(uu[j] >> 16);
      }
    }
    if (w) {
      const float mean = hn_head_sum<LPH, true>(x, 0.f) * (1.f / D);
      const float rstd = hn_rstd(hn_head_sum<LPH, false>(x, mean), 1.f / D, eps);
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = hn_affine(x[j], mean, rstd, wv[j], bv[j]);
    }
    if constexpr (MODE != VGGT_ROPE_NONE) {
      // rotate_half partner lives RD/2 elements away = (RD/16) lanes away
      constexpr int RD = (MODE == VGGT_ROPE_2D) ? D / 2 : D;
      constexpr int PL = RD / 16;  // partner lane distance
      const int er = e0 % RD;      // element index inside the rotated block
      const int pp = (MODE == VGGT_ROPE_2D && e0 >= D / 2) ? p1 : p0;
      const bool first = er < RD / 2;
      // 8 consecutive table entries from a 32-B aligned offset: two 16-B loads each
      const float4* cp = (const float4*)(cs + pp * RD + er);
      const float4* sp = (const float4*)(sn + pp * RD + er);
      const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
      const float cv[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float partner = __shfl_xor(x[j], PL, 64);
        const float rot = first ? -partner : partner;
        y[j] = hn_rotate(x[j], cv[j], rot, sv[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = y[j];
    }
    if (act) {
      uint4 u;
      u.x = pack_bf2(x[0], x[1]);
      u.y = pack_bf2(x[2], x[3]);
      u.z = pack_bf2(x[4], x[5]);
      u.w = pack_bf2(x[6], x[7]);
      *(uint4*)p = u;
    }
  }
}

using hnr_kernel_t = decltype(&headnorm_rope_kernel<64, VGGT_ROPE_NONE>);

template <int D>
hnr_kernel_t hnr_kernel(int mode) {
  switch (mode) {
    case VGGT_ROPE_NONE: return headnorm_rope_kernel<D, VGGT_ROPE_NONE>;
    case VGGT_ROPE_2D: return headnorm_rope_kernel<D, VGGT_ROPE_2D>;
    case VGGT_ROPE_1D: return headnorm_rope_kernel<D, VGGT_ROPE_1D>;
    default: return nullptr;
  }
}

// The four bf16 head-norm entry points: `heads` heads of D columns from column col_off of src into the
// same columns of dst (dst == src: in place), heads [0, hsplit) with (w, b), the rest with (w2, b2).
int hnr(const void* src, int64_t lds, void* dst, int64_t ldd, int col_off, int M, int heads, int hsplit, int D,
        const float* w, const float* b, const float* w2, const float* b2, float eps, int mode, const int32_t* pos,
        int period, const float* cs, const float* sn, int tab_len, void* stream) {
  if (M <= 0) return M == 0 ? VGGT_OK : VGGT_ERR_SHAPE;
  if (heads <= 0 || (D != 64 && D != 128) || !src || !dst) return VGGT_ERR_SHAPE;
  if ((lds % 8) || (ldd % 8) || (col_off % 8) || ((uintptr_t)src | (uintptr_t)dst) % 16) return VGGT_ERR_ALIGN;
  if ((w == nullptr) != (w2 == nullptr)) return VGGT_ERR_SHAPE;
  if (mode != VGGT_ROPE_NONE && (!pos || !cs || !sn || period <= 0 || tab_len <= 0)) return VGGT_ERR_SHAPE;
  if (((uintptr_t)cs | (uintptr_t)sn) % 16) return VGGT_ERR_ALIGN;
  const hnr_kernel_t k = D == 64 ? hnr_kernel<64>(mode) : hnr_kernel<128>(mode);
  if (!k) return VGGT_ERR_UNSUPPORTED;
  k<<<(M + 3) / 4, 256, 0, (hipStream_t)stream>>>((const bf16_t*)src, lds, (bf16_t*)dst, ldd, col_off, M, heads, w, b,
                                                  eps, pos, period, cs, sn, tab_len, hsplit, w2, b2);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

}  // namespace

extern "C" int vggt_layernorm_grouped(const void* x, int in_dtype, int64_t ldx, const float* w, const float* b,
                                      float eps, int M, int C, void* y, int out_dtype, int64_t ldy, int group,
                                      int x_group_stride, int x_row_offset, int y_group_stride, int y_row_offset,
                                      void* stream) {
  if (M <= 0) return M == 0 ? VGGT_OK : VGGT_ERR_SHAPE;
  if (group <= 0) return VGGT_ERR_SHAPE;
  RowMap rm{group, x_group_stride, x_row_offset, y_group_stride, y_row_offset};
  if (C % 256 || C > 4096 || C <= 0 || !x || !y) return VGGT_ERR_SHAPE;
  if ((in_dtype != VGGT_DTYPE_F32 && in_dtype != VGGT_DTYPE_BF16) ||
      (out_dtype != VGGT_DTYPE_F32 && out_dtype != VGGT_DTYPE_BF16))
    return VGGT_ERR_UNSUPPORTED;
  if ((ldx % 4) || (ldy % 4) || ((uintptr_t)x % 8) || ((uintptr_t)y % 8)) return VGGT_ERR_ALIGN;
  if (!in_dtype && ((uintptr_t)x % 16)) return VGGT_ERR_ALIGN;
  if (!out_dtype && ((uintptr_t)y % 16)) return VGGT_ERR_ALIGN;
  if ((w && ((uintptr_t)w % 16)) || (b && ((uintptr_t)b % 16))) return VGGT_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int ib = in_dtype == VGGT_DTYPE_BF16, ob = out_dtype == VGGT_DTYPE_BF16;
  switch (C / 256) {
    case 1: return launch_ln<1>(x, ib, ldx, w, b, eps, M, y, ob, ldy, rm, s);
    case 2: return launch_ln<2>(x, ib, ldx, w, b, eps, M, y, ob, ldy, rm, s);
    case 3: return launch_ln<3>(x, ib, ldx, w, b, eps, M, y, ob, ldy, rm, s);
    case 4: return launch_ln<4>(x, ib, ldx, w, b, eps, M, y, ob, ldy, rm, s);
    case 8: return launch_ln<8>(x, ib, ldx, w, b, eps, M, y, ob, ldy, rm, s);
    case 16: return launch_ln<16>(x, ib, ldx, w, b, eps, M, y, ob, ldy, rm, s);
    default: return VGGT_ERR_SHAPE;
  }
}

extern "C" int vggt_layernorm(const void* x, int in_dtype, int64_t ldx, const float* w, const float* b, float eps,
                              int M, int C, void* y, int out_dtype, int64_t ldy, void* stream) {
  return vggt_layernorm_grouped(x, in_dtype, ldx, w, b, eps, M, C, y, out_dtype, ldy, M > 0 ? M : 1, 0, 0, 0, 0,
                                stream);
}

extern "C" int vggt_resid_add_layernorm(float* x, int64_t ldx, const void* y, int64_t ldy, const float* gamma,
                                        float* out2, int64_t ldo2, const float* w, const float* b, float eps, int M,
                                        int C, void* xn, int64_t ldn, void* stream) {
  return raln(false, true, x, ldx, y, ldy, gamma, nullptr, 0, nullptr, out2, ldo2, w, b, eps, M, C, xn, ldn, stream);
}

extern "C" int vggt_resid_add_layernorm_nostore(const float* x, int64_t ldx, const void* y, int64_t ldy,
                                                const float* gamma, const float* w, const float* b, float eps, int M,
                                                int C, void* xn, int64_t ldn, void* stream) {
  // the kernel only reads x in this form
  return raln(false, false, const_cast<float*>(x), ldx, y, ldy, gamma, nullptr, 0, nullptr, nullptr, 0, w, b, eps, M,
              C, xn, ldn, stream);
}

extern "C" int vggt_resid_add2_layernorm(float* x, int64_t ldx, const void* y, int64_t ldy, const float* gamma,
                                         const void* y2, int64_t ldy2, const float* gamma2, float* out2, int64_t ldo2,
                                         const float* w, const float* b, float eps, int M, int C, void* xn,
                                         int64_t ldn, void* stream) {
  return raln(true, true, x, ldx, y, ldy, gamma, y2, ldy2, gamma2, out2, ldo2, w, b, eps, M, C, xn, ldn, stream);
}

extern "C" int vggt_headnorm_rope(void* buf, int64_t ld, int col_off, int M, int H, int D, const float* w,
                                  const float* b, float eps, int rope_mode, const int32_t* pos, int period,
                                  const float* cos_tab, const float* sin_tab, int tab_len, void* stream) {
  return hnr(buf, ld, buf, ld, col_off, M, H, H, D, w, b, w, b, eps, rope_mode, pos, period, cos_tab, sin_tab, tab_len,
             stream);
}

extern "C" int vggt_qknorm_rope(void* qkv, int64_t ld, int M, int H, int D, const float* qw, const float* qb,
                                const float* kw, const float* kb, float eps, int rope_mode, const int32_t* pos,
                                int period, const float* cos_tab, const float* sin_tab, int tab_len, void* stream) {
  return hnr(qkv, ld, qkv, ld, 0, M, 2 * H, H, D, qw, qb, kw, kb, eps, rope_mode, pos, period, cos_tab, sin_tab,
             tab_len, stream);
}

// Out-of-place form of vggt_qknorm_rope: the q|k columns [0, 2*H*D) of src
// (row stride lds) are normalised + rotated into dst (row stride ldd); src is
// left untouched (the training recompute keeps the pre-norm values for the
// backward, and the v columns are read from src directly).
extern "C" int vggt_qknorm_rope_out(const void* src, int64_t lds, void* dst, int64_t ldd, int M, int H, int D,
                                    const float* qw, const float* qb, const float* kw, const float* kb, float eps,
                                    int rope_mode, const int32_t* pos, int period, const float* cos_tab,
                                    const float* sin_tab, int tab_len, void* stream) {
  return hnr(src, lds, dst, ldd, 0, M, 2 * H, H, D, qw, qb, kw, kb, eps, rope_mode, pos, period, cos_tab, sin_tab,
             tab_len, stream);
}

// Out-of-place form of vggt_headnorm_rope: H heads of D columns starting at
// column 0 of src (row stride lds) normalised + rotated into dst (row stride ldd).
extern "C" int vggt_headnorm_rope_out(const void* src, int64_t lds, void* dst, int64_t ldd, int M, int H, int D,
                                      const float* w, const float* b, float eps, int rope_mode, const int32_t* pos,
                                      int period, const float* cos_tab, const float* sin_tab, int tab_len,
                                      void* stream) {
  return hnr(src, lds, dst, ldd, 0, M, H, H, D, w, b, w, b, eps, rope_mode, pos, period, cos_tab, sin_tab, tab_len,
             stream);
}
