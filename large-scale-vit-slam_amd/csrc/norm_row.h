// Device helpers of the one-wave-per-row norm kernels (norm.hip: layernorm_kernel, resid_add_ln_kernel;
// train.hip: ln_bwd_kernel).  A lane holds NV float4 of a row of C = 256 * NV values: value j of chunk i
// is column i * 256 + lane * 4 + j.
#pragma once
#include "common.h"

// Row r of the logical [M, C] input maps to group g = r / G, i = r % G:
//   x row = g*xgs + xoff + i,  y row = g*ygs + yoff + i   (identity: G = M).
struct RowMap {
  int G, xgs, xoff, ygs, yoff;
};

// Two-pass fp32 statistics of a row.  The one copy of this expression and of its summation order: the
// backward recomputes the forward's mean and rstd with it, and the residual forms give the bits of
// vggt_layernorm on the stored x (so the deferred forms the bits of the stored ones) because every
// kernel takes its statistics from here.
template <int NV>
__device__ __forceinline__ void row_stats_f32(const float (&v)[NV][4], float eps, float& mean, float& rstd) {
  constexpr int C = NV * 256;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += v[i][j];
  mean = wave_sum(s) * (1.f / C);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = v[i][j] - mean;
      q += d * d;
    }
  rstd = rsqrtf(wave_sum(q) * (1.f / C) + eps);
}

// out[c] = bf16((v - mean) * rstd * w[c] + b[c]) over the row that starts at out; w NULL: no affine
// step (b ignored), b NULL: no bias.  lane is the caller's threadIdx.x & 63: taken from it, the
// column offsets are the ones its load loop already holds; recomputed here, they were a second set
// that cost the residual kernels up to 11 VGPRs and two occupancy steps at NV = 8.
template <int NV>
__device__ __forceinline__ void row_affine_store_bf16(const float (&v)[NV][4], float mean, float rstd, const float* w,
                                                      const float* b, bf16_t* out, int lane) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 256 + lane * 4;
    float o[4];
    if (w) {
      const f32x4 wv = *(const f32x4*)(w + c);
      const f32x4 bv = b ? *(const f32x4*)(b + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * wv[j] + bv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd;
    }
    uint2 u;
    u.x = pack_bf2(o[0], o[1]);
    u.y = pack_bf2(o[2], o[3]);
    *(uint2*)(out + c) = u;
  }
}
