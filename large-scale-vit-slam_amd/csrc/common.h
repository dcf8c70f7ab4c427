// Shared device helpers for the gfx950 (CDNA4) kernels of the VGGT hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vggt_mi355x.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef uint16_t bf16_t;  // raw bf16 bits in global memory

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// Round-to-nearest-even fp32 -> bf16 (finite inputs; NaN stays NaN via the
// hardware convert path the compiler emits for __bf16 casts).
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ float round_bf(float f) { return bf2f(f2bf(f)); }

// pack two floats into a dword of 2 bf16 (lo, hi)
// (one v_cvt_pk_bf16_f32: the two scalar conversions + shift + or of the plain
// form cost four VALU, e.g. 192 extra per 256x256 GEMM tile epilogue per wave)
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 b16x2_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){lo, hi}, b16x2_t));
}

// Per-head LayerNorm + RoPE arithmetic shared by headnorm_rope_kernel (norm.hip) and the fused GEMM
// epilogues (gemm.hip: write_tile and the persistent form), so that all of them give the same bits.
// Left to the compiler's contraction, the copies of the same expressions rounded differently (about
// 2 outputs per million a bf16 ulp apart, several ulps where the affine term or the rotation
// cancels), so the fused multiply-adds are spelled out, and so is the order of the head's sums.
__device__ __forceinline__ float hn_sq_acc(float d, float q) { return __builtin_fmaf(d, d, q); }
__device__ __forceinline__ float hn_rstd(float q, float inv_d, float eps) { return rsqrtf(__builtin_fmaf(q, inv_d, eps)); }
__device__ __forceinline__ float hn_affine(float x, float mean, float rstd, float w, float b) {
  return __builtin_fmaf((x - mean) * rstd, w, b);
}
__device__ __forceinline__ float hn_rotate(float x, float c, float rot, float s) { return __builtin_fmaf(x, c, rot * s); }

// Bilinear resize (align_corners) arithmetic shared by upsample_kernel (conv.hip) and the patch build
// of conv_up_kernel (conv_up.hip), so that the fused resize + conv sees the very operands the unfused
// upsample writes.  Left to the compiler's contraction, the same source expression became
// fma(lx, v01, hx * v00) in one file and fma(hx, v00, lx * v01) in the other (an fp32 ulp apart,
// a whole bf16 lo-half apart after the split), so the fused multiply-adds are spelled out.
//   bl_coord: source coordinate f = s * o of output index o; i0 = (int)f, l = s * o - i0 in one
//             rounding (may be a rounding below zero when f rounds up onto an integer), h = 1 - l
//   bl_lerp:  hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11) + pos, evaluated as
//             fma(hy, fma(lx, v01, hx * v00), ly * fma(lx, v11, hx * v10)), then the table add
__device__ __forceinline__ void bl_coord(float s, int o, int& i0, float& l, float& h) {
  const float of = (float)o;
  const float f = s * of;
  i0 = (int)f;
  l = __builtin_fmaf(s, of, -(float)i0);
  h = 1.f - l;
}
__device__ __forceinline__ f32x4 bl_lerp(float hy, float ly, float hx, float lx, f32x4 v00, f32x4 v01, f32x4 v10,
                                         f32x4 v11) {
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float top = __builtin_fmaf(lx, v01[j], hx * v00[j]);
    const float bot = __builtin_fmaf(lx, v11[j], hx * v10[j]);
    o[j] = __builtin_fmaf(hy, top, ly * bot);
  }
  return o;
}
// split of (relu?) o into packed bf16 hi / lo: hi = bf16(o), lo = bf16(o - hi)
__device__ __forceinline__ void bl_split(f32x4 o, uint2& ph, uint2& pl) {
  float h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = round_bf(o[j]);
  ph.x = pack_bf2(h[0], h[1]);
  ph.y = pack_bf2(h[2], h[3]);
  pl.x = pack_bf2(o[0] - h[0], o[1] - h[1]);
  pl.y = pack_bf2(o[2] - h[2], o[3] - h[3]);
}

// Sum over a head whose LPH consecutive lanes hold 8 consecutive values each: MEAN = false the sum
// of (x[j] - mean)^2, MEAN = true the sum of x[j] (mean unused).
// 64-wide heads (LPH = 8) take the order of the persistent GEMM's epilogue, whose lane (row group
// rg = 0..3 of the MFMA fragment layout) holds values 16 ni + 4 rg + 0..3 of the head for ni = 0..3:
// four chains over ni, one per rg, then (chain 0 + chain 1) + (chain 2 + chain 3).  Here lane l of
// the head holds fragment ni = l / 2, row groups 2 (l % 2) and 2 (l % 2) + 1, so a chain runs over
// lanes l, l + 2, l + 4, l + 6 (three hops), and lanes 6 and 7 end up with the four chain sums.
template <int LPH, bool MEAN>
__device__ __forceinline__ float hn_head_sum(const float (&x)[8], float mean) {
  if constexpr (LPH == 8) {
    const int lane = threadIdx.x & 63, l = lane & 7;
    float ca = 0.f, cb = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float ia = 0.f, ib = 0.f;
      if (k) {
        ia = __shfl(ca, lane - 2, 64);
        ib = __shfl(cb, lane - 2, 64);
      }
      float na, nb;
      if constexpr (MEAN) {
        na = ia + ((x[0] + x[1]) + (x[2] + x[3]));
        nb = ib + ((x[4] + x[5]) + (x[6] + x[7]));
      } else {
        na = ia;
        nb = ib;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          na = hn_sq_acc(x[j] - mean, na);
          nb = hn_sq_acc(x[4 + j] - mean, nb);
        }
      }
      if ((l >> 1) == k) {
        ca = na;
        cb = nb;
      }
    }
    const float t = ca + cb;
    return __shfl(t, (lane & ~7) + 6, 64) + __shfl(t, (lane & ~7) + 7, 64);
  } else {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = MEAN ? s + x[j] : hn_sq_acc(x[j] - mean, s);
#pragma unroll
    for (int o = 1; o < LPH; o <<= 1) s += __shfl_xor(s, o, 64);
    return s;
  }
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// GELU(x) = x * Phi(x) through a branch-free erfc (Chebyshev fit, fractional
// error < 1.2e-7 over the whole real line, i.e. ~1 fp32 ulp): one rcp, one
// exp2 and ten FMAs, no divergence.  Used where the result is rounded to
// bf16 (the GEMM fc1 epilogue), where it matches the libm erf form up to
// rare round-to-nearest ties.
__device__ __forceinline__ float gelu_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
  float p = 0.17087277f;
  p = fmaf(p, t, -0.82215223f);
  p = fmaf(p, t, 1.48851587f);
  p = fmaf(p, t, -1.13520398f);
  p = fmaf(p, t, 0.27886807f);
  p = fmaf(p, t, -0.18628806f);
  p = fmaf(p, t, 0.09678418f);
  p = fmaf(p, t, 0.37409196f);
  p = fmaf(p, t, 1.00002368f);
  p = fmaf(p, t, -1.26551223f);
  const float e = t * __builtin_amdgcn_exp2f(fmaf(-z, z, p) * 1.4426950408889634f);  // erfc(z)
  return x * (x >= 0.f ? fmaf(-0.5f, e, 1.0f) : 0.5f * e);
}

// Two GELUs at once: the polynomial, the final products and the select run as
// packed fp32 (v_pk_fma_f32 / v_pk_mul_f32: two lanes of work per
// instruction); only rcp and exp2 stay scalar.  Same formula and error as
// gelu_fast.  For pure-VALU epilogues (no MFMA in flight on the wave).
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ f32x2 gelu_fast2(f32x2 x) {
  const f32x2 z = f32x2{fabsf(x[0]), fabsf(x[1])} * 0.70710678118654752440f;
  const f32x2 d = z * 0.5f + 1.0f;
  const f32x2 t = f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
  f32x2 p = f32x2{0.17087277f, 0.17087277f};
  p = p * t + -0.82215223f;
  p = p * t + 1.48851587f;
  p = p * t + -1.13520398f;
  p = p * t + 0.27886807f;
  p = p * t + -0.18628806f;
  p = p * t + 0.09678418f;
  p = p * t + 0.37409196f;
  p = p * t + 1.00002368f;
  p = p * t + -1.26551223f;
  const f32x2 arg = (p - z * z) * 1.4426950408889634f;
  const f32x2 e = t * f32x2{__builtin_amdgcn_exp2f(arg[0]), __builtin_amdgcn_exp2f(arg[1])};  // erfc(z)
  const f32x2 h = e * 0.5f;
  const f32x2 phi = f32x2{x[0] >= 0.f ? 1.0f - h[0] : h[0], x[1] >= 0.f ? 1.0f - h[1] : h[1]};
  return x * phi;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// The same butterfly for the fp64 sums (every lane ends with the same bits: the order of the additions
// is fixed by the offsets alone) and for integer counts.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// XCD-aware bijective remap of a linear block id (cdna_hip_programming.md §5
// "XCD swizzle must be bijective"): consecutive logical tiles land on the
// same XCD (blocks b and b+8 share one), so tiles that share an operand panel
// hit the same L2.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
  const int q = nwg / 8, r = nwg % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// Workgroups of 256 threads for a grid-stride pass over `total` elements: one thread each, at most `cap` groups
inline int grid_for(int64_t total, int cap) {
  const int64_t g = (total + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

#define HIP_LAUNCH_CHECK()                         \
  do {                                             \
    hipError_t e_ = hipGetLastError();             \
    if (e_ != hipSuccess) return VGGT_ERR_HIP;     \
  } while (0)
