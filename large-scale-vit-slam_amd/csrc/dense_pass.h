// What the dense one-pass kernels of points.hip (k-th value), loss.hip (depth loss), gt_align.hip (GT
// depth scale) and gt_points.hip (GT point alignment) share: the classification of a float on its bits,
// the order-preserving key of the radix selects and the histogram step of a select pass, the
// four-element loads and stores, the 256-bin scan of the pick kernels, the fixed-order
// reduction of a workgroup's partial record, and the grid size.  No function here holds a floating-point
// multiply followed by an add, so the contraction setting of the including file changes nothing in it;
// the per-pixel arithmetic (ga_term, dl_term, bl_axis, bl_value) stays in its own file under that
// file's `#pragma clang fp contract(off)`.
#pragma once
#include "common.h"

constexpr unsigned int F32_QNAN = 0x7fc00000u;

__device__ __forceinline__ bool f32_is_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool f32_is_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// torch's order (-inf < finite < +inf < NaN) as an unsigned key: negative floats flip all bits, the
// others set the sign bit, every NaN takes the largest key.  Every key is above 0.
//   f32_key              -0 keys just below +0, and f32_unkey gives it back as -0.  The depth loss's amax
//                        (dl_amax_kernel) needs this: torch.amax of a frame whose confidences are all -0
//                        is -0, and vggt_depth_loss_values writes that value out.
//   f32_key_zeros_equal  -0 takes +0's key, as torch.kthvalue and torch.sort compare them (-0 == +0).  The
//                        radix selects (vggt_kth_value_f32, the ratio of vggt_depth_scale_l1) need this:
//                        the rank of a zero must not depend on its sign, and the selected zero is +0.
__device__ __forceinline__ unsigned int f32_key(float v) {
  const unsigned int b = __float_as_uint(v);
  if (f32_is_nan(v)) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned int f32_key_zeros_equal(float v) {
  return __float_as_uint(v) == 0x80000000u ? 0x80000000u : f32_key(v);
}
__device__ __forceinline__ float f32_unkey(unsigned int k) {
  if (k == 0xffffffffu) return __uint_as_float(F32_QNAN);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One element of a radix-select histogram pass (vggt_kth_value_f32, the threshold of vggt_gt_points_align): the
// digit at `shift` of v's key is counted in the workgroup's 256-bin LDS histogram when the element exists and
// its higher digits (mask) equal the prefix.  Every lane of the wave calls it together (ballots).
__device__ __forceinline__ void radix_digit_add(unsigned int* hist, float v, unsigned int prefix, unsigned int mask,
                                                int shift, bool in_range) {
  const unsigned int key = f32_key_zeros_equal(v);  // torch.kthvalue's order: -0 == +0
  const bool take = in_range && (key & mask) == prefix;
  const unsigned int digit = (key >> shift) & 255u;
  const unsigned long long takers = __ballot(take);
  if (takers == 0) return;  // wave-uniform
  // Confidences share their top digits: when one digit holds the whole wave, one add of the lane count.
  const unsigned int first = __shfl(digit, __ffsll((long long)takers) - 1, 64);
  if (__ballot(take && digit == first) == takers) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)takers) - 1) atomicAdd(&hist[first], (unsigned int)__popcll(takers));
  } else if (take) {
    atomicAdd(&hist[digit], 1u);
  }
}

// Four consecutive elements from e of `total`: one 128-bit (mask: 32-bit) access when VEC and all four
// exist, else one by one (a missing element reads as 0 / false and is not written).
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, unsigned int e, unsigned int total, float (&v)[4]) {
  if (VEC && e + 4 <= total) {
    const float4 t = *reinterpret_cast<const float4*>(p + e);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = e + j < total ? p[e + j] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void load4_mask(const uint8_t* __restrict__ p, unsigned int e, unsigned int total,
                                           bool (&v)[4]) {
  if (VEC && e + 4 <= total) {
    const unsigned int t = *reinterpret_cast<const unsigned int*>(p + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((t >> (8 * j)) & 0xffu) != 0;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = e + j < total && p[e + j] != 0;
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, unsigned int e, unsigned int total, const float (&v)[4]) {
  if (VEC && e + 4 <= total) {
    *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e + j < total) p[e + j] = v[j];
  }
}

// Inclusive scan of the 256 counters in LDS, one per lane of a 256-lane workgroup; cum[tid] is written and
// a barrier passed before the call, and every lane may read any cum[] after it.
__device__ __forceinline__ void scan256_inclusive(unsigned long long* cum, int tid) {
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long add = tid >= o ? cum[tid - o] : 0ull;
    __syncthreads();
    cum[tid] += add;
    __syncthreads();
  }
}

// A workgroup's partial record (fp64 sums and integer counts, one per lane) to one record, in a fixed
// order: the wave butterfly of every field (Rec::wave), lane 0 of each wave to LDS, then thread 0 adds
// waves 1 .. WAVES - 1 to wave 0 in index order (Rec::add).  Only thread 0's return value is the total.
template <typename Rec, int WAVES>
__device__ __forceinline__ Rec block_reduce_record(Rec rec, Rec* s_part) {
  rec = rec.wave();
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_part[tid >> 6] = rec;
  __syncthreads();
  if (tid == 0) {
    rec = s_part[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) rec.add(s_part[k]);
  }
  return rec;
}

// Workgroups of a grid-stride pass over n elements: one per threads * per_thread elements, between 1 and cap.
inline int grid_for(int64_t n, int threads, int per_thread, int cap) {
  const int64_t per_block = (int64_t)threads * per_thread;
  const int64_t want = (n + per_block - 1) / per_block;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}
