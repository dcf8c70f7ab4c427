// GT depth-scale alignment of a training step: the reference's scale_align_from_depths (utils/alignment.py:244-323),
// the per-batch-element weighted median  argmin_a sum_i w_i |a x_i - y_i|  of the ratios r_i = y_i / x_i with the
// weights w_i x_i, between the model and the loss of every step run with gt_alignment_type: scale_from_depths.
//
// The reference sorts the ratios, gathers the weights, takes a cumulative sum, searches it for half the total and
// reads one value per element back on the host.  A median needs no sort, and nothing here visits the host:
//
//   sums    cnt = sum m and the fp64 sum of y m: per-lane partials -> a fixed tree per workgroup -> one record per
//           workgroup (dl_sums_kernel's scheme, loss.hip); which lane takes which pixel depends on n alone;
//   mean    one workgroup per element combines the records in a fixed order: mean, min_depth = 0.1f * mean, and
//           clears the element's histograms and selection state;
//   wmax    the largest finite w_eff (an integer atomic max on the bits of a non-negative float) and the smallest
//           ratio key (an integer atomic min: what a total of 0 selects);
//   4 x     hist   digit `pass` (8 bits, from the top) of the ratio's order-preserving key, over the pixels whose
//                  higher digits equal the prefix chosen so far: sum of q per digit, q = rint(w_eff 2^e) a uint64.
//                  A lane keeps a (digit, sum) run in registers and adds it to the workgroup's LDS histogram when
//                  the digit changes (64-bit integer LDS atomics); the LDS histogram is flushed once per workgroup
//                  with 64-bit integer global atomics;
//           pick   one workgroup per element scans the 256 sums and picks the first digit at which twice the
//                  cumulative sum reaches the total; the residual is carried as the sum below the prefix.
//
// Every pass recomputes (key, q) from the 13 input bytes of a pixel, 5 x 13 = 65 bytes after the sums.  Materialising
// key and w_eff (8 bytes written once, read four times) would move 13 + 8 + 4 x 8 = 53, a fifth less, for 8 n bytes
// more device memory and a dense write: not taken.
//
// Integer sums only and no floating-point atomic anywhere: the selected ratio is a function of the inputs alone,
// bitwise repeatable, independent of the grid and of the other batch elements.
//
// Layout: an element's n pixels go in groups of four from its first pixel, one group per lane per round.  A group is
// one 128-bit load per float input (one 32-bit load of the mask) when every element's four base addresses allow it
// (float pointers 16-byte, mask 4-byte aligned, bstride a multiple of 4 when B > 1), and four scalar loads
// otherwise; the last group of an element is always partial-safe.  The lane-to-pixel map is the same either way.
//
// Floating-point contraction is off for this file: every operation of the per-pixel arithmetic is rounded to fp32 on
// its own, as the reference's torch ops are.
#include <math.h>

#include "dense_pass.h"

#pragma clang fp contract(off)

namespace {

constexpr int GA_THREADS = 256;
constexpr int GA_WAVES = GA_THREADS / 64;
constexpr int GA_BINS = 256;
constexpr int GA_PASSES = 4;
constexpr int GA_PER_THREAD = 16;   // pixels a lane takes before the grid stops growing
constexpr int GA_MAX_BLOCKS = 1024;  // workgroups per element: one partial record each
constexpr int64_t GA_MAX_N = 100000000;

// state_out: one record per element (VGGT_DEPTH_SCALE_STATE_BYTES)
struct GaState {
  long long cnt;               // set mask pixels
  unsigned long long total;    // sum q
  unsigned long long below;    // sum q over r < r*
  unsigned long long through;  // sum q over r <= r*
  float mean;
  int e;
  unsigned int key;   // the selected ratio's key
  unsigned int wmax;  // bits of the largest finite w_eff
};
static_assert(sizeof(GaState) == VGGT_DEPTH_SCALE_STATE_BYTES, "state layout");

// per-element selection state in ws
struct GaWork {
  unsigned long long below;  // sum q over the keys below the prefix's range
  unsigned long long total;
  unsigned int wmax;    // bits of the largest finite non-negative w_eff
  unsigned int minkey;  // the smallest ratio key
  unsigned int prefix;  // the key's digits chosen so far (lower digits zero)
  float min_depth;
};

struct GaPartial {
  double sum;
  unsigned long long cnt;
  __device__ GaPartial wave() const { return GaPartial{wave_sum(sum), wave_sum(cnt)}; }
  __device__ void add(const GaPartial& o) { sum += o.sum, cnt += o.cnt; }
};

// ws: [B] GaWork | [B * GA_PASSES * GA_BINS] uint64 | [B * GA_MAX_BLOCKS] GaPartial
size_t ga_work_bytes(int B) { return ((size_t)B * sizeof(GaWork) + 15) / 16 * 16; }
size_t ga_hist_bytes(int B) { return (size_t)B * GA_PASSES * GA_BINS * sizeof(unsigned long long); }
size_t ga_partials_bytes(int B) { return (size_t)B * GA_MAX_BLOCKS * sizeof(GaPartial); }

// torch.max(a, b) / clamp_min: a NaN operand gives NaN
__device__ __forceinline__ float ga_max(float a, float b) {
  if (f32_is_nan(a) || f32_is_nan(b)) return __uint_as_float(F32_QNAN);
  return a < b ? b : a;
}

// One pixel (reference :281-295): the ratio and its weight, every operation rounded to fp32 on its own.
struct GaTerm {
  float r, w_eff;
};
__device__ __forceinline__ GaTerm ga_term(float x, float conf, float y, bool m, float min_depth) {
  GaTerm t;
  const float w = ((m ? 1.f : 0.f) * conf) * (1.f / ga_max(ga_max(y, min_depth), 1e-6f));
  const float sign = x < 0.f ? -1.f : 1.f;
  const float x_pos = x * sign;
  t.r = (y * sign) / ga_max(x_pos, 1e-6f);
  t.w_eff = w * x_pos;
  return t;
}
// A weight that is NaN, +-inf or negative counts as 0.
__device__ __forceinline__ bool ga_weight_ok(float w_eff) { return f32_is_finite(w_eff) && !(w_eff < 0.f); }

// e with ldexp(wmax, e) in (2^35, 2^36]; 0 when wmax == 0
__device__ __forceinline__ int ga_exponent(unsigned int wmax_bits) {
  if (wmax_bits == 0) return 0;
  int k;
  const double f = frexp((double)__uint_as_float(wmax_bits), &k);  // wmax = f 2^k, f in [0.5, 1)
  return 36 - k + (f == 0.5 ? 1 : 0);
}
__device__ __forceinline__ unsigned long long ga_q(float w_eff, int e) {
  if (!ga_weight_ok(w_eff)) return 0ull;
  return (unsigned long long)rint(ldexp((double)w_eff, e));
}

struct GaIn {
  const float* pred;
  const float* conf;
  const float* gt;
  const uint8_t* mask;
  int64_t bstride;
  unsigned int n;
};

// ------------------------------------------------------------------------------------------------------ sums
// Workgroup (x, b): record x of element b.
template <bool VEC>
__global__ __launch_bounds__(GA_THREADS) void ga_sums_kernel(GaIn in, GaPartial* __restrict__ partials) {
  __shared__ GaPartial s_part[GA_WAVES];
  const float* gt = in.gt + (int64_t)blockIdx.y * in.bstride;
  const uint8_t* mask = in.mask + (int64_t)blockIdx.y * in.bstride;
  double sum = 0.0;
  unsigned long long cnt = 0;
  const unsigned int stride = 4u * gridDim.x * GA_THREADS;
  for (unsigned int e = 4u * (blockIdx.x * GA_THREADS + threadIdx.x); e < in.n; e += stride) {
    float y[4];
    bool m[4];
    load4<VEC>(gt, e, in.n, y);
    load4_mask<VEC>(mask, e, in.n, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e + j < in.n) {
        sum += (double)(y[j] * (m[j] ? 1.f : 0.f));  // the reference's y * m: an inf or NaN under the mask stays
        cnt += m[j] ? 1u : 0u;
      }
    }
  }
  const GaPartial t = block_reduce_record<GaPartial, GA_WAVES>(GaPartial{sum, cnt}, s_part);
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// One workgroup per element: the records in a fixed order, the mean, and the cleared selection state.
__global__ __launch_bounds__(GA_THREADS) void ga_mean_kernel(const GaPartial* __restrict__ partials, int blocks,
                                                             GaWork* __restrict__ work,
                                                             unsigned long long* __restrict__ hist,
                                                             GaState* __restrict__ state) {
  __shared__ GaPartial s_part[GA_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int i = tid; i < GA_PASSES * GA_BINS; i += GA_THREADS) hist[(size_t)b * GA_PASSES * GA_BINS + i] = 0ull;
  double sum = 0.0;
  unsigned long long cnt = 0;
  for (int i = tid; i < blocks; i += GA_THREADS) {
    const GaPartial t = partials[(size_t)b * blocks + i];
    sum += t.sum, cnt += t.cnt;
  }
  const GaPartial t = block_reduce_record<GaPartial, GA_WAVES>(GaPartial{sum, cnt}, s_part);
  if (tid != 0) return;
  const float mean = (float)(t.sum / (double)(t.cnt < 1 ? 1ull : t.cnt));
  GaWork w;
  w.below = 0, w.total = 0, w.wmax = 0, w.minkey = 0xffffffffu, w.prefix = 0;
  w.min_depth = 0.1f * mean;
  work[b] = w;
  state[b].cnt = (long long)t.cnt;
  state[b].mean = mean;
}

// ------------------------------------------------------------------------------------------------------ wmax
template <bool VEC>
__global__ __launch_bounds__(GA_THREADS) void ga_wmax_kernel(GaIn in, GaWork* __restrict__ work) {
  __shared__ unsigned int s_max[GA_WAVES], s_min[GA_WAVES];
  const int64_t off = (int64_t)blockIdx.y * in.bstride;
  const float *pred = in.pred + off, *conf = in.conf + off, *gt = in.gt + off;
  const uint8_t* mask = in.mask + off;
  const float min_depth = work[blockIdx.y].min_depth;
  unsigned int wmax = 0, minkey = 0xffffffffu;
  const unsigned int stride = 4u * gridDim.x * GA_THREADS;
  for (unsigned int e = 4u * (blockIdx.x * GA_THREADS + threadIdx.x); e < in.n; e += stride) {
    float x[4], c[4], y[4];
    bool m[4];
    load4<VEC>(pred, e, in.n, x);
    load4<VEC>(conf, e, in.n, c);
    load4<VEC>(gt, e, in.n, y);
    load4_mask<VEC>(mask, e, in.n, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e + j < in.n) {
        const GaTerm t = ga_term(x[j], c[j], y[j], m[j], min_depth);
        minkey = min(minkey, f32_key_zeros_equal(t.r));
        // a non-negative finite float's bits order as the floats do; -0 counts as 0
        if (ga_weight_ok(t.w_eff) && t.w_eff > 0.f) wmax = max(wmax, __float_as_uint(t.w_eff));
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wmax = max(wmax, (unsigned int)__shfl_xor((int)wmax, o, 64));
    minkey = min(minkey, (unsigned int)__shfl_xor((int)minkey, o, 64));
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_max[tid >> 6] = wmax, s_min[tid >> 6] = minkey;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < GA_WAVES; ++k) wmax = max(wmax, s_max[k]), minkey = min(minkey, s_min[k]);
    if (wmax) atomicMax(&work[blockIdx.y].wmax, wmax);
    atomicMin(&work[blockIdx.y].minkey, minkey);
  }
}

// ------------------------------------------------------------------------------------------------------ hist
// One pass: sum of q per digit `pass` (from the top) over the pixels whose key matches the element's prefix.
template <bool VEC>
__global__ __launch_bounds__(GA_THREADS) void ga_hist_kernel(GaIn in, int pass, const GaWork* __restrict__ work,
                                                             unsigned long long* __restrict__ hist_all) {
  __shared__ unsigned long long hist[GA_BINS];
  const int tid = threadIdx.x;
  hist[tid] = 0ull;
  const int64_t off = (int64_t)blockIdx.y * in.bstride;
  const float *pred = in.pred + off, *conf = in.conf + off, *gt = in.gt + off;
  const uint8_t* mask = in.mask + off;
  const GaWork wk = work[blockIdx.y];
  const int e2 = ga_exponent(wk.wmax);
  const int shift = 24 - 8 * pass;
  const unsigned int kmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  const unsigned int prefix = pass == 0 ? 0u : wk.prefix;
  __syncthreads();
  // the lane's run: consecutive taken pixels of one digit are summed in registers
  unsigned int run_digit = 0;
  unsigned long long run_sum = 0ull;
  const unsigned int stride = 4u * gridDim.x * GA_THREADS;
  // wmax == 0: every q is 0 and the pick takes the smallest key
  for (unsigned int e = 4u * (blockIdx.x * GA_THREADS + tid); wk.wmax != 0 && e < in.n; e += stride) {
    float x[4], c[4], y[4];
    bool m[4];
    load4<VEC>(pred, e, in.n, x);
    load4<VEC>(conf, e, in.n, c);
    load4<VEC>(gt, e, in.n, y);
    load4_mask<VEC>(mask, e, in.n, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e + j < in.n && m[j]) {  // an unset pixel's weight is +-0 or NaN: q = 0
        const GaTerm t = ga_term(x[j], c[j], y[j], true, wk.min_depth);
        const unsigned int key = f32_key_zeros_equal(t.r);
        if ((key & kmask) == prefix) {
          const unsigned long long q = ga_q(t.w_eff, e2);
          const unsigned int digit = (key >> shift) & (GA_BINS - 1);
          if (q != 0ull) {
            if (digit != run_digit && run_sum != 0ull) {
              atomicAdd(&hist[run_digit], run_sum);
              run_sum = 0ull;
            }
            run_digit = digit;
            run_sum += q;
          }
        }
      }
    }
  }
  if (run_sum != 0ull) atomicAdd(&hist[run_digit], run_sum);
  __syncthreads();
  const unsigned long long s = hist[tid];
  if (s) atomicAdd(&hist_all[((size_t)blockIdx.y * GA_PASSES + pass) * GA_BINS + tid], s);
}

// One workgroup per element: the first digit at which twice the cumulative sum reaches the total.
__global__ __launch_bounds__(GA_BINS) void ga_pick_kernel(const unsigned long long* __restrict__ hist_all, int pass,
                                                          GaWork* __restrict__ work, GaState* __restrict__ state,
                                                          float* __restrict__ scale_out) {
  __shared__ unsigned long long cum[GA_BINS];
  const int tid = threadIdx.x, b = blockIdx.x;
  const unsigned long long own = hist_all[((size_t)b * GA_PASSES + pass) * GA_BINS + tid];
  cum[tid] = own;
  __syncthreads();
  scan256_inclusive(cum, tid);
  const GaWork wk = work[b];
  const unsigned long long total = pass == 0 ? cum[GA_BINS - 1] : wk.total;
  const unsigned long long upto = wk.below + cum[tid], below = upto - own;
  __syncthreads();  // every lane has read the state before one rewrites it
  const bool last = pass == GA_PASSES - 1;
  unsigned int key = 0;
  unsigned long long sel_below = 0, sel_through = 0;
  bool mine = false;
  if (total == 0ull) {
    // the reference's searchsorted(cumsum, 0) on an all-zero cumsum: index 0, the smallest ratio
    mine = tid == 0;
    key = wk.minkey;
    if (mine && pass == 0) work[b].total = 0ull;
  } else if (2ull * below < total && 2ull * upto >= total) {  // exactly one bin; total < 2^63
    mine = true;
    const int shift = 24 - 8 * pass;
    key = wk.prefix | ((unsigned int)tid << shift);
    sel_below = below, sel_through = upto;
    work[b].prefix = key;
    work[b].below = below;
    if (pass == 0) work[b].total = total;
  }
  if (mine && last) {
    const float r = f32_unkey(key);
    scale_out[b] = r <= 0.f ? -r : r;  // reference :312; a NaN stays
    state[b].total = total;
    state[b].below = sel_below;
    state[b].through = sel_through;
    state[b].e = ga_exponent(wk.wmax);
    state[b].key = key;
    state[b].wmax = wk.wmax;
  }
}

template <bool VEC>
int ga_run(const GaIn& in, int B, float* scale_out, GaState* state, GaWork* work, unsigned long long* hist,
           GaPartial* partials, hipStream_t st) {
  const int blocks = grid_for(in.n, GA_THREADS, GA_PER_THREAD, GA_MAX_BLOCKS);
  const dim3 grid((unsigned)blocks, (unsigned)B);
  ga_sums_kernel<VEC><<<grid, GA_THREADS, 0, st>>>(in, partials);
  HIP_LAUNCH_CHECK();
  ga_mean_kernel<<<B, GA_THREADS, 0, st>>>(partials, blocks, work, hist, state);
  HIP_LAUNCH_CHECK();
  ga_wmax_kernel<VEC><<<grid, GA_THREADS, 0, st>>>(in, work);
  HIP_LAUNCH_CHECK();
  for (int pass = 0; pass < GA_PASSES; ++pass) {
    ga_hist_kernel<VEC><<<grid, GA_THREADS, 0, st>>>(in, pass, work, hist);
    HIP_LAUNCH_CHECK();
    ga_pick_kernel<<<B, GA_BINS, 0, st>>>(hist, pass, work, state, scale_out);
    HIP_LAUNCH_CHECK();
  }
  return VGGT_OK;
}

}  // namespace

extern "C" size_t vggt_depth_scale_ws_bytes(int B, int64_t n) {
  if (B < 1 || B > 65535 || n < 1 || n > GA_MAX_N) return 0;
  return ga_work_bytes(B) + ga_hist_bytes(B) + ga_partials_bytes(B);
}

extern "C" int vggt_depth_scale_l1(const float* pred, const float* conf, const float* gt, const void* mask, int B,
                                   int64_t n, int64_t bstride, float* scale_out, void* state_out, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (B < 1 || B > 65535 || n < 1) return VGGT_ERR_SHAPE;
  if (n > GA_MAX_N) return VGGT_ERR_UNSUPPORTED;
  if (B > 1 && bstride < n) return VGGT_ERR_SHAPE;
  if (!pred || !conf || !gt || !mask || !scale_out || !state_out || !ws || (uintptr_t)ws % 16 ||
      ws_bytes < vggt_depth_scale_ws_bytes(B, n))
    return VGGT_ERR_SHAPE;
  if ((uintptr_t)pred % 4 || (uintptr_t)conf % 4 || (uintptr_t)gt % 4 || (uintptr_t)scale_out % 4 ||
      (uintptr_t)state_out % 8)
    return VGGT_ERR_ALIGN;
  GaIn in;
  in.pred = pred, in.conf = conf, in.gt = gt, in.mask = (const uint8_t*)mask;
  in.bstride = B > 1 ? bstride : 0;
  in.n = (unsigned int)n;
  char* base = (char*)ws;
  GaWork* work = (GaWork*)base;
  unsigned long long* hist = (unsigned long long*)(base + ga_work_bytes(B));
  GaPartial* partials = (GaPartial*)(base + ga_work_bytes(B) + ga_hist_bytes(B));
  const bool vec = (uintptr_t)pred % 16 == 0 && (uintptr_t)conf % 16 == 0 && (uintptr_t)gt % 16 == 0 &&
                   (uintptr_t)mask % 4 == 0 && (B == 1 || bstride % 4 == 0);
  hipStream_t st = (hipStream_t)stream;
  return vec ? ga_run<true>(in, B, scale_out, (GaState*)state_out, work, hist, partials, st)
             : ga_run<false>(in, B, scale_out, (GaState*)state_out, work, hist, partials, st);
}
