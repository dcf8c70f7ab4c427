// Training losses: the depth term of the reference's MultitaskLoss (compute_depth_loss and filter_by_quantile,
// training/loss.py:308-351 and :421-457), the one dense computation of a training step's objective.
//
// The reference gathers the masked pixels, takes logs, scales by the per-frame normalised confidence, clamps,
// selects a quantile with torch.kthvalue, filters, scrubs non-finite values and averages; every branch it takes
// on a count visits the host.  Here nothing is gathered and nothing visits the host:
//
//   vggt_depth_loss_values   amax pass   per-frame amax of conf (an integer atomic max on the order-preserving key
//                                        of the float bits: any order gives the same bits; NaN is the largest key,
//                                        as torch.amax propagates it) and n, the number of set mask pixels;
//                            value pass  val = |logf(max(pred, 1e-8)) - logf(max(gt', 1e-8))| * (conf / max(amax,
//                                        1e-8)) at set pixels, the quiet NaN at unset ones.  NaN sorts last in
//                                        torch.kthvalue's order, so a rank <= n over the dense buffer selects what
//                                        the reference selects over its gathered vector.
//   vggt_depth_loss_reduce   rank        k = round_half_even(q (n - 1)) + 1, or 0 where no quantile is taken;
//                            select      vggt_kth_value_f32_devrank (points.hip) over val;
//                            sums        one pass over val: m = #(min(val, 100) < thr'), the filtered sum, the
//                                        clamped sum and the scrubbed sum, fp64, per-lane partials -> a fixed tree
//                                        per workgroup -> one combining workgroup in a fixed order;
//                            pick        the reference's branch, the loss and the state the backward reads.
//   vggt_depth_loss_bwd      one pass that recomputes val from the inputs (the same device function: the same
//                            bits) and applies the state's decision.
//
// Floating-point contraction is off for this file: which pixels pass `< thr'` must not depend on the compiler.
#include <math.h>

#include "dense_pass.h"

#pragma clang fp contract(off)

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_PER_THREAD = 16;         // elements a lane takes before the grid stops growing
constexpr int DL_MAX_BLOCKS = 2048;       // elementwise passes
constexpr int DL_RED_MAX_BLOCKS = 1024;   // the sums: one partial record per workgroup
constexpr int DL_AMAX_CHUNK = DL_THREADS * DL_PER_THREAD;  // pixels of a frame per amax workgroup (at least)
constexpr int DL_AMAX_MAX_CHUNKS = 64;
constexpr int64_t DL_MAX_TOTAL = 100000000;  // past it the reference subsamples at random (loss.py:441)
constexpr float DL_HARD_MAX = 100.f;
constexpr float DL_EPS = 1e-8f;

// the state vggt_depth_loss_reduce leaves for vggt_depth_loss_bwd (VGGT_DEPTH_LOSS_STATE_BYTES)
struct DlState {
  long long n;     // set mask pixels
  long long m;     // of them, min(val, 100) < thr'
  long long k;     // 1-based rank of the quantile, 0: none taken
  long long kind;  // VGGT_DEPTH_LOSS_*
  double denom;    // the mean's denominator (0 when skipped)
  float thr;       // thr' (NaN when k == 0)
  float pad;
};
static_assert(sizeof(DlState) == VGGT_DEPTH_LOSS_STATE_BYTES, "state layout");

struct DlPartial {
  double sum_f, sum_c, sum_u;
  unsigned long long m;
  __device__ DlPartial wave() const { return DlPartial{wave_sum(sum_f), wave_sum(sum_c), wave_sum(sum_u), wave_sum(m)}; }
  __device__ void add(const DlPartial& o) { sum_f += o.sum_f, sum_c += o.sum_c, sum_u += o.sum_u, m += o.m; }
};

// ws: [B * S] amax keys | {rank int64, thr float} | DL_RED_MAX_BLOCKS partial records | the select's ws
size_t dl_keys_bytes(int64_t frames) { return ((size_t)frames * sizeof(unsigned int) + 15) / 16 * 16; }
constexpr size_t DL_SCALARS_BYTES = 16;
constexpr size_t DL_PARTIALS_BYTES = (size_t)DL_RED_MAX_BLOCKS * sizeof(DlPartial);

// torch.clamp_min / clamp(max=): a NaN operand stays NaN
__device__ __forceinline__ float dl_clamp_min(float x, float lo) { return f32_is_nan(x) ? x : (x < lo ? lo : x); }
__device__ __forceinline__ float dl_clamp_max(float x, float hi) { return f32_is_nan(x) ? x : (x > hi ? hi : x); }
// check_and_fix_inf_nan with hard_max = 100: non-finite -> 0, then clamp to +-100
__device__ __forceinline__ double dl_scrub(float x) {
  if (!f32_is_finite(x)) return 0.0;
  return (double)(x > DL_HARD_MAX ? DL_HARD_MAX : (x < -DL_HARD_MAX ? -DL_HARD_MAX : x));
}

// One set pixel: the clamped prediction, the log difference, the normalised confidence and their product's
// absolute value.  Forward and backward both come through here.
struct DlTerm {
  float p, diff, cn, val;
};
__device__ __forceinline__ DlTerm dl_term(float pred, float conf, float gt, float amax) {
  DlTerm t;
  const float g = f32_is_finite(gt) ? gt : 0.f;  // check_and_fix_inf_nan(gt, hard_max=None)
  t.p = dl_clamp_min(pred, DL_EPS);
  t.diff = logf(t.p) - logf(dl_clamp_min(g, DL_EPS));
  t.cn = conf / dl_clamp_min(amax, DL_EPS);
  t.val = fabsf(t.diff) * t.cn;
  return t;
}

// ----------------------------------------------------------------------------------------------- amax and n
// Workgroup (f, c): chunk c of frame f.  The frame's pixels [f hw, (f + 1) hw) split into a scalar head up to the
// first multiple of 4, 128-bit groups, and a scalar tail: hw need not be a multiple of 4.
template <bool VEC>
__global__ __launch_bounds__(DL_THREADS) void dl_amax_kernel(const float* __restrict__ conf,
                                                             const uint8_t* __restrict__ mask, unsigned int hw,
                                                             unsigned int* __restrict__ keys,
                                                             unsigned long long* __restrict__ n_out) {
  __shared__ unsigned int s_key[DL_WAVES], s_cnt[DL_WAVES];
  const int tid = threadIdx.x;
  const unsigned int begin = blockIdx.x * hw, end = begin + hw;
  unsigned int vb = VEC ? (begin + 3u) & ~3u : end;
  if (vb > end) vb = end;
  const unsigned int ve = VEC ? (vb + ((end - vb) & ~3u)) : end;
  unsigned int key = 0, cnt = 0;
  // at most three pixels at either end with VEC (the first lanes of chunk 0), all of them without
  const unsigned int first = blockIdx.y * DL_THREADS + tid, step = gridDim.y * DL_THREADS;
  for (unsigned int e = begin + first; e < vb; e += step) {
    key = max(key, f32_key(conf[e]));
    cnt += mask[e] ? 1u : 0u;
  }
  for (unsigned int e = ve + first; e < end; e += step) {
    key = max(key, f32_key(conf[e]));
    cnt += mask[e] ? 1u : 0u;
  }
  for (unsigned int e = vb + 4u * (blockIdx.y * DL_THREADS + tid); e < ve; e += 4u * gridDim.y * DL_THREADS) {
    const float4 c = *reinterpret_cast<const float4*>(conf + e);
    const unsigned int m = *reinterpret_cast<const unsigned int*>(mask + e);
    key = max(max(key, f32_key(c.x)), max(f32_key(c.y), max(f32_key(c.z), f32_key(c.w))));
    cnt += ((m & 0xffu) ? 1u : 0u) + ((m & 0xff00u) ? 1u : 0u) + ((m & 0xff0000u) ? 1u : 0u) +
           ((m & 0xff000000u) ? 1u : 0u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    key = max(key, (unsigned int)__shfl_xor((int)key, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = key, s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < DL_WAVES; ++k) key = max(key, s_key[k]), cnt += s_cnt[k];
    if (key) atomicMax(&keys[blockIdx.x], key);
    if (cnt) atomicAdd(n_out, (unsigned long long)cnt);
  }
}

// ---------------------------------------------------------------------------------------------------- values
// Frame and offset of element e; the next elements step through dl_next.
struct DlPos {
  unsigned int f, r;
};
__device__ __forceinline__ DlPos dl_pos(unsigned int e, unsigned int hw) {
  DlPos p;
  p.f = e / hw;
  p.r = e - p.f * hw;
  return p;
}
__device__ __forceinline__ void dl_next(DlPos& p, unsigned int hw) {
  if (++p.r == hw) p.r = 0, ++p.f;
}

template <bool VEC>
__global__ __launch_bounds__(DL_THREADS) void dl_values_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ conf,
                                                               const float* __restrict__ gt,
                                                               const uint8_t* __restrict__ mask, unsigned int hw,
                                                               unsigned int total,
                                                               const unsigned int* __restrict__ keys,
                                                               float* __restrict__ val, float* __restrict__ amax) {
  const unsigned int stride = 4u * gridDim.x * DL_THREADS;
  for (unsigned int e = 4u * (blockIdx.x * DL_THREADS + threadIdx.x); e < total; e += stride) {
    float p[4], c[4], g[4], v[4];
    bool m[4];
    load4<VEC>(pred, e, total, p);
    load4<VEC>(conf, e, total, c);
    load4<VEC>(gt, e, total, g);
    load4_mask<VEC>(mask, e, total, m);
    DlPos pos = dl_pos(e, hw);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e + j < total) {
        const float a = f32_unkey(keys[pos.f]);
        if (pos.r == 0) amax[pos.f] = a;
        v[j] = m[j] ? dl_term(p[j], c[j], g[j], a).val : __uint_as_float(F32_QNAN);
        dl_next(pos, hw);
      }
    }
    store4<VEC>(val, e, total, v);
  }
}

// ------------------------------------------------------------------------------------------------------ rank
// Python's round(q * (n - 1)) + 1 (round half to even on the double product), as quantile_rank; 0: no quantile.
__global__ void dl_rank_kernel(const long long* __restrict__ n_in, double q, long long* __restrict__ rank) {
  const long long n = *n_in;
  long long k = 0;
  if (q > 0.0 && n > 1000) k = (long long)rint(q * (double)(n - 1)) + 1;
  *rank = k;
}

// ------------------------------------------------------------------------------------------------------ sums
template <bool VEC>
__global__ __launch_bounds__(DL_THREADS) void dl_sums_kernel(const float* __restrict__ val, unsigned int total,
                                                             const float* __restrict__ thr_in,
                                                             DlPartial* __restrict__ partials) {
  __shared__ DlPartial s_part[DL_WAVES];
  const float thr = dl_clamp_max(*thr_in, DL_HARD_MAX);  // min(thr, 100); a NaN stays and keeps nothing
  double sum_f = 0.0, sum_c = 0.0, sum_u = 0.0;
  unsigned long long m = 0;
  const unsigned int stride = 4u * gridDim.x * DL_THREADS;
  for (unsigned int e = 4u * (blockIdx.x * DL_THREADS + threadIdx.x); e < total; e += stride) {
    float v[4];
    load4<VEC>(val, e, total, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e + j >= total) v[j] = __uint_as_float(F32_QNAN);  // as an unset pixel: no count, no sum
      const float c = dl_clamp_max(v[j], DL_HARD_MAX);
      const double sc = dl_scrub(c);
      if (c < thr) ++m, sum_f += sc;
      sum_c += sc;
      sum_u += dl_scrub(v[j]);
    }
  }
  const DlPartial t = block_reduce_record<DlPartial, DL_WAVES>(DlPartial{sum_f, sum_c, sum_u, m}, s_part);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// One workgroup: the partial records in a fixed order, then the reference's branch.
__global__ __launch_bounds__(DL_THREADS) void dl_pick_kernel(const DlPartial* __restrict__ partials, int blocks,
                                                             const long long* __restrict__ n_in,
                                                             const long long* __restrict__ rank,
                                                             const float* __restrict__ thr_in,
                                                             float* __restrict__ loss, DlState* __restrict__ state) {
  __shared__ DlPartial s_part[DL_WAVES];
  const int tid = threadIdx.x;
  double sum_f = 0.0, sum_c = 0.0, sum_u = 0.0;
  unsigned long long m = 0;
  for (int i = tid; i < blocks; i += DL_THREADS) {
    const DlPartial t = partials[i];
    sum_f += t.sum_f, sum_c += t.sum_c, sum_u += t.sum_u, m += t.m;
  }
  const DlPartial t = block_reduce_record<DlPartial, DL_WAVES>(DlPartial{sum_f, sum_c, sum_u, m}, s_part);
  if (tid != 0) return;
  const long long n = *n_in, k = *rank;
  DlState s;
  s.n = n, s.k = k, s.m = k ? (long long)t.m : 0;
  s.thr = k ? dl_clamp_max(*thr_in, DL_HARD_MAX) : __uint_as_float(F32_QNAN);
  s.pad = 0.f;
  double sum = 0.0;
  if (n < 100) {
    s.kind = VGGT_DEPTH_LOSS_SKIPPED, s.denom = 0.0;
  } else if (k != 0 && s.m > 1000) {
    s.kind = VGGT_DEPTH_LOSS_FILTERED, s.denom = (double)s.m, sum = t.sum_f;
  } else if (k != 0) {
    s.kind = VGGT_DEPTH_LOSS_CLAMPED, s.denom = (double)n, sum = t.sum_c;
  } else {
    s.kind = VGGT_DEPTH_LOSS_UNCLAMPED, s.denom = (double)n, sum = t.sum_u;
  }
  *loss = s.kind == VGGT_DEPTH_LOSS_SKIPPED ? 0.f : (float)(sum / s.denom);
  *state = s;
}

// -------------------------------------------------------------------------------------------------- backward
template <bool VEC>
__global__ __launch_bounds__(DL_THREADS) void dl_bwd_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ conf,
                                                            const float* __restrict__ gt,
                                                            const uint8_t* __restrict__ mask,
                                                            const float* __restrict__ amax,
                                                            const DlState* __restrict__ state,
                                                            const float* __restrict__ gout, unsigned int hw,
                                                            unsigned int total, float* __restrict__ dpred) {
  const long long kind = state->kind;
  const float thr = state->thr, up = *gout, denom = (float)state->denom;
  const unsigned int stride = 4u * gridDim.x * DL_THREADS;
  for (unsigned int e = 4u * (blockIdx.x * DL_THREADS + threadIdx.x); e < total; e += stride) {
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (kind != VGGT_DEPTH_LOSS_SKIPPED) {  // uniform
      float p[4], c[4], g[4];
      bool m[4];
      load4<VEC>(pred, e, total, p);
      load4<VEC>(conf, e, total, c);
      load4<VEC>(gt, e, total, g);
      load4_mask<VEC>(mask, e, total, m);
      DlPos pos = dl_pos(e, hw);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e + j < total) {
          if (m[j]) {
            const DlTerm t = dl_term(p[j], c[j], g[j], amax[pos.f]);
            // the scrub and every clamp pass gradient on [-100, 100] only; the filter keeps val < thr'
            bool on = f32_is_finite(t.val) && t.val <= DL_HARD_MAX && t.val >= -DL_HARD_MAX && p[j] >= DL_EPS;
            if (kind == VGGT_DEPTH_LOSS_FILTERED) on = on && t.val < thr;
            const float sign = t.diff > 0.f ? 1.f : (t.diff < 0.f ? -1.f : 0.f);
            if (on) d[j] = up * sign * t.cn / t.p / denom;
          }
          dl_next(pos, hw);
        }
      }
    }
    store4<VEC>(dpred, e, total, d);
  }
}

bool dl_dims_ok(int B, int S, int H, int W) { return B >= 1 && S >= 1 && H >= 1 && W >= 1; }
int64_t dl_total(int B, int S, int H, int W) { return (int64_t)B * S * H * W; }
bool dl_aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" size_t vggt_depth_loss_ws_bytes(int B, int S, int H, int W) {
  if (!dl_dims_ok(B, S, H, W) || dl_total(B, S, H, W) > DL_MAX_TOTAL) return 0;
  return dl_keys_bytes((int64_t)B * S) + DL_SCALARS_BYTES + DL_PARTIALS_BYTES +
         vggt_kth_value_ws_bytes(dl_total(B, S, H, W));
}

extern "C" int vggt_depth_loss_values(const float* pred, const float* conf, const float* gt, const void* mask, int B,
                                      int S, int H, int W, float* val, float* amax, int64_t* n_out, void* ws,
                                      size_t ws_bytes, void* stream) {
  if (!dl_dims_ok(B, S, H, W)) return VGGT_ERR_SHAPE;
  const int64_t total = dl_total(B, S, H, W), frames = (int64_t)B * S;
  if (total > DL_MAX_TOTAL) return VGGT_ERR_UNSUPPORTED;
  if (!pred || !conf || !gt || !mask || !val || !amax || !n_out || !ws || ws_bytes < dl_keys_bytes(frames))
    return VGGT_ERR_SHAPE;
  if ((uintptr_t)pred % 4 || (uintptr_t)conf % 4 || (uintptr_t)gt % 4 || (uintptr_t)val % 4 || (uintptr_t)amax % 4 ||
      (uintptr_t)n_out % 8 || (uintptr_t)ws % 16)
    return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  unsigned int* keys = (unsigned int*)ws;
  if (hipMemsetAsync(keys, 0, (size_t)frames * sizeof(unsigned int), st) != hipSuccess) return VGGT_ERR_HIP;
  if (hipMemsetAsync(n_out, 0, sizeof(int64_t), st) != hipSuccess) return VGGT_ERR_HIP;
  const unsigned int hw = (unsigned int)((int64_t)H * W);
  const bool vec = dl_aligned16(pred) && dl_aligned16(conf) && dl_aligned16(gt) && dl_aligned16(val) &&
                   (uintptr_t)mask % 4 == 0;
  int chunks = (int)((hw + DL_AMAX_CHUNK - 1) / DL_AMAX_CHUNK);
  chunks = chunks > DL_AMAX_MAX_CHUNKS ? DL_AMAX_MAX_CHUNKS : chunks;
  const dim3 agrid((unsigned)frames, (unsigned)chunks);
  const int blocks = grid_for(total, DL_THREADS, DL_PER_THREAD, DL_MAX_BLOCKS);
  const uint8_t* mk = (const uint8_t*)mask;
  if (vec) {
    dl_amax_kernel<true><<<agrid, DL_THREADS, 0, st>>>(conf, mk, hw, keys, (unsigned long long*)n_out);
    HIP_LAUNCH_CHECK();
    dl_values_kernel<true><<<blocks, DL_THREADS, 0, st>>>(pred, conf, gt, mk, hw, (unsigned int)total, keys, val, amax);
  } else {
    dl_amax_kernel<false><<<agrid, DL_THREADS, 0, st>>>(conf, mk, hw, keys, (unsigned long long*)n_out);
    HIP_LAUNCH_CHECK();
    dl_values_kernel<false><<<blocks, DL_THREADS, 0, st>>>(pred, conf, gt, mk, hw, (unsigned int)total, keys, val, amax);
  }
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_depth_loss_reduce(const float* val, const int64_t* n, int B, int S, int H, int W,
                                      double valid_range, float* loss, void* state, void* ws, size_t ws_bytes,
                                      void* stream) {
  if (!dl_dims_ok(B, S, H, W)) return VGGT_ERR_SHAPE;
  const int64_t total = dl_total(B, S, H, W);
  if (total > DL_MAX_TOTAL) return VGGT_ERR_UNSUPPORTED;
  if (!val || !n || !loss || !state || !ws || ws_bytes < vggt_depth_loss_ws_bytes(B, S, H, W)) return VGGT_ERR_SHAPE;
  if ((uintptr_t)val % 4 || (uintptr_t)n % 8 || (uintptr_t)loss % 4 || (uintptr_t)state % 8 || (uintptr_t)ws % 16)
    return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws + dl_keys_bytes((int64_t)B * S);
  long long* rank = (long long*)base;
  float* thr = (float*)(base + 8);
  DlPartial* partials = (DlPartial*)(base + DL_SCALARS_BYTES);
  void* kth_ws = base + DL_SCALARS_BYTES + DL_PARTIALS_BYTES;
  dl_rank_kernel<<<1, 1, 0, st>>>((const long long*)n, valid_range, rank);
  HIP_LAUNCH_CHECK();
  const int rc = vggt_kth_value_f32_devrank(val, total, (const int64_t*)rank, thr, kth_ws,
                                            vggt_kth_value_ws_bytes(total), stream);
  if (rc != VGGT_OK) return rc;
  const int blocks = grid_for(total, DL_THREADS, DL_PER_THREAD, DL_RED_MAX_BLOCKS);
  if (dl_aligned16(val))
    dl_sums_kernel<true><<<blocks, DL_THREADS, 0, st>>>(val, (unsigned int)total, thr, partials);
  else
    dl_sums_kernel<false><<<blocks, DL_THREADS, 0, st>>>(val, (unsigned int)total, thr, partials);
  HIP_LAUNCH_CHECK();
  dl_pick_kernel<<<1, DL_THREADS, 0, st>>>(partials, blocks, (const long long*)n, rank, thr, loss, (DlState*)state);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_depth_loss_bwd(const float* pred, const float* conf, const float* gt, const void* mask,
                                   const float* amax, const void* state, const float* grad_loss, int B, int S, int H,
                                   int W, float* dpred, void* stream) {
  if (!dl_dims_ok(B, S, H, W)) return VGGT_ERR_SHAPE;
  const int64_t total = dl_total(B, S, H, W);
  if (total > DL_MAX_TOTAL) return VGGT_ERR_UNSUPPORTED;
  if (!pred || !conf || !gt || !mask || !amax || !state || !grad_loss || !dpred) return VGGT_ERR_SHAPE;
  if ((uintptr_t)pred % 4 || (uintptr_t)conf % 4 || (uintptr_t)gt % 4 || (uintptr_t)amax % 4 ||
      (uintptr_t)grad_loss % 4 || (uintptr_t)dpred % 4 || (uintptr_t)state % 8)
    return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const unsigned int hw = (unsigned int)((int64_t)H * W);
  const bool vec = dl_aligned16(pred) && dl_aligned16(conf) && dl_aligned16(gt) && dl_aligned16(dpred) &&
                   (uintptr_t)mask % 4 == 0;
  const int blocks = grid_for(total, DL_THREADS, DL_PER_THREAD, DL_MAX_BLOCKS);
  const uint8_t* mk = (const uint8_t*)mask;
  if (vec)
    dl_bwd_kernel<true><<<blocks, DL_THREADS, 0, st>>>(pred, conf, gt, mk, amax, (const DlState*)state, grad_loss, hw,
                                                       (unsigned int)total, dpred);
  else
    dl_bwd_kernel<false><<<blocks, DL_THREADS, 0, st>>>(pred, conf, gt, mk, amax, (const DlState*)state, grad_loss, hw,
                                                        (unsigned int)total, dpred);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}
