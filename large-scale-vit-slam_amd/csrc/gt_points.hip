// GT alignment sim3_from_points on the device: the reference's umeyama_alignment_from_points
// (utils/alignment.py:372-426, called from data.py:144-150) and its umeyama (:6-59), with no host visit.
//
// Per batch element b, over the first P = W H Wimg pixels of that element (W = min(seq_width, S)): pred and gt
// are points (P, 3) fp32, conf is (P,) fp32, mask is (P,) one byte per pixel.  Element b of each tensor starts at
// its own batch stride (the call is [:, :seq_width] of (B, S, ...) tensors, so a stride is S H Wimg >= P, in
// elements of that tensor: floats for conf, floats for the points (>= 3P), bytes for the mask).
//
// Threshold.  thr = np.percentile(conf, q), method "linear", as numpy computes it for a float32 array and a
// Python-float q: every step in fp32, every operation rounded on its own, no fused multiply-add:
//     h  = (float)(P - 1) * ((float)q / 100.0f)
//     lo = min((int64)floorf(h), P - 1)        (h can round above P - 1 once P > 2^24; numpy takes the last there)
//     g  = h - floorf(h)
//     hi = min(lo + 1, P - 1)
//     a  = v[lo], c = v[hi]                    order statistics, 0-based, vggt_kth_value_f32's order
//     d  = c - a
//     thr = a + d * g;  if (g >= 0.5f) thr = c - d * (1.0f - g)
//   h, lo, g and hi depend on P and q alone and are formed on the host; a, c and thr on the device.  If any conf
//   of the prefix is NaN, thr is NaN (numpy: the largest order statistic is then NaN).  The select compares -0
//   and +0 equal (torch.kthvalue's order) and gives a selected zero back as +0; no comparison with thr can tell.
// Selection.  A pixel is kept when mask > 0 && conf >= thr && conf > 1e-5f; n counts them.  X and Y are the kept
//   pred and gt rows in row-major (S, H, W) order, boolean indexing's order.
// Columns.  REFERENCE: sample i is x_i = (Xf[i], Xf[n + i], Xf[2n + i]) with Xf = X.reshape(-1), Y alike: the
//   reference's reshape(3, -1) of an (n, 3) selection, sic.  POINTS: x_i = X[i], the per-point fit of the
//   reference's docstring.
// Umeyama.  Means, sigma_x = E|x - mx|^2 and the centred cross-covariance E[(y - my)(x - mx)^T] in fp64 from
//   the fp32 values, two passes; umeyama3 (small_eig.h) solves; t = my - c R mx; R, t and c are rounded to fp32
//   once.  n = 0: NaN in T[:3] and in the scale (the host route raises inside LAPACK there).  n = 1: sigma_x = 0,
//   so c is 0 / 0 and t is NaN, as the reference's 1 / sigma_x makes them.  An unselected pixel's pred and gt
//   are never read, so a NaN or inf there reaches no sum (skipped, not multiplied by 0: irls_pass1/2's rule).
//
// Launch plan.  A workgroup owns GP_GROUP = 4096 consecutive pixels of one element (grid: ceil(P / 4096) x B, no
// cap), or in the two sum passes 4096 consecutive samples; every count stays on the device.
//   init     the element's histograms and selection state;
//   4 x      hist  digit `pass` of the confidences' keys under the prefix so far (radix_digit_add, dense_pass.h:
//                  LDS histogram, integer atomics; four pixels per lane and round, one 128-bit load when the
//                  base and the stride allow it); pass 0 also counts the NaNs;
//            pick  one workgroup per element takes the digit that holds rank lo + 1; the last one also leaves how
//                  many keys are <= a's;
//   next     when hi > lo and fewer than lo + 2 keys are <= a's: the smallest key above a's (integer atomic min),
//            which is c; otherwise c = a and the pass returns at once;
//   thr      one lane per element forms thr and writes the state record;
//   count    a lane decides one pixel per round; the wave ballots go to ws, the workgroup's total too;
//   scan     one workgroup per element: exclusive offsets in workgroup order, and n;
//   scatter  a kept pixel's pred and gt rows go to row (offset + kept pixels before it in the workgroup) of the
//            element's X and Y: the order of boolean indexing, whatever the launch geometry (points.hip's
//            pc_count / pc_scan / pc_scatter);
//   mean     six fp64 sums over the samples i < n, read through the layout's index function: per-lane partials
//            -> the fixed tree of block_reduce_record -> one record per workgroup; a workgroup past n returns;
//   mean_fin one workgroup per element adds the ceil(n / 4096) records in a fixed order and divides by n;
//   cov      the ten centred sums, the same way;
//   solve    one workgroup per element adds the records; lane 0 solves and writes T, the scale and the state.
// Which lane adds which sample, and the order of every addition, depend on n alone: no floating-point atomic
// anywhere, two runs are bitwise equal, and an element's result does not depend on the rest of the batch.
//
// Floating-point contraction is off for this file: thr's operations are rounded to fp32 one by one.
#include <math.h>

#include "dense_pass.h"
#include "small_eig.h"

#pragma clang fp contract(off)

namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_WAVES = GP_THREADS / 64;
constexpr int GP_BINS = 256;
constexpr int GP_PASSES = 4;
constexpr int GP_GROUP = VGGT_GT_POINTS_GROUP;          // pixels (samples) of one workgroup
constexpr int GP_CHUNKS = GP_GROUP / GP_THREADS;        // rounds of one pixel per lane
constexpr int GP_ROUNDS = GP_GROUP / (4 * GP_THREADS);  // rounds of four pixels per lane (hist, next)
constexpr int64_t GP_MAX_P = ((int64_t)1 << 31) - 256;  // P below this: 32-bit pixel indices and totals
static_assert(GP_BINS == GP_THREADS && GP_GROUP % (4 * GP_THREADS) == 0, "one bin per lane, whole rounds");

// state: one record per element (VGGT_GT_POINTS_STATE_BYTES)
struct GpState {
  long long n;    // kept pixels
  long long nan;  // NaN confidences of the prefix
  float thr, a, c;
  float pad;
};
static_assert(sizeof(GpState) == VGGT_GT_POINTS_STATE_BYTES, "state layout");

// per-element selection state in ws
struct GpWork {
  unsigned long long rank;  // 1-based rank still to find under prefix
  unsigned long long le;    // keys <= a's key (after the last pick)
  unsigned long long nan;
  unsigned long long n;
  unsigned int prefix;  // the key's digits chosen so far; a's key after the last pick
  unsigned int next;    // the smallest key above a's
  float thr;
  float pad;
  double mean[6];  // x, then y
};

template <int N>
struct GpRec {
  double v[N];
  __device__ GpRec wave() const {
    GpRec r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.v[j] = wave_sum(v[j]);
    return r;
  }
  __device__ void add(const GpRec& o) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] += o.v[j];
  }
};
using GpRec10 = GpRec<10>;

size_t gp_align16(size_t v) { return (v + 15) / 16 * 16; }
int64_t gp_groups(int64_t P) { return (P + GP_GROUP - 1) / GP_GROUP; }

// ws: [B] GpWork | [B 4 256] uint64 hist | [B nb] uint32 totals -> offsets | [B nb 16 4] uint64 ballot words |
//     [B nb] GpRec10 | [B 3P] float X | [B 3P] float Y
struct GpLayout {
  size_t work, hist, totals, words, recs, X, Y, end;
};
GpLayout gp_layout(int B, int64_t P) {
  const size_t nb = (size_t)gp_groups(P), b = (size_t)B;
  GpLayout l;
  l.work = 0;
  l.hist = gp_align16(l.work + b * sizeof(GpWork));
  l.totals = gp_align16(l.hist + b * GP_PASSES * GP_BINS * sizeof(unsigned long long));
  l.words = gp_align16(l.totals + b * nb * sizeof(unsigned int));
  l.recs = gp_align16(l.words + b * nb * GP_CHUNKS * GP_WAVES * sizeof(unsigned long long));
  l.X = gp_align16(l.recs + b * nb * sizeof(GpRec10));
  l.Y = gp_align16(l.X + b * 3 * (size_t)P * sizeof(float));
  l.end = gp_align16(l.Y + b * 3 * (size_t)P * sizeof(float));
  return l;
}

struct GpIn {
  const float* pred;
  const float* conf;
  const float* gt;
  const uint8_t* mask;
  int64_t pred_bs, conf_bs, gt_bs, mask_bs;
  unsigned int P;
};

// ------------------------------------------------------------------------------------------------- threshold
__global__ __launch_bounds__(GP_THREADS) void gp_init_kernel(GpWork* __restrict__ work,
                                                             unsigned long long* __restrict__ hist,
                                                             unsigned long long rank) {
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int i = tid; i < GP_PASSES * GP_BINS; i += GP_THREADS) hist[(size_t)b * GP_PASSES * GP_BINS + i] = 0ull;
  if (tid != 0) return;
  GpWork w;
  w.rank = rank, w.le = 0, w.nan = 0, w.n = 0;
  w.prefix = 0, w.next = 0xffffffffu;
  w.thr = 0.f, w.pad = 0.f;
  for (int j = 0; j < 6; ++j) w.mean[j] = 0.0;
  work[b] = w;
}

// One pass: the histogram of digit `pass` (from the top) over the element's confidences that match its prefix.
template <bool VEC>
__global__ __launch_bounds__(GP_THREADS) void gp_hist_kernel(const float* __restrict__ conf_all, int64_t conf_bs,
                                                             unsigned int P, int pass, GpWork* __restrict__ work,
                                                             unsigned long long* __restrict__ hist_all) {
  __shared__ unsigned int hist[GP_BINS];
  __shared__ unsigned int s_nan[GP_WAVES];
  const int tid = threadIdx.x, b = blockIdx.y;
  hist[tid] = 0;
  const float* conf = conf_all + (int64_t)b * conf_bs;
  const int shift = 24 - 8 * pass;
  const unsigned int kmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  const unsigned int prefix = pass == 0 ? 0u : work[b].prefix;
  __syncthreads();
  unsigned int nan = 0;
  const unsigned int base = blockIdx.x * (unsigned int)GP_GROUP;
#pragma unroll
  for (int r = 0; r < GP_ROUNDS; ++r) {  // every lane of a wave stays in the loop for the ballots
    const unsigned int e = base + 4u * (unsigned int)(r * GP_THREADS + tid);
    float v[4];
    if (e < P) load4<VEC>(conf, e, P, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = e + j < P;
      const float x = in ? v[j] : 0.f;
      radix_digit_add(hist, x, prefix, kmask, shift, in);
      nan += in && f32_is_nan(x) ? 1u : 0u;
    }
  }
  if (pass == 0) {
    nan = wave_sum(nan);
    if ((tid & 63) == 0) s_nan[tid >> 6] = nan;
  }
  __syncthreads();
  const unsigned int c = hist[tid];
  if (c) atomicAdd(&hist_all[((size_t)b * GP_PASSES + pass) * GP_BINS + tid], (unsigned long long)c);
  if (pass == 0 && tid == 0) {
    unsigned int s = 0;
#pragma unroll
    for (int k = 0; k < GP_WAVES; ++k) s += s_nan[k];
    if (s) atomicAdd(&work[b].nan, (unsigned long long)s);
  }
}

// One workgroup per element: the digit whose counter range holds the rank, and the rank inside it.
__global__ __launch_bounds__(GP_BINS) void gp_pick_kernel(const unsigned long long* __restrict__ hist_all, int pass,
                                                          GpWork* __restrict__ work, unsigned long long rank0) {
  __shared__ unsigned long long cum[GP_BINS];
  const int tid = threadIdx.x, b = blockIdx.x;
  const unsigned long long own = hist_all[((size_t)b * GP_PASSES + pass) * GP_BINS + tid];
  cum[tid] = own;
  __syncthreads();
  scan256_inclusive(cum, tid);
  const unsigned long long rank = work[b].rank;
  const unsigned int prefix = work[b].prefix;
  const unsigned long long upto = cum[tid], below = upto - own;
  __syncthreads();  // every lane has read the state before one rewrites it
  if (below < rank && rank <= upto) {  // exactly one bin: the counters of a pass sum to at least the rank
    work[b].prefix = prefix | ((unsigned int)tid << (24 - 8 * pass));
    work[b].rank = rank - below;
    if (pass == GP_PASSES - 1) work[b].le = rank0 - (rank - below) + own;  // keys below a's, then a's own
  }
}

// c when it is not a: the smallest key above a's.
template <bool VEC>
__global__ __launch_bounds__(GP_THREADS) void gp_next_kernel(const float* __restrict__ conf_all, int64_t conf_bs,
                                                             unsigned int P, GpWork* __restrict__ work,
                                                             unsigned long long rank0) {
  __shared__ unsigned int s_min[GP_WAVES];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (work[b].le > rank0) return;  // rank lo + 2 holds a's key too
  const float* conf = conf_all + (int64_t)b * conf_bs;
  const unsigned int akey = work[b].prefix;
  unsigned int mn = 0xffffffffu;
  const unsigned int base = blockIdx.x * (unsigned int)GP_GROUP;
#pragma unroll
  for (int r = 0; r < GP_ROUNDS; ++r) {
    const unsigned int e = base + 4u * (unsigned int)(r * GP_THREADS + tid);
    if (e >= P) continue;
    float v[4];
    load4<VEC>(conf, e, P, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned int key = f32_key_zeros_equal(v[j]);
      if (e + j < P && key > akey) mn = min(mn, key);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = min(mn, (unsigned int)__shfl_xor((int)mn, o, 64));
  if ((tid & 63) == 0) s_min[tid >> 6] = mn;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < GP_WAVES; ++k) mn = min(mn, s_min[k]);
    if (mn != 0xffffffffu) atomicMin(&work[b].next, mn);
  }
}

// One lane per element: numpy's _lerp of the two order statistics.
__global__ void gp_thr_kernel(GpWork* __restrict__ work, GpState* __restrict__ state, int B, float g, int two,
                              unsigned long long rank0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const GpWork w = work[b];
  const float a = f32_unkey(w.prefix);
  const float c = (two && w.le <= rank0) ? f32_unkey(w.next) : a;
  const float d = c - a;
  float thr = a + d * g;
  if (g >= 0.5f) thr = c - d * (1.0f - g);
  if (w.nan) thr = __uint_as_float(F32_QNAN);
  work[b].thr = thr;
  GpState s;
  s.n = 0, s.nan = (long long)w.nan;
  s.thr = thr, s.a = a, s.c = c, s.pad = 0.f;
  state[b] = s;
}

// ------------------------------------------------------------------------------------- select and compact
__global__ __launch_bounds__(GP_THREADS) void gp_count_kernel(GpIn in, const GpWork* __restrict__ work,
                                                              unsigned int* __restrict__ totals,
                                                              unsigned long long* __restrict__ words) {
  __shared__ unsigned int part[GP_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y;
  const float* conf = in.conf + (int64_t)b * in.conf_bs;
  const uint8_t* mask = in.mask + (int64_t)b * in.mask_bs;
  const float thr = work[b].thr;
  const size_t wgi = (size_t)b * gridDim.x + blockIdx.x;
  const unsigned int base = blockIdx.x * (unsigned int)GP_GROUP;
  unsigned int kept = 0;  // wave-uniform
#pragma unroll 4
  for (int c = 0; c < GP_CHUNKS; ++c) {
    const unsigned int px = base + (unsigned int)(c * GP_THREADS + tid);
    bool keep = false;
    if (px < in.P) {
      const float v = conf[px];
      keep = mask[px] != 0 && v >= thr && v > 1e-5f;  // a NaN thr or conf keeps nothing
    }
    const unsigned long long bits = __ballot(keep);
    kept += (unsigned int)__popcll(bits);
    if (lane == 0) words[(wgi * GP_CHUNKS + c) * GP_WAVES + wave] = bits;
  }
  if (lane == 0) part[wave] = kept;
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
#pragma unroll
    for (int k = 0; k < GP_WAVES; ++k) s += part[k];
    totals[wgi] = s;
  }
}

// One workgroup per element: totals -> exclusive offsets in workgroup order (in place), and n.
__global__ __launch_bounds__(GP_THREADS) void gp_scan_kernel(unsigned int* __restrict__ totals, int nb,
                                                             GpWork* __restrict__ work, GpState* __restrict__ state) {
  __shared__ unsigned int sc[GP_THREADS];
  const int tid = threadIdx.x, b = blockIdx.x;
  unsigned int* t = totals + (size_t)b * nb;
  unsigned int carry = 0;
  for (int base = 0; base < nb; base += GP_THREADS) {
    const int i = base + tid;
    const unsigned int v = i < nb ? t[i] : 0u;
    sc[tid] = v;
    __syncthreads();
    for (int o = 1; o < GP_THREADS; o <<= 1) {
      const unsigned int a = tid >= o ? sc[tid - o] : 0u;
      __syncthreads();
      sc[tid] += a;
      __syncthreads();
    }
    if (i < nb) t[i] = carry + sc[tid] - v;
    carry += sc[GP_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) {
    work[b].n = carry;
    state[b].n = (long long)carry;
  }
}

__global__ __launch_bounds__(GP_THREADS) void gp_scatter_kernel(GpIn in, const unsigned int* __restrict__ offsets,
                                                                const unsigned long long* __restrict__ words,
                                                                float* __restrict__ X_all, float* __restrict__ Y_all) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y;
  const float* pred = in.pred + (int64_t)b * in.pred_bs;
  const float* gt = in.gt + (int64_t)b * in.gt_bs;
  float* X = X_all + (size_t)b * 3 * in.P;
  float* Y = Y_all + (size_t)b * 3 * in.P;
  const size_t wgi = (size_t)b * gridDim.x + blockIdx.x;
  const unsigned int base = blockIdx.x * (unsigned int)GP_GROUP;
  unsigned int at = offsets[wgi];  // rows written before this chunk
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int c = 0; c < GP_CHUNKS; ++c) {
    const unsigned long long* wp = words + (wgi * GP_CHUNKS + c) * GP_WAVES;
    unsigned long long mine = 0;
    unsigned int my_at = at;
#pragma unroll
    for (int k = 0; k < GP_WAVES; ++k) {
      const unsigned long long w = wp[k];
      if (k < wave) my_at += (unsigned int)__popcll(w);
      if (k == wave) mine = w;
      at += (unsigned int)__popcll(w);
    }
    if (!((mine >> lane) & 1)) continue;  // a set bit's pixel is below P, and its row below n <= P
    const size_t px = (size_t)base + (size_t)(c * GP_THREADS + tid);
    const size_t o = (size_t)my_at + (size_t)__popcll(mine & below);
    X[3 * o] = pred[3 * px], X[3 * o + 1] = pred[3 * px + 1], X[3 * o + 2] = pred[3 * px + 2];
    Y[3 * o] = gt[3 * px], Y[3 * o + 1] = gt[3 * px + 1], Y[3 * o + 2] = gt[3 * px + 2];
  }
}

// ---------------------------------------------------------------------------------------------------- sums
// Component k of sample i of an element's compacted rows.
template <int COLS>
__device__ __forceinline__ float gp_at(const float* __restrict__ Xf, size_t n, size_t i, int k) {
  return COLS == VGGT_GT_POINTS_REFERENCE ? Xf[(size_t)k * n + i] : Xf[3 * i + k];
}

template <int COLS>
__global__ __launch_bounds__(GP_THREADS) void gp_mean_kernel(const float* __restrict__ X_all,
                                                             const float* __restrict__ Y_all, unsigned int P,
                                                             const GpWork* __restrict__ work,
                                                             GpRec10* __restrict__ recs) {
  __shared__ GpRec<6> s_part[GP_WAVES];
  const int b = blockIdx.y;
  const size_t n = (size_t)work[b].n;
  const size_t base = (size_t)blockIdx.x * GP_GROUP;
  if (base >= n) return;  // workgroup-uniform; mean_fin reads ceil(n / GP_GROUP) records
  const float* X = X_all + (size_t)b * 3 * P;
  const float* Y = Y_all + (size_t)b * 3 * P;
  GpRec<6> acc;
#pragma unroll
  for (int j = 0; j < 6; ++j) acc.v[j] = 0.0;
#pragma unroll 4
  for (int c = 0; c < GP_CHUNKS; ++c) {
    const size_t i = base + (size_t)(c * GP_THREADS + (int)threadIdx.x);
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        acc.v[k] += (double)gp_at<COLS>(X, n, i, k);
        acc.v[3 + k] += (double)gp_at<COLS>(Y, n, i, k);
      }
    }
  }
  const GpRec<6> t = block_reduce_record<GpRec<6>, GP_WAVES>(acc, s_part);
  if (threadIdx.x == 0) {
    GpRec10* o = recs + (size_t)b * gridDim.x + blockIdx.x;
#pragma unroll
    for (int j = 0; j < 6; ++j) o->v[j] = t.v[j];
  }
}

// The first `count` records of element b, lane-strided, then the workgroup's fixed tree.
template <int N>
__device__ __forceinline__ GpRec<N> gp_combine(const GpRec10* __restrict__ recs, size_t count, GpRec<N>* s_part) {
  GpRec<N> acc;
#pragma unroll
  for (int j = 0; j < N; ++j) acc.v[j] = 0.0;
  for (size_t i = threadIdx.x; i < count; i += GP_THREADS) {
#pragma unroll
    for (int j = 0; j < N; ++j) acc.v[j] += recs[i].v[j];
  }
  return block_reduce_record<GpRec<N>, GP_WAVES>(acc, s_part);
}

__global__ __launch_bounds__(GP_THREADS) void gp_mean_fin_kernel(const GpRec10* __restrict__ recs, int nb,
                                                                 GpWork* __restrict__ work) {
  __shared__ GpRec<6> s_part[GP_WAVES];
  const int b = blockIdx.x;
  const size_t n = (size_t)work[b].n;
  const GpRec<6> t = gp_combine<6>(recs + (size_t)b * nb, (n + GP_GROUP - 1) / GP_GROUP, s_part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) work[b].mean[j] = t.v[j] / (double)n;  // n == 0: NaN
  }
}

template <int COLS>
__global__ __launch_bounds__(GP_THREADS) void gp_cov_kernel(const float* __restrict__ X_all,
                                                            const float* __restrict__ Y_all, unsigned int P,
                                                            const GpWork* __restrict__ work,
                                                            GpRec10* __restrict__ recs) {
  __shared__ GpRec10 s_part[GP_WAVES];
  const int b = blockIdx.y;
  const size_t n = (size_t)work[b].n;
  const size_t base = (size_t)blockIdx.x * GP_GROUP;
  if (base >= n) return;
  const float* X = X_all + (size_t)b * 3 * P;
  const float* Y = Y_all + (size_t)b * 3 * P;
  double mean[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) mean[j] = work[b].mean[j];
  GpRec10 acc;
#pragma unroll
  for (int j = 0; j < 10; ++j) acc.v[j] = 0.0;
#pragma unroll 2
  for (int c = 0; c < GP_CHUNKS; ++c) {
    const size_t i = base + (size_t)(c * GP_THREADS + (int)threadIdx.x);
    if (i < n) {
      double x[3], y[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[k] = (double)gp_at<COLS>(X, n, i, k) - mean[k];
        y[k] = (double)gp_at<COLS>(Y, n, i, k) - mean[3 + k];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc.v[3 * r + k] += y[r] * x[k];
      acc.v[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    }
  }
  const GpRec10 t = block_reduce_record<GpRec10, GP_WAVES>(acc, s_part);
  if (threadIdx.x == 0) recs[(size_t)b * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(GP_THREADS) void gp_solve_kernel(const GpRec10* __restrict__ recs, int nb,
                                                              const GpWork* __restrict__ work, float* __restrict__ T,
                                                              float* __restrict__ scale) {
  __shared__ GpRec10 s_part[GP_WAVES];
  const int b = blockIdx.x;
  const size_t n = (size_t)work[b].n;
  const GpRec10 t = gp_combine<10>(recs + (size_t)b * nb, (n + GP_GROUP - 1) / GP_GROUP, s_part);
  if (threadIdx.x != 0) return;
  float* to = T + (size_t)b * 16;
  to[12] = 0.f, to[13] = 0.f, to[14] = 0.f, to[15] = 1.f;
  if (n == 0) {
    const float nanv = __uint_as_float(F32_QNAN);
    for (int i = 0; i < 12; ++i) to[i] = nanv;
    scale[b] = nanv;
    return;
  }
  double Sg[3][3], R[3][3], c, mean[6];
  for (int j = 0; j < 6; ++j) mean[j] = work[b].mean[j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Sg[i][j] = t.v[3 * i + j] / (double)n;
  umeyama3(Sg, t.v[9] / (double)n, R, &c);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) to[i * 4 + j] = (float)R[i][j];
    to[i * 4 + 3] = (float)(mean[3 + i] - c * ((R[i][0] * mean[0] + R[i][1] * mean[1]) + R[i][2] * mean[2]));
  }
  scale[b] = (float)c;
}

template <bool VEC>
int gp_threshold(const GpIn& in, int B, int nb, unsigned long long rank0, bool two, float g, GpWork* work,
                 unsigned long long* hist, GpState* state, hipStream_t st) {
  const dim3 grid((unsigned)nb, (unsigned)B);
  gp_init_kernel<<<B, GP_THREADS, 0, st>>>(work, hist, rank0);
  HIP_LAUNCH_CHECK();
  for (int pass = 0; pass < GP_PASSES; ++pass) {
    gp_hist_kernel<VEC><<<grid, GP_THREADS, 0, st>>>(in.conf, in.conf_bs, in.P, pass, work, hist);
    HIP_LAUNCH_CHECK();
    gp_pick_kernel<<<B, GP_BINS, 0, st>>>(hist, pass, work, rank0);
    HIP_LAUNCH_CHECK();
  }
  if (two) {
    gp_next_kernel<VEC><<<grid, GP_THREADS, 0, st>>>(in.conf, in.conf_bs, in.P, work, rank0);
    HIP_LAUNCH_CHECK();
  }
  gp_thr_kernel<<<(B + 63) / 64, 64, 0, st>>>(work, state, B, g, two ? 1 : 0, rank0);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

template <int COLS>
int gp_sums(const float* X, const float* Y, unsigned int P, int B, int nb, GpWork* work, GpRec10* recs, float* T,
            float* scale, hipStream_t st) {
  const dim3 grid((unsigned)nb, (unsigned)B);
  gp_mean_kernel<COLS><<<grid, GP_THREADS, 0, st>>>(X, Y, P, work, recs);
  HIP_LAUNCH_CHECK();
  gp_mean_fin_kernel<<<B, GP_THREADS, 0, st>>>(recs, nb, work);
  HIP_LAUNCH_CHECK();
  gp_cov_kernel<COLS><<<grid, GP_THREADS, 0, st>>>(X, Y, P, work, recs);
  HIP_LAUNCH_CHECK();
  gp_solve_kernel<<<B, GP_THREADS, 0, st>>>(recs, nb, work, T, scale);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

}  // namespace

extern "C" size_t vggt_gt_points_align_ws_bytes(int B, int64_t P) {
  if (B < 1 || B > 65535 || P < 1 || P >= GP_MAX_P) return 0;
  return gp_layout(B, P).end;
}

extern "C" int vggt_gt_points_align(const float* pred, int64_t pred_bs, const float* conf, int64_t conf_bs,
                                    const float* gt, int64_t gt_bs, const void* mask, int64_t mask_bs, int B,
                                    int64_t P, float q, int columns, float* T, float* scale, void* state, void* ws,
                                    size_t ws_bytes, void* stream) {
  if (B < 1 || B > 65535 || P < 1 || P >= GP_MAX_P) return VGGT_ERR_SHAPE;
  if (B > 1 && (pred_bs < 3 * P || gt_bs < 3 * P || conf_bs < P || mask_bs < P)) return VGGT_ERR_SHAPE;
  if (!(q >= 0.f && q <= 100.f)) return VGGT_ERR_SHAPE;
  if (!pred || !conf || !gt || !mask || !T || !scale || !state || !ws || (uintptr_t)ws % 16 ||
      ws_bytes < vggt_gt_points_align_ws_bytes(B, P))
    return VGGT_ERR_SHAPE;
  if (columns != VGGT_GT_POINTS_REFERENCE && columns != VGGT_GT_POINTS_POINTS) return VGGT_ERR_UNSUPPORTED;
  if ((uintptr_t)pred % 4 || (uintptr_t)conf % 4 || (uintptr_t)gt % 4 || (uintptr_t)T % 4 || (uintptr_t)scale % 4 ||
      (uintptr_t)state % 8)
    return VGGT_ERR_ALIGN;
  // numpy's virtual index of the percentile, in fp32
  const float h = (float)(P - 1) * (q / 100.0f);
  const float fl = floorf(h);
  int64_t lo = (int64_t)fl;
  if (lo > P - 1) lo = P - 1;
  const float g = h - fl;
  const int64_t hi = lo + 1 < P - 1 ? lo + 1 : P - 1;
  GpIn in;
  in.pred = pred, in.conf = conf, in.gt = gt, in.mask = (const uint8_t*)mask;
  in.pred_bs = B > 1 ? pred_bs : 0, in.conf_bs = B > 1 ? conf_bs : 0;
  in.gt_bs = B > 1 ? gt_bs : 0, in.mask_bs = B > 1 ? mask_bs : 0;
  in.P = (unsigned int)P;
  const GpLayout l = gp_layout(B, P);
  char* base = (char*)ws;
  GpWork* work = (GpWork*)(base + l.work);
  unsigned long long* hist = (unsigned long long*)(base + l.hist);
  unsigned int* totals = (unsigned int*)(base + l.totals);
  unsigned long long* words = (unsigned long long*)(base + l.words);
  GpRec10* recs = (GpRec10*)(base + l.recs);
  float* X = (float*)(base + l.X);
  float* Y = (float*)(base + l.Y);
  const int nb = (int)gp_groups(P);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (uintptr_t)conf % 16 == 0 && (B == 1 || conf_bs % 4 == 0);
  const unsigned long long rank0 = (unsigned long long)lo + 1;
  int rc = vec ? gp_threshold<true>(in, B, nb, rank0, hi != lo, g, work, hist, (GpState*)state, st)
               : gp_threshold<false>(in, B, nb, rank0, hi != lo, g, work, hist, (GpState*)state, st);
  if (rc != VGGT_OK) return rc;
  const dim3 grid((unsigned)nb, (unsigned)B);
  gp_count_kernel<<<grid, GP_THREADS, 0, st>>>(in, work, totals, words);
  HIP_LAUNCH_CHECK();
  gp_scan_kernel<<<B, GP_THREADS, 0, st>>>(totals, nb, work, (GpState*)state);
  HIP_LAUNCH_CHECK();
  gp_scatter_kernel<<<grid, GP_THREADS, 0, st>>>(in, totals, words, X, Y);
  HIP_LAUNCH_CHECK();
  return columns == VGGT_GT_POINTS_REFERENCE
             ? gp_sums<VGGT_GT_POINTS_REFERENCE>(X, Y, in.P, B, nb, work, recs, T, scale, st)
             : gp_sums<VGGT_GT_POINTS_POINTS>(X, Y, in.P, B, nb, work, recs, T, scale, st);
}
