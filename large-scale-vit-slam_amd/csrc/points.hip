// Point-cloud preparation before ICP: the middle of the reference's test-mode reconstruction protocol
// (Metrics.prepare_data_for_metrics, training/training_metrics.py:264-358), between the model's dense outputs and
// iterative_closest_point / ChamferDistanceMetrics (nn.hip).
//
// vggt_kth_value_f32: the exact k-th smallest of n floats (torch.kthvalue's order), radix select on the
//   order-preserving unsigned key of the float bits, four passes of 8 bits from the top.  A pass histograms the
//   digit of every element whose higher digits equal the prefix chosen so far: per-workgroup histogram in LDS
//   (integer LDS atomics; a wave whose lanes all hold one digit adds its lane count once), flushed with integer
//   global atomics into the pass's 256 counters.  A one-workgroup launch then scans the 256 counters, picks the
//   digit that holds the remaining rank, and leaves (prefix, rank) in ws for the next pass; after the fourth it
//   turns the key back into the float.  The host never sees any of it.  Integer sums only: the result is a
//   function of the multiset and two runs are bitwise equal.  vggt_kth_value_f32_devrank is the same select with
//   the rank read from device memory (the depth loss's quantile, loss.hip): only the init kernel differs.
//
// vggt_subsample_mask_count: how many output pixels of the bilinear subsample (F.interpolate, align_corners =
//   False) of a bool mask exceed 0.5: one step of the reference's subsampling-factor search.
//
// vggt_prepare_clouds: select and compact.  A workgroup owns `rows_per_workgroup` consecutive output rows of one
//   batch element; its pixels, in row-major order, go 256 at a time, one per lane.
//     count   every lane decides its pixel's two mask bits (GT; prediction = confidence and GT); a wave ballot
//             per bit is kept in ws (16 bytes per 64 pixels) and the workgroup's two totals go to ws;
//     scan    one workgroup per batch element turns the totals into exclusive offsets, in workgroup order, and
//             writes the two lengths;
//     scatter a lane whose bit is set writes its point at (workgroup offset + bits set in the workgroup's
//             earlier ballot words + bits set below its lane in its own word): the row-major order boolean
//             indexing gives, whatever the launch geometry.  The decisions are the count pass's, read back from
//             ws, never taken twice.
//   Only a selected pixel's taps are unprojected (ray = Kinv (u, v, 1), cam = ray * depth, world = R cam + t, the
//   reference's order); the full-resolution point map is never formed.
//
// Floating-point contraction is off for this file: every product and sum below is rounded on its own, and the
// one fused multiply-add the arithmetic has (the source coordinate, as torch's) is written as fmaf.  No
// contraction choice of the compiler can then move a mask decision or a point's last bit (bl_axis / bl_value
// below, SPEC_ASSUMPTIONS.md).  (HIP's __fmul_rn / __fadd_rn are plain operators and contract like them.)
#include <math.h>

#include "dense_pass.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------ k-th value
constexpr int KTH_THREADS = 256;
constexpr int KTH_BINS = 256;
constexpr int KTH_PASSES = 4;
constexpr int KTH_MAX_BLOCKS = 2048;
constexpr int KTH_PER_THREAD = 16;  // elements a lane takes before the grid stops growing
constexpr int KTH_UNROLL = 4;       // loads in flight per lane

// ws of vggt_kth_value_f32: KTH_PASSES * KTH_BINS 64-bit counters, then the selection state.
struct KthState {
  unsigned long long rank;  // 1-based rank still to find among the elements that match prefix
  unsigned int prefix;      // the key's digits chosen so far (lower digits zero)
  unsigned int pad;
};
constexpr size_t KTH_HIST_BYTES = (size_t)KTH_PASSES * KTH_BINS * sizeof(unsigned long long);
constexpr size_t KTH_WS_BYTES = KTH_HIST_BYTES + sizeof(KthState);

// One pass: the histogram of digit `pass` (from the top) over the elements that match the state's prefix.
__global__ __launch_bounds__(KTH_THREADS) void kth_hist_kernel(const float* __restrict__ x, int64_t n, int pass,
                                                               unsigned long long* __restrict__ hist_all,
                                                               const KthState* __restrict__ state) {
  __shared__ unsigned int hist[KTH_BINS];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  const int shift = 24 - 8 * pass;
  const unsigned int mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
  const unsigned int prefix = pass == 0 ? 0u : state->prefix;
  __syncthreads();
  // whole rounds of gridDim * 256 elements, so that every lane of a wave is in the loop for the ballots
  const int64_t stride = (int64_t)gridDim.x * KTH_THREADS;
  const int64_t rounds = (n + stride - 1) / stride;
  int64_t i = (int64_t)blockIdx.x * KTH_THREADS + tid;
  for (int64_t r = 0; r < rounds; r += KTH_UNROLL, i += KTH_UNROLL * stride) {
    float v[KTH_UNROLL];
#pragma unroll
    for (int u = 0; u < KTH_UNROLL; ++u) v[u] = i + u * stride < n ? x[i + u * stride] : 0.f;  // loads first
#pragma unroll
    for (int u = 0; u < KTH_UNROLL; ++u) radix_digit_add(hist, v[u], prefix, mask, shift, i + u * stride < n);
  }
  __syncthreads();
  const unsigned int c = hist[tid];
  if (c) atomicAdd(&hist_all[(size_t)pass * KTH_BINS + tid], (unsigned long long)c);
}

// Between passes: the digit whose counter range holds the rank, the rank inside it; after the last pass the value.
__global__ __launch_bounds__(KTH_BINS) void kth_pick_kernel(const unsigned long long* __restrict__ hist_all, int pass,
                                                            KthState* __restrict__ state, float* __restrict__ out) {
  __shared__ unsigned long long cum[KTH_BINS];
  const int tid = threadIdx.x;
  const unsigned long long own = hist_all[(size_t)pass * KTH_BINS + tid];
  cum[tid] = own;
  __syncthreads();
  scan256_inclusive(cum, tid);
  const unsigned long long rank = state->rank;
  const unsigned long long upto = cum[tid], below = upto - own;
  __syncthreads();  // every lane has read the rank before one rewrites it
  if (below < rank && rank <= upto) {  // exactly one bin: the counters of a pass sum to at least the rank
    const int shift = 24 - 8 * pass;
    const unsigned int prefix = state->prefix | ((unsigned int)tid << shift);
    state->prefix = prefix;
    state->rank = rank - below;
    if (pass == KTH_PASSES - 1) *out = f32_unkey(prefix);
  }
}

__global__ void kth_init_kernel(KthState* __restrict__ state, unsigned long long k) {
  state->rank = k;
  state->prefix = 0;
  state->pad = 0;
}
// The rank from device memory; outside [1, n] (0: "no quantile") nothing is selected and *out is NaN.
__global__ void kth_init_devrank_kernel(KthState* __restrict__ state, const long long* __restrict__ k, long long n,
                                        float* __restrict__ out) {
  const long long rank = *k;
  const bool ok = rank >= 1 && rank <= n;
  state->rank = ok ? (unsigned long long)rank : 0ull;  // rank 0 falls in no bin: the picks leave *out alone
  state->prefix = 0;
  state->pad = 0;
  if (!ok) *out = __uint_as_float(0x7fc00000u);
}

// The four histogram / pick rounds, after the state is initialised.
int kth_passes(const float* x, int64_t n, float* out, unsigned long long* hist, KthState* state, hipStream_t st) {
  const int blocks = grid_for(n, KTH_THREADS, KTH_PER_THREAD, KTH_MAX_BLOCKS);
  for (int pass = 0; pass < KTH_PASSES; ++pass) {
    kth_hist_kernel<<<blocks, KTH_THREADS, 0, st>>>(x, n, pass, hist, state);
    HIP_LAUNCH_CHECK();
    kth_pick_kernel<<<1, KTH_BINS, 0, st>>>(hist, pass, state, out);
    HIP_LAUNCH_CHECK();
  }
  return VGGT_OK;
}

// ------------------------------------------------------------------------------------------ bilinear subsample
// One axis of F.interpolate(mode="bilinear", align_corners=False): the two taps and their weights of output
// index dst.  scale = (float)in / (float)out; the source coordinate is one fused multiply-add, as torch's is.
struct BlAxis {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ BlAxis bl_axis(int dst, int in, float scale) {
  float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  BlAxis a;
  a.i0 = min((int)src, in - 1);
  a.i1 = min(a.i0 + 1, in - 1);
  const float l = src - (float)a.i0;
  a.l1 = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  a.l0 = 1.f - a.l1;
  return a;
}
// l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d), every product and sum rounded on its own.
__device__ __forceinline__ float bl_value(const BlAxis& h, const BlAxis& w, float a, float b, float c, float d) {
  const float top = w.l0 * a + w.l1 * b;
  const float bot = w.l0 * c + w.l1 * d;
  return h.l0 * top + h.l1 * bot;
}

// Image `img` (H x W), output pixel (ho, wo): the subsampled bool mask.
__device__ __forceinline__ bool sub_mask(const uint8_t* __restrict__ m, int64_t img, int H, int W, const BlAxis& h,
                                         const BlAxis& w) {
  const uint8_t* p = m + img * H * W;
  const float a = p[(int64_t)h.i0 * W + w.i0] ? 1.f : 0.f, b = p[(int64_t)h.i0 * W + w.i1] ? 1.f : 0.f;
  const float c = p[(int64_t)h.i1 * W + w.i0] ? 1.f : 0.f, d = p[(int64_t)h.i1 * W + w.i1] ? 1.f : 0.f;
  return bl_value(h, w, a, b, c, d) > 0.5f;
}
// The subsampled (conf > thr) mask.
__device__ __forceinline__ bool sub_conf(const float* __restrict__ conf, float thr, int64_t img, int H, int W,
                                         const BlAxis& h, const BlAxis& w) {
  const float* p = conf + img * H * W;
  const float a = p[(int64_t)h.i0 * W + w.i0] > thr ? 1.f : 0.f, b = p[(int64_t)h.i0 * W + w.i1] > thr ? 1.f : 0.f;
  const float c = p[(int64_t)h.i1 * W + w.i0] > thr ? 1.f : 0.f, d = p[(int64_t)h.i1 * W + w.i1] > thr ? 1.f : 0.f;
  return bl_value(h, w, a, b, c, d) > 0.5f;
}

constexpr int MC_THREADS = 256;
constexpr int MC_MAX_BLOCKS = 4096;

__global__ __launch_bounds__(MC_THREADS) void mask_count_kernel(const uint8_t* __restrict__ mask, int64_t nimg, int H,
                                                                int W, int Ho, int Wo, float sh, float sw,
                                                                unsigned long long* __restrict__ count) {
  __shared__ unsigned int part[MC_THREADS / 64];
  const int tid = threadIdx.x;
  const bool same = Ho == H && Wo == W;
  const int64_t total = nimg * Ho * Wo;
  unsigned int mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * MC_THREADS + tid; i < total; i += (int64_t)gridDim.x * MC_THREADS) {
    if (same) {
      mine += mask[i] ? 1u : 0u;
    } else {
      const int wo = (int)(i % Wo);
      const int64_t row = i / Wo;
      const int ho = (int)(row % Ho);
      mine += sub_mask(mask, row / Ho, H, W, bl_axis(ho, H, sh), bl_axis(wo, W, sw)) ? 1u : 0u;
    }
  }
  mine = wave_sum(mine);
  if ((tid & 63) == 0) part[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    unsigned int s = 0;
#pragma unroll
    for (int k = 0; k < MC_THREADS / 64; ++k) s += part[k];
    if (s) atomicAdd(count, (unsigned long long)s);
  }
}

// --------------------------------------------------------------------------------------------- prepare clouds
constexpr int PC_THREADS = 256;
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr int PC_AUTO_PIXELS = 4096;  // pixels a workgroup takes when rows_per_workgroup = 0

struct PcGeom {
  int rpw;      // output rows per workgroup
  int wgpb;     // workgroups per batch element
  int chunks;   // 256-pixel chunks per workgroup
};
PcGeom pc_geom(int S, int Ho, int Wo, int rows_per_workgroup) {
  const int64_t rows = (int64_t)S * Ho;
  int64_t rpw = rows_per_workgroup > 0 ? rows_per_workgroup : (PC_AUTO_PIXELS + Wo - 1) / Wo;
  if (rpw > rows) rpw = rows;
  if (rpw < 1) rpw = 1;
  PcGeom g;
  g.rpw = (int)rpw;
  g.wgpb = (int)((rows + rpw - 1) / rpw);
  g.chunks = (int)((rpw * Wo + PC_THREADS - 1) / PC_THREADS);
  return g;
}
// ws: [B * wgpb] {gt, pred} 32-bit totals (offsets after the scan), then [B * wgpb * chunks * PC_WAVES] {gt, pred}
// 64-bit ballot words.
size_t pc_totals_bytes(int B, const PcGeom& g) { return ((size_t)B * g.wgpb * 2 * sizeof(unsigned int) + 15) / 16 * 16; }
size_t pc_words_bytes(int B, const PcGeom& g) {
  return (size_t)B * g.wgpb * g.chunks * PC_WAVES * 2 * sizeof(unsigned long long);
}

struct PcArgs {
  const float* depth;      // (B, S, H, W) or null
  const float* kinv;       // (B, S, 3, 3)
  const float* c2w;        // (B, S, 3, 4)
  const float* pmap;       // (B, S, H, W, 3), used when depth is null
  const float* conf;       // (B, S, H, W)
  const float* thr;        // device scalar
  const float* gt_points;  // (B, S, H, W, 3)
  const uint8_t* gt_mask;  // (B, S, H, W)
  int S, H, W, Ho, Wo;
  float sh, sw;
  int rpw, wgpb, chunks;
};

// Pixel p of workgroup (b, wg): its image, output row and column; false past the workgroup's rows.
__device__ __forceinline__ bool pc_pixel(const PcArgs& a, int b, int wg, int p, int64_t& img, int& ho, int& wo) {
  const int64_t rows = (int64_t)a.S * a.Ho;
  const int64_t row = (int64_t)wg * a.rpw + p / a.Wo;
  if (p >= a.rpw * a.Wo || row >= rows) return false;
  wo = p % a.Wo;
  ho = (int)(row % a.Ho);
  img = (int64_t)b * a.S + row / a.Ho;
  return true;
}

__global__ __launch_bounds__(PC_THREADS) void pc_count_kernel(PcArgs a, unsigned int* __restrict__ totals,
                                                              unsigned long long* __restrict__ words) {
  __shared__ unsigned int part[PC_WAVES][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wg = blockIdx.x, b = blockIdx.y;
  const bool same = a.Ho == a.H && a.Wo == a.W;
  const float thr = *a.thr;
  const size_t wgi = (size_t)b * a.wgpb + wg;
  unsigned int n_gt = 0, n_pred = 0;  // wave-uniform
  for (int c = 0; c < a.chunks; ++c) {
    int64_t img;
    int ho, wo;
    bool gt = false, pred = false;
    if (pc_pixel(a, b, wg, c * PC_THREADS + tid, img, ho, wo)) {
      if (same) {
        const int64_t px = (img * a.H + ho) * a.W + wo;
        gt = a.gt_mask[px] != 0;
        pred = gt && a.conf[px] > thr;
      } else {
        const BlAxis h = bl_axis(ho, a.H, a.sh), w = bl_axis(wo, a.W, a.sw);
        gt = sub_mask(a.gt_mask, img, a.H, a.W, h, w);
        pred = gt && sub_conf(a.conf, thr, img, a.H, a.W, h, w);
      }
    }
    const unsigned long long bg = __ballot(gt), bp = __ballot(pred);
    n_gt += (unsigned int)__popcll(bg);
    n_pred += (unsigned int)__popcll(bp);
    if (lane == 0) {
      unsigned long long* wp = words + ((wgi * a.chunks + c) * PC_WAVES + wave) * 2;
      wp[0] = bg;
      wp[1] = bp;
    }
  }
  if (lane == 0) part[wave][0] = n_gt, part[wave][1] = n_pred;
  __syncthreads();
  if (tid < 2) {
    unsigned int s = 0;
#pragma unroll
    for (int k = 0; k < PC_WAVES; ++k) s += part[k][tid];
    totals[wgi * 2 + tid] = s;
  }
}

// One workgroup per batch element: totals -> exclusive offsets in workgroup order (in place), and the lengths.
__global__ __launch_bounds__(PC_THREADS) void pc_scan_kernel(unsigned int* __restrict__ totals, int wgpb,
                                                             int64_t* __restrict__ gt_len,
                                                             int64_t* __restrict__ pred_len) {
  __shared__ unsigned int sc[2][PC_THREADS];
  const int tid = threadIdx.x, b = blockIdx.x;
  unsigned int* t = totals + (size_t)b * wgpb * 2;
  unsigned int carry0 = 0, carry1 = 0;
  for (int base = 0; base < wgpb; base += PC_THREADS) {
    const int i = base + tid;
    const unsigned int v0 = i < wgpb ? t[2 * i] : 0u, v1 = i < wgpb ? t[2 * i + 1] : 0u;
    sc[0][tid] = v0;
    sc[1][tid] = v1;
    __syncthreads();
    for (int o = 1; o < PC_THREADS; o <<= 1) {
      const unsigned int a0 = tid >= o ? sc[0][tid - o] : 0u, a1 = tid >= o ? sc[1][tid - o] : 0u;
      __syncthreads();
      sc[0][tid] += a0;
      sc[1][tid] += a1;
      __syncthreads();
    }
    if (i < wgpb) {
      t[2 * i] = carry0 + sc[0][tid] - v0;
      t[2 * i + 1] = carry1 + sc[1][tid] - v1;
    }
    carry0 += sc[0][PC_THREADS - 1];
    carry1 += sc[1][PC_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) {
    gt_len[b] = (int64_t)carry0;
    pred_len[b] = (int64_t)carry1;
  }
}

// The predicted point of full-resolution pixel (v, u) of image img.
__device__ __forceinline__ void pc_pred_tap(const PcArgs& a, int64_t img, int v, int u, float (&o)[3]) {
  const int64_t px = (img * a.H + v) * a.W + u;
  if (!a.depth) {
    o[0] = a.pmap[3 * px], o[1] = a.pmap[3 * px + 1], o[2] = a.pmap[3 * px + 2];
    return;
  }
  const float* K = a.kinv + img * 9;
  const float* M = a.c2w + img * 12;
  const float d = a.depth[px], uf = (float)u, vf = (float)v;
  float cam[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float ray = (K[3 * r] * uf + K[3 * r + 1] * vf) + K[3 * r + 2];
    cam[r] = ray * d;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float dot = (M[4 * r] * cam[0] + M[4 * r + 1] * cam[1]) + M[4 * r + 2] * cam[2];
    o[r] = dot + M[4 * r + 3];
  }
}

__global__ __launch_bounds__(PC_THREADS) void pc_scatter_kernel(PcArgs a, const unsigned int* __restrict__ offsets,
                                                                const unsigned long long* __restrict__ words,
                                                                float* __restrict__ pred_cloud, int64_t cap_p,
                                                                float* __restrict__ gt_cloud, int64_t cap_g) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wg = blockIdx.x, b = blockIdx.y;
  const bool same = a.Ho == a.H && a.Wo == a.W;
  const size_t wgi = (size_t)b * a.wgpb + wg;
  int64_t at_gt = offsets[wgi * 2], at_pred = offsets[wgi * 2 + 1];  // rows written before this chunk
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int c = 0; c < a.chunks; ++c) {
    const unsigned long long* wp = words + (wgi * a.chunks + c) * PC_WAVES * 2;
    unsigned long long bg = 0, bp = 0;
    int64_t my_gt = at_gt, my_pred = at_pred;
#pragma unroll
    for (int k = 0; k < PC_WAVES; ++k) {
      const unsigned long long g = wp[2 * k], p = wp[2 * k + 1];
      if (k < wave) my_gt += __popcll(g), my_pred += __popcll(p);
      if (k == wave) bg = g, bp = p;
      at_gt += __popcll(g);
      at_pred += __popcll(p);
    }
    const bool gt = (bg >> lane) & 1, pred = (bp >> lane) & 1;
    if (!gt) continue;  // pred implies gt
    int64_t img;
    int ho, wo;
    if (!pc_pixel(a, b, wg, c * PC_THREADS + tid, img, ho, wo)) continue;
    const int64_t o_gt = my_gt + __popcll(bg & below), o_pred = my_pred + __popcll(bp & below);
    const bool w_gt = o_gt < cap_g, w_pred = pred && o_pred < cap_p;
    float g[3], q[3];
    if (same) {
      const int64_t px = (img * a.H + ho) * a.W + wo;
      g[0] = a.gt_points[3 * px], g[1] = a.gt_points[3 * px + 1], g[2] = a.gt_points[3 * px + 2];
      if (w_pred) pc_pred_tap(a, img, ho, wo, q);
    } else {
      const BlAxis h = bl_axis(ho, a.H, a.sh), w = bl_axis(wo, a.W, a.sw);
      const float* gp = a.gt_points + img * a.H * a.W * 3;
      const int64_t p00 = (int64_t)h.i0 * a.W + w.i0, p01 = (int64_t)h.i0 * a.W + w.i1;
      const int64_t p10 = (int64_t)h.i1 * a.W + w.i0, p11 = (int64_t)h.i1 * a.W + w.i1;
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = bl_value(h, w, gp[3 * p00 + k], gp[3 * p01 + k], gp[3 * p10 + k], gp[3 * p11 + k]);
      if (w_pred) {
        float t00[3], t01[3], t10[3], t11[3];
        pc_pred_tap(a, img, h.i0, w.i0, t00);
        pc_pred_tap(a, img, h.i0, w.i1, t01);
        pc_pred_tap(a, img, h.i1, w.i0, t10);
        pc_pred_tap(a, img, h.i1, w.i1, t11);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = bl_value(h, w, t00[k], t01[k], t10[k], t11[k]);
      }
    }
    if (w_gt) {
      float* o = gt_cloud + ((int64_t)b * cap_g + o_gt) * 3;
      o[0] = g[0], o[1] = g[1], o[2] = g[2];
    }
    if (w_pred) {
      float* o = pred_cloud + ((int64_t)b * cap_p + o_pred) * 3;
      o[0] = q[0], o[1] = q[1], o[2] = q[2];
    }
  }
}

bool pc_dims_ok(int B, int S, int H, int W, int Ho, int Wo) {
  if (B < 1 || B > 65535 || S < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || Ho > H || Wo > W) return false;
  // a batch element's pixels index 32-bit totals; a workgroup's pixel index is an int
  return (int64_t)S * H * W < ((int64_t)1 << 31) - PC_THREADS;
}

}  // namespace

extern "C" size_t vggt_kth_value_ws_bytes(int64_t n) { return n > 0 ? KTH_WS_BYTES : 0; }

extern "C" int vggt_kth_value_f32(const float* x, int64_t n, int64_t k, float* out, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (n < 1 || k < 1 || k > n) return VGGT_ERR_SHAPE;
  if (!x || !out || !ws || ws_bytes < KTH_WS_BYTES) return VGGT_ERR_SHAPE;
  if ((uintptr_t)ws % 8 || (uintptr_t)x % 4 || (uintptr_t)out % 4) return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* hist = (unsigned long long*)ws;
  KthState* state = (KthState*)((char*)ws + KTH_HIST_BYTES);
  if (hipMemsetAsync(hist, 0, KTH_HIST_BYTES, st) != hipSuccess) return VGGT_ERR_HIP;
  kth_init_kernel<<<1, 1, 0, st>>>(state, (unsigned long long)k);
  HIP_LAUNCH_CHECK();
  return kth_passes(x, n, out, hist, state, st);
}

extern "C" int vggt_kth_value_f32_devrank(const float* x, int64_t n, const int64_t* k, float* out, void* ws,
                                          size_t ws_bytes, void* stream) {
  if (n < 1) return VGGT_ERR_SHAPE;
  if (!x || !k || !out || !ws || ws_bytes < KTH_WS_BYTES) return VGGT_ERR_SHAPE;
  if ((uintptr_t)ws % 8 || (uintptr_t)x % 4 || (uintptr_t)out % 4 || (uintptr_t)k % 8) return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* hist = (unsigned long long*)ws;
  KthState* state = (KthState*)((char*)ws + KTH_HIST_BYTES);
  if (hipMemsetAsync(hist, 0, KTH_HIST_BYTES, st) != hipSuccess) return VGGT_ERR_HIP;
  kth_init_devrank_kernel<<<1, 1, 0, st>>>(state, (const long long*)k, (long long)n, out);
  HIP_LAUNCH_CHECK();
  return kth_passes(x, n, out, hist, state, st);
}

extern "C" int vggt_subsample_mask_count(const void* gt_mask, int B, int S, int H, int W, int Ho, int Wo,
                                         int64_t* count_out, void* stream) {
  if (B < 1 || S < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || Ho > H || Wo > W) return VGGT_ERR_SHAPE;
  if (!gt_mask || !count_out) return VGGT_ERR_SHAPE;
  if ((uintptr_t)count_out % 8) return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(count_out, 0, sizeof(int64_t), st) != hipSuccess) return VGGT_ERR_HIP;
  const int64_t nimg = (int64_t)B * S, total = nimg * Ho * Wo;
  const int64_t want = (total + MC_THREADS - 1) / MC_THREADS;
  const int blocks = (int)(want > MC_MAX_BLOCKS ? MC_MAX_BLOCKS : want);
  mask_count_kernel<<<blocks, MC_THREADS, 0, st>>>((const uint8_t*)gt_mask, nimg, H, W, Ho, Wo, (float)H / (float)Ho,
                                                   (float)W / (float)Wo, (unsigned long long*)count_out);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" size_t vggt_prepare_clouds_ws_bytes(int B, int S, int Ho, int Wo, int rows_per_workgroup) {
  if (B < 1 || S < 1 || Ho < 1 || Wo < 1 || rows_per_workgroup < 0) return 0;
  const PcGeom g = pc_geom(S, Ho, Wo, rows_per_workgroup);
  return pc_totals_bytes(B, g) + pc_words_bytes(B, g);
}

extern "C" int vggt_prepare_clouds(const float* depth, const float* kinv, const float* c2w, const float* point_map,
                                   const float* conf, const float* thr, const float* gt_points, const void* gt_mask,
                                   int B, int S, int H, int W, int Ho, int Wo, float* pred_cloud, int64_t cap_p,
                                   float* gt_cloud, int64_t cap_g, int64_t* pred_len, int64_t* gt_len,
                                   int rows_per_workgroup, int phase, void* ws, size_t ws_bytes, void* stream) {
  if (!pc_dims_ok(B, S, H, W, Ho, Wo) || rows_per_workgroup < 0 || cap_p < 0 || cap_g < 0) return VGGT_ERR_SHAPE;
  if (phase < VGGT_PREPARE_ALL || phase > VGGT_PREPARE_SCATTER) return VGGT_ERR_UNSUPPORTED;
  const bool count = phase != VGGT_PREPARE_SCATTER, scatter = phase != VGGT_PREPARE_COUNT;
  if (!conf || !thr || !gt_points || !gt_mask || !(depth ? (kinv && c2w) : point_map != nullptr))
    return VGGT_ERR_SHAPE;
  if (count && (!pred_len || !gt_len)) return VGGT_ERR_SHAPE;
  if (scatter && ((cap_p > 0 && !pred_cloud) || (cap_g > 0 && !gt_cloud))) return VGGT_ERR_SHAPE;
  const PcGeom g = pc_geom(S, Ho, Wo, rows_per_workgroup);
  if (g.wgpb > 0x7fffffff / 2) return VGGT_ERR_SHAPE;
  const size_t tb = pc_totals_bytes(B, g);
  if (!ws || ws_bytes < tb + pc_words_bytes(B, g)) return VGGT_ERR_SHAPE;
  if ((uintptr_t)ws % 8 || (uintptr_t)pred_len % 8 || (uintptr_t)gt_len % 8) return VGGT_ERR_ALIGN;
  PcArgs a;
  a.depth = depth, a.kinv = kinv, a.c2w = c2w, a.pmap = point_map, a.conf = conf, a.thr = thr;
  a.gt_points = gt_points, a.gt_mask = (const uint8_t*)gt_mask;
  a.S = S, a.H = H, a.W = W, a.Ho = Ho, a.Wo = Wo;
  a.sh = (float)H / (float)Ho, a.sw = (float)W / (float)Wo;
  a.rpw = g.rpw, a.wgpb = g.wgpb, a.chunks = g.chunks;
  unsigned int* totals = (unsigned int*)ws;
  unsigned long long* words = (unsigned long long*)((char*)ws + tb);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.wgpb, (unsigned)B);
  if (count) {
    pc_count_kernel<<<grid, PC_THREADS, 0, st>>>(a, totals, words);
    HIP_LAUNCH_CHECK();
    pc_scan_kernel<<<B, PC_THREADS, 0, st>>>(totals, g.wgpb, gt_len, pred_len);
    HIP_LAUNCH_CHECK();
  }
  if (scatter && (cap_p > 0 || cap_g > 0)) {
    pc_scatter_kernel<<<grid, PC_THREADS, 0, st>>>(a, totals, words, pred_cloud, cap_p, gt_cloud, cap_g);
    HIP_LAUNCH_CHECK();
  }
  return VGGT_OK;
}
