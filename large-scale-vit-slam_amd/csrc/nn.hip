// Exact batched 1-nearest-neighbour search in 3-D (fp32) and the per-iteration
// sums of rigid ICP (vggt_nn1, vggt_nn1_plan, vggt_nn1_workspace_bytes,
// vggt_nn1_pair_stats): the reconstruction half of the evaluation protocol
// (eval/reconstruction_metrics.py ChamferDistanceMetrics and the
// iterative_closest_point call of eval/training_metrics.py:343-364), which the
// reference runs through PyTorch3D's knn_points(K=1).
//
// vggt_nn1, brute force, exact for any input:
//   * a workgroup of 256 lanes owns 1024 query points, four per lane, held in
//     registers as two packed pairs (the differences, the square and the two
//     FMAs of a pair issue as v_pk_* instructions);
//   * the reference cloud streams through LDS in tiles of 1024 points kept in
//     their global x,y,z order (12 bytes a point), double buffered: the next
//     tile's global loads are issued before the current tile is searched and
//     written to the other buffer after it, one barrier per tile.  Slots past
//     the reference length are filled with NaN, which never compares below;
//   * every lane reads the same reference point at the same time (a
//     wave-uniform LDS address: one broadcast read serves 256 pairs), forms
//     the distance from coordinate differences -- never |q|^2+|r|^2-2q.r, which
//     cancels to nothing for clouds far from the origin.  The running minimum
//     is kept per group of 16 reference points (fminf, which drops a NaN
//     operand; the compiler folds two into one v_min3_f32) and a strict `<`
//     with two selects keeps (best, first group that reached it) once per
//     group instead of once per point: 3/16 select instructions a pair in
//     place of 3.  After the last tile each query recomputes its winning
//     group's 16 distances with the same arithmetic and takes the first strict
//     minimum, so ties keep the smallest index and a NaN distance is never
//     taken;
//   * when the query blocks alone cannot fill the device the reference range
//     is cut into `split` parts of whole tiles (grid.y); each part merges its
//     result with a 64-bit unsigned atomicMin on (dist bits << 32 | index) in
//     ws -- distances are >= +0, so their bits order as unsigned and the low
//     word gives the smallest-index tie-break -- and a small second launch
//     unpacks.  min over (dist, index) is associative and commutative: the
//     result is bitwise the unsplit one for any split and any arrival order.
//     No floating-point atomics.
//
// vggt_nn1_pair_stats: fp64 sums over the matched pairs in a fixed order
// (per-lane strided partials, a fixed shuffle tree, per-workgroup partials in
// ws, one final pass in workgroup order): two runs are bitwise equal.
#include <math.h>

#include "common.h"

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_QPT = 4;                    // query points per lane
constexpr int NN_QB = NN_THREADS * NN_QPT;   // query points per workgroup
constexpr int NN_TILE = 1024;                // reference points per LDS tile
constexpr int NN_GROUP = 16;                 // reference points per minimum group (divides NN_TILE)
constexpr int NN_SLOTS_PER_CU = 4;          // resident workgroups per compute unit the plan fills
constexpr int NN_ROUNDS = 4;                 // rounds of slots the plan wants before it stops splitting
constexpr int NN_MAX_SPLIT = 4096;
constexpr int PS_THREADS = 256;
constexpr int PS_MAX_BLOCKS = 256;
constexpr int PS_VALS = 17;

__device__ __forceinline__ int64_t clamp_len(const int64_t* len, int b, int64_t cap) {
  if (!len) return cap;
  const int64_t v = len[b];
  return v < 0 ? 0 : (v > cap ? cap : v);
}

// Global -> registers: this lane's 12 floats of the tile starting at point `base` (float k * 256 + tid of the
// tile's 3072); floats at or past point r_end read nothing and become NaN.
__device__ __forceinline__ void nn_tile_load(float (&st)[12], const float* __restrict__ rb, int64_t base, int64_t r_end,
                                             int tid) {
  const int64_t lim = (r_end - base) * 3;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int f = k * NN_THREADS + tid;
    st[k] = f < lim ? rb[base * 3 + f] : __builtin_nanf("");
  }
}

// The distance of two queries (packed) to one reference point, from coordinate differences.  The search and the
// index resolution both call this, so the value a group's minimum was built from is met again bit for bit.
template <int NORM>
__device__ __forceinline__ f32x2 nn_dist(f32x2 qx, f32x2 qy, f32x2 qz, float rx, float ry, float rz) {
  const f32x2 dx = qx - rx, dy = qy - ry, dz = qz - rz;
  if (NORM == 2) return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
  return (__builtin_elementwise_abs(dx) + __builtin_elementwise_abs(dy)) + __builtin_elementwise_abs(dz);
}

template <int NORM>
__global__ __launch_bounds__(NN_THREADS) void nn1_kernel(const float* __restrict__ q, int64_t q_bs,
                                                         const int64_t* __restrict__ q_len, int64_t nq_max,
                                                         const float* __restrict__ r, int64_t r_bs,
                                                         const int64_t* __restrict__ r_len, int64_t nr_max,
                                                         float* __restrict__ dist, int64_t* __restrict__ idx,
                                                         unsigned long long* __restrict__ ws, int tiles_per_part) {
  __shared__ float tile[2][NN_TILE * 3];
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int64_t nq = clamp_len(q_len, b, nq_max);
  const int64_t nr = clamp_len(r_len, b, nr_max);
  const int64_t q0 = (int64_t)blockIdx.x * NN_QB;
  const float* qb = q + b * q_bs;
  const float* rb = r + b * r_bs;

  f32x2 qx[NN_QPT / 2], qy[NN_QPT / 2], qz[NN_QPT / 2];
  float best[NN_QPT];
  int bg[NN_QPT];  // the first group of NN_GROUP reference points whose minimum is `best`
#pragma unroll
  for (int u = 0; u < NN_QPT; ++u) {
    const int64_t i = q0 + u * NN_THREADS + tid;
    const bool ok = i < nq;
    qx[u >> 1][u & 1] = ok ? qb[3 * i] : 0.f;
    qy[u >> 1][u & 1] = ok ? qb[3 * i + 1] : 0.f;
    qz[u >> 1][u & 1] = ok ? qb[3 * i + 2] : 0.f;
    best[u] = INFINITY;
    bg[u] = -1;
  }

  const int64_t r_begin = (int64_t)blockIdx.y * tiles_per_part * NN_TILE;
  const int64_t r_stop = r_begin + (int64_t)tiles_per_part * NN_TILE;
  const int64_t r_end = r_stop < nr ? r_stop : nr;
  if (r_begin < r_end && q0 < nq) {  // workgroup-uniform
    const int ntiles = (int)((r_end - r_begin + NN_TILE - 1) / NN_TILE);
    float st[12];
    nn_tile_load(st, rb, r_begin, r_end, tid);
#pragma unroll
    for (int k = 0; k < 12; ++k) tile[0][k * NN_THREADS + tid] = st[k];
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
      const int64_t base = r_begin + (int64_t)t * NN_TILE;
      const bool more = t + 1 < ntiles;
      if (more) nn_tile_load(st, rb, base + NN_TILE, r_end, tid);
      const float* s = tile[t & 1];
      const int left = (int)(r_end - base < NN_TILE ? r_end - base : NN_TILE);
      const int groups = (left + NN_GROUP - 1) / NN_GROUP;  // the last group's slots past r_end hold NaN
      const int g0 = (int)(base / NN_GROUP);
      for (int g = 0; g < groups; ++g) {
        float m[NN_QPT];
#pragma unroll
        for (int u = 0; u < NN_QPT; ++u) m[u] = INFINITY;
#pragma unroll
        for (int k = 0; k < NN_GROUP; ++k) {
          const int j = g * NN_GROUP + k;
          const float rx = s[3 * j], ry = s[3 * j + 1], rz = s[3 * j + 2];
#pragma unroll
          for (int p = 0; p < NN_QPT / 2; ++p) {
            const f32x2 d = nn_dist<NORM>(qx[p], qy[p], qz[p], rx, ry, rz);
            m[2 * p] = fminf(m[2 * p], d[0]);  // fminf drops a NaN operand
            m[2 * p + 1] = fminf(m[2 * p + 1], d[1]);
          }
        }
#pragma unroll
        for (int u = 0; u < NN_QPT; ++u) {
          const bool lt = m[u] < best[u];
          best[u] = lt ? m[u] : best[u];
          bg[u] = lt ? g0 + g : bg[u];
        }
      }
      if (more) {
        float* w = tile[(t + 1) & 1];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k * NN_THREADS + tid] = st[k];
      }
      __syncthreads();
    }
  }

  // The index inside the winning group: its points again, from global memory (a per-lane gather of at most
  // NN_GROUP points, once per query), first strict minimum.
  int bi[NN_QPT];
#pragma unroll
  for (int u = 0; u < NN_QPT; ++u) {
    bi[u] = -1;
    if (bg[u] < 0) continue;
    const f32x2 x = {qx[u >> 1][u & 1], 0.f}, y = {qy[u >> 1][u & 1], 0.f}, z = {qz[u >> 1][u & 1], 0.f};
    float bd = INFINITY;
    for (int k = 0; k < NN_GROUP; ++k) {
      const int64_t j = (int64_t)bg[u] * NN_GROUP + k;
      if (j >= r_end) break;
      const float d = nn_dist<NORM>(x, y, z, rb[3 * j], rb[3 * j + 1], rb[3 * j + 2])[0];
      if (d < bd) bd = d, bi[u] = (int)j;
    }
    best[u] = bd;
  }

#pragma unroll
  for (int u = 0; u < NN_QPT; ++u) {
    const int64_t i = q0 + u * NN_THREADS + tid;
    if (i >= nq_max) continue;
    const int64_t o = (int64_t)b * nq_max + i;
    if (ws) {
      if (i < nq && bi[u] >= 0)
        atomicMin(ws + o, ((unsigned long long)__float_as_uint(best[u]) << 32) | (unsigned)bi[u]);
    } else {
      dist[o] = i < nq ? best[u] : 0.f;
      if (idx) idx[o] = i < nq ? (int64_t)bi[u] : (int64_t)-1;
    }
  }
}

__global__ __launch_bounds__(256) void nn1_unpack_kernel(const unsigned long long* __restrict__ ws,
                                                         const int64_t* __restrict__ q_len, int64_t nq_max,
                                                         float* __restrict__ dist, int64_t* __restrict__ idx) {
  const int b = blockIdx.y;
  const int64_t nq = clamp_len(q_len, b, nq_max);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq_max; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = (int64_t)b * nq_max + i;
    const unsigned long long key = ws[o];
    float d = 0.f;
    int64_t j = -1;
    if (i < nq) {
      const bool none = key == ~0ull;
      d = none ? INFINITY : __uint_as_float((unsigned)(key >> 32));
      j = none ? (int64_t)-1 : (int64_t)(unsigned)(key & 0xffffffffull);
    }
    dist[o] = d;
    if (idx) idx[o] = j;
  }
}

// Stage 1: workgroup blockIdx.x sums rows blockIdx.x * 256 + tid + k * gridDim.x * 256 (fixed for a given n_max).
__global__ __launch_bounds__(PS_THREADS) void pair_stats_partial_kernel(
    const float* __restrict__ x, int64_t x_bs, const int64_t* __restrict__ x_len, int64_t n_max,
    const float* __restrict__ y, int64_t y_bs, const int64_t* __restrict__ y_len, int64_t m_max,
    const int64_t* __restrict__ idx, double* __restrict__ part) {
  __shared__ double red[PS_THREADS / 64][PS_VALS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n = clamp_len(x_len, b, n_max);
  const int64_t m = clamp_len(y_len, b, m_max);
  const float* xb = x + b * x_bs;
  const float* yb = y + b * y_bs;
  const int64_t* ib = idx + (int64_t)b * n_max;
  double a[PS_VALS];
#pragma unroll
  for (int k = 0; k < PS_VALS; ++k) a[k] = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)PS_THREADS + tid; i < n; i += (int64_t)gridDim.x * PS_THREADS) {
    const int64_t j = ib[i];
    if (j < 0 || j >= m) continue;
    const double x0 = xb[3 * i], x1 = xb[3 * i + 1], x2 = xb[3 * i + 2];
    const double y0 = yb[3 * j], y1 = yb[3 * j + 1], y2 = yb[3 * j + 2];
    a[0] += 1.0;
    a[1] += x0, a[2] += x1, a[3] += x2;
    a[4] += y0, a[5] += y1, a[6] += y2;
    a[7] += x0 * y0, a[8] += x0 * y1, a[9] += x0 * y2;
    a[10] += x1 * y0, a[11] += x1 * y1, a[12] += x1 * y2;
    a[13] += x2 * y0, a[14] += x2 * y1, a[15] += x2 * y2;
    const double d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
    a[16] += d0 * d0 + d1 * d1 + d2 * d2;
  }
#pragma unroll
  for (int k = 0; k < PS_VALS; ++k) {
    const double v = wave_sum(a[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < PS_VALS) {
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < PS_THREADS / 64; ++w) v += red[w][tid];
    part[((int64_t)b * gridDim.x + blockIdx.x) * PS_VALS + tid] = v;
  }
}

// Stage 2: one 64-lane workgroup per batch item adds the partials in workgroup order.
__global__ __launch_bounds__(64) void pair_stats_final_kernel(const double* __restrict__ part, int nblk,
                                                              double* __restrict__ out) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= PS_VALS) return;
  double v = 0.0;
  for (int i = 0; i < nblk; ++i) v += part[((int64_t)b * nblk + i) * PS_VALS + k];
  out[b * PS_VALS + k] = v;
}

int ps_blocks(int64_t n_max) {
  const int64_t nb = (n_max + PS_THREADS - 1) / PS_THREADS;
  return (int)(nb < 1 ? 1 : (nb > PS_MAX_BLOCKS ? PS_MAX_BLOCKS : nb));
}

// The current device's compute units, asked on every call (an attribute lookup; a cached count would be wrong
// after a switch between devices of different sizes).  Only the split choice depends on it, never the result.
int device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
    return 256;
  return n;
}

}  // namespace

// The automatic split count: 1 while the query workgroups alone make NN_ROUNDS rounds of the device's
// NN_SLOTS_PER_CU * cus workgroup slots (a last partial round then costs at most a fifth), else enough parts to
// get there, never more parts than the reference has tiles (a part is a whole number of 1024-point tiles).
extern "C" int vggt_nn1_plan(int B, int64_t nq_max, int64_t nr_max, int cus) {
  if (B < 1 || nq_max <= 0 || nr_max <= 0 || cus <= 0) return 1;
  const int64_t qblocks = (nq_max + NN_QB - 1) / NN_QB * B;
  const int64_t want = (int64_t)cus * NN_SLOTS_PER_CU * NN_ROUNDS;
  if (qblocks >= want) return 1;
  int64_t split = (want + qblocks - 1) / qblocks;
  const int64_t tiles = (nr_max + NN_TILE - 1) / NN_TILE;
  if (split > tiles) split = tiles;
  if (split > NN_MAX_SPLIT) split = NN_MAX_SPLIT;
  return (int)(split < 1 ? 1 : split);
}

// Enough for either call on these shapes: the 8-byte merge keys of a split vggt_nn1 (B * nq_max) or the
// per-workgroup partials of vggt_nn1_pair_stats with n_max = nq_max.
extern "C" size_t vggt_nn1_workspace_bytes(int B, int64_t nq_max, int64_t nr_max) {
  if (B < 1 || nq_max <= 0) return 0;
  (void)nr_max;
  const size_t keys = (size_t)B * (size_t)nq_max * sizeof(unsigned long long);
  const size_t stats = (size_t)B * ps_blocks(nq_max) * PS_VALS * sizeof(double);
  return keys > stats ? keys : stats;
}

extern "C" int vggt_nn1(const float* q, int64_t q_bs, const int64_t* q_len, const float* r, int64_t r_bs,
                        const int64_t* r_len, int B, int64_t nq_max, int64_t nr_max, int norm, float* dist,
                        int64_t* idx, int split, void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || B > 65535 || nq_max < 0 || nr_max < 0 || nr_max >= ((int64_t)1 << 31) || split < 0)
    return VGGT_ERR_SHAPE;
  if (norm != 1 && norm != 2) return VGGT_ERR_UNSUPPORTED;
  if (nq_max == 0) return VGGT_OK;
  const int64_t qblocks = (nq_max + NN_QB - 1) / NN_QB;
  if (qblocks >= ((int64_t)1 << 31)) return VGGT_ERR_SHAPE;
  const int64_t tiles = (nr_max + NN_TILE - 1) / NN_TILE;
  int64_t parts = split > 0 ? split : vggt_nn1_plan(B, nq_max, nr_max, device_cus());
  if (parts > tiles) parts = tiles;
  if (parts > 65535) parts = 65535;
  if (parts < 1) parts = 1;
  const int tpp = (int)(tiles > 0 ? (tiles + parts - 1) / parts : 1);
  parts = tiles > 0 ? (tiles + tpp - 1) / tpp : 1;  // no empty trailing part
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = nullptr;
  if (parts > 1) {
    const size_t need = (size_t)B * (size_t)nq_max * sizeof(unsigned long long);
    if (!ws || ws_bytes < need) return VGGT_ERR_SHAPE;
    if ((uintptr_t)ws % 8) return VGGT_ERR_ALIGN;
    keys = (unsigned long long*)ws;
    if (hipMemsetAsync(keys, 0xff, need, st) != hipSuccess) return VGGT_ERR_HIP;
  }
  const dim3 grid((unsigned)qblocks, (unsigned)parts, (unsigned)B);
  if (norm == 2)
    nn1_kernel<2><<<grid, NN_THREADS, 0, st>>>(q, q_bs, q_len, nq_max, r, r_bs, r_len, nr_max, dist, idx, keys, tpp);
  else
    nn1_kernel<1><<<grid, NN_THREADS, 0, st>>>(q, q_bs, q_len, nq_max, r, r_bs, r_len, nr_max, dist, idx, keys, tpp);
  HIP_LAUNCH_CHECK();
  if (keys) {
    const int64_t blocks = (nq_max + 255) / 256;
    nn1_unpack_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096), B), 256, 0, st>>>(keys, q_len, nq_max, dist,
                                                                                         idx);
    HIP_LAUNCH_CHECK();
  }
  return VGGT_OK;
}

extern "C" int vggt_nn1_pair_stats(const float* x, int64_t x_bs, const int64_t* x_len, const float* y, int64_t y_bs,
                                   const int64_t* y_len, const int64_t* idx, int B, int64_t n_max, int64_t m_max,
                                   double* out, void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || B > 65535 || n_max < 0 || m_max < 0) return VGGT_ERR_SHAPE;
  const int nblk = ps_blocks(n_max);
  if (!ws || ws_bytes < (size_t)B * nblk * PS_VALS * sizeof(double)) return VGGT_ERR_SHAPE;
  if ((uintptr_t)ws % 8) return VGGT_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  pair_stats_partial_kernel<<<dim3(nblk, B), PS_THREADS, 0, st>>>(x, x_bs, x_len, n_max, y, y_bs, y_len, m_max, idx,
                                                                  (double*)ws);
  HIP_LAUNCH_CHECK();
  pair_stats_final_kernel<<<B, 64, 0, st>>>((const double*)ws, nblk, out);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}
