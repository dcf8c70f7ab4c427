// Flash-attention forward for the VGGT hot path (include/vggt_mi355x.h:
// vggt_attention_fwd): softmax(Q K^T * scale) V, bf16 in/out, fp32 online
// softmax, head_dim D in {64, 128}, non-causal, ragged nk (masked last tile).
//
// gfx950 design:
//  * Workgroup = 4 waves = 128 query rows (32 per wave); KV tiles of 64 keys
//    staged global->LDS by LDS-DMA (buffer_load_dwordx4 ... lds),
//    double-buffered.  The buffer descriptor is re-based per tile by SALU
//    (base += 64 rows, num_records = remaining rows), so the per-lane offsets
//    are loop-invariant (no VALU address math in the loop) and rows past nk
//    read as zeros by the hardware range check.
//  * "Swapped" QK^T: each wave computes S^T = K . Q^T with
//    v_mfma_f32_32x32x16_bf16, so a lane owns one query row (lane & 31) and
//    the two lanes l, l+32 hold all 64 keys of the tile -> the row max needs a
//    single v_permlane32_swap, the row sum stays lane-partial until the end.
//  * The S^T accumulator, rounded to bf16, is directly the B operand of
//    O^T = V^T . P^T (no LDS round trip for P); the V^T A-operand comes from
//    ds_read_b64_tr_b16 transposed reads of the row-major V tile.
//  * LDS images are XOR-swizzled on the DMA source offset so that the K
//    ds_read_b128 fragment reads and the V transposed reads are bank-conflict
//    free; the swizzles touch only row bits that are lane-constant, so every
//    LDS read is a loop-invariant base register + immediate offset (the tile
//    loop is unrolled x2 so the double-buffer index is compile-time).
//  * Online softmax in the log2 domain with a deferred rescale (T13): O and l
//    are rescaled only when some row's max grows by more than THR=8 (P <= 2^8).
//  * XCD-aware block order: consecutive query blocks of one (batch, head)
//    share an XCD so its K/V stream is served from one L2.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#include "tune.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef int int32x4 __attribute__((ext_vector_type(4)));

constexpr int BKV = 64;
constexpr float THR = 8.0f;

struct AttnArgs {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  int64_t ldq, ldk, ldv, ldo;
  int64_t qbs, kbs, vbs, obs;
  int batch, heads, nq, nk;
  float c;     // scale * log2(e)
  float* lse;  // optional [batch*heads*nq]: log2 sum exp2(scores * c) per row (training recompute)
  // key-split tail (VAR & V_KEY_SPLIT only): of every `unit_period` consecutive (b, h, row block) units the first
  // `full_pp` are whole and the rest the tail.  Workgroups [0, n_full) are the whole units of all periods in
  // linear order; behind them every tail unit runs as `parts` workgroups, part p over the keys
  // [p * part_tiles * 64, ...) (the last part takes the rest), and leaves (m, l, O) in ws -- slab
  // (tail unit in linear order) * parts + p.  unit_period: one batch element's units, or the whole launch's
  int n_full, parts, part_tiles;
  float* ws;
  int unit_period, full_pp;
};

// Partial of one (tail unit, part): the fp32 O accumulators in register order
// [wave][db * 4 + gq][lane] float4 (every store instruction writes 1 KiB
// contiguous), then per row (m, l) as float2.
constexpr int SPLIT_BQ = 256;
constexpr int SPLIT_SLAB = SPLIT_BQ * 64 + 2 * SPLIT_BQ;  // floats

// LDS-DMA: 16 B per lane from buffer `rsrc` at per-lane byte offset `voff`
// into the wave-uniform LDS address `lds` (+lane*16).  Inline asm keeps the
// pending LDS write invisible to hipcc's alias analysis (it would otherwise
// drain vmcnt(0) before reads of the other buffer); completion is waited for
// by the explicit vmcnt(0) + barrier at the end of every tile.
__device__ __forceinline__ void dma16(int32x4 rsrc, uint32_t voff, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rsrc), "s"(lds)
               : "memory");
}

__device__ __forceinline__ int32x4 make_rsrc(const void* base, uint32_t nbytes) {
  const uint64_t b = (uint64_t)base;
  int32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
  r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) & 0xffff;
  r[2] = __builtin_amdgcn_readfirstlane(nbytes);
  r[3] = 0x00020000;
  return r;
}

template <int D>
__device__ __forceinline__ int k_swz(int row, int chunk) {
  if constexpr (D == 64) return chunk ^ ((row >> 1) & 7);
  else return chunk ^ (row & 15);
}
template <int D>
__device__ __forceinline__ int v_swz(int row, int chunk) {
  if constexpr (D == 64) return chunk ^ (((row >> 1) & 1) << 2);
  else return chunk ^ ((row & 3) << 2);
}

// VAR: the schedule bits of attn_fwd_kernel (A/B-tested through vggt_tune).  A kernel is a (D, NW, VAR) triple of
// VGGT_ATTN_KERNELS; attn_resolve maps the knobs to one.  The values are part of the kernels' mangled names.
constexpr int V_HOIST_K = 1;       // all K fragment reads before the QK^T MFMAs
constexpr int V_MAX4 = 2;          // max-tracking form: four-chain row max
constexpr int V_SUM4 = 4;          // max-tracking form: four partial row sums
constexpr int V_MFMA_SUM = 8;      // max-tracking form: row sums on the matrix core (an all-ones V^T block times P^T:
                                   // 4 MFMAs per tile replace 32 VALU adds per lane), over the bf16-rounded P of P.V
constexpr int V_PIPE_QK = 16;      // QK^T of tile t+1 issued before tile t's softmax (3 K|V slots; max-tracking form)
constexpr int V_OFFSET_FREE = 32;  // offset-free online softmax (soft_pv): no row max on the common path
constexpr int V_EXACT = 64;        // offset-free with exact scores: s * c per element instead of the Q prescale, O
                                   // normalised by the sum of the bf16-rounded p (the training forward)
constexpr int V_SPLIT_TILE = 256;  // offset-free, full tiles as two software-pipelined 32-key halves (tile_split)
constexpr int V_DMA_AHEAD = 512;   // offset-free, 3 K|V slots, LDS-DMA two tiles ahead
constexpr int V_STAMPS = 1024;     // diagnostic (vggt_attention_stamps): s_memtime stamps per tile segment, summed per
                                   // wave into a.lse as unsigned long long[nwg][NW][STAMP_N]; the kernel writes no lse
constexpr int V_DMA_HALF = 2048;   // 8-wave form: only the priority half (waves 4-7) issues the LDS-DMA
constexpr int V_NO_PRIO = 4096;    // 8-wave form: no priority raise for waves 4-7
constexpr int V_KEY_SPLIT = 8192;  // key-split tail: workgroups past n_full run one key range of a tail unit each
// The public variant ids (VGGT_TUNE_ATTN_VARIANT) are these bits OR'd; 128 is no kernel bit, only the 16x16x32 form's id
constexpr int ID_FORM16 = 128;
constexpr int V_33 = V_OFFSET_FREE | V_HOIST_K;  // the default
constexpr int V_96 = V_OFFSET_FREE | V_EXACT;    // the training forward (vggt_attention_fwd_lse)
constexpr int V_161 = V_33 | ID_FORM16;
constexpr int V_289 = V_33 | V_SPLIT_TILE;
constexpr int V_545 = V_33 | V_DMA_AHEAD;
constexpr int V_2081 = V_33 | V_DMA_HALF;
constexpr int V_4129 = V_33 | V_NO_PRIO;
constexpr int V_19 = V_PIPE_QK | V_MAX4 | V_HOIST_K;
constexpr int V_23 = V_19 | V_SUM4;
constexpr int V_LEGACY = V_HOIST_K | V_MAX4 | V_SUM4 | V_MFMA_SUM;  // the max-tracking form's own bits (3, 7, 11, 15)
constexpr int STAMP_N = 8;
template <int D, int NW, int VAR>
__global__ __launch_bounds__(NW * 64, 8 / NW) void attn_fwd_kernel(AttnArgs a) {
  constexpr int BQ = NW * 32;            // query rows per workgroup (32 per wave)
  constexpr int ROWB = D * 2;            // bytes per K/V row in LDS
  constexpr int TILEB = BKV * ROWB;      // bytes per K (or V) tile
  constexpr int NKS = D / 16;            // k-steps of the QK^T MFMA
  constexpr int NDB = D / 32;            // 32-row output blocks of O^T
  constexpr int RPI = 1024 / ROWB;       // rows per 1-KiB DMA instruction
  constexpr int CPR = ROWB / 16;         // 16-B chunks per row
  constexpr int IPW = TILEB / 1024 / NW;  // DMA instructions per wave per operand
  constexpr int NSLOT = (VAR & (V_PIPE_QK | V_DMA_AHEAD)) ? 3 : 2;  // K|V tile slots (3: pipelined QK^T / DMA two ahead)
  __shared__ __attribute__((aligned(16))) char smem[NSLOT * 2 * TILEB];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hl = lane >> 5;
  // 8-wave form: the second-dispatched half (waves 4-7) shares each SIMD with
  // an older wave and loses VALU arbitration on every segment; one static
  // priority raise for it (cdna_hip_programming.md T5, static form).
  // (VAR & V_NO_PRIO: no priority raise -- re-measured with the segment stamps, r11)
  if constexpr (NW == 8 && !(VAR & V_NO_PRIO)) {
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  }
  const int nqb = (a.nq + BQ - 1) / BQ;
  // VAR & V_KEY_SPLIT (key-split tail): the first n_full workgroups are whole units,
  // the others one part of a tail unit each -- its keys [key0, key0 + nk); the
  // XCD remap runs within either range (dispatch follows the block index, so
  // the whole units keep the low indices).  Whole unit w is unit w % full_pp of
  // period w / full_pp, tail unit tu unit full_pp + tu % tail_pp of period
  // tu / tail_pp (AttnArgs); all of it wave-uniform, on the scalar unit
  constexpr bool SPLIT = (VAR & V_KEY_SPLIT) != 0;
  int bid, nk = a.nk, key0 = 0, slab = -1;
  if constexpr (SPLIT) {
    const int bx = blockIdx.x;
    if (bx < a.n_full) {
      const int w = xcd_remap(bx, a.n_full);
      bid = w / a.full_pp * a.unit_period + w % a.full_pp;
    } else {
      slab = xcd_remap(bx - a.n_full, (int)gridDim.x - a.n_full);
      const int part = slab % a.parts, tu = slab / a.parts, tail_pp = a.unit_period - a.full_pp;
      bid = tu / tail_pp * a.unit_period + a.full_pp + tu % tail_pp;
      key0 = part * a.part_tiles * BKV;
      nk = part == a.parts - 1 ? a.nk - key0 : a.part_tiles * BKV;
    }
  } else {
    bid = xcd_remap(blockIdx.x, nqb * a.heads * a.batch);
  }
  const int qb = bid % nqb;
  const int bh = bid / nqb;
  const int h = bh % a.heads;
  const int b = bh / a.heads;

  const bf16_t* qp = a.q + (int64_t)b * a.qbs * a.ldq + h * D;
  const bf16_t* kp = a.k + ((int64_t)b * a.kbs + key0) * a.ldk + h * D;
  const bf16_t* vp = a.v + ((int64_t)b * a.vbs + key0) * a.ldv + h * D;

  // ---- Q fragments = B operand of S^T = K Q^T: Q[q][16ks + 8*hl + j]
  const int qrow = qb * BQ + wave * 32 + (lane & 31);
  const int qr = min(qrow, a.nq - 1);
  bf16x8 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const bf16x8*)(qp + (int64_t)qr * a.ldq + ks * 16 + 8 * hl);
  if constexpr ((VAR & V_OFFSET_FREE) && !(VAR & V_EXACT)) {
    // scores come out of the MFMA already in log2 units: Q * (scale log2 e),
    // re-rounded to bf16 (one extra rounding of Q, ~2^-9 relative)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[ks][j] = (__bf16)((float)qf[ks][j] * a.c);
  }
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qf[ks]));  // retire the Q loads before the loop

  // ---- loop-invariant DMA offsets and LDS destinations
  // VAR & V_DMA_HALF (8-wave form): only the priority-1 half (waves 4-7) issues the
  // tile's LDS-DMA, two pieces per operand each.  Segment stamps (VAR & V_STAMPS,
  // profiles/r11) showed those waves finish each tile ~870 cycles before their
  // SIMD partners and wait at the barrier, while the partners' tile work is the
  // tile's critical path: the DMA issue moves off it.
  constexpr bool DMAH = (VAR & V_DMA_HALF) && NW == 8;
  constexpr int IPWX = DMAH ? 2 * IPW : IPW;  // pieces per issuing wave per operand
  const int pbase = DMAH ? (wave >= 4 ? wave - 4 : 0) * IPWX : wave * IPW;
  uint32_t koff[IPWX], voff[IPWX];
#pragma unroll
  for (int i = 0; i < IPWX; ++i) {
    const int row = (pbase + i) * RPI + lane / CPR;
    const int cp = lane % CPR;
    koff[i] = (uint32_t)(row * a.ldk + k_swz<D>(row, cp) * 8) * 2u;
    voff[i] = (uint32_t)(row * a.ldv + v_swz<D>(row, cp) * 8) * 2u;
  }
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)LDS_PTR(smem)) + pbase * 1024;
  // 32-bit scalar descriptor arithmetic (host: nk * ld * 2 < 2^31): a 64-bit
  // "remaining bytes" compare has no SALU form and would run on the VALU
  const int kstep = BKV * (int)a.ldk * 2, vstep = BKV * (int)a.ldv * 2;
  const int kbytes = nk * (int)a.ldk * 2, vbytes = nk * (int)a.ldv * 2;

  auto stage = [&](int buf, int t) {
    const int ko = kstep * t, vo = vstep * t;
    const int32x4 kr = make_rsrc((const char*)kp + ko, (uint32_t)max(kbytes - ko, 0));
    const int32x4 vr = make_rsrc((const char*)vp + vo, (uint32_t)max(vbytes - vo, 0));
    const uint32_t d = lds0 + buf * 2 * TILEB;
    if (!DMAH || wave >= 4) {
#pragma unroll
      for (int i = 0; i < IPWX; ++i) {
        dma16(kr, koff[i], d + i * 1024);
        dma16(vr, voff[i], d + TILEB + i * 1024);
      }
    }
  };

  // ---- loop-invariant LDS read addresses (bytes within one K|V buffer pair)
  uint32_t ka[NKS];
  {
    const int key = lane & 31;  // + kb*32: swizzle-invariant
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) ka[ks] = key * ROWB + (k_swz<D>(key, 2 * ks + hl) << 4);
  }
  uint32_t va[NDB];
  {
    const int g = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
    const int r0 = 4 * hl + qq;  // + kb*32 + 16*ss + 8*half: swizzle-invariant
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int col = db * 32 + 16 * g + 4 * pp;
      va[db] = TILEB + r0 * ROWB + (v_swz<D>(r0, col >> 3) << 4) + (col & 7) * 2;
    }
  }

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  // VAR & V_OFFSET_FREE starts from a finite "unset" offset: masked scores (-inf) minus
  // it stay -inf (-inf - -inf would be a NaN, and the kernel is built with
  // -fno-honor-nans, so a NaN could slip past the range guard)
  constexpr float M_UNSET = -1e30f;
  float m_run = (VAR & V_OFFSET_FREE) ? M_UNSET : -INFINITY, l_run = 0.f;
  // VAR & V_EXACT (the exact-score form, the training forward): a second row sum, over the
  // bf16-rounded p that feed P.V, normalises O; l_run (unrounded p) stays the lse's.  At
  // offset 0 the row's largest p = exp2(s) is no power of two, and its bf16 rounding
  // (up to 2^-8) would not cancel against an unrounded sum: with one key, or one dominant
  // key, O = v (1 + eps) for the whole row, and the backward's delta = dO . O leaves
  // dO . v eps behind where dP - delta should cancel.  For the same reason this form
  // takes the row max of its first tile as the offset whatever its size (p = 1 exactly at
  // that key, as in a max-subtracting softmax), and so runs the shifted tile loop.
  float lb_run = 0.f;
  f32x16 lsum = f32x16{};  // VAR & V_MFMA_SUM: every row of the ones-block product holds l[q]
  // VAR & V_OFFSET_FREE: per-row bound exponent of the offset mode (60 at offset 0, THR
  // once the row carries a max offset) and whether every row of the wave sits
  // at offset 0 (then p = exp2(s) with no subtraction at all)
  float lim = THR, limv = 256.0f;
  bool zero_off = false;
  const float c = a.c;
  const int nt = (nk + BKV - 1) / BKV;
  // VAR & V_STAMPS: per-wave cycle sums of the tile segments (s_memtime, one scalar
  // statement with its lgkmcnt(0)); 32-bit sums, no tile counter (the host
  // knows the tile count): so instrumented, the kernel keeps the default's 113
  // VGPRs and occupancy (a per-tile counter, VGPR-pinned sums or scheduling
  // barriers around the stamps each pushed it to 119-153)
  uint32_t st_acc[STAMP_N] = {}, st_prev = 0;
#define VGGT_SEG(i)                                                                                  \
  do {                                                                                               \
    if constexpr (VAR & V_STAMPS) {                                                                  \
      /* no sched_barrier: it pushed the kernel to 150 VGPRs */                                     \
      unsigned long long now_;                                                                       \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");                     \
      if ((i) >= 0) st_acc[(i) >= 0 ? (i) : 0] += (uint32_t)now_ - st_prev;                          \
      st_prev = (uint32_t)now_;                                                                      \
      /* no sched_barrier: it pushed the kernel to 150 VGPRs */                                     \
    }                                                                                                \
  } while (0)

  struct S2 {
    f32x16 v[2];
  };
  // ---- S^T = K . Q^T for the two 32-key blocks of the tile in slot BUF
  auto qk = [&](auto bufc) -> S2 {
    constexpr int BUF = decltype(bufc)::value;
    const char* base = smem + BUF * 2 * TILEB;
    f32x16 s[2];
    if constexpr (VAR & V_HOIST_K) {
      // all K fragment reads first, then the two 32-key accumulator chains
      // interleaved (no MFMA waits on a just-issued LDS read)
      bf16x8 kf[2][NKS];
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) kf[kb][ks] = *(const bf16x8*)(base + ka[ks] + kb * 32 * ROWB);
      s[0] = f32x16{};
      s[1] = f32x16{};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb][ks], qf[ks], s[kb], 0, 0, 0);
    } else {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        s[kb] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const bf16x8 kf = *(const bf16x8*)(base + ka[ks] + kb * 32 * ROWB);
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kb], 0, 0, 0);
        }
      }
    }
    return S2{{s[0], s[1]}};
  };
  // ---- the same scores recomputed on a rare path (VAR & V_OFFSET_FREE): the LDS offset
  // goes through an empty asm so the reads are not CSE'd with the common
  // path's (which would keep 32 K-fragment registers live across the tile)
  // and the MFMAs cannot be speculated out of the branch
  auto qk_again = [&](auto bufc) -> S2 {
    constexpr int BUF = decltype(bufc)::value;
    uint32_t opq = BUF * 2 * TILEB;
    asm volatile("" : "+v"(opq));
    const char* base = smem + opq;
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      s[kb] = f32x16{};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8 kf = *(const bf16x8*)(base + ka[ks] + kb * 32 * ROWB);
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kb], 0, 0, 0);
      }
    }
    return S2{{s[0], s[1]}};
  };
  // ---- O^T[db] += V^T . P^T over the 16 keys from `row` of the V tile behind `base`
  auto pv16 = [&](const char* base, int db, int row, const bf16x8& p) {
    const char* p0 = base + va[db] + row * ROWB;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p0));
    const s16x4 hi =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p0 + 8 * ROWB));
    const bf16x8 vf = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, p, o[db], 0, 0, 0);
  };
  // ---- mask, online softmax and O^T += V^T . P^T for the tile in slot BUF
  auto soft_pv = [&](auto bufc, int t, S2 sc, auto zc) {
    constexpr int BUF = decltype(bufc)::value;
    const char* base = smem + BUF * 2 * TILEB;
    f32x16 s[2] = {sc.v[0], sc.v[1]};
    const int kv0 = t * BKV;
    auto mask = [&]() {
      if (kv0 + BKV > nk) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kv0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
            if (key >= nk) s[kb][r] = -INFINITY;
          }
      }
    };
    mask();
    bf16x8 pf[2][2];
    if constexpr (VAR & V_OFFSET_FREE) {
      // Offset-free online softmax.  softmax is shift-invariant, and bf16 / fp32
      // keep their relative precision at any exponent, so the max subtraction
      // only guards the exponent range.  Each row carries an offset m_run
      // (log2 units), fixed at its first tile: 0 when that tile's max lies in
      // [-60, 60] (then p = exp2(s) -- no max, no subtraction; the first
      // tile's max term keeps l >= 2^-60), else the max itself.  A lane's
      // partial sum over its 32 keys <= 2^lim bounds every p of it by 2^lim
      // (lim = 60 at offset 0, THR otherwise -- the T13 bound), so no row max
      // is computed on the common path.  Only when some lane's sum exceeds its
      // bound (first tile: m_run = -inf -> p = inf) does the wave recompute the
      // raw scores from LDS, take the true row max and move the offset of the
      // rows that need it -- before this tile's P.V (the textbook order).
      // VAR & V_EXACT: exact scores (s * c per element, no Q prescale).
      float rs[4], rb = 0.f;
      auto exps = [&](auto shc) {
        constexpr bool shifted = decltype(shc)::value;
#pragma unroll
        for (int i = 1; i < 4; ++i) rs[i] = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int ss = 0; ss < 2; ++ss) {
            bf16x8 t;  // whole-vector write: the previous pf is dead here, not an insert operand
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float x = s[kb][8 * ss + j];
              if constexpr (VAR & V_EXACT) x = shifted ? fmaf(x, c, -m_run) : x * c;
              else if constexpr (shifted) x -= m_run;
              const float p = __builtin_amdgcn_exp2f(x);
              // one chain: split sums get SLP-packed into v_pk_add_f32; started from the
              // first p (p >= +0, so 0 + p == p bitwise: one v_add fewer per tile)
              if (kb == 0 && ss == 0 && j == 0) rs[0] = p;
              else rs[0] += p;
              t[j] = (__bf16)p;
            }
            pf[kb][ss] = t;
            if constexpr (VAR & V_EXACT) {
              // v_dot2c_f32_bf16 against packed ones: one VALU per two rounded p
              typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
              const bf16x2 ones = {(__bf16)1.0f, (__bf16)1.0f};
              if (kb == 0 && ss == 0) rb = 0.f;
#pragma unroll
              for (int j = 0; j < 8; j += 2) {
                const bf16x2 t2 = {t[j], t[j + 1]};
                rb = __builtin_amdgcn_fdot2_f32_bf16(t2, ones, rb, false);
              }
            }
          }
      };
      // zero-offset loop (zc true): p = exp2(s); a wave that has left offset 0
      // (zero_off false: also before its first tile) takes the rare path
      constexpr bool ZL = decltype(zc)::value;
      exps(std::integral_constant<bool, !ZL>{});
      float rsum = (rs[0] + rs[1]) + (rs[2] + rs[3]);
      // the ballot of the compare alone (a v_cmp straight into an SGPR mask), OR'd with the
      // wave-uniform mode flag on the scalar side (one ballot over both materialised the
      // mask into a VGPR and compared it again: two VALU per tile)
      if ((__builtin_amdgcn_ballot_w64(!(rsum <= limv)) != 0) || (ZL && !zero_off)) {
        const S2 raw = qk_again(bufc);
        s[0] = raw.v[0];
        s[1] = raw.v[1];
        mask();
        float mx = fmaxf(s[0][0], s[0][1]);
#pragma unroll
        for (int r = 2; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s[0][r]), s[0][r + 1]);
#pragma unroll
        for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s[1][r]), s[1][r + 1]);
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        if constexpr (VAR & V_EXACT) mx *= c;
        // a lane sum > 2^lim implies a p > 2^(lim-5): move the offset exactly
        // for those rows (mx > m_run + lim - 5), so afterwards p <= 1 there and
        // every other row still has p <= 2^(lim-5), sum <= 2^lim
        float m_new = m_run;
        if (m_run == M_UNSET) m_new = (!(VAR & V_EXACT) && fabsf(mx) <= 60.f) ? 0.f : mx;
        else if (mx > m_run + (lim - 5.f)) m_new = mx;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        lim = m_run == 0.f ? 60.f : THR;
        limv = m_run == 0.f ? 0x1p60f : 256.0f;  // 2^lim
        zero_off = __builtin_amdgcn_ballot_w64(m_run != 0.f) == 0;
        l_run *= alpha;
        if constexpr (VAR & V_EXACT) lb_run *= alpha;
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] *= alpha;
        exps(std::true_type{});
        rsum = (rs[0] + rs[1]) + (rs[2] + rs[3]);
      }
      l_run += rsum;
      if constexpr (VAR & V_EXACT) lb_run += rb;
    } else {
    // ---- row max (lane-partial over 32 keys, then the partner half)
    float mx;
    if constexpr (VAR & V_MAX4) {
      // four independent v_max3 chains (built with -fno-honor-nans), merged:
      // dependency depth 5 instead of 16
      float mc[4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const f32x16& sv = s[cc >> 1];
        const int r0 = (cc & 1) * 8;
        float m = fmaxf(sv[r0], sv[r0 + 1]);
#pragma unroll
        for (int r = r0 + 2; r < r0 + 8; r += 2) m = fmaxf(fmaxf(m, sv[r]), sv[r + 1]);
        mc[cc] = m;
      }
      mx = fmaxf(fmaxf(mc[0], mc[1]), fmaxf(mc[2], mc[3]));
    } else {
      mx = fmaxf(s[0][0], s[0][1]);  // one v_max3 chain
#pragma unroll
      for (int r = 2; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s[0][r]), s[0][r + 1]);
#pragma unroll
      for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, s[1][r]), s[1][r + 1]);
    }
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * c;
    }
    // ---- deferred rescale: only when some row's max grew by > THR
    if (__builtin_amdgcn_ballot_w64(mx > m_run + THR) != 0) {
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      if constexpr (VAR & V_MFMA_SUM) lsum *= alpha;
      else l_run *= alpha;
#pragma unroll
      for (int db = 0; db < NDB; ++db) o[db] *= alpha;
    }
    float rs[4] = {0.f, 0.f, 0.f, 0.f};  // four partial row sums (short add chains)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kb][8 * ss + j], c, -m_run));
          if constexpr (!(VAR & V_MFMA_SUM)) rs[(VAR & V_SUM4) ? 2 * kb + ss : 0] += p;
          pf[kb][ss][j] = (__bf16)p;
        }
    if constexpr (!(VAR & V_MFMA_SUM)) l_run += (rs[0] + rs[1]) + (rs[2] + rs[3]);
    }
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) pv16(base, db, kb * 32 + 16 * ss, pf[kb][ss]);
    if constexpr (VAR & V_MFMA_SUM) {
      bf16x8 ones;
#pragma unroll
      for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) lsum = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pf[kb][ss], lsum, 0, 0, 0);
    }
  };

  // ---- VAR & V_SPLIT_TILE (offset-free only; full tiles): the tile as two 32-key
  // halves, software-pipelined inside the wave -- the QK^T MFMAs of half 1
  // are issued between the exps of half 0, and the P.V MFMAs of half 0
  // between the exps of half 1, so a wave keeps its own matrix pipe busy
  // while its VALU works (the default form runs QK^T, softmax and P.V of a
  // tile as three phases and relies on the other waves of the SIMD for
  // overlap).  The range guard runs per half: a half whose lane sum (16
  // keys) exceeds 2^lim moves the offsets of its rows exactly as the whole-
  // tile guard does (a 16-key sum > 2^lim implies a p > 2^(lim-4)), and a
  // P.V already accumulated for half 0 is rescaled with O and l (its p were
  // finite).  Same products in the same order per row: results equal the
  // default form's up to the order of the fp32 row-sum adds.
  auto tile_split = [&](auto bufc, auto zc) {
    constexpr int BUF = decltype(bufc)::value;
    constexpr bool ZL = decltype(zc)::value;
    const char* base = smem + BUF * 2 * TILEB;
    f32x16 s0 = f32x16{}, s1 = f32x16{};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const bf16x8 kf = *(const bf16x8*)(base + ka[ks]);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s0, 0, 0, 0);
    }
    bf16x8 k1[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) k1[ks] = *(const bf16x8*)(base + ka[ks] + 32 * ROWB);
    bf16x8 p0[2], p1[2];
    auto exph = [&](const f32x16& sv, bf16x8 (&pf)[2], auto shc) -> float {
      constexpr bool shifted = decltype(shc)::value;
      float r = 0.f;
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        bf16x8 tv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float x = sv[8 * ss + j];
          if constexpr (shifted) x -= m_run;
          const float pv = __builtin_amdgcn_exp2f(x);
          if (ss == 0 && j == 0) r = pv;
          else r += pv;
          tv[j] = (__bf16)pv;
        }
        pf[ss] = tv;
      }
      return r;
    };
    auto pv_half = [&](int kb, const bf16x8 (&pf)[2]) {
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) pv16(base, db, kb * 32 + 16 * ss, pf[ss]);
    };
    auto rowmax = [&](const f32x16& a0, const f32x16* a1) {
      float mx = fmaxf(a0[0], a0[1]);
#pragma unroll
      for (int r = 2; r < 16; r += 2) mx = fmaxf(fmaxf(mx, a0[r]), a0[r + 1]);
      if (a1) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, (*a1)[r]), (*a1)[r + 1]);
      }
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    };
    auto move_offset = [&](float mx) {
      float m_new = m_run;
      if (m_run == M_UNSET) m_new = fabsf(mx) <= 60.f ? 0.f : mx;
      else if (mx > m_run + (lim - 5.f)) m_new = mx;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      lim = m_run == 0.f ? 60.f : THR;
      limv = m_run == 0.f ? 0x1p60f : 256.0f;
      zero_off = __builtin_amdgcn_ballot_w64(m_run != 0.f) == 0;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < NDB; ++db) o[db] *= alpha;
    };
    // QK^T of half 1 beside the exps of half 0
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1[ks], qf[ks], s1, 0, 0, 0);
    float r0 = exph(s0, p0, std::integral_constant<bool, !ZL>{});
    if ((__builtin_amdgcn_ballot_w64(!(r0 <= limv)) != 0) || (ZL && !zero_off)) {
      // rare: the whole tile from raw scores (first tile, or an offset move in half 0)
      const S2 raw = qk_again(bufc);
      move_offset(rowmax(raw.v[0], &raw.v[1]));
      l_run += exph(raw.v[0], p0, std::true_type{});
      l_run += exph(raw.v[1], p1, std::true_type{});
      pv_half(0, p0);
      pv_half(1, p1);
      return;
    }
    l_run += r0;
    // P.V of half 0 beside the exps of half 1
    pv_half(0, p0);
    float r1 = exph(s1, p1, std::integral_constant<bool, !ZL>{});
    if (__builtin_amdgcn_ballot_w64(!(r1 <= limv)) != 0) {
      const S2 raw = qk_again(bufc);
      move_offset(rowmax(raw.v[1], nullptr));
      r1 = exph(raw.v[1], p1, std::true_type{});
    }
    l_run += r1;
    pv_half(1, p1);
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;

  if constexpr (VAR & V_PIPE_QK) {
    // Pipelined: the QK^T MFMAs of tile t+1 are issued before tile t's softmax
    // (T15), so the matrix pipe works while the VALU does exp / max / cvt.
    // 3 slots: t (V read by P.V), t+1 (K read by QK^T), t+2 (DMA in flight,
    // issued after the barrier that retires slot t-1).
    stage(0, 0);
    if (nt > 1) stage(1, 1);
    if (nt > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    S2 cur = qk(I0{});
    auto step = [&](auto sc, auto sn, auto sf, int t) {
      // tile t+1 landed everywhere; every wave done with slot (t-1)%3 = (t+2)%3
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (t + 2 < nt) stage(decltype(sf)::value, t + 2);
      S2 nxt = cur;
      if (t + 1 < nt) nxt = qk(sn);
      soft_pv(sc, t, cur, std::false_type{});
      cur = nxt;
    };
    for (int t = 0; t < nt; t += 3) {
      step(I0{}, I1{}, I2{}, t);
      if (t + 1 >= nt) break;
      step(I1{}, I2{}, I0{}, t + 1);
      if (t + 2 >= nt) break;
      step(I2{}, I0{}, I1{}, t + 2);
    }
  } else if constexpr (VAR & V_DMA_AHEAD) {
    // Three K|V slots, the DMA two tiles ahead: tile t+2 is staged at the start
    // of tile t (into the slot tile t-1 used, retired by the barrier that ended
    // tile t-1), and the end of tile t waits only for tile t+1's pieces
    // (vmcnt counts in order: the 2*IPW pieces of t+2 may stay in flight), so
    // each tile's loads have two tiles' compute to land instead of one.
    stage(0, 0);
    if (nt > 1) stage(1, 1);
    if (nt > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    auto step = [&](auto sc, auto sf, auto zc, int t) {
      if (t + 2 < nt) stage(decltype(sf)::value, t + 2);
      soft_pv(sc, t, qk(sc), zc);
      if (t + 2 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    };
    // the offset mode may change only at a multiple of 3 tiles (slot = t % 3)
    auto run = [&](auto zc, int t0) -> int {
      for (int t = t0; t < nt; t += 3) {
        step(I0{}, I2{}, zc, t);
        if (t + 1 >= nt) break;
        step(I1{}, I0{}, zc, t + 1);
        if (t + 2 >= nt) break;
        step(I2{}, I1{}, zc, t + 2);
        if constexpr (decltype(zc)::value) {
          if (!zero_off) return t + 3;
        }
      }
      return nt;
    };
    const int t1 = run(std::true_type{}, 0);
    if (t1 < nt) run(std::false_type{}, t1);
  } else {
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // VAR & V_OFFSET_FREE: two copies of the tile loop, one per offset mode (one loop with
    // a per-tile choice between the two exp forms costs ~25 VGPRs at the merge:
    // occupancy 4 -> 3).  Every wave starts in the zero-offset loop and leaves
    // it for good, at a tile pair boundary, once one of its rows took an offset.
    // VAR & V_STAMPS segments of one tile: [2] the tile's work (DMA issue, QK^T, softmax,
    // P.V issue, up to its last LDS read), [3] end-of-tile vmcnt(0) wait for the next
    // tile's DMA, [4] barrier.  (Stamps inside the tile body, between the
    // DMA issue and QK^T or between the softmax and P.V, serialise what the compiler
    // overlaps there and pushed the kernel from 113 to 152 VGPRs: not kept.)
    auto run = [&](auto zc, int t0) -> int {
      for (int t = t0; t < nt; t += 2) {
        VGGT_SEG(-1);
        if (t + 1 < nt) stage(1, t + 1);
        if ((VAR & V_SPLIT_TILE) && (t + 1) * BKV <= nk) tile_split(I0{}, zc);
        else soft_pv(I0{}, t, qk(I0{}), zc);
        VGGT_SEG(2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        VGGT_SEG(3);
        __syncthreads();
        VGGT_SEG(4);
        if (t + 1 >= nt) break;
        if (t + 2 < nt) stage(0, t + 2);
        if ((VAR & V_SPLIT_TILE) && (t + 2) * BKV <= nk) tile_split(I1{}, zc);
        else soft_pv(I1{}, t + 1, qk(I1{}), zc);
        VGGT_SEG(2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        VGGT_SEG(3);
        __syncthreads();
        VGGT_SEG(4);
        if constexpr (decltype(zc)::value) {
          if (!zero_off) return t + 2;
        }
      }
      return nt;
    };
    if constexpr (VAR & V_OFFSET_FREE) {
      const int t1 = run(std::true_type{}, 0);
      if (t1 < nt) run(std::false_type{}, t1);
    } else {
      run(std::false_type{}, 0);
    }
  }

  // ---- epilogue: normalise, O[q][d] bf16
  if constexpr (VAR & V_MFMA_SUM) {
    l_run = lsum[0];
  } else {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
    l_run = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  if constexpr (SPLIT) {
    // a part does not normalise: (m, l, O) to the workspace, merged by attn_split_merge_kernel
    if (slab >= 0) {
      float* sp = a.ws + (int64_t)slab * SPLIT_SLAB;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          *(f32x4*)(sp + ((wave * (NDB * 4) + db * 4 + gq) * 64 + lane) * 4) =
              f32x4{o[db][4 * gq], o[db][4 * gq + 1], o[db][4 * gq + 2], o[db][4 * gq + 3]};
      if (hl == 0) *(f32x2*)(sp + BQ * D + (wave * 32 + lane) * 2) = f32x2{m_run, l_run};
      return;
    }
  }
  float inv = 1.f / l_run;
  if constexpr ((VAR & V_OFFSET_FREE) && (VAR & V_EXACT)) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(lb_run), __float_as_uint(lb_run), false, false);
    inv = 1.f / (__uint_as_float(sw[0]) + __uint_as_float(sw[1]));
  }
  if constexpr (VAR & V_STAMPS) {
    VGGT_SEG(-1);
    st_acc[6] = st_prev;  // the wave's end (low 32 bits), to place it against the others of its workgroup
    if (lane == 0) {
      unsigned long long* out = (unsigned long long*)(void*)a.lse + ((int64_t)blockIdx.x * NW + wave) * STAMP_N;
#pragma unroll
      for (int i = 0; i < STAMP_N; ++i) out[i] = st_acc[i];
    }
  } else {
    if (a.lse && hl == 0 && qrow < a.nq) a.lse[((int64_t)b * a.heads + h) * a.nq + qrow] = m_run + __log2f(l_run);
  }
  if (qrow < a.nq) {
    bf16_t* op = a.o + ((int64_t)b * a.obs + qrow) * a.ldo + h * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        uint2 pk;
        pk.x = pack_bf2(o[db][4 * gq] * inv, o[db][4 * gq + 1] * inv);
        pk.y = pack_bf2(o[db][4 * gq + 2] * inv, o[db][4 * gq + 3] * inv);
        *(uint2*)(op + db * 32 + 8 * gq + 4 * hl) = pk;
      }
  }
}

// ---------------------------------------------------------------------------
// D = 64 forward on v_mfma_f32_16x16x32_bf16 (variant 161 = 33 | 128).
//  * Matrix-core shape: per wave 32 query rows = two 16-query blocks qb, per
//    64-key tile four 16-key blocks kb; S^T[kb][qb] = K_kb . Q_qb^T leaves
//    lane l with keys kb*16 + 4*(l/16) + i (i < 4) of query qb*16 + (l & 15).
//    Under sustained load the chip holds a higher clock on 16x16x32 than on
//    32x32x16 for the same work (MI355X_MICROARCH.md 'DVFS give-back' item 7).
//  * P^T is the B operand of O^T += V^T . P^T straight from the accumulators:
//    register j of lane group g in P.V k-step kk is the key
//    32*kk + 16*(j/4) + 4*g + (j&3) -- a permutation of the tile's keys, which
//    the sum over keys does not see; the V^T A operand reads exactly those
//    keys with two ds_read_b64_tr_b16 (rows 32kk + 4g + 0..3 and +16).
//  * Softmax without any per-tile max or branch: softmax is shift-invariant
//    and fp32 / bf16 keep their relative precision at any exponent, so every
//    row uses offset 0 (p = exp2(s), s already in log2 units through the Q
//    prescale).  That is exact as long as the row's p stay inside the fp32
//    range with room to spare; the sum says so at the end: 2^-60 <= l <= 2^100
//    (a row max below -60 or a p overflow to inf fails it).  If any row of the
//    workgroup fails, the workgroup recomputes its rows in two exact passes
//    (row max over all keys, then exp2(s - max) and P.V) -- a path only
//    extreme scores take (tests/test_gpu_kernels.py offset-free extremes).
//  * K swizzle as attn_fwd_kernel<64> (conflict-free for this read pattern
//    too); V swizzle chunk ^ (((row >> 1) & 3) << 1): conflict-free for the
//    8 rows x 32 B each half-wave of the transposed reads covers.
__device__ __forceinline__ int k16_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int v16_swz(int row, int chunk) { return chunk ^ (((row >> 1) & 3) << 1); }

template <int NW>
__global__ __launch_bounds__(NW * 64, 16 / NW) void attn16_fwd_kernel(AttnArgs a) {
  constexpr int D = 64;
  constexpr int BQ = NW * 32;
  constexpr int ROWB = D * 2;
  constexpr int TILEB = BKV * ROWB;
  constexpr int RPI = 1024 / ROWB;
  constexpr int CPR = ROWB / 16;
  constexpr int IPW = TILEB / 1024 / NW;
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILEB];
  __shared__ int redo;  // workgroup vote: some row needs the exact two-pass path

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  if constexpr (NW == 8) {
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  }
  const int nqb = (a.nq + BQ - 1) / BQ;
  const int bid = xcd_remap(blockIdx.x, nqb * a.heads * a.batch);
  const int qblk = bid % nqb;
  const int bh = bid / nqb;
  const int h = bh % a.heads;
  const int b = bh / a.heads;

  const bf16_t* qp = a.q + (int64_t)b * a.qbs * a.ldq + h * D;
  const bf16_t* kp = a.k + (int64_t)b * a.kbs * a.ldk + h * D;
  const bf16_t* vp = a.v + (int64_t)b * a.vbs * a.ldv + h * D;
  const int q0 = qblk * BQ + wave * 32 + c16;  // query of block qb: q0 + 16 qb

  // ---- Q fragments (B operand of S^T = K Q^T), prescaled into log2 units
  bf16x8 qf[2][2];  // [qb][ks]: Q[query][32 ks + 8 g + j] * scale * log2(e)
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qr = min(q0 + 16 * qb, a.nq - 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[qb][ks] = *(const bf16x8*)(qp + (int64_t)qr * a.ldq + ks * 32 + 8 * g);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[qb][ks][j] = (__bf16)((float)qf[qb][ks][j] * a.c);
    }
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) asm volatile("" : "+v"(qf[qb][ks]));

  // ---- loop-invariant DMA offsets
  uint32_t koff[IPW], voff[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int row = (wave * IPW + i) * RPI + lane / CPR;
    const int cp = lane % CPR;
    koff[i] = (uint32_t)(row * a.ldk + k16_swz(row, cp) * 8) * 2u;
    voff[i] = (uint32_t)(row * a.ldv + v16_swz(row, cp) * 8) * 2u;
  }
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)LDS_PTR(smem)) + wave * IPW * 1024;
  const int kstep = BKV * (int)a.ldk * 2, vstep = BKV * (int)a.ldv * 2;
  const int kbytes = a.nk * (int)a.ldk * 2, vbytes = a.nk * (int)a.ldv * 2;
  auto stage = [&](int buf, int t) {
    const int ko = kstep * t, vo = vstep * t;
    const int32x4 kr = make_rsrc((const char*)kp + ko, (uint32_t)max(kbytes - ko, 0));
    const int32x4 vr = make_rsrc((const char*)vp + vo, (uint32_t)max(vbytes - vo, 0));
    const uint32_t d = lds0 + buf * 2 * TILEB;
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      dma16(kr, koff[i], d + i * 1024);
      dma16(vr, voff[i], d + TILEB + i * 1024);
    }
  };

  // ---- loop-invariant LDS read addresses (the kb / kk / half row steps keep the swizzles)
  uint32_t ka[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) ka[ks] = c16 * ROWB + (k16_swz(c16, 4 * ks + g) << 4);
  uint32_t va[4];
  {
    const int qq = (lane >> 2) & 3, pp = lane & 3;
    const int r0 = 4 * g + qq;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const int col = db * 16 + 4 * pp;
      va[db] = TILEB + r0 * ROWB + (v16_swz(r0, col >> 3) << 4) + (col & 7) * 2;
    }
  }
  const int nt = (a.nk + BKV - 1) / BKV;

  struct S8 {
    f32x4 v[4][2];
  };
  // S^T of the tile in slot BUF, keys past nk at -inf
  auto scores = [&](auto bufc, int t) -> S8 {
    constexpr int BUF = decltype(bufc)::value;
    const char* base = smem + BUF * 2 * TILEB;
    S8 s;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8 k0 = *(const bf16x8*)(base + ka[0] + kb * 16 * ROWB);
      const bf16x8 k1 = *(const bf16x8*)(base + ka[1] + kb * 16 * ROWB);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        s.v[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[qb][0], f32x4{}, 0, 0, 0);
        s.v[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[qb][1], s.v[kb][qb], 0, 0, 0);
      }
    }
    const int kv0 = t * BKV;
    if (kv0 + BKV > a.nk) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (kv0 + kb * 16 + 4 * g + i >= a.nk) {
            s.v[kb][0][i] = -INFINITY;
            s.v[kb][1][i] = -INFINITY;
          }
    }
    return s;
  };

  f32x4 o[4][2];  // [db][qb]: O^T[db*16 + 4g + i][query q0 + 16 qb]
  float l[2];     // lane-partial row sums
  float m[2] = {0.f, 0.f};  // row offsets (0 on the fast path)

  // p = exp2(s - m) rounded to bf16, row sums, O^T += V^T . P^T
  auto soft_pv = [&](auto bufc, int t, auto shc) {
    constexpr int BUF = decltype(bufc)::value;
    constexpr bool SHIFT = decltype(shc)::value;
    const char* base = smem + BUF * 2 * TILEB;
    const S8 s = scores(bufc, t);
    bf16x8 pf[2][2];  // [qb][kk]
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float rs = 0.f;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 tv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float x = s.v[2 * kk + (j >> 2)][qb][j & 3];
          if constexpr (SHIFT) x -= m[qb];
          const float p = __builtin_amdgcn_exp2f(x);
          rs += p;
          tv[j] = (__bf16)p;
        }
        pf[qb][kk] = tv;
      }
      l[qb] += rs;
    }
    const char* vb = base;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const char* p0 = vb + va[db] + kk * 32 * ROWB;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p0));
        const s16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_PTR(p0 + 16 * ROWB));
        const bf16x8 vf = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
          o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb][kk], o[db][qb], 0, 0, 0);
      }
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  // one sweep over the key tiles, double-buffered: body(slot, t)
  auto sweep = [&](auto body) {
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nt; t += 2) {
      if (t + 1 < nt) stage(1, t + 1);
      body(I0{}, t);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (t + 1 >= nt) break;
      if (t + 2 < nt) stage(0, t + 2);
      body(I1{}, t + 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  };
  auto reset = [&]() {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) o[db][qb] = f32x4{};
    l[0] = l[1] = 0.f;
  };
  // sum (or max) over the four 16-lane groups holding one query's keys
  auto allsum = [](float x) {
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
  };
  auto allmax = [](float x) {
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
  };

  // ---- fast path: offset 0 everywhere
  if (threadIdx.x == 0) redo = 0;  // ordered before the reads by the sweep's barriers
  reset();
  sweep([&](auto bufc, int t) { soft_pv(bufc, t, std::false_type{}); });
  l[0] = allsum(l[0]);
  l[1] = allsum(l[1]);
  const bool bad = !(l[0] >= 0x1p-60f && l[0] <= 0x1p100f) || !(l[1] >= 0x1p-60f && l[1] <= 0x1p100f);
  if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) redo = 1;
  __syncthreads();
  if (redo) {
    // ---- exact two-pass path: row max over all keys, then exp2(s - max)
    float mx[2] = {-INFINITY, -INFINITY};
    sweep([&](auto bufc, int t) {
      const S8 s = scores(bufc, t);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          mx[qb] = fmaxf(fmaxf(mx[qb], fmaxf(s.v[kb][qb][0], s.v[kb][qb][1])), fmaxf(s.v[kb][qb][2], s.v[kb][qb][3]));
    });
    m[0] = allmax(mx[0]);
    m[1] = allmax(mx[1]);
    reset();
    sweep([&](auto bufc, int t) { soft_pv(bufc, t, std::true_type{}); });
    l[0] = allsum(l[0]);
    l[1] = allsum(l[1]);
  }

  // ---- epilogue: normalise, O[q][d] bf16
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qrow = q0 + 16 * qb;
    const float inv = 1.f / l[qb];
    if (a.lse && g == 0 && qrow < a.nq) a.lse[((int64_t)b * a.heads + h) * a.nq + qrow] = m[qb] + __log2f(l[qb]);
    if (qrow < a.nq) {
      bf16_t* op = a.o + ((int64_t)b * a.obs + qrow) * a.ldo + h * D;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        uint2 pk;
        pk.x = pack_bf2(o[db][qb][0] * inv, o[db][qb][1] * inv);
        pk.y = pack_bf2(o[db][qb][2] * inv, o[db][qb][3] * inv);
        *(uint2*)(op + db * 16 + 4 * g) = pk;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Merge of the key-split tail (attn_fwd_kernel, VAR & V_KEY_SPLIT): for every row of
// the tail units, over its parts in index order (a fixed order: bitwise stable
// from run to run), M = max m_i, o = sum 2^(m_i - M) O_i / sum 2^(m_i - M) l_i,
// rounded to bf16 into the caller's o.  One thread per float4 of a partial, in
// the partial's own (register) order, so the loads are contiguous per wave and
// the stores are those of the unsplit epilogue.  Plain loads and stores only.
__global__ __launch_bounds__(256) void attn_split_merge_kernel(AttnArgs a, int n_tail) {
  constexpr int D = 64;
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int lane = tid & 63, c = (tid >> 6) & 7, wave = (tid >> 9) & 7, tu = tid >> 12;
  if (tu >= n_tail) return;
  const int nqb = (a.nq + SPLIT_BQ - 1) / SPLIT_BQ;
  const int tail_pp = a.unit_period - a.full_pp;  // the forward kernel's decode of tail unit tu
  const int bid = tu / tail_pp * a.unit_period + a.full_pp + tu % tail_pp;
  const int qb = bid % nqb, bh = bid / nqb;
  const int h = bh % a.heads, b = bh / a.heads;
  const int r = wave * 32 + (lane & 31), hl = lane >> 5;
  const int qrow = qb * SPLIT_BQ + r;
  if (qrow >= a.nq) return;
  const float* sp = a.ws + (int64_t)tu * a.parts * SPLIT_SLAB;
  float mx = -INFINITY;
  for (int p = 0; p < a.parts; ++p) mx = fmaxf(mx, sp[(int64_t)p * SPLIT_SLAB + SPLIT_BQ * D + r * 2]);
  f32x4 num = f32x4{0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
  for (int p = 0; p < a.parts; ++p) {
    const float* pp = sp + (int64_t)p * SPLIT_SLAB;
    const f32x2 ml = *(const f32x2*)(pp + SPLIT_BQ * D + r * 2);
    const float w = __builtin_amdgcn_exp2f(ml[0] - mx);
    num += w * *(const f32x4*)(pp + ((wave * 8 + c) * 64 + lane) * 4);
    den += w * ml[1];
  }
  const float inv = 1.f / den;
  uint2 pk;
  pk.x = pack_bf2(num[0] * inv, num[1] * inv);
  pk.y = pack_bf2(num[2] * inv, num[3] * inv);
  bf16_t* op = a.o + ((int64_t)b * a.obs + qrow) * a.ldo + h * D;
  *(uint2*)(op + (c >> 2) * 32 + 8 * (c & 3) + 4 * hl) = pk;
}

// The CUs the launch's split plan counts: the device's, whatever CU mask the stream
// carries -- a launch's bits depend on its shape and the device, not on its stream
inline int attn_cu_count() {
  static int dev_cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return dev_cus;
}

// ---- key-split plan: the slot model (host only, no device call) -----------
// A CU holds two 8-wave workgroups; the matrix pipe is what they share, so a
// workgroup alone on its CU runs twice as fast: a CU is one server of rate 2
// (tiles per tile time) shared by its residents.  Workgroups are dispatched in
// index order to the CU with the fewest residents as slots free up.  Lengths
// in 64-key tiles, plus PLAN_UNIT_OVH tiles per workgroup for what does not
// overlap (Q fragments, the first tile's DMA, the epilogue).
constexpr double PLAN_UNIT_OVH = 2.0;
// one tile time of a paired workgroup: 1.284 ms / (2 rounds x 344 tiles) at
// nq = nk = 16,384 (profiles/r10/attn_quant_r10l.txt); the partials move at
// about 3.5 TB/s (written once, read once), the merge launch costs ~5 us
constexpr double PLAN_TILE_US = 1.87, PLAN_BYTES_PER_US = 3.5e6, PLAN_MERGE_US = 5.0;
// Split only for a modelled gain of at least this fraction of the launch.  The
// model over-predicts: at 21,984 x 16 heads on 256 CUs it gives 6.5 / 4.8 / 2.7 %
// for 2 / 4 / 3 parts, measured 2.9 / 2.4 / 1.1 % (1.701 -> 1.651 / 1.656-1.667 /
// 1.680 ms, spread within an arm 0.3 %: profiles/r12/ab_attn_tail_split.md), so
// 3 % modelled is about 1.3 % measured, four times that spread.
constexpr double PLAN_MIN_GAIN = 0.03;
// ... and only with parts no shorter than the shortest measured to pay (4 parts of
// 21,984 keys): a part's fixed cost (Q fragments, first tile, partial store, its
// share of the merge) is unmeasured against fewer tiles
constexpr int PLAN_MIN_PART_TILES = 86;

struct PlanSeg {
  int count;
  double len;
};
double plan_makespan(int cus, const PlanSeg* segs, int nseg) {
  std::vector<double> rem((size_t)cus * 2, 0.0);
  std::vector<int> cnt((size_t)cus, 0);
  int seg = 0, left = nseg > 0 ? segs[0].count : 0, resident = 0;
  double now = 0.0;
  auto more = [&]() {
    while (seg < nseg && left == 0) {
      ++seg;
      if (seg < nseg) left = segs[seg].count;
    }
    return seg < nseg;
  };
  for (;;) {
    // dispatch: every free slot takes the next workgroup, emptiest CUs first
    for (int want = 0; want < 2; ++want)
      for (int cu = 0; cu < cus; ++cu)
        if (cnt[cu] == want && more()) {
          rem[cu * 2 + cnt[cu]] = segs[seg].len;
          ++cnt[cu];
          --left;
          ++resident;
        }
    if (resident == 0) return now;
    double dt = 1e300;
    for (int cu = 0; cu < cus; ++cu)
      for (int i = 0; i < cnt[cu]; ++i) dt = std::min(dt, rem[cu * 2 + i] * cnt[cu] * 0.5);
    now += dt;
    for (int cu = 0; cu < cus; ++cu) {
      const int n = cnt[cu];
      const double done = dt * 2.0 / (n > 0 ? n : 1);
      int keep = 0;
      for (int i = 0; i < n; ++i) {
        const double r = rem[cu * 2 + i] - done;
        if (r > 1e-9) rem[cu * 2 + keep++] = r;
        else --resident;
      }
      cnt[cu] = keep;
    }
  }
}

// parts as run: whole tiles per part, the last part takes the rest and is not empty
inline void split_shape(int nt, int want, int* parts, int* part_tiles) {
  const int p = std::max(1, std::min(want, nt));
  *part_tiles = (nt + p - 1) / p;
  *parts = (nt + *part_tiles - 1) / *part_tiles;
}

}  // namespace

// Host policy of the key-split tail (see vggt_attention_fwd_ws): 1 and
// (*tail_blocks, *parts) when a launch of this shape on `cus` CUs should run
// the last *tail_blocks row-block units of every batch element split over the
// keys, else 0.  The plan is that of one batch element alone -- the row blocks
// of its last, partial round of workgroups -- whatever `batch` is: an element
// gets the same split rows in the same parts alone or in any batch, so its
// bits do not depend on what it is batched with.  Pure host arithmetic: no
// device is touched.
extern "C" int vggt_attention_split_plan(int batch, int heads, int nq, int nk, int D, int cus, int* tail_blocks,
                                         int* parts) {
  if (tail_blocks) *tail_blocks = 0;
  if (parts) *parts = 0;
  if (batch <= 0 || heads <= 0 || nq < 4096 || nk <= 0 || D != 64 || cus <= 0) return 0;
  const int64_t units64 = (int64_t)((nq + SPLIT_BQ - 1) / SPLIT_BQ) * heads;
  const int slots = 2 * cus, nt = (nk + BKV - 1) / BKV;
  if (units64 < slots || units64 > (1 << 24) || units64 % slots == 0 || nt < 2) return 0;
  const int units = (int)units64, tail = units % slots;
  struct Entry {
    int key[4], tail, parts;
  };
  static std::mutex mu;
  static std::vector<Entry> cache;
  const int key[4] = {units, nq, nk, cus};
  std::lock_guard<std::mutex> lk(mu);
  const Entry* hit = nullptr;
  for (const Entry& e : cache)
    if (!memcmp(e.key, key, sizeof key)) hit = &e;
  if (!hit) {
    const PlanSeg whole[1] = {{units, nt + PLAN_UNIT_OVH}};
    const double t0 = plan_makespan(cus, whole, 1);
    double best = t0;
    int best_p = 0;
    for (int want = 2; want <= 4; ++want) {
      int p, pt;
      split_shape(nt, want, &p, &pt);
      if (p != want || pt < PLAN_MIN_PART_TILES) continue;
      const PlanSeg segs[3] = {{units - tail, nt + PLAN_UNIT_OVH},
                               {tail * (p - 1), pt + PLAN_UNIT_OVH},
                               {tail, nt - (p - 1) * pt + PLAN_UNIT_OVH}};
      // the dispatch order interleaves the parts of a unit; the p - 1 equal parts first is
      // the same multiset of lengths, and the last part differs by less than a tile per part
      const double bytes = 2.0 * tail * p * SPLIT_SLAB * 4.0;
      const double t = plan_makespan(cus, segs, 3) + (bytes / PLAN_BYTES_PER_US + PLAN_MERGE_US) / PLAN_TILE_US;
      if (t < best) best = t, best_p = want;
    }
    if (cache.size() >= 64) cache.clear();
    cache.push_back(Entry{{units, nq, nk, cus}, tail, (t0 - best) >= PLAN_MIN_GAIN * t0 ? best_p : 0});
    hit = &cache.back();
  }
  if (hit->parts < 2) return 0;
  if (tail_blocks) *tail_blocks = hit->tail;
  if (parts) *parts = hit->parts;
  return 1;
}

namespace {
// what the VGGT_TUNE_ATTN_TAIL_SPLIT knob and the plan make of a launch that takes the
// 8-wave D = 64 default path, as run (0 parts: unsplit): of every `period` consecutive units the last `tail`
// in `parts` workgroups each.  The plan and the per-element forced form split within each batch element
// (period: its units), the launch-global forced form within the whole launch (one period)
struct TailSplit {
  int period, periods, tail, parts, part_tiles;
  size_t ws_bytes() const { return (size_t)periods * tail * parts * SPLIT_SLAB * sizeof(float); }
};
TailSplit tail_split_of(int batch, int heads, int nq, int nk) {
  TailSplit ts = {0, 0, 0, 0, 0};
  const int knob = g_vggt_attn_tail_split;
  const int64_t per_elem = (int64_t)((nq + SPLIT_BQ - 1) / SPLIT_BQ) * heads, units = per_elem * batch;
  const int nt = (nk + BKV - 1) / BKV;
  int t = 0, p = 0;
  if (knob < 0 || units > (1 << 18)) return ts;  // (the merge kernel indexes 4096 threads per tail unit in 32 bits)
  bool global = false;
  if (knob > 0) {
    p = knob & 0xff;
    global = !(knob & VGGT_ATTN_TAIL_SPLIT_PER_ELEMENT);
    t = (int)std::min<int64_t>((knob & ~VGGT_ATTN_TAIL_SPLIT_PER_ELEMENT) >> 8, global ? units : per_elem);
  } else if (!vggt_attention_split_plan(1, heads, nq, nk, 64, attn_cu_count(), &t, &p)) {
    return ts;
  }
  int pr, pt;
  split_shape(nt, std::min(p, 4), &pr, &pt);
  if (pr < 2 || t <= 0) return ts;
  ts.period = (int)(global ? units : per_elem);
  ts.periods = global ? 1 : batch;
  ts.tail = t;
  ts.parts = pr;
  ts.part_tiles = pt;
  return ts;
}

// ---- which kernel a launch runs -------------------------------------------
struct AttnForm {
  bool form16;     // attn16_fwd_kernel<nw> (var 0: it has no schedule bits), else attn_fwd_kernel<D, nw, var>
  int nw, var;
  bool key_split;  // the one form whose launch may take the key-split tail (var | V_KEY_SPLIT)
};

// The one place that maps the knobs to a kernel: (public variant id, VGGT_TUNE_ATTN_WAVES,
// VGGT_TUNE_ATTN16, VGGT_ATTN_DMA_HALF, D, nq) -> form.  Pure arithmetic, first match wins.
AttnForm attn_resolve(int variant, int waves, int attn16, int dma_half, int D, int nq) {
  // 8-wave workgroups (256 query rows) for long sequences; 4-wave ones (128 rows) when the query count is short
  // enough that the padding of a 256-row block would cost more than the pairing gains; 2-wave ones (64 rows) for grids
  // that fill a fraction of one round of slots -- only ids that reduce to 33 below (hoisted K, offset-free, not exact)
  const bool two_ok = (variant & V_OFFSET_FREE) && (variant & (V_EXACT | V_HOIST_K)) == V_HOIST_K;
  const int nw = (waves == 8 && nq >= 4096) ? 8 : (waves == 2 && two_ok) ? 2 : 4;
  const bool d64 = D == 64, wide = d64 && nw != 2;  // the special forms below are D = 64 only, most 4 / 8 waves only
  // 16x16x32 matrix-core form: 161 forces it; 33 takes it with VGGT_ATTN16=1, or =2 (default) for the 4-wave
  // (nq < 4096: frame / DINOv2) launches only.  All launches: faster back to back in kbench (profiles/r6c: global 1.80
  // vs 1.83 ms, frame 128-134 vs 135-137 us) but not in the model (r6d: global 1.87 vs 1.84 ms, step 100.8 vs 100.5 ms)
  if (wide && (variant == V_161 || (variant == V_33 && (attn16 == 1 || (attn16 == 2 && nw == 4)))))
    return {true, nw, 0, false};
  if (d64 && (variant == V_19 || variant == V_23)) return {false, nw, variant, false};  // (never 2 waves: not two_ok)
  // Default (round 6): the 8-wave D = 64 form of 33 issues its LDS-DMA from the priority half only (2081): global
  // attention 1,858-1,860 -> 1,814-1,819 us, aggregator step 97.66-97.75 -> 96.56-97.21 ms, interleaved on one box
  // (profiles/r11/ab_attn_dma_half.md).  VGGT_ATTN_DMA_HALF=0: every wave issues its piece.
  if (d64 && nw == 8 && variant == V_33 && dma_half) return {false, 8, V_2081, true};
  // 2081 / 4129 differ from 33 in the 8-wave form only
  if (wide && (variant == V_2081 || variant == V_4129)) return {false, nw, nw == 8 ? variant : V_33, false};
  if (wide && (variant == V_545 || variant == V_289)) return {false, nw, variant, false};
  // Every other offset-free launch keeps the hoist and exact-score bits alone: 32 / 33 / 96 / 97
  // as they are, and 161 / 289 / 545 / 2081 / 4129 run 33 at D = 128 and in 2-wave groups
  // (their own forms are D = 64, 4 / 8 waves; two_ok admits exactly the ids that land on 33 here)
  if (variant & V_OFFSET_FREE) return {false, nw, variant & (V_OFFSET_FREE | V_EXACT | V_HOIST_K), false};
  // The max-tracking form: 3 / 7 / 11 / 15, and 19 / 23 at D = 128 (no 3-slot form there) run 3 / 7
  return {false, nw, variant & V_LEGACY, false};
}

AttnForm attn_resolve_now(int D, int nq) {
  return attn_resolve(g_vggt_attn_variant, g_vggt_attn_waves, g_vggt_attn16, g_vggt_attn_dma_half, D, nq);
}

// Every attn_fwd_kernel the library holds, as X(D, NW, VAR)
#define VGGT_ATTN_D_NW(X, V) X(64, 4, V) X(64, 8, V) X(128, 4, V) X(128, 8, V)
#define VGGT_ATTN_KERNELS(X)                                                                              \
  VGGT_ATTN_D_NW(X, V_HOIST_K | V_MAX4) VGGT_ATTN_D_NW(X, V_HOIST_K | V_MAX4 | V_SUM4)                    \
  VGGT_ATTN_D_NW(X, V_HOIST_K | V_MAX4 | V_MFMA_SUM) VGGT_ATTN_D_NW(X, V_LEGACY)                          \
  VGGT_ATTN_D_NW(X, V_OFFSET_FREE) VGGT_ATTN_D_NW(X, V_33)                                                \
  VGGT_ATTN_D_NW(X, V_96) VGGT_ATTN_D_NW(X, V_96 | V_HOIST_K)                                             \
  X(64, 2, V_33) X(128, 2, V_33)                                                                          \
  X(64, 4, V_19) X(64, 8, V_19) X(64, 4, V_23) X(64, 8, V_23)                                             \
  X(64, 4, V_289) X(64, 8, V_289) X(64, 4, V_545) X(64, 8, V_545)                                         \
  X(64, 8, V_2081) X(64, 8, V_2081 | V_KEY_SPLIT) X(64, 8, V_4129)                                        \
  X(64, 4, V_33 | V_STAMPS) X(64, 8, V_33 | V_STAMPS) X(64, 8, V_2081 | V_STAMPS) X(64, 8, V_4129 | V_STAMPS)

// Whether the library holds the kernel of form `f`
bool attn_has(const AttnForm& f, int D) {
  if (f.form16) return D == 64 && (f.nw == 4 || f.nw == 8);
#define VGGT_ATTN_IS(DD, NWW, V) \
  if (D == DD && f.nw == NWW && f.var == (V)) return true;
  VGGT_ATTN_KERNELS(VGGT_ATTN_IS)
#undef VGGT_ATTN_IS
  return false;
}

// Launches the kernel of form `f` on `grid` workgroups (VGGT_ERR_UNSUPPORTED: the library does not hold it)
int attn_launch(const AttnForm& f, int D, const AttnArgs& a, int grid, hipStream_t s) {
  if (!attn_has(f, D)) return VGGT_ERR_UNSUPPORTED;
  if (f.form16) {
    if (f.nw == 8) attn16_fwd_kernel<8><<<grid, 512, 0, s>>>(a);
    else attn16_fwd_kernel<4><<<grid, 256, 0, s>>>(a);
  }
#define VGGT_ATTN_TRY(DD, NWW, V) \
  else if (D == DD && f.nw == NWW && f.var == (V)) attn_fwd_kernel<DD, NWW, (V)><<<grid, NWW * 64, 0, s>>>(a);
  VGGT_ATTN_KERNELS(VGGT_ATTN_TRY)
#undef VGGT_ATTN_TRY
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

// The stamped form (vggt_attention_stamps): always D = 64 on the 32x32x16 kernel (VGGT_TUNE_ATTN16
// is ignored), 2 waves taken as 4.  In the 8-wave form 2081 when the variant is 2081, or is 33 with
// dma_half; 4129 when it is 4129; 33 for every other variant.  In the 4-wave form always 33.
AttnForm attn_resolve_stamps(int variant, int waves, int dma_half, int nq) {
  const int v = (variant == V_2081 || variant == V_4129) ? variant : V_33;
  AttnForm f = attn_resolve(v, waves == 2 ? 4 : waves, 0, variant == V_33 && dma_half, 64, nq);
  f.var |= V_STAMPS;
  return f;
}

// The checks and the kernel arguments every forward entry shares (lse: see AttnArgs)
int attn_args(AttnArgs* a, const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
              int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o, int64_t ldo, int64_t o_bstride,
              int batch, int heads, int nq, int nk, int D, float scale, float* lse) {
  if (batch <= 0 || heads <= 0 || nq <= 0 || nk <= 0) return VGGT_ERR_SHAPE;
  if (D != 64 && D != 128) return VGGT_ERR_UNSUPPORTED;
  if ((ldq | ldk | ldv | ldo) % 8 || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16)
    return VGGT_ERR_ALIGN;
  // 32-bit DMA offsets and descriptor arithmetic: K / V of one (batch, head) must span < 2 GiB
  if ((uint64_t)nk * (uint64_t)(ldk > ldv ? ldk : ldv) * 2 >= (1ull << 31)) return VGGT_ERR_SHAPE;
  *a = AttnArgs{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, ldq, ldk, ldv, ldo,
                q_bstride, k_bstride, v_bstride, o_bstride, batch, heads, nq, nk,
                scale * 1.4426950408889634f, lse};
  return VGGT_OK;
}

int attn_grid(int nw, int batch, int heads, int nq) { return ((nq + nw * 32 - 1) / (nw * 32)) * heads * batch; }
}  // namespace

// Which forward kernel vggt_attention_fwd launches for (D, nq) under the current knobs: the
// sibling of vggt_attention_split_plan (host arithmetic, no device call).
extern "C" int vggt_attention_fwd_form(int D, int nq, int* form16, int* waves, int* var) {
  const AttnForm f = attn_resolve_now(D, nq);
  if (form16) *form16 = f.form16;
  if (waves) *waves = f.nw;
  if (var) *var = f.var;
  if (D != 64 && D != 128) return VGGT_ERR_UNSUPPORTED;
  return attn_has(f, D) ? VGGT_OK : VGGT_ERR_UNSUPPORTED;
}

// The same for vggt_attention_stamps (D = 64; *var includes the stamps bit)
extern "C" int vggt_attention_stamps_form(int nq, int* waves, int* var) {
  const AttnForm f = attn_resolve_stamps(g_vggt_attn_variant, g_vggt_attn_waves, g_vggt_attn_dma_half, nq);
  if (waves) *waves = f.nw;
  if (var) *var = f.var;
  return attn_has(f, 64) ? VGGT_OK : VGGT_ERR_UNSUPPORTED;
}

extern "C" size_t vggt_attention_ws_bytes(int batch, int heads, int nq, int nk, int D, void* stream) {
  if (batch <= 0 || heads <= 0 || nq <= 0 || nk <= 0 || !attn_resolve_now(D, nq).key_split) return 0;
  (void)stream;  // the split is a function of the shape, the knob and the device alone
  return tail_split_of(batch, heads, nq, nk).ws_bytes();
}

// vggt_attention_fwd with a workspace: the only entry that may run the last, partial round of workgroups of the
// 8-wave D = 64 default path split over the keys (vggt_attention_ws_bytes says how much it needs for this shape
// under the current VGGT_TUNE_ATTN_TAIL_SPLIT; with ws == NULL it never splits).
extern "C" int vggt_attention_fwd_ws(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                                     int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o,
                                     int64_t ldo, int64_t o_bstride, int batch, int heads, int nq, int nk, int D,
                                     float scale, void* ws, size_t ws_bytes, void* stream) {
  if (ws && (uintptr_t)ws % 16) return VGGT_ERR_ALIGN;
  AttnArgs a;
  const int rc = attn_args(&a, q, ldq, q_bstride, k, ldk, k_bstride, v, ldv, v_bstride, o, ldo, o_bstride, batch, heads,
                           nq, nk, D, scale, nullptr);
  if (rc != VGGT_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  AttnForm f = attn_resolve_now(D, nq);
  const int nwg = attn_grid(f.nw, batch, heads, nq);
  TailSplit ts = {0, 0, 0, 0, 0};
  if (f.key_split && ws) ts = tail_split_of(batch, heads, nq, nk);
  if (ts.parts < 2) return attn_launch(f, D, a, nwg, s);
  // key-split tail: the last `tail` units of every period as `parts` workgroups each behind all
  // the whole units, in the same launch; then the merge of their partials, on the same stream
  if (ws_bytes < ts.ws_bytes()) return VGGT_ERR_SHAPE;
  const int tail = ts.periods * ts.tail;
  a.n_full = nwg - tail;
  a.parts = ts.parts;
  a.part_tiles = ts.part_tiles;
  a.ws = (float*)ws;
  a.unit_period = ts.period;
  a.full_pp = ts.period - ts.tail;
  f.var |= V_KEY_SPLIT;
  const int rc2 = attn_launch(f, D, a, a.n_full + tail * ts.parts, s);
  if (rc2 != VGGT_OK) return rc2;
  attn_split_merge_kernel<<<tail * 16, 256, 0, s>>>(a, tail);
  HIP_LAUNCH_CHECK();
  return VGGT_OK;
}

extern "C" int vggt_attention_fwd(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                                  int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o,
                                  int64_t ldo, int64_t o_bstride, int batch, int heads, int nq, int nk, int D,
                                  float scale, void* stream) {
  return vggt_attention_fwd_ws(q, ldq, q_bstride, k, ldk, k_bstride, v, ldv, v_bstride, o, ldo, o_bstride, batch,
                               heads, nq, nk, D, scale, nullptr, 0, stream);
}

// Diagnostic: the default forward with s_memtime segment stamps (V_STAMPS; the form: attn_resolve_stamps)
extern "C" int vggt_attention_stamps(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                                     int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o,
                                     int64_t ldo, int64_t o_bstride, unsigned long long* stamps, int batch, int heads,
                                     int nq, int nk, float scale, void* stream) {
  if (!stamps) return VGGT_ERR_SHAPE;
  AttnArgs a;
  const int rc = attn_args(&a, q, ldq, q_bstride, k, ldk, k_bstride, v, ldv, v_bstride, o, ldo, o_bstride, batch, heads,
                           nq, nk, 64, scale, (float*)(void*)stamps);
  if (rc != VGGT_OK) return rc;
  const AttnForm f = attn_resolve_stamps(g_vggt_attn_variant, g_vggt_attn_waves, g_vggt_attn_dma_half, nq);
  return attn_launch(f, 64, a, attn_grid(f.nw, batch, heads, nq), (hipStream_t)stream);
}

// Training recompute (alignment-head frame blocks under checkpoint, SURVEY §8f
// row 4): the exact-score offset-free form (variant 96: no Q prescale, so the
// backward's recomputed scores match bit for bit) that also stores the per-row
// log2-sum-exp consumed by vggt_attention_bwd; its rows take their first tile's
// max as the offset, O is normalised by the sum of the bf16-rounded p (lb_run),
// the lse comes from the unrounded sum.  Always the 4-wave 32x32x16 form.
extern "C" int vggt_attention_fwd_lse(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                                      int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o,
                                      int64_t ldo, int64_t o_bstride, float* lse, int batch, int heads, int nq, int nk,
                                      int D, float scale, void* stream) {
  if (!lse) return VGGT_ERR_SHAPE;
  AttnArgs a;
  const int rc = attn_args(&a, q, ldq, q_bstride, k, ldk, k_bstride, v, ldv, v_bstride, o, ldo, o_bstride, batch, heads,
                           nq, nk, D, scale, lse);
  if (rc != VGGT_OK) return rc;
  return attn_launch(AttnForm{false, 4, V_96, false}, D, a, attn_grid(4, batch, heads, nq), (hipStream_t)stream);
}
