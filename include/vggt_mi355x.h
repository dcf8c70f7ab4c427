/*
 * vggt_mi355x.h -- C ABI of the MI355X (gfx950) hot path for the per-chunk
 * VGGT forward + feature-alignment head of ruppelb/Large-Scale-ViT-SLAM.
 *
 * The reference has no FFI: every op on its hot path is a stock PyTorch op
 * called from Python.  Each entry point below replaces one
 * such op (or a fused group of them); the reference call site it stands in
 * for is cited per function.  All pointers are DEVICE pointers owned by the
 * caller; nothing here allocates.  `stream` is a hipStream_t passed as void*.
 * Every function returns VGGT_OK (0) or a negative error code and never
 * throws; the Python host layer turns codes into RuntimeError, mirroring the
 * reference's assert/ValueError conventions (alignment_head.py:86,:251;
 * cross_attention.py:30,:50).
 *
 * Data types: "bf16" buffers hold raw bfloat16 bits (uint16); "f32" is IEEE
 * float.  Leading dimensions (ld*) are in ELEMENTS.  Row-major everywhere.
 */
#ifndef VGGT_MI355X_H
#define VGGT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGT_OK 0
#define VGGT_ERR_SHAPE (-1)       /* unsupported / inconsistent shape        */
#define VGGT_ERR_ALIGN (-2)       /* pointer or leading dim misaligned       */
#define VGGT_ERR_HIP (-3)         /* HIP launch / runtime error              */
#define VGGT_ERR_UNSUPPORTED (-4) /* unsupported mode / dtype                */

#define VGGT_DTYPE_F32 0
#define VGGT_DTYPE_BF16 1

/* GEMM epilogues (all round acc+bias to bf16 first, = autocast Linear out) */
#define VGGT_EPI_BF16 0      /* out_bf16 = bf16(acc + bias)                               */
#define VGGT_EPI_GELU_BF16 1 /* out_bf16 = bf16(gelu(bf16(acc + bias)))   (Mlp fc1 + GELU) */
#define VGGT_EPI_RESID_F32 2 /* out_f32 += gamma * bf16(acc + bias) [; out2 = out_f32]      */
#define VGGT_EPI_F32 3       /* out_f32 = bf16(acc + bias) widened to f32                  */

/* RoPE modes of vggt_headnorm_rope */
#define VGGT_ROPE_NONE 0
#define VGGT_ROPE_2D 1 /* VGGT RotaryPositionEmbedding2D: half D by y, half by x      */
#define VGGT_ROPE_1D 2 /* aligned_vggt/layers/rope.py RotaryPositionEmbedding          */

/* Library identification (build string) -- for load checks. */
const char* vggt_version(void);

/* Process-wide kernel-variant knobs (defaults: the VGGT_GEMM / VGGT_ATTN_WAVES
 * environment variables, else the tuned choice).  Returns the previous value,
 * or VGGT_ERR_UNSUPPORTED for an unknown knob / value.  Results do not depend
 * on the variant beyond fp32 summation order inside one MFMA tile. */
#define VGGT_TUNE_GEMM_TILE 1  /* -1 auto, 0: 128x128 tile, 1: 256x256 ring, 2: 256x128 ring, 3: ping-pong (width by
                                  round quantisation), 4/5/6: ping-pong 256/192/128 wide, 7: ping-pong 256 wide when
                                  that fills two rounds of CUs, else as 3, 8: two-per-CU 256x128 (32x32x16 MFMA),
                                  9: persistent 256x256 ping-pong with register epilogue (bf16 / GELU / f32
                                  epilogues, N <= 4096; others as 7) */
#define VGGT_TUNE_ATTN_WAVES 2 /* 2, 4 or 8 waves (64 / 128 / 256 query rows) per attention workgroup */
#define VGGT_TUNE_ATTN_VARIANT 3 /* attention forward schedule, one of: 33 offset-free softmax (default), 32 the same
                                    without hoisted K reads, 96 / 97 = 32 / 33 with exact scores, 3 / 7 / 11 / 15 the
                                    max-tracking kernel (the other values below 16 are retired: VGGT_ERR_UNSUPPORTED),
                                    19 / 23 pipelined QK^T, 161 = 33 on the 16x16x32 matrix-core form, 289 split-tile
                                    pipeline, 545 DMA two tiles ahead, 2081 DMA from the priority half, 4129 no
                                    priority raise (D = 64 forms: at D = 128 these run 33, and 19 / 23 run 3 / 7).
                                    Env VGGT_ATTN_VARIANT (a value not listed here: the default) */
#define VGGT_TUNE_CONV_PF2 4     /* split-bf16 conv gather: 1 two-deep (buffer loads, default), 0 one-deep */
#define VGGT_TUNE_ATTN16 5       /* 1: D = 64 attention on the 16x16x32 matrix-core form, 0: 32x32x16 (default),
                                    2: 16x16x32 for 4-wave (nq < 4096) launches only */
#define VGGT_TUNE_LINEAR_ONE_LAUNCH 6 /* vggt_linear_f32_ws split-K: 1 the last split block of a tile combines the
                                         partials in the same launch (default), 0 a separate reduce launch (same
                                         fixed summation order: bitwise equal; kept for A/B and tests) */
#define VGGT_TUNE_LINEAR_SPLIT_K 7 /* vggt_linear_f32_ws split-K: split while each split keeps at least this many
                                      k (power of two, 16..4096; default 128).  Changes the fp32 summation order */
#define VGGT_TUNE_LINEAR_WK 8 /* vggt_linear_f32_ws with M <= 256: 0 the split-K form above, else the k range
                                 (power of two, 64..4096; default 64) each wave of an in-workgroup split keeps (2..8 waves on
                                 16 columns x 64 rows, partials summed in LDS: no scratch, no counters; the split depends
                                 on K only, so each row's bits do not depend on M) */
/* (knob 9 is unassigned: a round-balance split of the global attention measured no faster) */
#define VGGT_TUNE_GEMM_BALANCE 10 /* vggt_gemm_bf16 on the persistent form: 1 the whole rounds of row panels
                                     persistent and the remaining rows on the 128x128 form when the last round
                                     would be under 60 % full (bitwise equal), 0 one launch */
#define VGGT_TUNE_ATTN_TAIL_SPLIT 11 /* vggt_attention_fwd_ws, 8-wave D = 64 default path: 0 (default) the row blocks
                                        of the last, partial round of workgroups of ONE batch element run split over
                                        the keys, in every batch element alike, when the slot model says it pays
                                        (vggt_attention_split_plan on the device's CUs: an element's bits depend on
                                        its shape and the device, not on the batch or the stream's CU mask), -1 never
                                        (bitwise vggt_attention_fwd), parts | tail_blocks << 8 forced: the last
                                        tail_blocks (batch, head, row block) units of the launch in parts (2..4,
                                        clamped to the 64-key tile count) workgroups each;
                                        VGGT_ATTN_TAIL_SPLIT_PER_ELEMENT | parts | tail_blocks << 8 forced: the last
                                        tail_blocks (head, row block) units of every batch element (tail_blocks
                                        below 2^22).  Env VGGT_ATTN_TAIL_SPLIT */
#define VGGT_ATTN_TAIL_SPLIT_PER_ELEMENT (1 << 30)
/* (knob 6, the persistent GEMM's DMA-placement bits, is retired: its measured-best placement is the only
   one compiled; vggt_tune(6, ...) returns VGGT_ERR_UNSUPPORTED) */
int vggt_tune(int knob, int value);

/* Per-stream launch configuration, host-side only (no GPU call); no reference
 * counterpart: the MI355X multi-GPU pipeline's encode stream (aligned_vggt/dist/pipeline.py).
 *   cus    the CUs launches on `stream` may occupy (a stream created with
 *          hipExtStreamCreateWithCUMask; 0 = the device's): the persistent kernels size
 *          their one-workgroup-per-CU grids and tile-rounding heuristics to it;
 *   flags  VGGT_STREAM_SHORT_WORKGROUPS: no persistent GEMM forms on this stream -- every
 *          workgroup runs one output tile, so kernels of a concurrent high-priority stream
 *          (the alignment recurrence) find free CUs within microseconds instead of
 *          waiting for a whole persistent launch.  Results are unchanged up to fp32
 *          summation order inside a tile.
 * cus = flags = 0 forgets the stream.  Returns the previous setting (cus | flags << 16,
 * 0 if none), or VGGT_ERR_* (up to 16 streams). */
#define VGGT_STREAM_SHORT_WORKGROUPS 1
int vggt_set_stream_config(void* stream, int cus, int flags);

/*
 * out[M,N] = epi( A[M,K] . W[N,K]^T + bias[N] ), bf16 MFMA (v_mfma_f32_16x16x32_bf16),
 * fp32 accumulation.  Replaces every autocast nn.Linear on the bf16 tier:
 * vggt Attention.qkv/proj, Mlp.fc1/fc2 (aggregator / DINOv2 blocks, via
 * featureAligned_vggt.py:78), CrossAttention.q/k/v/proj (cross_attention.py:37-43,55-57,76),
 * AlignmentHead.project_in (alignment_head.py:242), and the DINOv2 patch-embed
 * conv as an im2col GEMM.  Requires N % 128 == 0, K % 32 == 0, 16-B aligned
 * rows (rows past M are never read or written).  `gamma`/`out2`/`ldo2`
 * are used by VGGT_EPI_RESID_F32 only (LayerScale; out2 may be NULL).
 */
int vggt_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int M, int N, int K,
                   int epi, void* out, int64_t ldo, const float* gamma, float* out2, int64_t ldo2, void* stream);

/*
 * vggt_gemm_bf16 with VGGT_EPI_GELU_BF16 that also stores the bf16 pre-activation A.W^T + bias to `pre`
 * (row stride ldp): the training recompute of Mlp.fc1 -> GELU keeps both for the GELU backward
 * (alignment_head.py:351-393 under checkpoint), in one pass instead of a GEMM + a separate GELU kernel.
 */
int vggt_gemm_bf16_gelu_pre(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int M, int N,
                            int K, void* out, int64_t ldo, void* pre, int64_t ldp, void* stream);

/*
 * Fused attention input projection: qkv[M, 3*H*D] = bf16(A . W^T + bias), then,
 * in the same epilogue, the q and k column blocks get the per-head LayerNorm
 * (q_norm / k_norm: weights [D], eps; NULL weights = no norm) and RoPE
 * (rope_mode/pos/period/cos/sin as vggt_headnorm_rope), computed in fp32 on
 * the bf16 linear outputs and rounded once; the v block is stored as is.
 * Every tile form gives bitwise the values of vggt_gemm_bf16 followed by
 * vggt_qknorm_rope (the same helpers and test).
 * Replaces qkv Linear + q_norm/k_norm + rope of VGGT Attention.forward (ext
 * layers/attention.py; aggregator frame/global blocks and the alignment
 * head's frame blocks, alignment_head.py:351-366).  D in {64, 128},
 * (H*D) % 128 == 0, K % 32 == 0.
 */
int vggt_gemm_qkv(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int M, int H, int D, int K,
                  void* out, int64_t ldo, const float* qw, const float* qb, const float* kw, const float* kb, float eps,
                  int rope_mode, const int32_t* pos, int period, const float* cos_tab, const float* sin_tab,
                  int tab_len, void* stream);

/*
 * The same fused epilogue on the separate projections of a cross attention:
 * out[M, N] = bf16(A . W^T + bias) with the FIRST H*D columns normalised
 * (weights nw/nb [D], NULL = no norm) and rotated (rope_mode/pos/period as
 * above; row m takes position pos[m % period]) and, for N = 2*H*D, the
 * second block stored as is.  N = H*D: a q projection (+ q_norm + RoPE);
 * N = 2*H*D: a packed kv projection (+ k_norm + RoPE on k).  Replaces the
 * q / kv Linears + vggt_headnorm_rope pair of the alignment head's temporal
 * blocks (CrossAttention, alignment_head.py:369-380): bitwise the same
 * values on every tile form (one fp32 evaluation order, csrc/common.h hn_*;
 * asserted by tests/test_gpu_gemm_edges.py), one HBM pass fewer.  Shape rules
 * as vggt_gemm_qkv.
 */
int vggt_gemm_headnorm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int M, int N, int H,
                       int D, int K, void* out, int64_t ldo, const float* nw, const float* nb, float eps, int rope_mode,
                       const int32_t* pos, int period, const float* cos_tab, const float* sin_tab, int tab_len,
                       void* stream);

/*
 * Which kernel the four GEMM entry points above launch: host arithmetic only, no device call (without a
 * device the device CU count is taken as 256).  The answer is the dispatcher's own (gemm_resolve in
 * csrc/gemm.hip), under the process's current VGGT_TUNE_GEMM_TILE / VGGT_TUNE_GEMM_BALANCE and VGGT_GEMM_* /
 * VGGT_HEADNORM_TILE environment knobs (INTEGRATION.md lists them).
 *   entry         VGGT_GEMM_ENTRY_*; epi is read for ENTRY_BF16 only, has_out2 for GELU_PRE only (whether `pre`
 *                 is given), N for ENTRY_BF16 / GELU_PRE / HEADNORM (QKV: 3 H D), H / D / rope_mode / period /
 *                 tab_len for the two fused entries;
 *   lda .. ldo2   the leading dimensions of the call (they feed the two 2^31-byte offset guards);
 *   stream_cus    what vggt_set_stream_config gave the stream (0: unconfigured), stream_flags likewise;
 *   force         -1; 9 / 0 ask for the first / second launch of a balance split (M = split_rows / the rest).
 * The rule: a fixed tile mode runs its form -- 0 the 128x128 form, 1 / 2 the 256- / 128-wide ring, 3-7 the
 * ping-pong form (3 / 7 pick the width by rounds of 256-row tiles over the device's CUs, 4 / 5 / 6 ask for
 * 256 / 192 / 128 and fall back to the pick where N is no multiple; 192 never with D = 128 heads), 8 the
 * two-per-CU form, 9 the persistent form -- after these fallbacks: K % 64 != 0 takes modes 0 and 3-7 (and a
 * persistent request) to the 128-wide ring; mode 1 needs N (fused: H D) % 256 == 0, else mode 2; mode 9
 * needs N % 256 == 0, N <= 4096, a 256-row output panel under 2^31 bytes, and for the fused entries
 * vggt_gemm_qkv with D = 64, RoPE none / 2-D, tab_len <= 256 and its tables within 160 KiB of LDS, else it
 * runs the 128x128 form (residual epilogue) or mode 7.  Every mode but 0 refuses (VGGT_ERR_SHAPE) a 256-row
 * operand panel of 2^31 bytes or more.  Auto (-1) is mode 0, or mode 7 (fused, N % 256 != 0: mode 6) from
 * M >= 4096 with K % 64 == 0 (vggt_gemm_bf16: also N % 256 == 0, N >= 2048, not the residual epilogue), and is
 * promoted to the persistent form for GELU and fused qkv from M >= 4096, for the other bf16 / f32 GEMMs with
 * N % 256 == 0 from M >= 16384, for the residual one from M >= 16384 with K >= 2048 -- never on a stream with
 * VGGT_STREAM_SHORT_WORKGROUPS.  The persistent form takes 192-row tiles for the residual epilogue and where
 * whole rounds over the stream's CUs cost 10 % less, else 256; with VGGT_TUNE_GEMM_BALANCE and a last round
 * at most 60 % full, split_rows rows run persistent and the rest as a second launch in mode 0.
 * Returns VGGT_OK when the library holds the kernel (the entry point would launch it), else the error the
 * entry point returns for these shapes.
 */
#define VGGT_GEMM_ENTRY_BF16 0
#define VGGT_GEMM_ENTRY_GELU_PRE 1
#define VGGT_GEMM_ENTRY_QKV 2
#define VGGT_GEMM_ENTRY_HEADNORM 3
#define VGGT_GEMM_FAMILY_128 0  /* gemm_bf16_kernel, 128 x 128 tiles                  */
#define VGGT_GEMM_FAMILY_RING 1 /* gemm_ring_kernel, 256 x bn                         */
#define VGGT_GEMM_FAMILY_TWO 2  /* gemm_two_kernel, 256 x 128, two workgroups per CU  */
#define VGGT_GEMM_FAMILY_PP 3   /* gemm_pp_kernel, ping-pong 256 x bn                 */
#define VGGT_GEMM_FAMILY_PPP 4  /* gemm_ppp_kernel, persistent ping-pong bm x 256     */
typedef struct {
  int family;     /* VGGT_GEMM_FAMILY_* */
  int bm, bn;     /* tile rows and columns */
  int epi;        /* VGGT_EPI_*, or internal: 16 / 17 fused q/k norm at D = 64 / 128, 18 GELU + pre-activation */
  int fk;         /* persistent form: 1 whole-K-tile segments, 0 half-K */
  int grid, lds;  /* workgroups launched, dynamic LDS bytes */
  int sched;      /* persistent form: M-tiles per tile group | split DMA << 8 */
  int split_rows; /* balance split: rows of this (first, persistent) launch; 0 = one launch */
  int rc;         /* VGGT_OK, or why there is nothing to launch */
  int dev_cus;    /* the device CU count used */
} vggt_gemm_form_t;
int vggt_gemm_form(int entry, int epi, int has_out2, int M, int N, int K, int H, int D, int rope_mode, int period,
                   int tab_len, int64_t lda, int64_t ldw, int64_t ldo, int64_t ldo2, int stream_cus, int stream_flags,
                   int force, vggt_gemm_form_t* form);

/*
 * Row LayerNorm over C: y = (x-mean)/sqrt(var+eps)*w + b (two-pass statistics in fp32 for bf16
 * outputs; in fp64, with one rounding per stored value, for fp32 outputs).
 * w/b may be NULL (elementwise_affine=False).  Replaces nn.LayerNorm
 * (norm1/norm2 of every Block, alignment_head.py:203-206, DPT norm, ...).
 * C must be 256 * {1, 2, 3, 4, 8, 16}; ldx, ldy multiples of 4; x, y 8-byte (bf16) or 16-byte (fp32)
 * aligned, w and b 16-byte aligned.  y == x (same dtype, same ld: in place) is allowed; no other
 * overlap of x and y is.  b is ignored when w is NULL.  x or y NULL with M > 0 is VGGT_ERR_SHAPE
 * (vggt_layernorm_grouped as well).
 */
int vggt_layernorm(const void* x, int in_dtype, int64_t ldx, const float* w, const float* b, float eps, int M, int C,
                   void* y, int out_dtype, int64_t ldy, void* stream);

/*
 * Residual LayerScale add fused with the NEXT LayerNorm:
 *   x[m] += gamma * y[m]          (x fp32 [M, C] in place, y bf16 [M, C])
 *   out2[m] = x[m]                (if out2 != NULL: the kept-layer concat half)
 *   xn[m] = LayerNorm(x[m]; w, b) (bf16, if xn != NULL; w/b may be NULL)
 * The add is the arithmetic of vggt_gemm_bf16's VGGT_EPI_RESID_F32 epilogue
 * on the bf16-rounded branch output.  Replaces `x = x + ls2(mlp(norm2(x)))`
 * followed by the next block's `norm1(x)` (vggt layers/block.py, ext; the
 * aggregator's frame/global alternation, featureAligned_vggt.py:78-82).
 * C a multiple of 256 in {256, 512, 1024, 2048}.
 * One check for this form and the two below: x, y or gamma NULL with M > 0 is VGGT_ERR_SHAPE; the
 * ld of every pointer given a multiple of 4; x, gamma, gamma2, out2, w, b 16-byte and y, y2, xn
 * 8-byte aligned (VGGT_ERR_ALIGN).
 */
int vggt_resid_add_layernorm(float* x, int64_t ldx, const void* y, int64_t ldy, const float* gamma, float* out2,
                             int64_t ldo2, const float* w, const float* b, float eps, int M, int C, void* xn,
                             int64_t ldn, void* stream);

/*
 * The two row passes of a block (after proj, after fc2) with the first one's
 * store of x deferred into the second; bitwise the results of two
 * vggt_resid_add_layernorm calls:
 *   vggt_resid_add_layernorm_nostore: xn[m] = LayerNorm(x[m] + gamma * y[m]);
 *     x is read only (xn required).
 *   vggt_resid_add2_layernorm: x[m] = (x[m] + gamma * y[m]) + gamma2 * y2[m]
 *     with the same y and gamma again, then out2 / xn as vggt_resid_add_layernorm.
 * y must stay unchanged between the two calls.
 */
int vggt_resid_add_layernorm_nostore(const float* x, int64_t ldx, const void* y, int64_t ldy, const float* gamma,
                                     const float* w, const float* b, float eps, int M, int C, void* xn, int64_t ldn,
                                     void* stream);
int vggt_resid_add2_layernorm(float* x, int64_t ldx, const void* y, int64_t ldy, const float* gamma, const void* y2,
                              int64_t ldy2, const float* gamma2, float* out2, int64_t ldo2, const float* w,
                              const float* b, float eps, int M, int C, void* xn, int64_t ldn, void* stream);

/*
 * In-place per-head LayerNorm (QK-norm) + RoPE on a bf16 [M, ld] buffer:
 * for each row m and head h, the D values at columns col_off + h*D are
 * normalised with (w,b,eps) (skipped if w == NULL) and rotated (rope_mode).
 * Positions: pos is int32 [period][2] (2D: y,x) or [period] (1D); row m uses
 * pos[m % period].  cos/sin tables are f32 [tab_len][rd] with rd = D/2 (2D)
 * or D (1D), layout cat(angles, angles) as in rope.py:23-44.
 * A position outside [0, tab_len) is clamped to the first / last table row.  b is ignored when w
 * is NULL (no normalisation at all, RoPE only).
 * One check for this entry point and the three below (vggt_qknorm_rope, the two _out forms): H > 0,
 * D in {64, 128}, and the data pointers (buf, qkv, src, dst) not NULL when M > 0 (VGGT_ERR_SHAPE);
 * ld, lds, ldd and col_off multiples of 8, data pointers and tables 16-byte aligned (VGGT_ERR_ALIGN);
 * qw and kw both given or both NULL; a rope_mode other than VGGT_ROPE_NONE needs pos, cos_tab,
 * sin_tab, period > 0 and tab_len > 0 (VGGT_ERR_SHAPE); an unknown rope_mode is VGGT_ERR_UNSUPPORTED.
 * Replaces Attention.q_norm/k_norm + rope (vggt attention.py, ext) and
 * CrossAttention q_norm/k_norm + rope1d (cross_attention.py:59-62).
 */
int vggt_headnorm_rope(void* buf, int64_t ld, int col_off, int M, int H, int D, const float* w, const float* b,
                       float eps, int rope_mode, const int32_t* pos, int period, const float* cos_tab,
                       const float* sin_tab, int tab_len, void* stream);

/*
 * Fused q_norm/k_norm + RoPE on a fused qkv row: q heads at columns [0, H*D)
 * normalised with (qw, qb), k heads at [H*D, 2*H*D) with (kw, kb); one launch
 * (vggt Attention.q_norm/k_norm + rope, ext; featureAligned_vggt.py:78).
 * Same position/table conventions as vggt_headnorm_rope.
 */
int vggt_qknorm_rope(void* qkv, int64_t ld, int M, int H, int D, const float* qw, const float* qb, const float* kw,
                     const float* kb, float eps, int rope_mode, const int32_t* pos, int period, const float* cos_tab,
                     const float* sin_tab, int tab_len, void* stream);

/*
 * Out-of-place forms (training recompute, alignment_head.py:351-393 under checkpoint: the backward needs the
 * pre-norm projections, so they are not overwritten): heads are read from src (row stride lds) and the
 * normalised + rotated values written to dst (row stride ldd).  vggt_qknorm_rope_out covers the q|k columns
 * [0, 2*H*D) of a fused projection, vggt_headnorm_rope_out H heads from column 0.
 */
int vggt_qknorm_rope_out(const void* src, int64_t lds, void* dst, int64_t ldd, int M, int H, int D, const float* qw,
                         const float* qb, const float* kw, const float* kb, float eps, int rope_mode,
                         const int32_t* pos, int period, const float* cos_tab, const float* sin_tab, int tab_len,
                         void* stream);
int vggt_headnorm_rope_out(const void* src, int64_t lds, void* dst, int64_t ldd, int M, int H, int D, const float* w,
                           const float* b, float eps, int rope_mode, const int32_t* pos, int period,
                           const float* cos_tab, const float* sin_tab, int tab_len, void* stream);

/*
 * Flash attention forward, bf16 in/out, fp32 online softmax, D in {64,128}.
 * For batch b, head h:  O = softmax(Q K^T * scale) V  with
 *   Q row i at q + (b*q_bstride + i)*ldq + h*D   (i < nq), same for K, V (j < nk)
 *   O row i at o + (b*o_bstride + i)*ldo + h*D.
 * Replaces F.scaled_dot_product_attention in vggt Attention (frame / global
 * blocks of the aggregator, DINOv2 blocks, alignment frame blocks).
 */
int vggt_attention_fwd(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                       const void* v, int64_t ldv, int64_t v_bstride, void* o, int64_t ldo, int64_t o_bstride,
                       int batch, int heads, int nq, int nk, int D, float scale, void* stream);

/*
 * vggt_attention_fwd with a workspace, the one entry that may split keys: on
 * the 8-wave D = 64 default path (nq >= 4096) the last (head, 256-row block)
 * units of every batch element -- those of the last, partial round of
 * workgroups of one element launched alone on the whole device -- run as 2..4
 * workgroups each, one per contiguous range of 64-key tiles, dispatched behind
 * all the whole units in the same launch; each leaves its row offsets, row sums
 * and unnormalised fp32 accumulator (m, l, O) in ws, and a second small launch
 * on the same stream merges them in a fixed order (run-to-run bitwise stable;
 * no atomics, no flags) and writes those rows of o.  All other rows are
 * bitwise those of vggt_attention_fwd.  ws: 16-byte aligned, at least
 * vggt_attention_ws_bytes(...) bytes for the same shape and
 * VGGT_TUNE_ATTN_TAIL_SPLIT value (0 bytes: the launch will not split; the
 * size scales with batch; `stream` is not consulted: the launch plans on the
 * device's CU count, also on a CU-masked stream, so that the split rows and
 * their bits depend on the element shape and the device alone); one
 * buffer may serve every launch of a stream.  ws == NULL never splits; a
 * buffer that is too small is VGGT_ERR_SHAPE and nothing is launched.
 * vggt_attention_split_plan is the policy alone (host arithmetic, no device
 * call): 1 and the per-element tail size / parts on `cus` compute units
 * (two 8-wave workgroups per CU), else 0; `batch` does not enter it.
 */
int vggt_attention_fwd_ws(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                          int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o, int64_t ldo,
                          int64_t o_bstride, int batch, int heads, int nq, int nk, int D, float scale, void* ws,
                          size_t ws_bytes, void* stream);
size_t vggt_attention_ws_bytes(int batch, int heads, int nq, int nk, int D, void* stream);
int vggt_attention_split_plan(int batch, int heads, int nq, int nk, int D, int cus, int* tail_blocks, int* parts);

/*
 * Which forward kernel vggt_attention_fwd launches for (D, nq) under the current
 * knobs (VGGT_TUNE_ATTN_VARIANT / _WAVES / ATTN16, env VGGT_ATTN_DMA_HALF): host
 * arithmetic, no device call.  *form16: 1 the 16x16x32 kernel (*var is 0 then),
 * 0 the 32x32x16 kernel with schedule bits *var (the variant's bits as run: 33
 * resolves to 2081 on the 8-wave D = 64 path; the key-split bit of a
 * vggt_attention_fwd_ws launch that splits is not included); *waves: waves per
 * workgroup (2, 4 or 8).  Null pointers are skipped.  Returns VGGT_OK when the
 * library holds that kernel, else VGGT_ERR_UNSUPPORTED (also for D not in {64, 128}).
 */
int vggt_attention_fwd_form(int D, int nq, int* form16, int* waves, int* var);
/* The same for vggt_attention_stamps (D = 64, always the 32x32x16 kernel; *var includes the stamps bit 1024). */
int vggt_attention_stamps_form(int nq, int* waves, int* var);

/*
 * DINOv2 patch-embed input: ResNet-normalise fp32 images (F,3,H,W) and write
 * the bf16 im2col matrix A[F*h*w, Kp] (k = c*p*p + ky*p + kx, zero pad to Kp).
 * (vggt aggregator.py normalisation + DINOv2 PatchEmbed conv, ext.)
 * `mean` / `std_` are HOST pointers to 3 floats each (the ResNet constants).
 */
int vggt_patch_im2col(const float* images, int F, int H, int W, int patch, const float* mean, const float* std_,
                      void* A, int Kp, void* stream);

/*
 * DINOv2 token assembly: x[f, t] (f32, P = 1 + nreg + hw rows per frame):
 *   t = 0: cls + pos[0];  1..nreg: reg[t-1];  t > nreg: patch[f*hw + t-1-nreg] + pos[t-nreg]
 * patch is the bf16 patch-embed GEMM output [F*hw, C]; pos is f32 [1+hw, C].
 */
int vggt_dino_assemble(const void* patch, const float* cls, const float* reg, const float* pos, int F, int hw,
                       int nreg, int C, float* x, void* stream);

/*
 * Write per-frame special tokens into rows [f*P, f*P + n) of x (f32, ld C):
 * frame (f % S) == 0 takes tok[0, :n], other frames tok[1, :n]
 * (slice_expand_and_flatten, alignment_head.py:543-568 / aggregator, ext).
 * tok is f32 [2, n, C].
 */
int vggt_special_tokens(float* x, int64_t ldx, int F, int S, int P, int n, int C, const float* tok, void* stream);

/* Strided 2-D copy of f32 rows: dst[r*ldd + c] = src[r*lds + c], r < rows, c < cols. */
int vggt_copy_rows_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int rows, int cols, void* stream);

/*
 * Row-remapped LayerNorm: logical row r (< M) = group g = r / group, i = r % group,
 * reads x row g*x_group_stride + x_row_offset + i and writes y row
 * g*y_group_stride + y_row_offset + i.  Used to skip/insert per-frame special
 * tokens without copies: DPT patch-token norm (dpt_head, ext, via
 * featureAligned_vggt.py:166) and AlignmentHead.token_norm writing after the
 * per-frame alignment token (alignment_head.py:247,269-270).
 */
int vggt_layernorm_grouped(const void* x, int in_dtype, int64_t ldx, const float* w, const float* b, float eps, int M,
                           int C, void* y, int out_dtype, int64_t ldy, int group, int x_group_stride,
                           int x_row_offset, int y_group_stride, int y_row_offset, void* stream);

/*
 * Skinny fp32 linear layer (weight-streaming, small M), exact-f32 MFMA:
 *   out[M,N] = epi( act_in(A)[M,K] . W[N,K]^T + bias )
 * act_in: 0 none, 1 SiLU.  epi: VGGT_EPI_F32 (plain), VGGT_EPI_GELU_BF16 (GELU,
 * f32 out here), VGGT_EPI_RESID_F32 (out += gamma * v; out is the residual).
 * Replaces the fp32 nn.Linear calls of the camera head (camera_head, ext:
 * embed_pose, poseLN_modulation, trunk Blocks, pose_branch), the alignment
 * decoder (alignment_head.py:463,475,534-538, cross blocks, gated_update.py:22-36).
 * A, W and out may be any 4-byte aligned row-major views: 16-byte loads are used when K, lda, ldw
 * are multiples of 4 and A and W are 16-byte aligned, scalar loads otherwise (the same sums).
 *
 * One check for the three entries (vggt_linear_f32, _ws, _grouped), in this order: M, N or K < 1, A, W or
 * out NULL, (grouped) M > 256 or groups outside [1, 65535], (not grouped) VGGT_EPI_RESID_F32 without gamma:
 * VGGT_ERR_SHAPE; then act_in not 0 / 1, an epi other than the three above, (grouped) VGGT_EPI_RESID_F32:
 * VGGT_ERR_UNSUPPORTED.  bias may be NULL.  Nothing is launched by a refused call.
 */
int vggt_linear_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, int M, int N, int K,
                    int act_in, int epi, float* out, int64_t ldo, const float* gamma, void* stream);
/* Same with a caller-provided scratch (device, >= VGGT_LINEAR_F32_WS_COUNTERS * 4 +
 * VGGT_LINEAR_F32_MAX_SPLITS * roundup(M,64) * N * 4 bytes to allow the maximum split;
 * a smaller one caps the split): skinny-M calls are
 * split along K into up to VGGT_LINEAR_F32_MAX_SPLITS deterministic partial sums combined in a fixed order
 * (camera head trunk, alignment decoder: M = 16 frames) by the last split block of
 * each output tile, in the same launch.  The scratch's first
 * VGGT_LINEAR_F32_WS_COUNTERS words are per-tile counters: zero-fill them before a
 * scratch's first use; every call leaves them zero.  ws == NULL: no split. */
/* `groups` independent skinny fp32 linears of one shape in one launch (M <= 256):
 * group g reads A + g*a_gstride, W + g*w_gstride, bias + g*b_gstride and writes
 * out + g*o_gstride (element strides); epi VGGT_EPI_F32 or VGGT_EPI_GELU_BF16.
 * Each group's values are bitwise those of its own vggt_linear_f32_ws call
 * (the in-workgroup split form).  Replaces GatedUpdate's per-token delta MLPs
 * (gated_update.py:51-57: one Linear pair per memory token). */
int vggt_linear_f32_grouped(const float* A, int64_t lda, int64_t a_gstride, const float* W, int64_t ldw,
                            int64_t w_gstride, const float* bias, int64_t b_gstride, int M, int N, int K, int groups,
                            int act_in, int epi, float* out, int64_t ldo, int64_t o_gstride, void* stream);
/* GatedUpdate's elementwise stages (gated_update.py:43-79, fp32; rows = B x Nt memory
 * tokens of D features, contiguous):
 *   prep: inp[b, i] = [update_b, |update_b| memory[b, i], |update_b| mean_j memory[b, j]]
 *         ([B*Nt, 3D]) and g_in[:, D:2D] = |update_b| memory[b, i]  ([B*Nt, 2D]);
 *   diff: g_in[:, 0:D] = deltas - memory;
 *   tail: out = normalize(memory + sigmoid(logit) normalize(diff - (diff . memory) memory))
 *         with F.normalize's max(|x|, 1e-12).
 * A size < 1 or a NULL pointer: VGGT_ERR_SHAPE. */
int vggt_gated_update_prep(const float* memory, const float* update, int B, int Nt, int D, float* inp, float* g_in,
                           void* stream);
int vggt_gated_update_diff(const float* memory, const float* deltas, int rows, int D, float* g_in, void* stream);
int vggt_gated_update_tail(const float* memory, const float* deltas, const float* logit, int rows, int D, float* out,
                           void* stream);
#define VGGT_LINEAR_F32_WS_COUNTERS 1024
#define VGGT_LINEAR_F32_MAX_SPLITS 32
int vggt_linear_f32_ws(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, int M, int N, int K,
                       int act_in, int epi, float* out, int64_t ldo, const float* gamma, void* ws, size_t ws_bytes,
                       void* stream);

/*
 * Which kernel the linear entries launch: what linear_resolve, the dispatcher the entries themselves call,
 * answers for these shapes under the current VGGT_TUNE_LINEAR_* knobs.  Host arithmetic only (no device
 * needed).  groups == 0 asks about vggt_linear_f32_ws with a scratch of ws_bytes (0: none, i.e.
 * vggt_linear_f32) and gamma given or not; any other value asks about vggt_linear_f32_grouped with that many
 * groups (has_gamma and ws_bytes unused).  Returns what the entry would return for non-NULL A, W and out.
 * The rule:
 *   grouped, or M <= 256 with VGGT_TUNE_LINEAR_WK > 0: FAMILY_WK, kw = 2, doubled up to 8 while K > kw * WK
 *     (64 when grouped with the knob at 0) waves of a workgroup on k ranges of kchunk = roundup(ceil(K / kw), 64),
 *     mt = 1 (M <= 16) or 4 accumulator tiles per wave, grid (ceil(N / 16), ceil(M / 64), groups), 64 kw threads;
 *   else splits = 1, doubled up to VGGT_LINEAR_F32_MAX_SPLITS while blocks * splits * 2 <= 512 (blocks =
 *     ceil(N / 64) ceil(M / 64)) and K / (2 splits) >= VGGT_TUNE_LINEAR_SPLIT_K, then halved until the scratch
 *     holds the counters and `splits` slabs of roundup(M, 64) x N floats:
 *     splits == 1: FAMILY_BLOCK, kchunk = K; else FAMILY_SPLIT, kchunk = roundup(ceil(K / splits), 16) and
 *     one_launch = 1 when blocks <= VGGT_LINEAR_F32_WS_COUNTERS and VGGT_TUNE_LINEAR_ONE_LAUNCH (the tile's
 *     last block combines), 0 for a second launch of linear_f32_reduce over min(ceil(M N / 256), 4096) groups;
 *     grid (ceil(N / 64), ceil(M / 64), splits), 256 threads.
 * No kernel uses dynamic LDS.
 */
#define VGGT_LINEAR_FAMILY_WK 0    /* linear_f32_wk_kernel<kw, mt, act_in, epi>: K split inside the workgroup */
#define VGGT_LINEAR_FAMILY_BLOCK 1 /* linear_f32_kernel<act_in, epi>, K not split                             */
#define VGGT_LINEAR_FAMILY_SPLIT 2 /* linear_f32_kernel<act_in, epi>, K split over blockIdx.z                 */
typedef struct {
  int family;      /* VGGT_LINEAR_FAMILY_* */
  int kw, mt;      /* FAMILY_WK: waves along K, accumulator tiles per wave (else 0, 4) */
  int splits;      /* FAMILY_SPLIT: K ranges over workgroups (else 1) */
  int kchunk;      /* k per wave (FAMILY_WK) or per split; K when nothing splits */
  int one_launch;  /* 0: FAMILY_SPLIT followed by linear_f32_reduce */
  int grid[3], threads;
  int rc;          /* VGGT_OK, or the entry point's error */
} vggt_linear_f32_form_t;
int vggt_linear_f32_form(int M, int N, int K, int act_in, int epi, int groups, int has_gamma, size_t ws_bytes,
                         vggt_linear_f32_form_t* form);

/*
 * Small-window attention (nk <= 128, D <= 256), one wave per (batch, head),
 * f32 softmax; dtype VGGT_DTYPE_BF16 or VGGT_DTYPE_F32 for all of q/k/v/o.
 * Layout as vggt_attention_fwd (v shares k's batch stride).  Replaces the SDPA
 * of CrossAttention (cross_attention.py:64-73) in the temporal blocks (S
 * queries x T keys per spatial token, alignment_head.py:368-390) and the
 * decoder (alignment_head.py:494-530), and the camera-head trunk attention.
 * bf16 windows of <= 16 queries x <= 16 keys (D % 16 == 0) run on the matrix cores
 * (fp32 scores, P rounded to bf16 for P.V, as the reference's bf16 SDPA) unless
 * dtype carries VGGT_ATTN_SMALL_EXACT: the training forward, whose backward
 * (vggt_attention_small_bwd) recomputes P in fp32 from the same formula.
 * batch, heads, nq, nk or D < 1, nk > 128, D > 256, (2 nk (D + 1) + D) 4 bytes over 160 KiB, or q, k, v or o
 * NULL: VGGT_ERR_SHAPE; then a dtype that is neither: VGGT_ERR_UNSUPPORTED.
 */
#define VGGT_ATTN_SMALL_EXACT 0x100
int vggt_attention_small(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                         const void* v, int64_t ldv, void* o, int64_t ldo, int64_t o_bstride, int dtype, int batch,
                         int heads, int nq, int nk, int D, float scale, void* stream);

/*
 * Which kernel vggt_attention_small launches: what attn_small_resolve, the dispatcher the entry itself calls,
 * answers.  Host arithmetic only.  dtype as the entry's (with or without VGGT_ATTN_SMALL_EXACT); ptr_align: the
 * largest power of two, in bytes, that divides all four base pointers (the entry caps it at 256).  Returns what
 * the entry would return for non-NULL pointers.  The rule, after the entry's checks:
 *   bf16 without EXACT, nq <= 16, nk <= 16, D % 16 == 0, all four leading dimensions % 4 == 0, ptr_align % 8 == 0
 *     and VGGT_ATTN_SMALL_MFMA (environment, default 1) nonzero: FAMILY_MFMA, dt = D for 64 / 128 (compile-time D)
 *     else 0, ceil(batch heads / 4) workgroups of 256 threads, 128 D bytes of LDS;
 *   else, with VGGT_ATTN_SMALL_WG (environment, default 1) nonzero, while ((nq + nk)(D + 1) + nk D + nq nk) 4
 *     <= 64 KiB: FAMILY_WG, batch heads workgroups of 256 threads and that much LDS;
 *   else FAMILY_WAVE: batch heads workgroups of 64 threads, (2 nk (D + 1) + D) 4 bytes of LDS.
 */
#define VGGT_ATTN_SMALL_FAMILY_MFMA 0 /* attn_small_mfma_kernel<dt>   */
#define VGGT_ATTN_SMALL_FAMILY_WG 1   /* attn_small_wg_kernel<dtype>  */
#define VGGT_ATTN_SMALL_FAMILY_WAVE 2 /* attn_small_kernel<dtype>     */
typedef struct {
  int family;             /* VGGT_ATTN_SMALL_FAMILY_* */
  int dt;                 /* FAMILY_MFMA: the compile-time D (64, 128), 0 for a runtime D */
  int grid, threads, lds; /* workgroups, threads per workgroup, dynamic LDS bytes */
  int rc;                 /* VGGT_OK, or the entry point's error */
} vggt_attention_small_form_t;
int vggt_attention_small_form(int dtype, int nq, int nk, int D, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                              int ptr_align, int batch, int heads, vggt_attention_small_form_t* form);

/* fp32 variant of vggt_headnorm_rope (decoder / camera head run in fp32): D a multiple of 4 up to
 * 1024, any col_off (scalar loads); positions clamped and b ignored without w as there.  M == 0: VGGT_OK,
 * nothing launched; M < 0, H < 1, D out of range, buf NULL, or a rope_mode other than VGGT_ROPE_NONE without
 * pos, cos_tab, sin_tab, period > 0 and tab_len > 0: VGGT_ERR_SHAPE; then an unknown rope_mode:
 * VGGT_ERR_UNSUPPORTED. */
int vggt_headnorm_rope_f32(float* buf, int64_t ld, int col_off, int M, int H, int D, const float* w, const float* b,
                           float eps, int rope_mode, const int32_t* pos, int period, const float* cos_tab,
                           const float* sin_tab, int tab_len, void* stream);

/* y_bf16[r, c] = bf16(x_f32[r, c])  (autocast input cast of a Linear).  rows < 0, cols, ldx or ldy % 4, x or y
 * NULL with rows > 0: VGGT_ERR_SHAPE; x off 16 bytes or y off 8: VGGT_ERR_ALIGN. */
int vggt_cast_f32_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int rows, int cols, void* stream);

/*
 * fp32 NHWC implicit-GEMM convolution (exact-f32 MFMA), DPT head
 * (dpt_head, ext; featureAligned_vggt.py:166,183):
 *   y[p, co] = relu_out?( sum act(x) * W + bias ) [+ pos[p % (ho*wo), co]]
 *              [+ (res1_relu ? relu(res1) : res1)[p, co]] [+ res2[p, co]]
 * x: [nimg, hi, wi, ci] with pixel stride ldx; W: [roundup(co',64), kh*kw*ci]
 * (K order ky, kx, ci; rows beyond co' zero-padded); ci % 32 == 0.
 * shuffle = s > 0 turns a 1x1 GEMM with co' = s*s*co columns (column
 * (dy*s+dx)*co + c) into a stride==kernel ConvTranspose2d pixel-shuffle store
 * onto the [nimg, hi*s, wi*s, co] grid.
 * Rows must not overlap: ldx < ci on a map of more than one pixel, or ldy < co,
 * is VGGT_ERR_SHAPE (here and in the two split-bf16 forms below, where ldy is
 * checked only when y is given).
 */
int vggt_conv2d_f32(const float* x, int64_t ldx, int nimg, int hi, int wi, int ci, const float* w, const float* bias,
                    int co, int kh, int kw, int stride, int pad, float* y, int64_t ldy, int relu_in, int relu_out,
                    const float* res1, int64_t ldr1, int res1_relu, const float* res2, int64_t ldr2, const float* pos,
                    int shuffle, void* stream);

/*
 * Same convolution as vggt_conv2d_f32 on the bf16 matrix path with split
 * operands: x = hi + lo (hi = bf16(x), lo = bf16(x - hi)), accumulating
 * hi.hi + hi.lo + lo.hi in fp32 (~2^-16 relative per product instead of
 * fp32's 2^-24; ~5x faster).  w_hi / w_lo: the vggt_conv2d_f32 weight layout
 * split by vggt_split_bf16x2 (bf16), rows zero-padded to a multiple of 128.
 */
int vggt_conv2d_bf16x3(const float* x, int64_t ldx, int nimg, int hi, int wi, int ci, const void* w_hi,
                       const void* w_lo, const float* bias, int co, int kh, int kw, int stride, int pad, float* y,
                       int64_t ldy, int relu_in, int relu_out, const float* res1, int64_t ldr1, int res1_relu,
                       const float* res2, int64_t ldr2, const float* pos, int shuffle, void* stream);

/*
 * vggt_conv2d_bf16x3 on an activation split beforehand (vggt_split_act_bf16x2,
 * which also applies the input ReLU): x_hi / x_lo bf16 [nimg, hi, wi, ci] with
 * pixel stride ldx (elements, % 8 == 0), whole map < 2 GiB.  The im2col gather
 * is LDS-DMA of the bf16 halves (out-of-image taps read as zeros); results are
 * bitwise equal to vggt_conv2d_bf16x3 with relu_in on the f32 input.  y (f32) and/or
 * y_hi / y_lo (the NEXT conv's pre-split input: split(split_relu ? max(y, 0) : y),
 * bf16 rows of stride ldys) are written; either may be NULL, not both.
 */
int vggt_conv2d_bf16x3_pre(const void* x_hi, const void* x_lo, int64_t ldx, int nimg, int hi, int wi, int ci,
                           const void* w_hi, const void* w_lo, const float* bias, int co, int kh, int kw, int stride,
                           int pad, float* y, int64_t ldy, int relu_out, const float* res1, int64_t ldr1,
                           int res1_relu, const float* res2, int64_t ldr2, const float* pos, int shuffle,
                           void* y_hi, void* y_lo, int64_t ldys, int split_relu, void* stream);

/* hi / lo = split(relu ? max(x, 0) : x) of a [rows, cols] f32 map (row stride ldx, cols % 4 == 0)
 * into contiguous bf16 [rows, cols] maps: hi = bf16(v), lo = bf16(v - hi) (DPT conv inputs). */
int vggt_split_act_bf16x2(const float* x, int64_t ldx, int64_t rows, int cols, int relu, void* hi, void* lo,
                          void* stream);

/* hi[i] = bf16(x[i]), lo[i] = bf16(x[i] - hi[i]) for i < n (weight split for vggt_conv2d_bf16x3). */
int vggt_split_bf16x2(const float* x, int64_t n, void* hi, void* lo, void* stream);

/* NHWC bilinear resize with align_corners=True (custom_interpolate, dpt_head ext), + optional pos table. */
int vggt_upsample_bilinear_f32(const float* x, int nimg, int hi, int wi, int C, float* y, int ho, int wo,
                               const float* pos, void* stream);
/* Same, writing y (f32, may be NULL) and/or the split bf16 halves of relu?(y) (contiguous [.., C]). */
int vggt_upsample_bilinear_split(const float* x, int nimg, int hi, int wi, int C, float* y, int ho, int wo,
                                 const float* pos, void* y_hi, void* y_lo, int split_relu, void* stream);
/* Same as vggt_upsample_bilinear_split with a SEPARABLE positional table (DPT's
 * UV sin/cos embedding, dpt_head ext `_apply_pos_embed`: channels [0, C/2) depend on
 * x only, [C/2, C) on y only): pos_sep = [wo + ho, C/2] fp32, rows 0..wo-1 the x
 * part, rows wo..wo+ho-1 the y part.  C % 8 == 0. */
int vggt_upsample_bilinear_split_sep(const float* x, int nimg, int hi, int wi, int C, float* y, int ho, int wo,
                                     const float* pos_sep, void* y_hi, void* y_lo, int split_relu, void* stream);

/*
 * Fused last stage of the DPT head (output_conv1's output -> F.interpolate(size=(ho, wo),
 * bilinear, align_corners=True) -> + _apply_pos_embed -> output_conv2[0], dpt_head ext,
 * featureAligned_vggt.py:166): y = conv3x3_pad1(split(resize(x) + pos)) without
 * materialising the resized map.  x [nimg, hi, wi, C] f32 NHWC (C % 32 == 0), pos_sep
 * [wo + ho, C/2] (the separable table of vggt_upsample_bilinear_split_sep) or NULL,
 * w_hi / w_lo the split packed weights of vggt_conv2d_bf16x3_pre ([>= 32 rows, 9*C], the
 * (ky, kx, ci) column order), co <= 32.  Outputs as conv2d_bf16x3_pre: y [nimg*ho*wo, ldy]
 * f32 and/or the split halves of relu?(y).  Same products and K order as the unfused
 * upsample + conv2d_bf16x3_pre, and the same resize arithmetic (common.h bl_*): bitwise
 * equal to vggt_upsample_bilinear_split_sep followed by vggt_conv2d_bf16x3_pre.
 */
int vggt_conv2d_upsample_bf16x3(const float* x, int nimg, int hi, int wi, int C, const float* pos_sep, int ho,
                                int wo, const void* w_hi, const void* w_lo, const float* bias, int co, int relu_out,
                                float* y, int64_t ldy, void* y_hi, void* y_lo, int64_t ldys, int split_relu,
                                void* stream);

/*
 * Which kernel the four convolution entry points above launch, or the error they return: host arithmetic
 * only, no device call.  The answer is the dispatcher's own (conv_resolve in csrc/conv.hip) under the
 * process's current VGGT_TUNE_CONV_PF2.
 *   entry    VGGT_CONV_ENTRY_*; the geometry integers and ldx / ldy / ldys are the entry point's.  ho / wo are
 *            read for ENTRY_UPSAMPLE only (the resize target; ci is its C, and kh / kw / stride / pad / shuffle /
 *            ldx are not read: 3 x 3, 1, 1, 0, C); ldys for ENTRY_PRE and ENTRY_UPSAMPLE.
 *   present  VGGT_CONV_HAS_* bits: which of y, y_hi, y_lo, res1, res2, pos the call gives.
 * Every pointer is taken as 16-byte aligned, so the VGGT_ERR_ALIGN answers are those of the leading dimension
 * alone (ldx % 4, for ENTRY_PRE ldx % 8).
 * The rule, in the order the checks apply: non-positive dimensions, ci % 32, overlapping rows (ldx < ci on
 * more than one pixel, ldy < co with y) are VGGT_ERR_SHAPE; a pixel shuffle with anything but a 1x1 stride-1
 * unpadded kernel and no res1 / res2 / pos is VGGT_ERR_UNSUPPORTED; then alignment; then more than 2^31 - 1
 * tiles of 128 pixels x 64 columns is VGGT_ERR_SHAPE (whichever width runs); ENTRY_PRE then asks for an
 * output, both split halves or none and ldys >= co (VGGT_ERR_SHAPE), ldx % 8, and a map below 0x7fffff00
 * bytes (VGGT_ERR_SHAPE).  The split forms run 128-column tiles from 128 GEMM columns (co, or s s co with a
 * shuffle), 64-column ones above 32, else 32; vggt_conv2d_f32 always 64.  vggt_conv2d_bf16x3 gathers two
 * deep (pf2) when VGGT_TUNE_CONV_PF2 is on and the f32 map ends below 0xffffff00 bytes.
 * w_rows is the contract on the packed weights: the kernel reads rows [0, w_rows) of W (w_hi / w_lo) through
 * an unbounded descriptor, so rows from co' up to w_rows must exist (and hold zeros).  w_rows is a multiple of
 * bn and never exceeds roundup(co', 128).
 */
#define VGGT_CONV_ENTRY_F32 0      /* vggt_conv2d_f32             */
#define VGGT_CONV_ENTRY_BF16X3 1   /* vggt_conv2d_bf16x3          */
#define VGGT_CONV_ENTRY_PRE 2      /* vggt_conv2d_bf16x3_pre      */
#define VGGT_CONV_ENTRY_UPSAMPLE 3 /* vggt_conv2d_upsample_bf16x3 */
#define VGGT_CONV_FAMILY_F32 0      /* conv_f32_kernel                 */
#define VGGT_CONV_FAMILY_SPLIT 1    /* conv_bf16x3_kernel<bn, pf2>     */
#define VGGT_CONV_FAMILY_PRE 2      /* conv_pre_kernel<bn>             */
#define VGGT_CONV_FAMILY_UPSAMPLE 3 /* conv_up_kernel<32>              */
#define VGGT_CONV_HAS_Y 1
#define VGGT_CONV_HAS_Y_HI 2
#define VGGT_CONV_HAS_Y_LO 4
#define VGGT_CONV_HAS_RES1 8
#define VGGT_CONV_HAS_RES2 16
#define VGGT_CONV_HAS_POS 32
typedef struct {
  int family;      /* VGGT_CONV_FAMILY_* */
  int bn;          /* tile columns (tile rows: 128 pixels) */
  int pf2;         /* split form: 1 two-deep gather, 0 one-deep */
  int grid, lds;   /* workgroups launched, static LDS bytes */
  unsigned xbytes; /* bytes of the input map the gather's descriptor covers (0: plain loads) */
  int w_rows;      /* weight rows the kernel reads: tiles_n * bn */
  int rc;          /* VGGT_OK, or the entry point's error */
} vggt_conv_form_t;
int vggt_conv_form(int entry, int nimg, int hi, int wi, int ci, int co, int kh, int kw, int stride, int pad,
                   int shuffle, int ho, int wo, int64_t ldx, int64_t ldy, int64_t ldys, int present,
                   vggt_conv_form_t* form);

/*
 * DPT activate_head (ext): x [npix, ncl] NHWC with the confidence last;
 * pts[p, j] = act(x[p, j]) * scale[p / pix_per_img]  (act 0 = exp, 1 = inv_log),
 * conf[p] = 1 + exp(x[p, ncl-1]) (expp1).  scale may be NULL (depth *= chunk
 * scale, featureAligned_vggt.py:171).
 */
int vggt_dpt_activate(const float* x, int64_t ldx, int64_t npix, int pix_per_img, int ncl, int act,
                      const float* scale, float* pts, float* conf, void* stream);

/*
 * Robust Sim(3) between two point-map sets, one per batch element:
 * irls_sim3_umeyama + weighted_umeyama_sim3 (aligned_vggt/models/
 * pointAligned_wrapped_vggt.py:159-305; called at :69-100).  src/dst:
 * n points x 3 fp32 per batch element (batch strides in floats), conf_src /
 * conf_dst: n fp32.  Points whose sqrt(conf_src*conf_dst) is below
 * factor * (lower) median get weight 0; Huber IRLS with `delta`, at most
 * max_iters iterations after the initial solve, stop when |dR|_F, |dt|, |ds|
 * all < tol.  Outputs R_out [B,3,3], t_out [B,3], s_out [B] fp32, written on
 * the stream (no host synchronisation); a batch element whose total weight
 * is < 1e-6 (the reference raises ValueError) gets NaN outputs.
 * conf_dst == NULL: conf_src holds the weights themselves; factor <= 0: no
 * confidence threshold; max_iters == 0 with both is weighted_umeyama_sim3
 * (pointAligned_wrapped_vggt.py:159-219).
 * A point of weight 0 (below the threshold, confidence 0, or a Huber weight
 * that underflowed) is skipped: it adds nothing to any sum, so its coordinates
 * may be NaN or inf, as with the reference's boolean mask.  NaN / inf
 * coordinates at a point that carries weight make that element's outputs NaN.
 * NaN or negative (combined) confidences are outside the reference's domain
 * (its median turns NaN): such a point never carries weight, and in the median
 * it counts as larger than every non-negative value (the select orders the bit
 * patterns).  If the median itself is NaN, every point is dropped and the
 * element's outputs are NaN; if it is negative, no threshold applies.
 * Rank-1 clouds (collinear points, two points): when the second singular value
 * of the covariance is <= 2^-40 of the first (fp64 rounding noise of the
 * sums), the rotation about the line is free and R is completed to SOME proper
 * rotation (R R^T = I, det R = +1) that maps the source line onto the
 * destination line; s and t are the unique ones.  The solve diagonalises
 * Sg^T Sg, so above that threshold R is as accurate as an fp64 SVD's only to
 * about 2^-53 (sv_0 / sv_1)^2: one fp32 ulp down to sv_1 / sv_0 ~ 4e-5 (a cloud
 * 150 times longer than wide); a needle with extents 1 : 1e-3 : 1e-6 measured
 * 1.5e-5 in R in a host restatement.
 * One source position (n == 1, or all weight on coincident points, var_x == 0):
 * no scale or rotation is defined (the reference divides 0 by 0): outputs NaN.
 * workspace: >= vggt_irls_workspace_bytes(B), 16-B aligned, device memory; it
 * needs no clearing between calls.
 */
size_t vggt_irls_workspace_bytes(int B);
int vggt_irls_sim3(const float* src, int64_t src_bs, const float* dst, int64_t dst_bs, const float* conf_src,
                   int64_t cs_bs, const float* conf_dst, int64_t cd_bs, int B, int64_t n, float factor, float delta,
                   int max_iters, float tol, float* R_out, float* t_out, float* s_out, void* workspace,
                   size_t ws_bytes, void* stream);

/*
 * out[b, i] = T_b[:3,:3] (scale_b * pts[b, i]) + T_b[:3,3] for n points (x,y,z)
 * per batch element; T: [B,4,4] fp32 device, scale: [B] device or NULL.
 * apply_sim3_alignment_on_point_maps (aligned_vggt/utils/alignment.py:491-526)
 * and the point transform of featureAligned_vggt.py:200-206.  In place allowed.
 */
int vggt_sim3_points(const float* pts, int64_t p_bs, int B, int64_t n, const float* T, const float* scale, float* out,
                     int64_t o_bs, void* stream);

/* x[b, i] *= scale[b] (i < n) in place; scale: [B] device (depth *= chunk scale,
 * featureAligned_vggt.py:171; pointAligned_wrapped_vggt.py:130-132). */
int vggt_scale_f32(float* x, int64_t bs, int B, int64_t n, const float* scale, void* stream);

/*
 * Exact batched 1-nearest-neighbour in 3-D, fp32 (PyTorch3D knn_points(K=1) as
 * eval/reconstruction_metrics.py:48-49 and the iterative_closest_point call of
 * eval/training_metrics.py:343-364 use it; SPEC_ASSUMPTIONS.md).  q: (B, nq_max, 3)
 * with batch stride q_bs floats, r: (B, nr_max, 3) with r_bs; q_len / r_len:
 * device int64[B] (clamped to [0, max]) or NULL for "all full".  For every query
 * row below q_len: dist (B, nq_max) = the smallest distance to a reference row
 * below r_len -- norm 2: the SQUARED Euclidean distance fma(dz,dz,fma(dy,dy,dx*dx)),
 * norm 1: (|dx|+|dy|)+|dz|, both from coordinate differences -- and idx
 * (B, nq_max) int64 (or NULL) its row; ties take the smallest row, a distance
 * that does not compare below +inf (NaN coordinates, overflow, no reference
 * rows) is never taken and a query without any gets dist = +inf, idx = -1.
 * Rows at or past q_len get dist = 0, idx = -1.  Nothing past a length is read.
 * split: 0 = vggt_nn1_plan's count for the device, n >= 1 = n parts of the
 * reference range (capped at its number of 1024-point tiles); with more than
 * one part ws (8-byte aligned, >= vggt_nn1_workspace_bytes) holds the merge
 * keys, else ws may be NULL.  The result is bitwise independent of split and of
 * run order.  B < 1, B > 65535 or nr_max >= 2^31: VGGT_ERR_SHAPE; norm not in
 * {1, 2}: VGGT_ERR_UNSUPPORTED; nq_max == 0: nothing to do, VGGT_OK.
 * vggt_nn1_plan is the policy alone (host arithmetic, no device call): the
 * split count of the automatic mode on `cus` compute units.
 */
int vggt_nn1(const float* q, int64_t q_bs, const int64_t* q_len, const float* r, int64_t r_bs, const int64_t* r_len,
             int B, int64_t nq_max, int64_t nr_max, int norm, float* dist, int64_t* idx, int split, void* ws,
             size_t ws_bytes, void* stream);
int vggt_nn1_plan(int B, int64_t nq_max, int64_t nr_max, int cus);
size_t vggt_nn1_workspace_bytes(int B, int64_t nq_max, int64_t nr_max);

/*
 * The sums one rigid-ICP iteration needs, over the rows i < x_len[b] with
 * 0 <= idx[b, i] < y_len[b] (other rows are skipped), 17 fp64 values per batch
 * item in out (B, 17): count; sum x (3); sum y[idx] (3); sum x^T y[idx] (9,
 * row-major, x on rows); sum |x - y[idx]|^2.  x: (B, n_max, 3), y: (B, m_max, 3)
 * fp32, idx: (B, n_max) int64.  fp64 accumulation in a fixed order (per-workgroup
 * partials in ws, then one pass): two runs are bitwise equal.  ws: 8-byte
 * aligned, >= vggt_nn1_workspace_bytes(B, n_max, m_max).
 */
int vggt_nn1_pair_stats(const float* x, int64_t x_bs, const int64_t* x_len, const float* y, int64_t y_bs,
                        const int64_t* y_len, const int64_t* idx, int B, int64_t n_max, int64_t m_max, double* out,
                        void* ws, size_t ws_bytes, void* stream);

/*
 * Point-cloud preparation before ICP (Metrics.prepare_data_for_metrics,
 * training/training_metrics.py:264-358; csrc/points.hip; SPEC_ASSUMPTIONS.md).
 *
 * vggt_kth_value_f32: *out (device) = the exact k-th smallest (1-based) of the n
 * contiguous fp32 values at x, in torch.kthvalue's order: -inf < finite < +inf <
 * NaN (a NaN comes back, as the quiet NaN 0x7fc00000, only for ranks past the
 * non-NaN count); -0 and +0 compare equal and +0 stands for both.  Radix select,
 * four 8-bit passes over x, integer atomics only: a function of the multiset,
 * bitwise repeatable, no host synchronisation.  ws: 8-byte aligned, >=
 * vggt_kth_value_ws_bytes(n).  n < 1 or k outside [1, n]: VGGT_ERR_SHAPE.
 */
size_t vggt_kth_value_ws_bytes(int64_t n);
int vggt_kth_value_f32(const float* x, int64_t n, int64_t k, float* out, void* ws, size_t ws_bytes, void* stream);
/* The same select with the 1-based rank read from *k (device int64, 8-byte aligned) when the
 * launch runs.  A rank of 0 means "skip" and a rank outside [1, n] selects nothing: *out is
 * then the quiet NaN. */
int vggt_kth_value_f32_devrank(const float* x, int64_t n, const int64_t* k, float* out, void* ws, size_t ws_bytes,
                               void* stream);

/*
 * The bilinear subsample used below is F.interpolate(mode="bilinear",
 * align_corners=False, size=(Ho, Wo)) restated; per axis, with in -> out:
 *   scale = (float)in / (float)out;  src = max(fmaf(scale, dst + 0.5f, -0.5f), 0);
 *   i0 = min((int)src, in - 1);  i1 = min(i0 + 1, in - 1);
 *   l1 = clamp(src - i0, 0, 1);  l0 = 1 - l1;
 *   value = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d),
 * every product and sum rounded to fp32 on its own.  Ho == H && Wo == W is a pass
 * through (no arithmetic: a non-finite neighbour cannot enter through a zero
 * weight); otherwise non-finite taps propagate as this arithmetic propagates them.
 *
 * vggt_subsample_mask_count: *count_out (device int64) = the number of output
 * pixels, over all B * S images, where the subsample of the bool mask gt_mask
 * (B, S, H, W; one byte a pixel, as 0 / 1 floats) exceeds 0.5: one step of the
 * reference's subsampling-factor search (:305-306).  1 <= Ho <= H, 1 <= Wo <= W.
 */
int vggt_subsample_mask_count(const void* gt_mask, int B, int S, int H, int W, int Ho, int Wo, int64_t* count_out,
                              void* stream);

/*
 * vggt_prepare_clouds: the two clouds ICP receives (:323-355), per batch element b
 *   gt_cloud[b]   = the subsampled gt_points where the subsampled gt_mask > 0.5,
 *   pred_cloud[b] = the subsampled predicted points where the subsampled
 *                   (conf > *thr) mask > 0.5 and the subsampled gt_mask > 0.5,
 * both in row-major (S, Ho, Wo) order (boolean indexing's), padded to cap_g /
 * cap_p rows ((B, cap, 3) fp32; rows past a cap are dropped, rows past a length
 * are left untouched), with the full counts in gt_len / pred_len (device int64[B]).
 * The predicted points are depth (B, S, H, W) unprojected tap by tap -- ray =
 * kinv (u, v, 1), cam = ray * depth, world = R cam + t with kinv (B, S, 3, 3) the
 * inverse intrinsics and c2w (B, S, 3, 4) = [R | t], each 3-term dot summed left
 * to right, unfused -- or, with depth == NULL, point_map (B, S, H, W, 3).  conf:
 * (B, S, H, W); thr: a device scalar (vggt_kth_value_f32's out); gt_points:
 * (B, S, H, W, 3); gt_mask: (B, S, H, W) bool bytes.  All tensors contiguous.
 * A workgroup takes rows_per_workgroup output rows of one batch element (0 = as
 * many as hold 4096 pixels); the result does not depend on it.
 * phase: VGGT_PREPARE_COUNT decides every pixel, keeps the decisions in ws and
 * writes the lengths (the clouds may be NULL); VGGT_PREPARE_SCATTER writes the
 * clouds from the ws a COUNT call with the same arguments left;
 * VGGT_PREPARE_ALL does both.  ws: 8-byte aligned, >=
 * vggt_prepare_clouds_ws_bytes(B, S, Ho, Wo, rows_per_workgroup).
 * B > 65535 or S * H * W >= 2^31 - 256: VGGT_ERR_SHAPE.
 */
#define VGGT_PREPARE_ALL 0
#define VGGT_PREPARE_COUNT 1
#define VGGT_PREPARE_SCATTER 2
size_t vggt_prepare_clouds_ws_bytes(int B, int S, int Ho, int Wo, int rows_per_workgroup);
int vggt_prepare_clouds(const float* depth, const float* kinv, const float* c2w, const float* point_map,
                        const float* conf, const float* thr, const float* gt_points, const void* gt_mask, int B, int S,
                        int H, int W, int Ho, int Wo, float* pred_cloud, int64_t cap_p, float* gt_cloud, int64_t cap_g,
                        int64_t* pred_len, int64_t* gt_len, int rows_per_workgroup, int phase, void* ws,
                        size_t ws_bytes, void* stream);

/*
 * Per-chunk pose / Sim(3) composition of FeatureAlignedVGGT.forward
 * (featureAligned_vggt.py:96-143 and the point transform of :187-196), one
 * launch, no host synchronisation:
 *   chunk_se3 = pose_encoding_to_extri(chunk_sim3[:7]), scale = chunk_sim3[7];
 *   per_frame_se3 = [chunk_se3, pose_encoding_to_extri(frame_se3[f]) @ chunk_se3];
 *   extr = camera extrinsics (pose_encoding_to_extri_intri of cam_pose_enc)
 *          @ inv(extr[0]), translation * scale;
 *   mean = I (no context) | gt_first[b] | Markley mean over the overlap of
 *          inv(extr[k]) @ pose_encoding_to_extri(ctx_pose_enc[S_prev-ov+k])
 *          (averagePoseEncodings, geometry.py:4-37; ov == 1: the one transform);
 *   aligned_pose_enc = extri_intri_to_pose_encoding(extr @ (per_frame_se3 @ mean)).
 * chunk_sim3 [B,8], frame_se3 [B,S-1,7], cam_pose_enc [B,S,9] (T, quat xyzw,
 * FoV h/w), ctx_pose_enc [B,S_prev,9] = context["pose_enc"][-1] or NULL (first
 * chunk), gt_first [B,4,4] = gt_poses[:, 0] or NULL; all fp32 contiguous device.
 * Outputs aligned_pose_enc [B,S,9]; point_transform [B,4,4] (or NULL) =
 * context ? inv(per_frame_se3[:,0]) @ extr_raw[:,0] : extr_raw[:,0].
 * Without a context the mean is I whether or not gt_first is given (the first
 * chunk defines the frame); with a context gt_first wins over the overlap mean,
 * and overlap is then neither read nor checked.
 * Requires 1 <= overlap <= min(S, S_prev, 64) when the Markley path runs.
 */
int vggt_pose_compose(const float* chunk_sim3, const float* frame_se3, const float* cam_pose_enc,
                      const float* ctx_pose_enc, int S_prev, const float* gt_first, int B, int S, int overlap, int H,
                      int W, float* aligned_pose_enc, float* point_transform, void* stream);

/*
 * Per-chunk pose algebra of the pose-aligned VGGT (poseAligned_wrapped_vggt.py
 * :74-130, :171-177) in one launch, one 64-lane workgroup per batch element:
 *   extr  = pose_encoding_to_extri(cam_pose_enc) @ inv(extr_raw[:,0]);
 *   scale = gt ? | sum x.y / sum x^2 | over the S x 3 translations, x = extr's,
 *           y = those of gt @ inv(gt[:,0]) (scale_lse_solver; x, y and the sums in
 *           fp64 from the raw encodings, the quotient rounded to fp32 once; 0/0
 *           gives NaN, which is kept) : 1;
 *   extr[:, :, :3, 3] *= scale;
 *   mean  = I (no context) | gt[:,0] (context and gt, not centred) | Markley
 *           mean over the overlap of inv(extr[k]) @
 *           pose_encoding_to_extri(ctx_pose_enc[S_prev-ov+k]) (ov == 1: the one
 *           transform);
 *   aligned_pose_enc = extri_intri_to_pose_encoding(extr @ mean).
 * cam_pose_enc [B,S,9], ctx_pose_enc [B,S_prev,9] = context["pose_enc"][-1] or
 * NULL (first chunk), gt [B,S,3,4] = gt_poses or NULL; all fp32 contiguous
 * device.  Outputs aligned_pose_enc [B,S,9]; point_transform [B,4,4] (or NULL) =
 * context ? inv(mean) @ extr_raw[:,0] : extr_raw[:,0]; scales [B].
 * VGGT_ERR_SHAPE (nothing written): non-positive sizes, a NULL required pointer,
 * gt with S == 1, overlap outside [1, min(S, S_prev, 64)] when the overlap path
 * runs (context without gt; otherwise overlap is neither read nor checked).
 */
int vggt_pose_align(const float* cam_pose_enc, const float* ctx_pose_enc, int S_prev, const float* gt, int B, int S,
                    int overlap, int H, int W, float* aligned_pose_enc, float* point_transform, float* scales,
                    void* stream);

/*
 * GT alignment of a merged sequence from its poses (aligned_vggt/utils/alignment.py
 * of the reference: :206-242, :131-165, :325-370 with :6-59), one launch, one
 * 64-lane workgroup per batch element, lane-strided over frames.  Sums are
 * per-lane fp64 partials combined in lane order (no atomics, results independent
 * of the grid); every result is an fp64 function of the fp32 inputs rounded once.
 * pose_enc [B,S,enc_width] (enc_width 7 or 9: T, quat xyzw[, FoV h/w]), gt_extr
 * [B,S,3,4] w2c; fp32 contiguous device.  W = -1 means S, else 1 <= W <= S.
 *   VGGT_GT_POSE_SCALE      scales[b] = |sum x.y / sum x.x| over x = pose_enc[b,:W,:3],
 *                           y = gt_extr[b,:W,:3,3]  (scales [B])
 *   VGGT_GT_POSE_PER_FRAME  scales[b,0] = 1, scales[b,f] the same quotient over frame f
 *                           alone (scales [B,S]; W is not used)
 *   VGGT_GT_POSE_SIM3       Umeyama x -> y over the first W camera centres -R^T t (x from
 *                           pose_enc with the raw quaternion, y from gt_extr): means,
 *                           sigma_x and the covariance in fp64, the 3x3 SVD by Jacobi on
 *                           C^T C, the det(u) det(v) < 0 reflection fix.  transform [B,4,4]
 *                           = [R | t; 0 0 0 1], scales [B] = c.  With pose_enc_out
 *                           [B,S,9] non-NULL also the aligned encoding of all S frames
 *                           (fp32 as the reference: w2c -> c2w, translation x c,
 *                           transform ., -> w2c, mat_to_quat; FoV through the focal
 *                           length and back in fp64 for an img_h x img_w image);
 *                           pose_enc_out may be pose_enc.  Needs W >= 3 centres that are
 *                           not collinear: with fewer, or collinear ones, the rotation
 *                           about their line is not determined and sigma_x == 0 gives a
 *                           non-finite scale, as the reference's 1 / sigma_x.
 * A quotient that is 0/0 in the reference is NaN here.  transform and pose_enc_out
 * are neither read nor written in the first two modes.
 * VGGT_ERR_SHAPE: non-positive B or S, a NULL pose_enc / gt_extr / scales, enc_width
 * not 7 or 9, W outside [1, S], SIM3 without transform or with pose_enc_out and a
 * non-positive image size.  VGGT_ERR_UNSUPPORTED: an unknown mode; SIM3 with
 * enc_width 7 (the reference fails there too).
 */
#define VGGT_GT_POSE_SCALE 0
#define VGGT_GT_POSE_PER_FRAME 1
#define VGGT_GT_POSE_SIM3 2
int vggt_gt_pose_align(const float* pose_enc, int enc_width, const float* gt_extr, int B, int S, int W, int mode,
                       int img_h, int img_w, float* scales, float* transform, float* pose_enc_out, void* stream);

/*
 * The per-frame terms of one ATE / RPE / ScaleConsistency update
 * (eval/trajectory_metrics.py of the reference: :28-48, :154-182, :306-331) for B
 * sequences in one launch, one 64-lane workgroup per sequence.  pred_c2w, gt_c2w
 * [B,S,4,4] fp32 contiguous device.  Any output may be NULL:
 *   ate_vec [B,S,3]      pred[:3,3] - gt[:3,3]
 *   ate_norm [B,S]       its Euclidean norm
 *   rpe_trans, rpe_rot [B,S-delta]  for the pairs (i, i + delta), with
 *                        err = inv(inv(g_i) g_j) . inv(p_i) p_j: |err[:3,3]| and
 *                        acos(clamp((tr(err[:3,:3]) - 1) / 2, -1, 1)) in radians;
 *                        S <= delta writes nothing to either
 *   scale_factor [B,S-1] for the frames 1..S-1, g.p / max(p.p, 1e-8f) over the
 *                        translations p of pred and g of gt
 * inv is the general 4x4 inverse (adjugate), not the rigid closed form, as
 * torch.linalg.inv in the reference.  Everything is computed in fp64 from the
 * fp32 inputs and rounded once.  A singular pose gives non-finite outputs where
 * the reference raises.  VGGT_ERR_SHAPE: non-positive B or S, delta < 1, a NULL
 * input.
 */
int vggt_trajectory_errors(const float* pred_c2w, const float* gt_c2w, int B, int S, int delta, float* ate_vec,
                           float* ate_norm, float* rpe_trans, float* rpe_rot, float* scale_factor, void* stream);

/* ======================================================================
 * Training (backward) entry points -- alignment-head training, SURVEY.md §8f
 * row 4: train_featureAlignedVGGT_vkitti.yaml freezes the aggregator, camera
 * and depth heads (:80-83) and trains AlignmentHead (alignment_head.py) under
 * bf16-mixed autocast (run_model.py:472), with checkpoint()-recomputed blocks
 * (alignment_head.py:351-426).  Gradients of bf16 tensors are bf16 (what
 * autocast produces), parameter gradients fp32.  Column / row reductions
 * into parameter gradients are deterministic: fixed row chunks write partial
 * sums to `ws` (>= the size the matching *_workspace_bytes returns) and a
 * second pass ADDS them, in chunk order, to the fp32 gradient buffer.
 *
 * Error returns of the entries below from vggt_attention_small_bwd on (one
 * check per entry, before anything is launched or written): a dimension or
 * workspace rule broken, or a required pointer NULL with M > 0:
 * VGGT_ERR_SHAPE; a dtype argument that is neither VGGT_DTYPE_F32 nor
 * VGGT_DTYPE_BF16: VGGT_ERR_UNSUPPORTED; a leading dimension or a base pointer
 * off the stated alignment: VGGT_ERR_ALIGN.  Pointers called "may be NULL" are
 * the optional ones; every other pointer is required.  Each comment states its
 * entry's rules and its answer for M == 0.
 * ====================================================================== */

/* Forward attention as vggt_attention_fwd (exact scores, no Q prescale) that
 * also stores lse[(b*heads + h)*nq + q] = log2 sum_k exp2(q.k * scale * log2 e),
 * consumed by vggt_attention_bwd (recompute of the frame blocks' SDPA).  o is
 * normalised by the row sum of the bf16-rounded p that enter P.V (with one key
 * o == v bit for bit); the lse is that of the unrounded p. */
int vggt_attention_fwd_lse(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                           int64_t k_bstride, const void* v, int64_t ldv, int64_t v_bstride, void* o, int64_t ldo,
                           int64_t o_bstride, float* lse, int batch, int heads, int nq, int nk, int D, float scale,
                           void* stream);

/*
 * Flash-attention backward (bf16, D in {64,128}; F.scaled_dot_product_attention
 * backward in vggt Attention, ext, called by the alignment head's frame blocks).
 * q/k/v/o/dout strided as vggt_attention_fwd (v shares k's batch stride, dout
 * shares o's layout); lse from vggt_attention_fwd_lse; delta: fp32
 * [batch*heads*nq] scratch (written).  Writes bf16 dq [.., lddq] (q's batch
 * stride) and dk, dv [.., lddkv] (k's batch stride), e.g. straight into the
 * dqkv buffer laid out like qkv.
 */
int vggt_attention_bwd(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                       const void* v, int64_t ldv, const void* o, const void* dout, int64_t ldo, int64_t o_bstride,
                       const float* lse, float* delta, void* dq, int64_t lddq, void* dk, void* dv, int64_t lddkv,
                       int batch, int heads, int nq, int nk, int D, float scale, void* stream);

/*
 * Small-window attention backward (vggt_attention_small's shapes: temporal
 * cross attention, cross_attention.py:64-75, and the fp32 decoder blocks):
 * one 256-thread workgroup per (batch, head), recomputes P; dtype for every
 * operand.  dq [.., lddq] batch stride dq_bstride; dk, dv [.., lddkv] batch
 * stride dkv_bstride.  q, dout, k and v are staged in LDS as fp32 rows of
 * D + 1 (one pad column), so it needs
 * (2*nq*(D+1) + 2*nk*(D+1) + 2*nq*nk)*4 <= 64 KiB, else VGGT_ERR_SHAPE with
 * nothing written (D = 128: nq = 29, nk = 28 fits, 29 x 29 does not; D = 64:
 * nq = 1, nk = 125 does not).  D even; operand rows that are all 16-B aligned
 * with D % 8 == 0 are read 16 B per lane, any other layout element by element.
 * VGGT_ERR_SHAPE: batch, heads, nq, nk or D < 1 (no empty call), D odd, the LDS
 * limit, any of the seven pointers NULL; VGGT_ERR_UNSUPPORTED: dtype;
 * VGGT_ERR_ALIGN: lddq or lddkv odd, dq, dk or dv off 4 bytes.
 */
int vggt_attention_small_bwd(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk,
                             int64_t k_bstride, const void* v, int64_t ldv, const void* dout, int64_t ldo,
                             int64_t o_bstride, void* dq, int64_t lddq, int64_t dq_bstride, void* dk, void* dv,
                             int64_t lddkv, int64_t dkv_bstride, int dtype, int batch, int heads, int nq, int nk, int D,
                             float scale, void* stream);

/*
 * LayerNorm backward (nn.LayerNorm / F.layer_norm backward; every norm of the
 * alignment head): x = the forward input, dy the output gradient, same row
 * map as vggt_layernorm_grouped (logical row r -> group r/group; x and dx rows
 * g*x_group_stride + x_row_offset + i, dy rows g*y_group_stride +
 * y_row_offset + i).  accumulate: bit VGGT_LN_BWD_DX_ACCUMULATE (1) dx += (f32
 * only, else dx =); dw/db (may be NULL) get the parameter gradients added, or
 * written with bit VGGT_LN_BWD_PARAMS_WRITE (2).  C % 256 == 0, C <= 1024.
 * M == 0: VGGT_OK, nothing launched.  VGGT_ERR_SHAPE: M < 0, C not 256, 512 or
 * 1024, group < 1, x, dy or dx NULL, ws NULL or below
 * vggt_layernorm_bwd_workspace_bytes when dw or db is given;
 * VGGT_ERR_UNSUPPORTED: a dtype, an unknown accumulate bit, dx += into bf16;
 * VGGT_ERR_ALIGN: ldx, ldy or lddx % 4, x, dy or dx off 8 bytes.
 */
#define VGGT_LN_BWD_DX_ACCUMULATE 1
#define VGGT_LN_BWD_PARAMS_WRITE 2
size_t vggt_layernorm_bwd_workspace_bytes(int M, int C);
int vggt_layernorm_bwd(const void* x, int xdtype, int64_t ldx, const float* w, float eps, const void* dy, int dydtype,
                       int64_t ldy, void* dx, int dxdtype, int64_t lddx, int accumulate, int M, int C, int group,
                       int x_group_stride, int x_row_offset, int y_group_stride, int y_row_offset, float* dw,
                       float* db, void* ws, size_t ws_bytes, void* stream);

/*
 * Per-head LayerNorm + RoPE backward (q_norm/k_norm + rope of vggt Attention,
 * ext, and CrossAttention, cross_attention.py:59-62): pre = the bf16/f32
 * values before the norm (the linear's output), grad = d(output) in, d(pre)
 * out, in place.  Heads [0, hsplit) use w0 (gradients into dw0/db0), heads
 * [hsplit, H) use w1 (dw1/db1); NULL w = no norm.  RoPE conventions as
 * vggt_headnorm_rope.
 * M == 0: VGGT_OK, nothing launched.  VGGT_ERR_SHAPE: M < 0, H < 1, D not 64 or
 * 128, hsplit outside [0, H], pre or grad NULL, with a RoPE mode pos, cos_tab or
 * sin_tab NULL or period or tab_len < 1, ws NULL or below
 * vggt_headnorm_rope_bwd_workspace_bytes when a norm and a gradient pointer are
 * given; VGGT_ERR_UNSUPPORTED: dtype, an unknown rope_mode; VGGT_ERR_ALIGN: ldp
 * or ldg % 8, pre or grad off 16 bytes.
 */
size_t vggt_headnorm_rope_bwd_workspace_bytes(int M, int D);
int vggt_headnorm_rope_bwd(const void* pre, int64_t ldp, void* grad, int64_t ldg, int dtype, int M, int H, int hsplit,
                           int D, const float* w0, const float* w1, float eps, int rope_mode, const int32_t* pos,
                           int period, const float* cos_tab, const float* sin_tab, int tab_len, float* dw0,
                           float* db0, float* dw1, float* db1, void* ws, size_t ws_bytes, void* stream);

/* Column-reduction workspace for vggt_colsum / vggt_layerscale_bwd / vggt_gelu_bwd.  The three share
 * their rules: M < 1 (M == 0 included), N < 1 or N % 4, a required pointer NULL, ws NULL or too small:
 * VGGT_ERR_SHAPE; a dtype: VGGT_ERR_UNSUPPORTED; a leading dimension % 4, a bf16 / f32 matrix off 8 bytes
 * (dout and gamma of vggt_layerscale_bwd: 16): VGGT_ERR_ALIGN. */
size_t vggt_colred_workspace_bytes(int M, int N);

/* out[n] (+)= sum_m x[m, n]  (Linear bias gradients).  N % 4 == 0.  x and out are required. */
int vggt_colsum(const void* x, int dtype, int64_t ldx, int M, int N, float* out, int accumulate, void* ws,
                size_t ws_bytes, void* stream);

/*
 * LayerScale + residual backward (x + gamma * branch, vggt layers/block.py /
 * cross_attention.py:130-131): dbranch = gamma * dout (rounded to odtype),
 * dgamma += sum_m dout * branch, dbias += sum_m dbranch (the bias gradient of
 * the Linear that produced the branch).  dgamma / dbias may be NULL; dout, branch, gamma and dbranch
 * are required.
 */
int vggt_layerscale_bwd(const float* dout, int64_t ldd, const void* branch, int bdtype, int64_t ldb,
                        const float* gamma, void* dbranch, int odtype, int64_t ldo, int M, int N, float* dgamma,
                        float* dbias, void* ws, size_t ws_bytes, void* stream);

/* y = GELU(x) (exact erf), any f32/bf16 combination (Mlp.act, unfused training form).
 * M == 0: VGGT_OK, nothing launched.  VGGT_ERR_SHAPE: M < 0, N < 1 or N % 4, x or y NULL;
 * VGGT_ERR_UNSUPPORTED: a dtype; VGGT_ERR_ALIGN: ldx or ldy % 4, x or y off 8 bytes. */
int vggt_gelu_fwd(const void* x, int xdtype, int64_t ldx, void* y, int ydtype, int64_t ldy, int M, int N,
                  void* stream);

/* dpre = dh * GELU'(pre) (rounded to odtype); dbias += sum_m dpre (fc1 bias gradient; may be NULL).
 * dpre may be dh itself (same pointer, leading dimension and dtype: in place, as the MLP backward
 * calls it) and then holds the same bits as the out-of-place call; it must not overlap pre, nor dh
 * in any other way.  dh, pre and dpre are required. */
int vggt_gelu_bwd(const void* dh, int dhdtype, int64_t lddh, const void* pre, int predtype, int64_t ldp, void* dpre,
                  int odtype, int64_t ldo, int M, int N, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* x_f32[m, n] += gamma[n] * branch[m, n]  (LayerScale residual add with a saved branch).
 * Rules as vggt_resid_scale_add_from with out == x. */
int vggt_resid_scale_add(float* x, int64_t ldx, const void* branch, int bdtype, int64_t ldb, const float* gamma, int M,
                         int N, void* stream);

/* out_f32[m, n] = x_f32[m, n] + gamma[n] * branch[m, n]  (out may equal x).
 * M == 0: VGGT_OK, nothing launched.  VGGT_ERR_SHAPE: M < 0, N < 1 or N % 4, out, x, branch or gamma
 * NULL; VGGT_ERR_UNSUPPORTED: bdtype; VGGT_ERR_ALIGN: ldo, ldx or ldb % 4, out, x or gamma off 16
 * bytes, branch off 8. */
int vggt_resid_scale_add_from(float* out, int64_t ldo, const float* x, int64_t ldx, const void* branch, int bdtype,
                              int64_t ldb, const float* gamma, int M, int N, void* stream);

/* dst[c, r] = src[r, c] for 2-byte elements; columns r in [rows, rows_pad) of dst are zero
 * (weight-gradient GEMM operands: dW = dY^T X as vggt_gemm_bf16(dY^T, X^T)).
 * rows_pad == 0: VGGT_OK, nothing launched.  VGGT_ERR_SHAPE: rows < 0, cols < 1, rows_pad < rows, dst
 * NULL, src NULL with rows > 0. */
int vggt_transpose_b16(const void* src, int64_t lds, int rows, int cols, void* dst, int64_t ldd, int rows_pad,
                       void* stream);

/* dW[n, k] (+)= bf16(sum_m dY[m, n] X[m, k]) for bf16 row-major dY [M, N], X [M, K] (the bf16-tier
 * Linear weight gradients, rounded like autocast's bf16 weight gradient): split-K over the token
 * dimension into fp32 partials in ws (>= vggt_wgrad_bf16_workspace_bytes), summed in split order.
 * N % 128 == 0, K % 128 == 0.  VGGT_ERR_SHAPE: M, N or K < 1 (M == 0 included), N or K % 128, dy, x or dw
 * NULL, ws NULL or too small; VGGT_ERR_ALIGN: ldy or ldx % 8, dy or x off 16 bytes. */
size_t vggt_wgrad_bf16_workspace_bytes(int M, int N, int K);
int vggt_wgrad_bf16(const void* dy, int64_t ldy, const void* x, int64_t ldx, int M, int N, int K, float* dw,
                    int64_t ldw, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* dW[n, k] (+)= sum_m dY[m, n] X[m, k]  fp32 (skinny-M decoder / gated-update Linear weight gradients).
 * VGGT_ERR_SHAPE (the one error of this entry and the next): M, N or K < 1 (M == 0 included), N > 65535,
 * dy, x, dw (or db) NULL. */
int vggt_wgrad_f32(const float* dy, int64_t ldy, const float* x, int64_t ldx, int M, int N, int K, float* dw,
                   int64_t ldw, int accumulate, void* stream);
/* The same and db[n] (+)= sum_m dY[m, n] in the one launch (LinearF32Fn backward: weight and bias gradients). */
int vggt_wgrad_bias_f32(const float* dy, int64_t ldy, const float* x, int64_t ldx, int M, int N, int K, float* dw,
                        int64_t ldw, float* db, int accumulate, void* stream);

/* out[b] = sum_{i<n} a[b*bs + i] * c[b*bs + i]  (d chunk_scale of depth *= chunk_scale,
 * featureAligned_vggt.py:171, in training).  ws >= vggt_batch_dot_workspace_bytes(B, n).
 * VGGT_ERR_SHAPE (its one error): B or n < 1, a, c or out NULL, ws NULL or too small. */
size_t vggt_batch_dot_workspace_bytes(int B, int64_t n);
int vggt_batch_dot_f32(const float* a, const float* c, int64_t bs, int B, int64_t n, float* out, void* ws,
                       size_t ws_bytes, void* stream);

/* ======================================================================
 * Training losses -- the depth term of MultitaskLoss (training/loss.py:
 * compute_depth_loss :308-351, filter_by_quantile :421-457; csrc/loss.hip;
 * aligned_vggt/training/loss.py).  pred, conf, gt: (B, S, H, W) contiguous
 * fp32; mask: (B, S, H, W) bool bytes.  n = the number of set mask pixels.
 * Every branch the reference takes on n, on the threshold or on the
 * surviving count is taken on the device: no entry synchronises with the
 * host.  B * S * H * W > 100,000,000 (the reference's random-subsample
 * branch): VGGT_ERR_UNSUPPORTED.  Rows are read 128 bits per lane when
 * the float pointers are 16-byte and the mask 4-byte aligned, element by
 * element otherwise; H * W need not be a multiple of 4.
 *
 * vggt_depth_loss_values: amax[f] = the maximum of conf over frame f of the
 * B * S (NaN propagates, as torch.amax); *n_out (device int64) = n;
 *   val = |logf(max(pred, 1e-8f)) - logf(max(gt', 1e-8f))| * (conf / max(amax[f], 1e-8f))
 * at set pixels, gt' = gt with NaN and +-inf replaced by 0, and the quiet
 * NaN 0x7fc00000 at unset ones (NaN sorts last in torch.kthvalue's order: a
 * rank <= n over val selects what the reference selects over its gathered
 * vector).  max(x, c) keeps a NaN x, as torch.clamp_min.  ws: 16-byte
 * aligned, >= vggt_depth_loss_ws_bytes(B, S, H, W) (shared by the entries).
 *
 * vggt_depth_loss_reduce: from val and *n.  k = round_half_even(valid_range *
 * (n - 1)) + 1 (Python's round on the double product), or 0 when valid_range
 * <= 0 or n <= 1000; thr' = min(k-th smallest of val, 100) (a NaN stays);
 * m = #(min(val, 100) < thr').  *loss and the branch (state.kind):
 *   VGGT_DEPTH_LOSS_SKIPPED    n < 100: 0;
 *   VGGT_DEPTH_LOSS_FILTERED   k != 0 and m > 1000: the mean of the m kept min(val, 100);
 *   VGGT_DEPTH_LOSS_CLAMPED    k != 0 otherwise: the mean of min(val, 100) over the n;
 *   VGGT_DEPTH_LOSS_UNCLAMPED  k == 0: the mean of val over the n,
 * where a NaN or +-inf term counts as 0 (and still counts in the
 * denominator) and every term is clamped to +-100: check_and_fix_inf_nan
 * before the mean.  fp64 sums in a fixed order (per-workgroup partials, one
 * combining pass): two runs are bitwise equal.  state: 8-byte aligned,
 * VGGT_DEPTH_LOSS_STATE_BYTES: int64 n, m, k, kind; double denom (m or n; 0
 * when skipped); float thr' (NaN when k == 0); 4 bytes of padding.
 *
 * vggt_depth_loss_bwd: dpred = *grad_loss * sign(log p - log g') * conf_n / p
 * / denom at the pixels that contribute, p = max(pred, 1e-8f), recomputed
 * from the inputs, amax and state; 0 at unset, filtered-out and non-finite
 * pixels, where pred < 1e-8f, where |val| > 100, and everywhere when skipped.
 * ====================================================================== */
#define VGGT_DEPTH_LOSS_SKIPPED 0
#define VGGT_DEPTH_LOSS_FILTERED 1
#define VGGT_DEPTH_LOSS_CLAMPED 2
#define VGGT_DEPTH_LOSS_UNCLAMPED 3
#define VGGT_DEPTH_LOSS_STATE_BYTES 48
size_t vggt_depth_loss_ws_bytes(int B, int S, int H, int W);
int vggt_depth_loss_values(const float* pred, const float* conf, const float* gt, const void* mask, int B, int S,
                           int H, int W, float* val, float* amax, int64_t* n_out, void* ws, size_t ws_bytes,
                           void* stream);
int vggt_depth_loss_reduce(const float* val, const int64_t* n, int B, int S, int H, int W, double valid_range,
                           float* loss, void* state, void* ws, size_t ws_bytes, void* stream);
int vggt_depth_loss_bwd(const float* pred, const float* conf, const float* gt, const void* mask, const float* amax,
                        const void* state, const float* grad_loss, int B, int S, int H, int W, float* dpred,
                        void* stream);

/* ======================================================================
 * GT scale alignment -- the reference's scale_align_from_depths
 * (utils/alignment.py:244-323; csrc/gt_align.hip): per batch element b the
 * weighted median argmin_a sum_i w_i |a x_i - y_i| over its n = S * H * W
 * pixels.  pred (x), conf, gt (y): fp32; mask (m): one byte per pixel;
 * element b of each starts bstride elements after element b - 1.
 *
 *   cnt = sum m;  mean = (float)(sum_fp64(y * m) / max(cnt, 1)), the sum in
 *   a fixed order that depends on n alone;  min_depth = 0.1f * mean;
 *   per pixel, every operation rounded to fp32 on its own (max keeps a NaN):
 *     w = m * conf * (1 / max(max(y, min_depth), 1e-6f));  sign = x < 0 ? -1 : 1;
 *     x_pos = x * sign;  r = (y * sign) / max(x_pos, 1e-6f);  w_eff = w * x_pos;
 *   a w_eff that is NaN, +-inf or negative counts as 0;
 *   wmax = the largest w_eff;  e = the integer with ldexp(wmax, e) in
 *   (2^35, 2^36] (0 when wmax == 0);  q = rint(ldexp((double)w_eff, e)), uint64;
 *   r* = the smallest r of the multiset with 2 * sum_{r_i <= r*} q_i >= sum q
 *   in vggt_kth_value_f32's order (-inf < finite < +inf < NaN, -0 == +0): the
 *   reference's searchsorted(cumsum, 0.5 * total, "left"), a total of 0
 *   selecting the smallest r;  scale_out[b] = r* <= 0 ? -r* : r*.
 *
 * Integer sums only: the result is a function of the inputs alone, bitwise
 * repeatable and independent of the other elements.  No host
 * synchronisation.  scale_out: B device floats.  state_out: B records of
 * VGGT_DEPTH_SCALE_STATE_BYTES, 8-byte aligned: int64 cnt; uint64 sum q, sum
 * q over r < r*, sum q over r <= r*; float mean; int32 e; uint32 key of r*;
 * uint32 bits of wmax.  Pixels are read 128 bits per lane when the float
 * pointers are 16-byte and the mask 4-byte aligned (and bstride % 4 == 0
 * when B > 1), element by element otherwise.  ws: 16-byte aligned, >=
 * vggt_depth_scale_ws_bytes(B, n).  B < 1, B > 65535, n < 1, bstride < n
 * with B > 1, a null pointer, a misaligned or short ws: VGGT_ERR_SHAPE;
 * n > 100,000,000: VGGT_ERR_UNSUPPORTED; pred, conf, gt or scale_out not
 * 4-byte aligned, or state_out not 8-byte aligned: VGGT_ERR_ALIGN.
 * ====================================================================== */
#define VGGT_DEPTH_SCALE_STATE_BYTES 48
size_t vggt_depth_scale_ws_bytes(int B, int64_t n);
int vggt_depth_scale_l1(const float* pred, const float* conf, const float* gt, const void* mask, int B, int64_t n,
                        int64_t bstride, float* scale_out, void* state_out, void* ws, size_t ws_bytes, void* stream);

/* ======================================================================
 * GT alignment sim3_from_points (csrc/gt_points.hip): the reference's
 * umeyama_alignment_from_points (utils/alignment.py:372-426) and umeyama
 * (:6-59) on the device: percentile threshold, selection, compaction and the
 * closed-form Sim(3), with no host visit.
 *
 * Per batch element b, over the first P = W H Wimg pixels of that element
 * (W = min(seq_width, S)): pred and gt are points (P, 3) fp32, conf is (P,)
 * fp32, mask is (P,) one byte per pixel.  Element b of each tensor starts
 * b * its own batch stride after the pointer, counted in that tensor's
 * elements (floats for pred, conf and gt; bytes for the mask): the call is
 * [:, :seq_width] of (B, S, ...) tensors, so conf_bs and mask_bs are
 * S H Wimg >= P and pred_bs and gt_bs are 3 S H Wimg >= 3 P.  The four
 * strides are independent and ignored when B == 1.
 *
 * Threshold: thr = np.percentile(conf, q), method "linear", as numpy
 * computes it for a float32 array and a Python-float q: every operation
 * rounded to fp32 on its own, no fused multiply-add:
 *     h  = (float)(P - 1) * ((float)q / 100.0f)
 *     lo = min((int64)floorf(h), P - 1)
 *     g  = h - floorf(h)
 *     hi = min(lo + 1, P - 1)
 *     a  = v[lo];  c = v[hi]        order statistics, 0-based, in
 *                                   vggt_kth_value_f32's order
 *     d  = c - a
 *     thr = a + d * g;  if (g >= 0.5f) thr = c - d * (1.0f - g)
 *   (lo is clamped because h can round above P - 1 once P > 2^24; numpy
 *   takes the last element there.)  If any conf of the prefix is NaN, thr is
 *   NaN, as numpy's.  The select compares -0 and +0 equal and reports a
 *   selected zero as +0; no comparison against thr can tell the difference.
 * Selection: a pixel is kept when mask > 0 && conf >= thr && conf > 1e-5f;
 *   n counts the kept pixels; X and Y are the kept pred and gt rows in
 *   row-major (S, H, W) order, the order of boolean indexing.
 * Columns: VGGT_GT_POINTS_REFERENCE: sample i is x_i = (Xf[i], Xf[n + i],
 *   Xf[2n + i]) with Xf = X.reshape(-1), and Y alike: the reference's
 *   reshape(3, -1) of an (n, 3) selection, sic.  VGGT_GT_POINTS_POINTS:
 *   x_i = X[i], the per-point fit that the reference's docstring describes.
 * Umeyama: the means, sigma_x = E|x - mx|^2 and the centred cross-covariance
 *   E[(y - my)(x - mx)^T] in fp64 from the fp32 values, in two passes:
 *   per-lane partials, then one record per workgroup, added in a fixed order
 *   that depends on n alone (no floating-point atomics); R = U diag(1, 1, d)
 *   V^T and c = tr(D diag(1, 1, d)) / sigma_x from the library's 3x3 SVD;
 *   t = my - c R mx; R, t and c rounded to fp32 once.
 *
 * T: B x 16 floats, row-major 4x4 [R t; 0 0 0 1].  scale: B floats (c).
 * state: B records of VGGT_GT_POINTS_STATE_BYTES, 8-byte aligned: int64 n;
 * int64 count of NaN confidences; float thr; float a; float c; 4 bytes of
 * padding.  n == 0 (which a NaN thr implies): NaN in T[:3] and in scale; the
 * host route raises inside LAPACK there.  n == 1: sigma_x == 0, so scale and
 * t are NaN (0 / 0), as the reference's 1 / sigma_x makes them.  pred and gt
 * of an unselected pixel are never read: a NaN or inf there reaches no sum.
 * The result is a function of the inputs alone: bitwise repeatable, and an
 * element's result does not depend on the rest of the batch.  No host
 * synchronisation.
 *
 * Geometry: one 256-lane workgroup takes VGGT_GT_POINTS_GROUP consecutive
 * pixels of one element (in the two sum passes: samples), so a pass launches
 * ceil(P / VGGT_GT_POINTS_GROUP) x B workgroups; there is no grid cap and no
 * workgroup makes a second trip.  The confidences of the threshold passes
 * are read 128 bits per lane when conf is 16-byte aligned (and conf_bs % 4
 * == 0 when B > 1), element by element otherwise.
 *
 * ws: 16-byte aligned, >= vggt_gt_points_align_ws_bytes(B, P) (about
 * 24.2 B P bytes: the compacted rows have room for n = P; 0 for a shape the
 * call refuses).  VGGT_ERR_SHAPE: B < 1, B > 65535, P < 1, P >= 2^31 - 256,
 * with B > 1 a stride below P (pred_bs, gt_bs: below 3 P), q outside
 * [0, 100] or NaN, a null pointer, a misaligned or short ws.  Then
 * VGGT_ERR_UNSUPPORTED: columns not one of the two.  Then VGGT_ERR_ALIGN:
 * pred, conf, gt, T or scale not 4-byte aligned, state not 8-byte aligned.
 * ====================================================================== */
#define VGGT_GT_POINTS_REFERENCE 0
#define VGGT_GT_POINTS_POINTS 1
#define VGGT_GT_POINTS_STATE_BYTES 32
#define VGGT_GT_POINTS_GROUP 4096
size_t vggt_gt_points_align_ws_bytes(int B, int64_t P);
int vggt_gt_points_align(const float* pred, int64_t pred_bs, const float* conf, int64_t conf_bs, const float* gt,
                         int64_t gt_bs, const void* mask, int64_t mask_bs, int B, int64_t P, float q, int columns,
                         float* T, float* scale, void* state, void* ws, size_t ws_bytes, void* stream);

/* MFMA peak probe (diagnostic; BASELINE.md §2 asks for a measured MFMA microbenchmark with its clock):
 * nwg workgroups of 4 waves issue iters x 8 v_mfma_f32_32x32x16_bf16 each on the bf16 operands
 * (nwg * 256 * 16 elements: random or zeros), 32768 FLOP per MFMA; stamps[4 * wg] = s_memtime before /
 * after the loop, s_memrealtime (100 MHz) before / after.  sink: nwg * 256 floats, never read. */
int vggt_mfma_probe(unsigned long long* stamps, float* sink, const void* operands, int nwg, int iters, void* stream);

/* Attention segment stamps (diagnostic; VERDICT r5: where the global attention's waits go).  Runs the
 * default D = 64 forward (variant 33, the 8- / 4-wave choice of vggt_attention_fwd, o written as there) with
 * s_memtime stamps at each tile's boundaries; per wave (index (blockIdx * NW + wave) * 8) the cycle sums
 * [2] the tile's work up to its last LDS read, [3] end-of-tile vmcnt(0), [4] barrier ([0], [1], [5] unused),
 * [6] the wave's final s_memtime (low 32 bits); every wave runs ceil(nk / 64) tiles.  stamps: nwg * NW * 8 entries, NW = 8 for nq >= 4096 else 4. */
int vggt_attention_stamps(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                          const void* v, int64_t ldv, int64_t v_bstride, void* o, int64_t ldo, int64_t o_bstride,
                          unsigned long long* stamps, int batch, int heads, int nq, int nk, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VGGT_MI355X_H */
