// Process-wide kernel-variant knobs behind vggt_tune() (capi.cpp).
#pragma once
extern int g_vggt_gemm_tile;   // -1 auto, 0 128x128, 1 256x256 ring, 2 256x128 ring, 3-7 ping-pong, 8 two-per-CU, 9 persistent ping-pong
extern int g_vggt_attn_waves;  // 2, 4 or 8 (8: only for nq >= 4096; 2: offset-free variant 33 only)
extern int g_vggt_attn_variant; // attention schedule variant: one of the public ids capi.cpp accepts (attention.hip)
extern int g_vggt_attn_dma_half; // env VGGT_ATTN_DMA_HALF only (default 1): variant 33 runs 2081 in the 8-wave D = 64 form
extern int g_vggt_attn16;       // 1: variant 33 runs the 16x16x32 form for D = 64 (attn16_fwd_kernel), 2 (default): only for 4-wave launches
extern int g_vggt_conv_pf2;     // split-bf16 conv: 1 two-deep buffer-load gather, 0 one-deep
extern int g_vggt_linear_split_k;    // split-K vggt_linear_f32_ws: split while each split keeps >= this many k (2 splits' worth)
extern int g_vggt_linear_one_launch; // split-K vggt_linear_f32_ws: 1 combine in the same launch (default), 0 reduce launch
extern int g_vggt_linear_wk;         // vggt_linear_f32_ws, M <= 256: in-workgroup split-K, ~this many k per wave (0: off)
extern int g_vggt_gemm_balance;      // 1: persistent GEMMs with a partial last round split (whole rounds persistent, rest 128x128)
extern int g_vggt_attn_tail_split;   // global attention key-split tail: 0 per-element plan (default), -1 off, parts | tail_blocks << 8 forced (| bit 30: per element)
// The GEMM dispatcher's environment-only knobs (A/B switches; read once when the library loads, no vggt_tune id;
// gemm.hip's gemm_resolve states what each one decides)
struct GemmKnobs {
  int mid;            // VGGT_GEMM_MID (0): bit 0 the 128-wide ping-pong form for the mid-M residual projections, bit 1 also plain ones
  int persist;        // VGGT_GEMM_PERSIST (7): auto takes the persistent form for bit 0 bf16 / GELU / f32, bit 1 fused qkv, bit 2 residual
  int bm;             // VGGT_GEMM_BM (0): 192 / 256 forces the persistent row tile, any other value picks by rounds
  int fullk;          // VGGT_GEMM_FULLK (5): whole-K-tile segments for bit 0 bf16 / GELU / f32, bit 1 qkv, bit 2 residual, bit 3 GELU + pre
  int gm;             // VGGT_GEMM_GM (4), & 255: M-tiles per tile group of the persistent form (0: row-major)
  int split_dma;      // VGGT_GEMM_SPLITDMA (1): 0 only when set and zero
  int headnorm_tile;  // VGGT_HEADNORM_TILE (-1): the tile mode of vggt_gemm_headnorm while VGGT_TUNE_GEMM_TILE is auto
};
extern const GemmKnobs g_vggt_gemm_knobs;
// The small-window attention dispatcher's environment-only switches (small.hip's attn_small_resolve; same terms)
struct SmallKnobs {
  int attn_mfma;  // VGGT_ATTN_SMALL_MFMA (1): 0 keeps bf16 windows of <= 16 x 16 off the matrix-core form
  int attn_wg;    // VGGT_ATTN_SMALL_WG (1): 0 sends every window the matrix cores do not take to the one-wave form
};
extern const SmallKnobs g_vggt_small_knobs;
// per-stream launch configuration (vggt_set_stream_config): the CUs a CU-masked
// stream may use (0: the device's) and its VGGT_STREAM_* flags
int vggt_stream_cu_count(void* stream);
int vggt_stream_flags(void* stream);
