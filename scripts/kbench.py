#!/usr/bin/env python3
"""Per-kernel microbenchmark on the aggregator's production shapes (one
16-frame 518x518 chunk: M = 16 x 1374 = 21984 token rows, C = 1024, 16 heads
of 64).  Each kernel is timed with HIP events over R back-to-back launches on
the current stream.  Used to iterate on single kernels between full bench runs.

    python scripts/kbench.py [--reps 20] [--only gemm,norm,attn]   (train, small: not in the default set)

--only small: the latency-bound calls of small.hip at the shapes one chunk of bench.py's configuration
(16 frames of 518 x 518, 1370 tokens per frame, 5 overlap frames, 8 memory tokens) issues; these run
for microseconds, so the figure includes the host's launch cost (use --reps 200).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "large-scale-vit-slam_amd"))

import torch  # noqa: E402

from aligned_vggt import _native as N  # noqa: E402
from aligned_vggt.backbone.layers import RopeTables  # noqa: E402


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="gemm,norm,attn")
    ap.add_argument("--gemm-modes", default="0,1,2")
    ap.add_argument("--attn-waves", default="4,8")
    ap.add_argument("--attn-variants", default="33")
    ap.add_argument("--rounds", type=int, default=1, help="repeat the attention sweep (A/B alternation)")
    ap.add_argument("--warm-s", type=float, default=3.0)
    ap.add_argument("--tokens", type=int, default=16 * 1374,
                    help="token rows M (6592 = the 154x518 sequence chunk, 16 x 412)")
    args = ap.parse_args()
    only = set(args.only.split(","))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    M, C, H, D = args.tokens, 1024, 16, 64
    res = {}
    if "gemm" in only:
        x = (torch.randn(M, 4096, device=dev) * 0.5).bfloat16()
        # clocks / power to the steady state before the first measured shape
        wq = (torch.randn(3 * C, C, device=dev) * C ** -0.5).bfloat16()
        oq = torch.empty(M, 3 * C, device=dev, dtype=torch.bfloat16)
        t_end = time.time() + args.warm_s
        while time.time() < t_end:
            N.gemm_bf16(x[:, :C], wq, torch.zeros(3 * C, device=dev), oq, N.EPI_BF16)
            torch.cuda.synchronize()
        for mode, (name, Nn, K, epi) in [(md, sh) for md in map(int, args.gemm_modes.split(",")) for sh in (
                ("qkv", 3 * C, C, N.EPI_BF16), ("proj", C, C, N.EPI_RESID_F32), ("fc1", 4 * C, C, N.EPI_GELU_BF16),
                ("fc1_plain", 4 * C, C, N.EPI_BF16), ("fc2", C, 4 * C, N.EPI_RESID_F32),
                ("fc2_plain", C, 4 * C, N.EPI_BF16), ("proj_plain", C, C, N.EPI_BF16))]:
            N.tune(N.TUNE_GEMM_TILE, mode)
            w = (torch.randn(Nn, K, device=dev) * K ** -0.5).bfloat16()
            bias = torch.randn(Nn, device=dev) * 0.1
            a = x[:, :K]
            if epi == N.EPI_RESID_F32:
                out = torch.randn(M, Nn, device=dev)
                gamma = torch.rand(Nn, device=dev)
            else:
                out = torch.empty(M, Nn, device=dev, dtype=torch.bfloat16)
                gamma = None
            us = timeit(lambda: N.gemm_bf16(a, w, bias, out, epi, gamma=gamma), args.reps)
            res[f"{name}/tile{mode}"] = {"us": round(us, 1), "tflops": round(2 * M * Nn * K / us / 1e6, 1)}
            print(f"{name}/tile{mode}", res[f"{name}/tile{mode}"], flush=True)
            if name == "qkv":  # the production form: q/k LayerNorm + RoPE2D in the epilogue
                yy, xx = torch.meshgrid(torch.arange(37), torch.arange(37), indexing="ij")
                pos = torch.cat([torch.zeros(5, 2, dtype=torch.long),
                                 torch.stack([yy.reshape(-1), xx.reshape(-1)], -1) + 1], 0)
                rp = RopeTables(pos, D, 100.0, dev)
                qw, qb, kw, kb = (torch.rand(D, device=dev) for _ in range(4))
                us = timeit(lambda: N.gemm_qkv(a, w, bias, out, H, D, qw, qb, kw, kb, 1e-5, rp.mode, rp.pos, rp.period,
                                               rp.cos, rp.sin), args.reps)
                res[f"qkv_fused/tile{mode}"] = {"us": round(us, 1), "tflops": round(2 * M * Nn * K / us / 1e6, 1)}
                print(f"qkv_fused/tile{mode}", res[f"qkv_fused/tile{mode}"], flush=True)
    if "norm" in only:
        xf = torch.randn(M, C, device=dev)
        y = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
        w, b = torch.rand(C, device=dev), torch.rand(C, device=dev)
        us = timeit(lambda: N.layernorm(xf, w, b, 1e-5, y), args.reps)
        res["layernorm"] = {"us": round(us, 1), "gbs": round(M * C * 6 / us / 1e3, 1)}
        qkv = torch.randn(M, 3 * C, device=dev).bfloat16()
        qw, qb, kw, kb = (torch.rand(D, device=dev) for _ in range(4))
        yy, xx = torch.meshgrid(torch.arange(37), torch.arange(37), indexing="ij")
        pos = torch.stack([yy.reshape(-1), xx.reshape(-1)], -1) + 1
        pos = torch.cat([torch.zeros(5, 2, dtype=pos.dtype), pos], 0)
        rp = RopeTables(pos, D, 100.0, dev)
        us = timeit(lambda: N.qknorm_rope(qkv, H, D, qw, qb, kw, kb, 1e-5, rp.mode, rp.pos, rp.period, rp.cos, rp.sin),
                    args.reps)
        res["qknorm_rope"] = {"us": round(us, 1), "gbs": round(M * 2 * C * 4 / us / 1e3, 1)}
        # the residual forms; gbs from the bytes each moves per element (x f32, y / xn bf16)
        yb, yb2 = torch.randn(M, C, device=dev).bfloat16(), torch.randn(M, C, device=dev).bfloat16()
        gam, gam2 = torch.rand(C, device=dev) * 1e-3, torch.rand(C, device=dev) * 1e-3
        for name, nbytes, fn in (
                ("resid_add_layernorm", 12, lambda: N.resid_add_layernorm(xf, yb, gam, None, w, b, 1e-5, y)),
                ("resid_add_layernorm_nostore", 8, lambda: N.resid_add_layernorm_nostore(xf, yb, gam, w, b, 1e-5, y)),
                ("resid_add2_layernorm", 14,
                 lambda: N.resid_add2_layernorm(xf, yb, gam, yb2, gam2, None, w, b, 1e-5, y))):
            us = timeit(fn, args.reps)
            res[name] = {"us": round(us, 1), "gbs": round(M * C * nbytes / us / 1e3, 1)}
        dy, dx = torch.randn(M, C, device=dev).bfloat16(), torch.empty(M, C, device=dev)
        dw, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        us = timeit(lambda: N.layernorm_bwd(xf, w, 1e-5, dy, dx, False, dw, db), args.reps)
        res["layernorm_bwd"] = {"us": round(us, 1), "gbs": round(M * C * 10 / us / 1e3, 1)}
    if "train" in only:
        # the backward kernels of train.hip at the alignment head's training shapes (layernorm_bwd: under "norm")
        bf = lambda *s: torch.randn(*s, device=dev).bfloat16()  # noqa: E731
        dy4, xk = bf(M, 4 * C), bf(M, C)
        for Nn in (4 * C, 3 * C):
            dw = torch.zeros(Nn, C, device=dev)
            us = timeit(lambda: N.wgrad_bf16(dy4[:, :Nn], xk, dw, False), args.reps)
            res[f"wgrad_bf16/{Nn}x{C}"] = {"us": round(us, 1), "tflops": round(2 * M * Nn * C / us / 1e6, 1)}
        for Nn in (C, 4 * C):
            out = torch.zeros(Nn, device=dev)
            us = timeit(lambda: N.colsum(dy4[:, :Nn], out), args.reps)
            res[f"colsum/{Nn}"] = {"us": round(us, 1), "gbs": round(M * Nn * 2 / us / 1e3, 1)}
        dout, gam, dbr = torch.randn(M, C, device=dev), torch.rand(C, device=dev), torch.empty_like(xk)
        dg, dbi = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        us = timeit(lambda: N.layerscale_bwd(dout, xk, gam, dbr, dg, dbi), args.reps)
        res["layerscale_bwd/1024"] = {"us": round(us, 1), "gbs": round(M * C * 8 / us / 1e3, 1)}
        pre4, dpre, db4 = bf(M, 4 * C), torch.empty_like(dy4), torch.zeros(4 * C, device=dev)
        us = timeit(lambda: N.gelu_bwd(dy4, pre4, dpre, db4), args.reps)
        res["gelu_bwd/4096"] = {"us": round(us, 1), "gbs": round(M * 4 * C * 6 / us / 1e3, 1)}
        yy, xx = torch.meshgrid(torch.arange(37), torch.arange(37), indexing="ij")
        pos = torch.cat([torch.zeros(5, 2, dtype=torch.long), torch.stack([yy.reshape(-1), xx.reshape(-1)], -1) + 1], 0)
        rp = RopeTables(pos, D, 100.0, dev)
        qpre, dq = bf(M, C), bf(M, C)
        hw, hdw, hdb = torch.rand(D, device=dev), torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        us = timeit(lambda: N.headnorm_rope_bwd(qpre, dq, H, H, D, hw, None, 1e-5, rp.mode, rp.pos, rp.period, rp.cos,
                                                rp.sin, hdw, hdb), args.reps)
        res["headnorm_rope_bwd/16x64"] = {"us": round(us, 1), "gbs": round(M * C * 6 / us / 1e3, 1)}
        # the temporal block as autograd.py calls it: one group per token position, the 16 frames attend each other
        S, Ha = 16, 8
        q, k, v, do = (bf(M, C) for _ in range(4))
        gq, gkv = torch.empty_like(q), torch.empty(M, 2 * C, device=dev, dtype=torch.bfloat16)
        us = timeit(lambda: N.attention_small_bwd(q, k, v, do, gq, gkv[:, :C], gkv[:, C:], M // S, Ha, S, S, C // Ha, S,
                                                  S, S, S, S), args.reps)
        res["attention_small_bwd/16x16"] = {"us": round(us, 1), "gbs": round(M * C * 14 / us / 1e3, 1)}
    if "small" in only:
        f32 = lambda *sh: torch.randn(*sh, device=dev)  # noqa: E731
        E = {"f32": N.EPI_F32, "gelu": N.EPI_GELU_BF16, "resid": N.EPI_RESID_F32}
        # (name, M, N, K, epilogue, act_in): camera_head.py (dim 2048, 16 heads, M = 16 frames), alignment_head.py's
        # decoder (dec 512, 8 heads: one chunk token against 16 frames + 8 memory tokens, 15 frame tokens against the
        # chunk token; cross_attention.py forward_f32) and gated_update.py's gate MLP (8 memory tokens)
        linears = [("cam_embed_pose", 16, 2048, 9, "f32", 0), ("cam_modulation", 16, 6144, 2048, "f32", 1),
                   ("cam_qkv", 16, 6144, 2048, "f32", 0), ("cam_proj", 16, 2048, 2048, "resid", 0),
                   ("cam_fc1", 16, 8192, 2048, "gelu", 0), ("cam_fc2", 16, 2048, 8192, "resid", 0),
                   ("cam_pose_fc1", 16, 1024, 2048, "gelu", 0), ("cam_pose_fc2", 16, 9, 1024, "f32", 0),
                   ("dec_project", 16, 512, 1024, "f32", 0), ("dec_frame_proj", 1, 4096, 512, "f32", 0),
                   ("dec_chunk_q", 1, 512, 512, "f32", 0), ("dec_chunk_kv", 24, 1024, 512, "f32", 0),
                   ("dec_chunk_fc1", 1, 2048, 512, "gelu", 0), ("dec_chunk_fc2", 1, 512, 2048, "resid", 0),
                   ("dec_frame_q", 15, 512, 512, "f32", 0), ("dec_frame_fc1", 15, 2048, 512, "gelu", 0),
                   ("dec_frame_fc2", 15, 512, 2048, "resid", 0), ("dec_se3_fc1", 15, 256, 512, "gelu", 0),
                   ("dec_se3_fc2", 15, 7, 256, "f32", 0), ("gate_fc1", 8, 512, 1024, "gelu", 0),
                   ("gate_fc2", 8, 1, 512, "f32", 0)]
        for name, m, n, k, epi, act in linears:
            a, w, bias, out, gam = f32(m, k), f32(n, k) * k ** -0.5, f32(n), f32(m, n), torch.rand(n, device=dev)
            us = timeit(lambda: N.linear_f32(a, w, bias, out, E[epi], act_in=act, gamma=gam if epi == "resid" else None),
                        args.reps)
            res[f"linear_f32/{name}/{m}x{n}x{k}"] = {"us": round(us, 2), "form": N.linear_f32_form(m, n, k)["name"]}
        # GatedUpdate (B = 1, Nt = 8, D = 512): its three stages and the grouped pair of the per-token delta MLPs
        Nt, Dm = 8, 512
        mem, upd, dl, logit = f32(1, Nt, Dm), f32(1, Dm), f32(1, Nt, Dm), f32(Nt)
        inp, g_in, go = f32(1, Nt, 3 * Dm), f32(Nt, 2 * Dm), f32(1, Nt, Dm)
        w1, b1, w2, b2, hid = f32(Nt, Dm, 3 * Dm) * 0.03, f32(Nt, Dm), f32(Nt, Dm, Dm) * 0.04, f32(Nt, Dm), f32(Nt, 1, Dm)
        for name, fn in (("gated_update_prep", lambda: N.gated_update_prep(mem, upd, inp, g_in)),
                         ("linear_f32_grouped/delta_fc1/8x1x512x1536",
                          lambda: N.linear_f32_grouped(inp.transpose(0, 1), w1, b1, hid, N.EPI_GELU_BF16)),
                         ("linear_f32_grouped/delta_fc2/8x1x512x512",
                          lambda: N.linear_f32_grouped(hid, w2, b2, dl.transpose(0, 1), N.EPI_F32)),
                         ("gated_update_diff", lambda: N.gated_update_diff(mem, dl, g_in)),
                         ("gated_update_tail", lambda: N.gated_update_tail(mem, dl, logit, go))):
            res[name] = {"us": round(timeit(fn, args.reps), 2)}
        # temporal windows (cross_attention.py forward_rows_bf16: one group per token position, 16 frames against the
        # 5 overlap frames or each other; 8 heads of 128, and of 64 at half the width), the decoder's and the
        # camera trunk's fp32 windows
        G = 1370
        for nq, nk, Hh, Dh in ((16, 5, 8, 128), (16, 16, 8, 128), (16, 5, 8, 64), (16, 16, 8, 64)):
            q, k, v = ((torch.randn(G * n, Hh * Dh, device=dev)).bfloat16() for n in (nq, nk, nk))
            o = torch.empty_like(q)
            us = timeit(lambda: N.attention_small(q, k, v, o, G, Hh, nq, nk, Dh, nq, nk, nq), max(3, args.reps // 4))
            res[f"attention_small/bf16/{nq}x{nk}x{Dh}"] = {"us": round(us, 2), "form": N.attention_small_form(
                N.DTYPE_BF16, nq, nk, Dh, batch=G, heads=Hh)["name"]}
        for name, nq, nk, Hh, Dh in (("dec_chunk", 1, 24, 8, 64), ("dec_frame", 15, 1, 8, 64), ("cam_trunk", 16, 16, 16, 128)):
            q, k, v = (f32(n, Hh * Dh) for n in (nq, nk, nk))
            o = torch.empty_like(q)
            us = timeit(lambda: N.attention_small(q, k, v, o, 1, Hh, nq, nk, Dh, nq, nk, nq), args.reps)
            res[f"attention_small/f32/{name}/{nq}x{nk}x{Dh}"] = {"us": round(us, 2), "form": N.attention_small_form(
                N.DTYPE_F32, nq, nk, Dh, heads=Hh)["name"]}
        # the fp32 head norm: the decoder's q with RoPE 1D (15 rows, 8 heads of 64), the camera trunk's q of the packed qkv
        pos = torch.arange(1, 16, dtype=torch.int32, device=dev)
        cos, sin, hw, hb = f32(32, 64), f32(32, 64), torch.rand(64, device=dev), f32(64)
        qd, qkv, cw, cb = f32(15, 512), f32(16, 6144), torch.rand(128, device=dev), f32(128)
        for name, fn in (("headnorm_rope_f32/dec_q_rope1d/15x8x64",
                          lambda: N.headnorm_rope_any(qd, 0, 8, 64, hw, hb, 1e-5, N.ROPE_1D, pos, 15, cos, sin)),
                         ("headnorm_rope_f32/cam_q/16x16x128", lambda: N.headnorm_rope_any(qkv, 0, 16, 128, cw, cb, 1e-5))):
            res[name] = {"us": round(timeit(fn, args.reps), 2)}
        # the alignment head's input cast (16 x 1369 patch tokens of 2048)
        xt = f32(16 * 1369, 2048)
        yt = torch.empty(16 * 1369, 2048, device=dev, dtype=torch.bfloat16)
        res["cast_f32_bf16/21904x2048"] = {"us": round(timeit(lambda: N.cast_f32_bf16(xt, yt), max(3, args.reps // 4)), 2)}
        for key in [k for k in res if k.split("/")[0] in ("linear_f32", "linear_f32_grouped", "attention_small",
                                                          "headnorm_rope_f32", "cast_f32_bf16") or k.startswith("gated_")]:
            print(key, res[key], flush=True)
    if "attn" in only:
        qkv = (torch.randn(M, 3 * C, device=dev)).bfloat16()
        o = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        # bring clocks / power to the steady state first (the first ~2 s of a
        # cold box measure 5-20% slow)
        t_end = time.time() + args.warm_s
        while time.time() < t_end:
            N.attention(q, k, v, o, 1, H, M, M, D, M, M, M)
            torch.cuda.synchronize()
        for rnd, var, nw, (name, batch, n) in [(r_, v_, w_, sh) for r_ in range(args.rounds)
                                          for v_ in map(int, args.attn_variants.split(","))
                                          for w_ in map(int, args.attn_waves.split(","))
                                          for sh in (("global_attn", 1, M), ("frame_attn", 16, M // 16))]:
            N.tune(N.TUNE_ATTN_WAVES, nw)
            N.tune(N.TUNE_ATTN_VARIANT, var)
            us = timeit(lambda: N.attention(q, k, v, o, batch, H, n, n, D, n, n, n),
                        max(3, args.reps // 4))
            key = f"{name}/w{nw}/v{var}" + (f"/r{rnd}" if args.rounds > 1 else "")
            res[key] = {"us": round(us, 1), "tflops": round(4 * batch * H * n * n * D / us / 1e6, 1)}
            print(key, res[key], flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
