#!/usr/bin/env python3
"""What dropout costs: the element kernels and the attention kernels with and without their dropout instances at the C2 step's shapes
(attention: the band kernels with DROP against what a p = 0 step runs - the pipelined forward and the fused backward for the global
layers, the band kernels for the window-64 ones), and a C2-shape training step (bench.py's workload and batch) at p = 0.1 on all three
fields against p = 0, interleaved on one model (the dropout fields are read per forward call).

    python tools/dropout_time.py [--iters 30] [--steps 6]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cm3p_amd import _lib  # noqa: E402
from cm3p_amd import kernels as K  # noqa: E402


def _timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(iters):
    T, S, H, I = 32 * 4096, 4096, 768, 1152
    thr = K.dropout_threshold(0.1)
    g = torch.Generator(device="cuda").manual_seed(0)
    h = torch.randn(T, 2 * I, device="cuda", generator=g).to(torch.bfloat16)
    dg = torch.randn(T, I, device="cuda", generator=g).to(torch.bfloat16)
    x = torch.randn(T, H, device="cuda", generator=g)
    rows = [("geglu forward", lambda: K.geglu_fwd(h), lambda: K.geglu_fwd_dropout(h, thr, 1, 3, S)),
            ("geglu backward", lambda: K.geglu_bwd(dg, h), lambda: K.geglu_bwd_dropout(dg, h, thr, 1, 3, S)),
            ("embedding x o Z", lambda: K.cast_bf16(x), lambda: K.dropout_f32(x, thr, 1, 0, K.SITE_EMBED, S))]
    for name, plain, drop in rows:
        a, b = [], []
        for _ in range(3):  # interleaved
            a.append(_timed(plain, iters))
            b.append(_timed(drop, iters))
        print(f"{name:16s} plain {min(a) * 1e3:8.1f} us   dropout {min(b) * 1e3:8.1f} us", flush=True)
    print("(embedding row: 'plain' is the fp32 -> bf16 cast of the same rows, a pass of comparable traffic; p = 0 launches nothing)")


def attention(iters):
    B, S, nh = 32, 4096, 12
    thr = K.dropout_threshold(0.1)
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = (torch.randn(B * S, 3 * nh * 64, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    do = torch.randn(B * S, nh * 64, device="cuda", generator=g).to(torch.bfloat16)
    for window in (-1, 64):
        drop = (thr, 1, 0)
        out, lse = K.attn_fwd(qkv, None, B, S, nh, window, 0.125, True)
        outd, lsed = K.attn_fwd(qkv, None, B, S, nh, window, 0.125, True, drop=drop)
        rows = [("forward", lambda: K.attn_fwd(qkv, None, B, S, nh, window, 0.125, True),
                 lambda: K.attn_fwd(qkv, None, B, S, nh, window, 0.125, True, drop=drop)),
                ("backward", lambda: K.attn_bwd(qkv, out, do, lse, None, B, S, nh, window, 0.125, None, False, True),
                 lambda: K.attn_bwd(qkv, outd, do, lsed, None, B, S, nh, window, 0.125, None, False, True, drop=drop))]
        for name, plain, dropped in rows:
            a, b = [], []
            for _ in range(3):
                a.append(_timed(plain, iters))
                b.append(_timed(dropped, iters))
            print(f"attention {'global' if window < 0 else 'window 64'} {name:8s} p = 0 kernels {min(a):7.3f} ms   dropout {min(b):7.3f} ms", flush=True)
    _lib.profile_begin()
    K.attn_bwd(qkv, outd, do, lsed, None, B, S, nh, -1, 0.125, None, False, True, drop=(thr, 1, 0))
    for tag, (n, ms, _) in sorted(_lib.profile_end().items()):
        print(f"  global dropout backward, {tag}: {ms:.3f} ms", flush=True)


def step(n_steps):
    import bench
    from cm3p_amd import CM3PConfig, CM3PModel

    w = dict(bench.WORKLOADS["c2"])
    config = CM3PConfig(beatmap_config=dict(cls_embed=False), metadata_config=dict(cls_embed=False))
    torch.manual_seed(0)
    model = CM3PModel(config).to("cuda").train()
    for p in model.beatmap_model.audio_encoder.parameters():
        p.requires_grad_(False)
    batch = bench.make_batch(config, w, 0, "cuda")
    towers = [model.beatmap_model.encoder.config, model.metadata_model.encoder.config]

    def run(p):
        for c in towers:
            c.embedding_dropout = c.attention_dropout = c.mlp_dropout = p
        for q in model.parameters():
            q.grad = None
        model(**batch).loss.backward()

    for p in (0.0, 0.1, 0.0, 0.1):
        run(p)
    times = {0.0: [], 0.1: []}
    for _ in range(n_steps):
        for p in (0.0, 0.1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(p)
            e1.record()
            torch.cuda.synchronize()
            times[p].append(e0.elapsed_time(e1))
    for p, t in times.items():
        t = sorted(t)
        print(f"C2 step p = {p:.1f}: median {t[len(t) // 2]:7.2f} ms  (min {t[0]:.2f}, max {t[-1]:.2f}, {len(t)} steps)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=6)
    args = ap.parse_args()
    kernels(args.iters)
    attention(max(3, args.iters // 5))
    step(args.steps)


if __name__ == "__main__":
    main()
