#!/usr/bin/env python3
"""Both routes of cm3p_gemm_f32 (the 16 x 16 kernel and the register-tiled kernel, CM3P_GEMM_F32_TILED) on the same call, timed in
one process (development aid, no pass/fail bar):

    python tools/ubench/gemm_f32_time.py [--rounds 7] [--block-ms 40] [--probe] [--out FILE]

The shape list is the gathered-variation head at N = 8 ranks, b = 32, V = 256, P = 512, H_meta = 256 (logits, their gradients, the
metadata projection and its gradients) and the local b x b head; --probe adds the projection of the b x b head and shapes around
kernels.GEMM_F32_TILED_MIN_OUTPUTS (1024 outputs) and around the 2^20 outputs from which the entry point takes its large tiles.  Per shape the routes alternate: --rounds blocks per route, a block = as many calls as fill
--block-ms (sized from a warm-up), timed by device events around the block; ms per call = the median block, `noise` = (max - min) /
median over a route's blocks.  The two results are compared bit for bit at the timed size.  TFLOP/s = 2 M N K / time; the share
is of the fp32 vector-FMA peak (157.3 TFLOP/s, which packed fp32 FMA reaches; there is no k split and no matrix core here).
`default` is the route kernels.gemm_f32 takes.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cm3p_amd import kernels as K  # noqa: E402
from cm3p_amd._lib import GEMM_F32_TILED, call, ptr, stream  # noqa: E402

PEAK_TFLOPS = 157.3
# name, M, N, K, A unit stride ('k' | 'r'), B unit stride
SHAPES = [
    ("logits meta-dir NT", 8192, 256, 512, "k", "k"),
    ("logits beat-dir NT", 32, 65536, 512, "k", "k"),
    ("d meta rows NN", 8192, 512, 256, "k", "r"),
    ("d gathered beatmaps TN", 256, 512, 8192, "r", "r"),
    ("d beat rows NN", 32, 512, 65536, "k", "r"),
    ("d gathered metadata TN", 65536, 512, 32, "r", "r"),
    ("projection NT", 8192, 512, 256, "k", "k"),
    ("projection d input NN", 8192, 256, 512, "k", "r"),
    ("projection d weight TN", 512, 256, 8192, "r", "r"),
    ("local head NT", 32, 32, 512, "k", "k"),
]
PROBES = [
    ("probe projection b=32 NT", 32, 512, 768, "k", "k"),
    ("probe projection b=32 d input NN", 32, 768, 512, "k", "r"),
    ("probe projection b=32 d weight TN", 512, 768, 32, "r", "r"),
    ("probe 8x8 NT", 8, 8, 512, "k", "k"),
    ("probe 16x16 NT", 16, 16, 768, "k", "k"),
    ("probe 4x512 NT", 4, 512, 768, "k", "k"),
    ("probe 128x128 NT", 128, 128, 512, "k", "k"),
    ("probe 256x256 NT", 256, 256, 512, "k", "k"),
    ("probe 512x512 NT", 512, 512, 512, "k", "k"),
    ("probe 1024x512 NT", 1024, 512, 512, "k", "k"),
    ("probe 2048x512 NT", 2048, 512, 512, "k", "k"),
    ("probe 2048x256 NN", 2048, 256, 512, "k", "r"),
    ("probe 1024x512 TN k=8192", 1024, 512, 8192, "r", "r"),
    ("probe 2048x512 TN k=8", 2048, 512, 8, "r", "r"),
    ("probe 8x2048 NT", 8, 2048, 512, "k", "k"),
    ("probe 32x8192 NT", 32, 8192, 512, "k", "k"),
    ("probe 32x16384 NT", 32, 16384, 512, "k", "k"),
    ("probe 32x32768 NT", 32, 32768, 512, "k", "k"),
    ("probe 64x16384 NT", 64, 16384, 512, "k", "k"),
]


def _operand(rows, Kd, unit, gen):
    x = torch.randn((rows, Kd) if unit == "k" else (Kd, rows), device="cuda", generator=gen)
    return x, ((Kd, 1) if unit == "k" else (1, rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=40.0)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name(0)}, hip {torch.version.hip}, torch {torch.__version__}; {args.rounds} blocks of >= {args.block_ms} ms per route, "
             f"routes alternating, median block; fp32 vector-FMA peak {PEAK_TFLOPS} TFLOP/s; GEMM_F32_TILED_MIN_OUTPUTS = {K.GEMM_F32_TILED_MIN_OUTPUTS}"]
    print(lines[0], flush=True)
    for name, M, N, Kd, ua, ub in SHAPES + (PROBES if args.probe else []):
        a, a_s = _operand(M, Kd, ua, gen)
        b, b_s = _operand(N, Kd, ub, gen)
        outs = {r: torch.empty(M, N, device="cuda") for r in ("16x16", "tiled")}
        flags = {"16x16": 0, "tiled": GEMM_F32_TILED}

        def run(r):
            call("cm3p_gemm_f32", ptr(a), ptr(b), ptr(outs[r]), M, N, Kd, a_s[0], a_s[1], b_s[0], b_s[1], N, 1.0, flags[r], stream())

        def block(r, iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run(r)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        iters = {}
        for r in outs:  # warm-up, and the block length
            run(r)
            torch.cuda.synchronize()
            iters[r] = max(3, min(2000, int(args.block_ms / max(block(r, 3), 1e-3)) + 1))
        same = torch.equal(outs["16x16"].view(torch.int32), outs["tiled"].view(torch.int32))
        ms = {r: [] for r in outs}
        for _ in range(args.rounds):
            for r in outs:
                ms[r].append(block(r, iters[r]))
        med = {r: sorted(v)[len(v) // 2] for r, v in ms.items()}
        res = {"shape": name, "M": M, "N": N, "K": Kd, "same_bits": same,
               "default": "tiled" if K.gemm_f32_route(M, N, a_s, b_s) else "16x16",
               "ms": {r: round(med[r], 4) for r in outs},
               "tflops": {r: round(2.0 * M * N * Kd / med[r] / 1e9, 2) for r in outs},
               "share_of_peak": {r: round(2.0 * M * N * Kd / med[r] / 1e9 / PEAK_TFLOPS, 3) for r in outs},
               "noise": {r: round((max(ms[r]) - min(ms[r])) / med[r], 3) for r in outs},
               "ratio_16x16_over_tiled": round(med["16x16"] / med["tiled"], 2), "iters": iters}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del a, b, outs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
