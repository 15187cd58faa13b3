#!/usr/bin/env python3
"""Attention forward and backward at head sizes 96 and 128 (csrc/attention_hd.hip) beside the head-64 kernels on the same amount of work.

    python tools/attn_hd_time.py [--rounds 7] [--iters 50] [--out profiles/attention_hd.txt]

B = 4, S = 4096, window = -1 (global) and window = 64, three arms with the same B S nh D (hidden 768) and the same FLOPs:
    (nh 6, D 128) and (nh 8, D 96) on K.attn_fwd_generic / K.attn_bwd_generic,
    (nh 12, D 64)                    on K.attn_fwd / K.attn_bwd (q not prescaled): the kernels every default tower runs.
One process, the arms interleaved: every round times each arm once (device events around `iters` launches), the figure of an arm is the
median over the rounds, the spread its (max - min) / median.  FLOPs are the algorithmic count: forward 4 B nh S keys D, backward twice that.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cm3p_amd import kernels as K  # noqa: E402

B, S = 4, 4096
ARMS = [("hd128", 6, 128), ("hd96", 8, 96), ("hd64", 12, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    fns = {}
    for window in (-1, 64):
        for name, nh, D in ARMS:
            qkv = (torch.randn(B, S, 3, nh, D, device="cuda", generator=g) * 0.8).to(torch.bfloat16)
            do = (torch.randn(B * S, nh * D, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
            scale = D ** -0.5
            if D == 64:
                fwd = lambda qkv=qkv, nh=nh, window=window, scale=scale: K.attn_fwd(qkv, None, B, S, nh, window, scale, prescaled=False)
                out, lse = fwd()
                bwd = lambda qkv=qkv, out=out, do=do, lse=lse, nh=nh, window=window, scale=scale: K.attn_bwd(qkv, out, do, lse, None, B, S, nh, window, scale, prescaled=False)
            else:
                fwd = lambda qkv=qkv, nh=nh, D=D, window=window, scale=scale: K.attn_fwd_generic(qkv, None, B, S, nh, D, window, scale)
                out, lse = fwd()
                bwd = lambda qkv=qkv, out=out, do=do, lse=lse, nh=nh, D=D, window=window, scale=scale: K.attn_bwd_generic(qkv, out, do, lse, None, B, S, nh, D, window, scale)
            fns[(window, name, "fwd")] = fwd
            fns[(window, name, "bwd")] = bwd
    for fn in fns.values():  # warm every shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.iters)
    lines = [f"attention at head sizes 128 / 96 / 64, B = {B}, S = {S}, hidden 768 (nh x D), no mask; {args.rounds} interleaved rounds x {args.iters} launches, "
             f"median ms per call (spread = (max - min) / median); {torch.cuda.get_device_name(0)}, torch {torch.__version__}"]
    for window in (-1, 64):
        keys = S if window < 0 else 2 * window + 1
        lines.append(f"window = {window} ({'global' if window < 0 else 'sliding'}):")
        for what, mult in (("fwd", 4.0), ("bwd", 8.0)):
            med = {name: statistics.median(times[(window, name, what)]) for name, _, _ in ARMS}
            for name, nh, D in ARMS:
                t = times[(window, name, what)]
                flops = mult * B * nh * S * keys * D
                lines.append(f"  {what} nh {nh:2d} D {D:3d}  {med[name]:8.3f} ms  spread {(max(t) - min(t)) / med[name]:5.1%}  {flops / med[name] / 1e9:8.1f} TFLOP/s"
                             f"  x{med[name] / med['hd64']:5.2f} of the head-64 arm")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
