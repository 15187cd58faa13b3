#!/usr/bin/env python3
"""Head cost of the gathered 3-D (metadata variations) step at a simulated world size (development aid, no pass/fail bar):

    python tools/bench_gathered_variations.py [--world 8] [--batches 8 32] [--variations 256] [--dim 512] [--iters 50] [--rounds 5]

One GPU, no process group: `cm3p_amd.dist.variation_head` has no collective in it, so one process drives it as rank 0 of `--world`
ranks with synthetic gathered buffers m_all (N*b*V, P) / b_all (N*b, P) that require gradients (the backward computes what the
reduce-scatter would carry).  Per batch size b it times, forward + backward,
  gathered: variation_head                          (logits (b*V, N*b) and (b, N*b*V), two cross-entropies);
  local:    _LogitsFn + cm3p_loss_hip at the same b, V  (logits (b*V, b), today's rank-local head).
The two alternate inside the process: --rounds blocks of --iters calls each after a warm-up of both; a block's window ends in a device
synchronise; ms per call = the median over a mode's blocks.  What it does NOT measure: the all-gathers and the reduce-scatter
themselves (they need N > 1 GPUs).  One JSON line per batch size.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cm3p_amd import modeling_cm3p as M  # noqa: E402
from cm3p_amd.dist import variation_head  # noqa: E402


def _unit(*shape, gen, dev):
    x = torch.randn(*shape, generator=gen)
    return (x / x.norm(dim=-1, keepdim=True)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--batches", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--variations", type=int, default=256)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, V, P = args.world, args.variations, args.dim
    gen = torch.Generator().manual_seed(0)
    print(f"# {torch.cuda.get_device_name(dev)}, hip {torch.version.hip}, torch {torch.__version__}; simulated world {N}, V {V}, P {P}; "
          f"{args.rounds} blocks of {args.iters} calls per mode, forward + backward, median block", flush=True)
    for b in args.batches:
        me = _unit(b, V, P, gen=gen, dev=dev).requires_grad_(True)
        be = _unit(b, P, gen=gen, dev=dev).requires_grad_(True)
        m_all = _unit(N * b * V, P, gen=gen, dev=dev).requires_grad_(True)
        b_all = _unit(N * b, P, gen=gen, dev=dev).requires_grad_(True)
        scale = torch.tensor(2.6592600, device=dev, requires_grad=True)
        classes = torch.randint(1, 3, (b, V), generator=gen)
        classes[torch.arange(b), torch.randint(0, V, (b,), generator=gen)] = 0
        classes = classes.to(dev)
        idx = M.K.first_zero_index(classes)
        leaves = (me, be, m_all, b_all, scale)

        def gathered():
            loss = variation_head(me, be, m_all, b_all, idx, 0, scale)[2]
            loss.backward()
            return loss

        def local():
            lpm = M._LogitsFn.apply(me.view(b * V, P), be, scale)
            loss = M.cm3p_loss_hip(lpm.view(b, V, b), classes)
            loss.backward()
            return loss

        def timed(fn):
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.iters

        modes = {"gathered": gathered, "local": local}
        res = {"world": N, "b": b, "V": V, "P": P, "iters": args.iters, "rounds": args.rounds}
        for m, fn in modes.items():  # warm-up
            res[f"loss_{m}"] = round(fn().item(), 6)
        ms = {m: [] for m in modes}
        for _ in range(args.rounds):
            for m, fn in modes.items():
                ms[m].append(timed(fn))
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        res["ms"] = {m: round(med[m], 3) for m in modes}
        res["ms_blocks"] = {m: [round(x, 3) for x in ms[m]] for m in modes}
        res["ratio_gathered_over_local"] = round(med["gathered"] / med["local"], 2)
        res["gathered_metadata_bytes"] = N * b * V * P * 4
        print(json.dumps(res), flush=True)
        del me, be, m_all, b_all
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
