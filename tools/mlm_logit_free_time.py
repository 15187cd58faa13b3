#!/usr/bin/env python3
"""What `logit_free_mlm_loss` costs and saves on the masked-LM head (development aid; bench.py's workload does not move):

    python tools/mlm_logit_free_time.py [--iters 3] [--rounds 5] [--shapes v7,mb16k,mb64k] [--out profiles/mlm_logit_free.txt]

The step: the head's autograd node alone - dense, bias-GELU, LayerNorm, decoder, masked cross entropy, forward + backward into every
parameter and h - on fp32 h [T, H] with labels on 15 % of the rows.  "off" is _MLMHeadLossFn (fp32 logits [T, Vp] written, kept, read
twice), "on" _MLMHeadLogitFreeLossFn (csrc/mlm_loss.hip: the decoder's tiles consumed in registers, recomputed in backward, the bf16
gradient in chunks of MLM_LOGIT_FREE_CHUNK_BYTES).  Shapes: v7 = the recipe's T = 131072, H = 768, V = 3167; mb16k / mb64k =
ModernBERT-base MLM, H = 768, V = 50368, T = 16384 / 65536.

One process per invocation.  Per shape the node is off, on and off again in every round - the two "off" series are the same code,
their ratio is the A/A spread the on / off ratio has to be read against - in --rounds alternating blocks of --iters steps after a
warm-up step of each; ms = the median over a series' blocks.  Times are HIP events around a block, ended by a synchronise.  Peak
memory: torch.cuda.max_memory_allocated over one step of each setting, above what is allocated before it (operands and parameters).
The loss of both settings is compared before anything is timed.  One JSON line per shape; --out also writes the text DESIGN section
4.12 quotes.
"""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cm3p_amd import modeling_cm3p as M  # noqa: E402

SHAPES = {"v7": (131072, 768, 3167), "mb16k": (16384, 768, 50368), "mb64k": (65536, 768, 50368)}
SERIES = (("off", False), ("on", True), ("off_again", False))


def timed(fn, iters):
    gc.collect()  # _MLMHeadLossFn's node keeps the logits it returned (a reference cycle): without this, 13 GB blocks pile up until Python's collector runs
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def median(v):
    return sorted(v)[len(v) // 2]


def run_shape(name, T, H, V, iters, rounds, dev):
    g = torch.Generator().manual_seed(7)
    p = dict(h=torch.randn(T, H, generator=g), Wd=torch.randn(H, H, generator=g) / H ** 0.5, bd=0.1 * torch.randn(H, generator=g),
             nw=1.0 + 0.1 * torch.randn(H, generator=g), Wdec=torch.randn(V, H, generator=g) * 2 / H ** 0.5, bdec=0.1 * torch.randn(V, generator=g))
    d = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
    lab = torch.where(torch.rand(T, generator=g) < 0.15, torch.randint(0, V, (T,), generator=g), torch.full((T,), -100)).to(dev)

    def step(on):
        for t in d.values():
            t.grad = None
        node = M._MLMHeadLogitFreeLossFn if on else M._MLMHeadLossFn
        out = node.apply(d["h"], d["Wd"], d["bd"], d["nw"], d["Wdec"], d["bdec"], 1e-5, lab, None)
        loss = out if on else out[1]
        loss.backward()
        return loss.detach()

    vals, peak = {}, {}
    for key, on in SERIES[:2]:  # warm-up of each setting, what it computes, and what it holds
        step(on)
        for t in d.values():
            t.grad = None
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        vals[key] = step(on).float().cpu()
        torch.cuda.synchronize()
        peak[key] = torch.cuda.max_memory_allocated() - base
    ms = {key: [] for key, _ in SERIES}
    for _ in range(rounds):
        for key, on in SERIES:
            ms[key].append(timed(lambda: step(on), iters))
    med = {k: median(v) for k, v in ms.items()}
    Vp = (V + 63) // 64 * 64
    return dict(shape=name, T=T, H=H, V=V, Vp=Vp, logits_fp32_bytes=T * Vp * 4, chunk_rows=M._mlm_logit_free_chunk_rows(Vp), iters=iters, rounds=rounds,
                ms={k: round(v, 3) for k, v in med.items()}, ms_blocks={k: [round(x, 3) for x in v] for k, v in ms.items()},
                ratio_on_over_off=round(med["on"] / med["off"], 4), ratio_off_again_over_off=round(med["off_again"] / med["off"], 4),
                peak_bytes_above_operands=peak, loss_abs_diff_on_vs_off=(vals["on"] - vals["off"]).abs().item(), loss=vals["off"].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="v7,mb16k,mb64k")
    ap.add_argument("--out", default=None, help="also write the results as a text table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mlm_logit_free_time.py measures on the GPU; there is no CPU path")
    dev = torch.device("cuda", 0)
    res = []
    for name in args.shapes.split(","):
        T, H, V = SHAPES[name]
        res.append(run_shape(name, T, H, V, args.iters, args.rounds, dev))
        print(json.dumps(res[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        prop = torch.cuda.get_device_properties(dev)
        with open(args.out, "w") as f:
            f.write("logit_free_mlm_loss off / on / off again on the masked-LM head node, alternating in one process: median of %d blocks of %d steps\n"
                    "per series, ms per forward + backward (tools/mlm_logit_free_time.py; fp32 h, labels on 15 %% of the rows; A/A = the second 'off'\n"
                    "series over the first; peak = max_memory_allocated over one step above the operands, GiB).\n"
                    "box: %s, %d CUs, HIP %s, torch %s\n\n" % (args.rounds, args.iters, prop.name, prop.multi_processor_count, torch.version.hip, torch.__version__))
            f.write("%-6s %7s %5s %6s %10s %10s %10s %8s %8s %9s %9s %12s %14s\n" % ("shape", "T", "H", "V", "off", "on", "off again", "on/off", "A/A",
                                                                                  "peak off", "peak on", "logits fp32", "|loss on-off|"))
            for r in res:
                f.write("%-6s %7d %5d %6d %10.3f %10.3f %10.3f %8.4f %8.4f %9.3f %9.3f %12.3f %14.2e\n" % (
                    r["shape"], r["T"], r["H"], r["V"], r["ms"]["off"], r["ms"]["on"], r["ms"]["off_again"], r["ratio_on_over_off"],
                    r["ratio_off_again_over_off"], r["peak_bytes_above_operands"]["off"] / 2 ** 30, r["peak_bytes_above_operands"]["on"] / 2 ** 30,
                    r["logits_fp32_bytes"] / 2 ** 30, r["loss_abs_diff_on_vs_off"]))
            f.write("\n")
            for r in res:
                f.write("%s blocks (ms per step, chunk rows %d): %s\n" % (r["shape"], r["chunk_rows"], json.dumps(r["ms_blocks"])))


if __name__ == "__main__":
    main()
