#!/usr/bin/env python3
"""What `predict_tokens` costs and saves against the full-logits route (development aid; bench.py's workload does not move):

    python tools/mlm_topk_time.py [--iters 2] [--rounds 5] [--shapes v7,mb] [--k 5] [--out profiles/mlm_topk.txt]

Both routes answer the same question on the same model and batch - the k most likely tokens at 15 % of the positions:
  full   `model(...).logits` (every position's fp32 logits, [B, S, V]), the listed rows of it, torch.topk: what a caller had before;
  topk   `model.predict_tokens(..., positions=rows, k=k)`: the last layer and the head on the listed rows, cm3p_mlm_topk, no logits.
Shapes: v7 = CM3PForMaskedLM on the default beatmap tower, 32 x 4096 tokens (V = 3167); mb = FusedModernBertForMaskedLM on the default
ModernBertConfig (V = 50368), 8 x 8192 tokens.  Randomly initialised weights, evaluation mode, no_grad.

One process per invocation.  Per shape the two routes alternate - full, topk, full again; the two "full" series are the same code, their
ratio is the A/A spread the topk / full ratio has to be read against - in --rounds blocks of --iters calls after a warm-up call of each;
ms = the median over a series' blocks.  Times are HIP events around a block, ended by a synchronise.  Peak memory:
torch.cuda.max_memory_allocated over one call of each route, above what is allocated before it (parameters and inputs).  The ids of
both routes are compared before anything is timed.  One JSON line per shape; --out also writes the text DESIGN section 4.13 quotes.
"""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"v7": (32, 4096), "mb": (8, 8192)}
SERIES = ("full", "topk", "full_again")


def build(name, dev):
    torch.manual_seed(0)
    if name == "v7":
        from cm3p_amd import CM3PBeatmapConfig
        from cm3p_amd.modeling_cm3p import CM3PForMaskedLM

        cfg = CM3PBeatmapConfig()
        return CM3PForMaskedLM(cfg).to(dev).eval(), cfg.vocab_size, cfg.hidden_size
    from transformers import ModernBertConfig

    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM

    cfg = ModernBertConfig()
    return FusedModernBertForMaskedLM(cfg).to(dev).eval(), cfg.vocab_size, cfg.hidden_size


def timed(fn, iters):
    gc.collect()
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


def run_shape(name, B, S, k, iters, rounds, dev):
    model, V, H = build(name, dev)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(5, V - 5, (B, S), generator=g).to(dev)
    mask = torch.ones(B, S, dtype=torch.int64, device=dev)
    rows = torch.nonzero(torch.rand(B * S, generator=g) < 0.15).flatten().to(dev)

    @torch.no_grad()
    def full():
        logits = model(input_ids=ids, attention_mask=mask).logits.reshape(B * S, -1)
        return torch.topk(logits[rows], k, dim=1).indices

    def topk():
        return model.predict_tokens(ids, attention_mask=mask, positions=rows, k=k).token_ids

    routes = {"full": full, "topk": topk, "full_again": full}
    out, peak = {}, {}
    for key in SERIES[:2]:  # warm-up of each route, what it answers, and what it holds
        routes[key]()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out[key] = routes[key]().cpu()
        torch.cuda.synchronize()
        peak[key] = torch.cuda.max_memory_allocated() - base
    ms = {key: [] for key in SERIES}
    for _ in range(rounds):
        for key in SERIES:
            ms[key].append(timed(routes[key], iters))
    med = {key: median(v) for key, v in ms.items()}
    Vp = (V + 63) // 64 * 64
    del model
    return dict(shape=name, B=B, S=S, rows=int(rows.numel()), H=H, V=V, k=k, logits_fp32_bytes=B * S * Vp * 4, iters=iters, rounds=rounds,
                ms={key: round(v, 3) for key, v in med.items()}, ms_blocks={key: [round(x, 3) for x in v] for key, v in ms.items()},
                ratio_topk_over_full=round(med["topk"] / med["full"], 4), ratio_full_again_over_full=round(med["full_again"] / med["full"], 4),
                peak_bytes_above_operands=peak, ids_equal_share=(out["full"] == out["topk"]).float().mean().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="v7,mb")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the results as a text table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mlm_topk_time.py measures on the GPU; there is no CPU path")
    dev = torch.device("cuda", 0)
    res = []
    for name in args.shapes.split(","):
        B, S = SHAPES[name]
        res.append(run_shape(name, B, S, args.k, args.iters, args.rounds, dev))
        print(json.dumps(res[-1]), flush=True)
        gc.collect()
        torch.cuda.empty_cache()
    if args.out:
        prop = torch.cuda.get_device_properties(dev)
        with open(args.out, "w") as f:
            f.write("The k = %d most likely tokens at 15 %% of the positions: model(...).logits + torch.topk ('full') / predict_tokens ('topk') / full\n"
                    "again on one model and batch, alternating in one process: median of %d blocks of %d calls per series, ms per call\n"
                    "(tools/mlm_topk_time.py; evaluation mode, no_grad, random weights; A/A = the second 'full' series over the first; peak =\n"
                    "max_memory_allocated over one call above parameters and inputs, GiB; ids = share of the ids equal in both routes).\n"
                    "box: %s, %d CUs, HIP %s, torch %s\n\n" % (args.k, args.rounds, args.iters, prop.name, prop.multi_processor_count, torch.version.hip,
                                                             torch.__version__))
            f.write("%-5s %3s %5s %6s %5s %6s %10s %10s %10s %9s %8s %9s %9s %12s %8s\n" % ("shape", "B", "S", "rows", "H", "V", "full", "topk", "full again",
                                                                                        "topk/full", "A/A", "peak full", "peak topk", "logits fp32", "ids"))
            for r in res:
                f.write("%-5s %3d %5d %6d %5d %6d %10.3f %10.3f %10.3f %9.4f %8.4f %9.3f %9.3f %12.3f %8.5f\n" % (
                    r["shape"], r["B"], r["S"], r["rows"], r["H"], r["V"], r["ms"]["full"], r["ms"]["topk"], r["ms"]["full_again"], r["ratio_topk_over_full"],
                    r["ratio_full_again_over_full"], r["peak_bytes_above_operands"]["full"] / 2 ** 30, r["peak_bytes_above_operands"]["topk"] / 2 ** 30,
                    r["logits_fp32_bytes"] / 2 ** 30, r["ids_equal_share"]))
            f.write("\n")
            for r in res:
                f.write("%s blocks (ms per call): %s\n" % (r["shape"], json.dumps(r["ms_blocks"])))


if __name__ == "__main__":
    main()
