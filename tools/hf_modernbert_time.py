#!/usr/bin/env python3
"""Forward + backward time of a Hugging Face ModernBERT-base on its three attention / model seams (a measurement, no bar):

    python tools/hf_modernbert_time.py [--shapes 8x4096 64x512] [--iters 3] [--rounds 5] [--precision autocast|fp32] [--layers N]

One process, one randomly initialised `ModernBertModel` of the default (base) configuration with fp32 master weights, and three arms over
the SAME parameters, timed alternating:

    sdpa      the installed model, attn_implementation="sdpa"
    cm3p_hip  the installed model, attn_implementation="cm3p_hip" (cm3p_amd/hf_attention.py: the attention function only)
    fused     cm3p_amd.hf_modernbert.fuse(model): the whole tower on the fused encoder stack

--rounds blocks of --iters steps per arm after a warm-up step of each; ms per step = the median over an arm's blocks
(tools/bench_train_stream.py's scheme).  A step is zero_grad(set_to_none=True), forward on full-length sequences (no padding mask),
`(last_hidden_state * w).sum()`, backward; no optimizer.  --precision autocast (default) runs the two torch arms under
torch.autocast(bfloat16), the recipe whose GEMM operands the fused stack reproduces (bf16 operands, fp32 masters and residual stream);
fp32 runs them as they are.  The fused arm's per-call split (HIP events around every C-ABI call of one more step: the sum is not the step
time) is added per shape.  One JSON line per shape.
"""
import argparse
import contextlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cm3p_amd.hf_attention as hf_attention  # noqa: E402,F401  (registers "cm3p_hip")
from cm3p_amd import _lib  # noqa: E402
from cm3p_amd.hf_modernbert import fuse  # noqa: E402

ARMS = ("sdpa", "cm3p_hip", "fused")


def main():
    from transformers import ModernBertConfig, ModernBertModel

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["8x4096", "64x512"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", choices=("autocast", "fp32"), default="autocast")
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the base configuration's 22 (a quick look)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = ModernBertConfig() if args.layers is None else ModernBertConfig(num_hidden_layers=args.layers)
    torch.manual_seed(0)
    torch_model = ModernBertModel._from_config(cfg, attn_implementation="sdpa").to(dev).train()
    fused_model = fuse(torch_model)  # the same nn.Parameter objects
    assert all(any(p is q for q in torch_model.parameters()) for p in fused_model.parameters())

    def autocast():
        return torch.autocast("cuda", dtype=torch.bfloat16) if args.precision == "autocast" else contextlib.nullcontext()

    for shape in args.shapes:
        B, S = (int(v) for v in shape.lower().split("x"))
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(0, 50000, (B, S), generator=g).to(dev)
        w = torch.randn(B, S, cfg.hidden_size, generator=g).to(dev)

        def step(arm):
            torch_model.zero_grad(set_to_none=True)
            if arm == "fused":
                y = fused_model(input_ids=ids).last_hidden_state
            else:
                torch_model.config._attn_implementation = arm
                with autocast():
                    y = torch_model(input_ids=ids).last_hidden_state
            loss = (y.float() * w).sum()
            loss.backward()
            return loss

        def timed(arm, iters):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(arm)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        res = {"model": "ModernBERT-base (random init)", "layers": cfg.num_hidden_layers, "batch": B, "seq": S, "precision": args.precision,
               "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        ms = {a: [] for a in ARMS}
        for a in ARMS:  # warm-up; the loss of each arm on the same weights and inputs, for the record
            res[f"loss_{a}"] = float(step(a).detach())
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step(a)
            torch.cuda.synchronize()
            res[f"max_memory_allocated_gib_{a}"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
        for _ in range(args.rounds):
            for a in ARMS:
                ms[a].append(timed(a, args.iters))
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        res["ms"] = {a: round(med[a], 3) for a in ARMS}
        res["ms_blocks"] = {a: [round(x, 3) for x in ms[a]] for a in ARMS}
        res["fastest"] = min(ARMS, key=lambda a: med[a])
        res["fused_over_sdpa"] = round(med["fused"] / med["sdpa"], 4)
        res["fused_over_cm3p_hip"] = round(med["fused"] / med["cm3p_hip"], 4)
        _lib.profile_begin()
        step("fused")
        prof = _lib.profile_end()
        res["fused_kernels_ms"] = {k: [v[0], round(v[1], 3)] for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:16]}
        res["fused_kernels_ms_total"] = round(sum(v[1] for v in prof.values()), 3)
        torch_model.config._attn_implementation = "sdpa"
        torch_model.zero_grad(set_to_none=True)
        del ids, w
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
