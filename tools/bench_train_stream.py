#!/usr/bin/env python3
"""Training-step time and peak memory of the two residual streams (development aid, the judged number comes from bench.py):

    python tools/bench_train_stream.py [c2] [c4] [--iters 3] [--rounds 5] [--kernels]

One process; per workload (bench.py's C2 / C4 shapes, default config, fp32 master weights) the fp32 stream (the default) and the bf16
stream (model.set_residual_dtype(torch.bfloat16, training=True)) are timed alternating: --rounds blocks of --iters steps per mode after
a warm-up step of each, ms per step = the median over a mode's blocks.  A step is forward + loss + backward with
zero_grad(set_to_none=True); no optimizer (both streams hand it the same fp32 gradients).  torch.cuda.max_memory_allocated is taken per
mode over one step after reset_peak_memory_stats.  --kernels adds each mode's per-call split (HIP events around every C-ABI call: the
sum is not the step time).  One JSON line per workload.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import WORKLOADS, make_batch  # noqa: E402
from cm3p_amd import CM3PConfig, CM3PModel, _lib  # noqa: E402

RESID = {"fp32": None, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["c2", "c4"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = CM3PConfig()
    torch.manual_seed(0)
    model = CM3PModel(cfg).to(dev).train()
    for name in args.what:
        w = dict(WORKLOADS[name])
        batch = make_batch(cfg, w, 0, dev)

        def step():
            model.zero_grad(set_to_none=True)
            out = model(**batch, return_loss=True)
            out.loss.backward()
            return out

        def timed(iters):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        ms = {m: [] for m in RESID}
        res = {"workload": name, "batch": w["B"], "seq": w["S"], "iters": args.iters, "rounds": args.rounds}
        for m in RESID:  # warm-up, the stream's dtype check, peak memory of one step
            model.set_residual_dtype(RESID[m], training=True)
            out = step()
            assert out.beatmap_model_output.last_hidden_state.dtype == (torch.bfloat16 if m == "bf16" else torch.float32)
            res[f"loss_{m}"] = float(out.loss)
            del out
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            res[f"max_memory_allocated_gib_{m}"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
        for _ in range(args.rounds):
            for m in RESID:
                model.set_residual_dtype(RESID[m], training=True)
                ms[m].append(timed(args.iters))
        med = {m: sorted(v)[len(v) // 2] for m, v in ms.items()}
        res["ms"] = {m: round(med[m], 3) for m in RESID}
        res["ms_blocks"] = {m: [round(x, 3) for x in ms[m]] for m in RESID}
        res["ratio_bf16_over_fp32"] = round(med["bf16"] / med["fp32"], 4)
        if args.kernels:
            for m in RESID:
                model.set_residual_dtype(RESID[m], training=True)
                _lib.profile_begin()
                step()
                prof = _lib.profile_end()
                res[f"kernels_ms_{m}"] = {k: [v[0], round(v[1], 3)] for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:14]}
        model.set_residual_dtype(None, training=True)
        model.zero_grad(set_to_none=True)
        del batch
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
