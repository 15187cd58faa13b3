#!/usr/bin/env python3
"""What `cls_only_last_layer` is worth on the calls the CLS recipes make (development aid; bench.py's workloads pool by mean and do not move):

    python tools/cls_last_layer_time.py [train] [extract] [variations] [--iters 3] [--rounds 5] [--out profiles/cls_last_layer.txt]

  train       a contrastive-only training step (forward + loss + backward, zero_grad(set_to_none=True), no optimizer) at the default
              tower sizes with cls_embed on both towers, B x S = 32 x 4096, metadata 32 x 256, fp32 stream
  extract     beatmap extraction under no_grad on the bf16 residual stream, 32 x 4096
  variations  the 1000-variation evaluation step of tools/bench_eval.py: 8 beatmaps, 8 x 1000 metadata rows of 256 tokens, no_grad, fp32

One process per invocation.  Per run the switch is off, on and off again in every round - the two "off" series are the same code, their
ratio is the A/A spread the on / off ratio has to be read against - in --rounds alternating blocks of --iters steps after a warm-up
step of each; ms = the median over a series' blocks (the scheme of tools/bench_train_stream.py).  Times are HIP events around a block,
ended by a synchronise.  The loss / embeddings of both settings are compared on the same inputs before anything is timed.  One JSON
line per run; --out also writes the table DESIGN section 4.10 quotes.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cm3p_amd import CM3PConfig, CM3PModel, _lib  # noqa: E402
from cm3p_amd.synthetic import synthetic_batch  # noqa: E402

SERIES = (("off", False), ("on", True), ("off_again", False))


def timed(fn, iters):
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


def measure(name, model, fn, value_of, args, extra):
    """fn() runs one step with the model's current switch; value_of(result) -> a tensor both settings must agree on."""
    vals = {}
    for key, on in SERIES[:2]:  # warm-up of each setting, and what it computes
        model.cls_only_last_layer = on
        vals[key] = value_of(fn()).detach().float().cpu()
    diff = ((vals["on"] - vals["off"]).norm() / vals["off"].norm().clamp_min(1e-30)).item()
    ms = {key: [] for key, _ in SERIES}
    for _ in range(args.rounds):
        for key, on in SERIES:
            model.cls_only_last_layer = on
            ms[key].append(timed(fn, args.iters))
    med = {k: median(v) for k, v in ms.items()}
    model.cls_only_last_layer = True
    _lib.profile_begin()
    fn()
    prof = _lib.profile_end()
    model.cls_only_last_layer = False
    row = {k: [v[0], round(v[1], 3)] for k, v in prof.items() if k.startswith("attn_row")}
    res = dict(run=name, **extra, iters=args.iters, rounds=args.rounds, ms={k: round(v, 3) for k, v in med.items()},
               ms_blocks={k: [round(x, 3) for x in v] for k, v in ms.items()}, ratio_on_over_off=round(med["on"] / med["off"], 4),
               ratio_off_again_over_off=round(med["off_again"] / med["off"], 4), rel_l2_on_vs_off=diff, row_kernels_launches_ms=row)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["train", "extract", "variations"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--variations", type=int, default=1000)
    ap.add_argument("--var-batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the results as a text table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cls_last_layer_time.py measures on the GPU; there is no CPU path")
    dev = torch.device("cuda", 0)
    cfg = CM3PConfig(beatmap_config=dict(cls_embed=True), metadata_config=dict(cls_embed=True))
    S, L = args.seq, 256
    torch.manual_seed(0)
    model = CM3PModel(cfg).to(dev)
    results = []
    if "train" in args.what:
        model.train()
        b = {k: v.to(dev) for k, v in synthetic_batch(cfg, args.batch, S, L, seed=1234).items()}

        def step():
            model.zero_grad(set_to_none=True)
            out = model(**b, return_loss=True)
            out.loss.backward()
            return out

        results.append(measure("train: contrastive step, cls_embed towers, fp32 stream", model, step, lambda o: o.loss, args,
                               dict(batch=args.batch, seq=S, metadata_seq=L)))
        model.zero_grad(set_to_none=True)
        del b
        torch.cuda.empty_cache()
    model.eval()
    if "extract" in args.what:
        b = {k: v.to(dev) for k, v in synthetic_batch(cfg, args.batch, S, L, seed=1234).items()}
        model.set_residual_dtype(torch.bfloat16)

        def extract():
            with torch.no_grad():
                return model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], return_loss=False).beatmap_embeds

        results.append(measure("extract: beatmap embeddings, no_grad, bf16 stream", model, extract, lambda e: e, args, dict(batch=args.batch, seq=S)))
        model.set_residual_dtype(None)
        del b
        torch.cuda.empty_cache()
    if "variations" in args.what:
        B, V = args.var_batch, args.variations
        b = {k: v.to(dev) for k, v in synthetic_batch(cfg, B, S, L, seed=99).items()}
        g = torch.Generator().manual_seed(7)
        mids = torch.randint(3, cfg.metadata_config.vocab_size - 3, (B, V, L), generator=g).to(dev)
        mmask = torch.ones(B, V, L, dtype=torch.int64, device=dev)
        classes = torch.randint(1, 4, (B, V), generator=g)
        classes[:, 0] = 0  # one original per row
        classes = classes.to(dev)

        def evaluate():
            with torch.no_grad():
                return model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], metadata_ids=mids, metadata_attention_mask=mmask,
                             metadata_variation_classes=classes, return_loss=True)

        results.append(measure(f"variations: {V}-variation evaluation step, no_grad, fp32 stream", model, evaluate, lambda o: o.logits_per_metadata, args,
                               dict(batch=B, seq=S, variations=V, metadata_seq=L)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("cls_only_last_layer off / on / off again, alternating in one process: median of %d blocks of %d steps per series, ms per step\n"
                    "(tools/cls_last_layer_time.py; default tower sizes with cls_embed on both towers; A/A = the second 'off' series over the first).\n\n"
                    % (args.rounds, args.iters))
            f.write("%-62s %10s %10s %10s %9s %9s %12s\n" % ("run", "off", "on", "off again", "on/off", "A/A", "on vs off"))
            for r in results:
                f.write("%-62s %10.3f %10.3f %10.3f %9.4f %9.4f %12.2e\n" % (r["run"], r["ms"]["off"], r["ms"]["on"], r["ms"]["off_again"],
                                                                            r["ratio_on_over_off"], r["ratio_off_again_over_off"], r["rel_l2_on_vs_off"]))
            f.write("\nblocks (ms per step) and the row kernels of one 'on' step (launches, ms under per-launch events):\n")
            for r in results:
                f.write("%s\n  %s\n  %s\n" % (r["run"], json.dumps(r["ms_blocks"]), json.dumps(r["row_kernels_launches_ms"])))


if __name__ == "__main__":
    main()
