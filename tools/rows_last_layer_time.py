#!/usr/bin/env python3
"""What `labelled_rows_last_layer` is worth on a training step of the published recipe's shape (development aid; bench.py's workload
pools by mean and does not move):

    python tools/rows_last_layer_time.py [--iters 3] [--rounds 5] [--batch 32] [--seq 4096] [--out profiles/rows_last_layer.txt]

The step: default tower sizes with cls_embed on both towers and the decoder head (loss_type ForMaskedLM), B x S = 32 x 4096, metadata
32 x 256, labels on 15 % of the positions, fp32 stream; forward + loss + backward, zero_grad(set_to_none=True), no optimizer.

One process.  The switch is off, on and off again in every round - the two "off" series are the same code, their ratio is the A/A spread
the on / off ratio has to be read against - in --rounds alternating blocks of --iters steps after a warm-up step of each; ms = the
median over a series' blocks (the scheme of tools/cls_last_layer_time.py).  Times are HIP events around a block, ended by a
synchronise.  The loss of both settings is compared on the same inputs before anything is timed.  Then one step of each setting runs
under per-launch events (cm3p_amd._lib.profile_begin): the kernels whose time differs between the two are the last layer's and the
head's - the per-kernel split --out writes below the table (per-launch events add ~2.5 us each: read the split as shares, the
table as the time).  One JSON line; --out also writes the text DESIGN section 4.11 quotes.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--label-prob", type=float, default=0.15)
    ap.add_argument("--out", default=None, help="also write the results as a text table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rows_last_layer_time.py measures on the GPU; there is no CPU path")
    dev = torch.device("cuda", 0)
    cfg = CM3PConfig(beatmap_config=dict(cls_embed=True), metadata_config=dict(cls_embed=True), has_decoder_head=True, loss_type="ForMaskedLM")
    S, L = args.seq, 256
    torch.manual_seed(0)
    model = CM3PModel(cfg).to(dev).train()
    b = synthetic_batch(cfg, args.batch, S, L, seed=1234)
    g = torch.Generator().manual_seed(5)
    pick = torch.rand(args.batch, S, generator=g) < args.label_prob
    if "attention_mask" in b:
        pick &= b["attention_mask"].bool()
    b["labels"] = torch.where(pick, b["input_ids"], torch.full_like(b["input_ids"], -100))
    b = {k: v.to(dev) for k, v in b.items()}
    n_rows = int((pick | (torch.arange(S)[None] == 0)).sum())

    def step():
        model.zero_grad(set_to_none=True)
        out = model(**b, return_loss=True)
        out.loss.backward()
        return out

    vals = {}
    for key, on in SERIES[:2]:  # warm-up of each setting, and what it computes
        model.labelled_rows_last_layer = on
        vals[key] = step().loss.detach().float().cpu()
    diff = (vals["on"] - vals["off"]).abs().item()
    ms = {key: [] for key, _ in SERIES}
    for _ in range(args.rounds):
        for key, on in SERIES:
            model.labelled_rows_last_layer = on
            ms[key].append(timed(step, args.iters))
    med = {k: median(v) for k, v in ms.items()}
    prof = {}
    for key, on in SERIES[:2]:
        model.labelled_rows_last_layer = on
        _lib.profile_begin()
        step()
        prof[key] = {k: (v[0], v[1]) for k, v in _lib.profile_end().items()}
    model.labelled_rows_last_layer = False
    split = []
    for tag in sorted(set(prof["off"]) | set(prof["on"])):
        (n0, t0), (n1, t1) = prof["off"].get(tag, (0, 0.0)), prof["on"].get(tag, (0, 0.0))
        if abs(t1 - t0) >= 0.05 or tag.startswith("attn_qrows"):
            split.append((tag, n0, round(t0, 3), n1, round(t1, 3)))
    res = dict(run="train: contrastive + MLM step, cls_embed towers, decoder head, fp32 stream", batch=args.batch, seq=S, metadata_seq=L,
               label_prob=args.label_prob, rows_selected=n_rows, rows_total=args.batch * S, iters=args.iters, rounds=args.rounds,
               ms={k: round(v, 3) for k, v in med.items()}, ms_blocks={k: [round(x, 3) for x in v] for k, v in ms.items()},
               ratio_on_over_off=round(med["on"] / med["off"], 4), ratio_off_again_over_off=round(med["off_again"] / med["off"], 4),
               loss_abs_diff_on_vs_off=diff, kernels_that_differ=split)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("labelled_rows_last_layer off / on / off again, alternating in one process: median of %d blocks of %d steps per series, ms per step\n"
                    "(tools/rows_last_layer_time.py; default tower sizes, cls_embed on both towers, decoder head, B x S = %d x %d, %d of %d rows selected;\n"
                    "A/A = the second 'off' series over the first).\n\n" % (args.rounds, args.iters, args.batch, S, n_rows, args.batch * S))
            f.write("%10s %10s %10s %9s %9s %14s\n" % ("off", "on", "off again", "on/off", "A/A", "|loss on-off|"))
            f.write("%10.3f %10.3f %10.3f %9.4f %9.4f %14.2e\n" % (med["off"], med["on"], med["off_again"], res["ratio_on_over_off"],
                                                                 res["ratio_off_again_over_off"], diff))
            f.write("\nblocks (ms per step): %s\n" % json.dumps(res["ms_blocks"]))
            f.write("\nkernels whose time differs between one 'off' and one 'on' step, under per-launch events (launches, ms):\n")
            f.write("%-72s %6s %10s %6s %10s\n" % ("kernel", "off n", "off ms", "on n", "on ms"))
            for tag, n0, t0, n1, t1 in split:
                f.write("%-72s %6d %10.3f %6d %10.3f\n" % (tag[:72], n0, t0, n1, t1))
            f.write("%-72s %6s %10.3f %6s %10.3f\n" % ("sum of the rows above", "", sum(s[2] for s in split), "", sum(s[4] for s in split)))


if __name__ == "__main__":
    main()
