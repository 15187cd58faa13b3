#!/usr/bin/env python3
"""Forward-only throughput of the two evaluation consumers of the hot-path kernels (development aid,
the judged number comes from bench.py):

  extract     ref:extract_beatmap_embeddings.py:217-234 - model(input_ids, attention_mask, return_loss=False) under no_grad,
              default config, B x 4096 beatmap tokens -> beatmap_embeds
  variations  evaluation with V metadata variations per row (ref:configs/train/default.yaml:147 test_metadata_variations: 1000):
              a (B, V, 256) metadata batch through the metadata tower + logits + loss

    python tools/bench_eval.py [extract] [variations] [--batch 32] [--variations 1000] [--var-batch 8] [--iters 5]
                               [--residual {fp32,bf16,both}]

--residual: the residual stream of the encoders (model.set_residual_dtype): fp32 (the default), bf16, or both - the two modes timed in
the same process, alternating (--rounds pairs of --iters calls each), with ms per call of each mode and the bf16 / fp32 ratio.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import tower_flops_fwd  # noqa: E402
from cm3p_amd import CM3PConfig, CM3PModel, _lib  # noqa: E402
from cm3p_amd.synthetic import synthetic_batch  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed_modes(model, fn, modes, iters, rounds):
    """-> {mode: ms per call}: with two modes, `rounds` alternating blocks of `iters` calls each (median over the blocks)."""
    ms = {m: [] for m in modes}
    for _ in range(rounds if len(modes) > 1 else 1):
        for m in modes:
            model.set_residual_dtype(RESID[m])
            ms[m].append(timed(fn, iters))
    model.set_residual_dtype(None)
    return {m: sorted(v)[len(v) // 2] for m, v in ms.items()}


def mode_fields(model, fn, modes, ms, top):
    """ms per mode, the bf16 / fp32 ratio, and each mode's per-kernel split."""
    out = {"residual": "+".join(modes), "ms": ms[modes[0]] if len(modes) == 1 else {m: round(ms[m], 3) for m in modes}}
    if len(modes) > 1:
        out["ratio_bf16_over_fp32"] = round(ms["bf16"] / ms["fp32"], 4)
    for m in modes:
        model.set_residual_dtype(RESID[m])
        out["kernels_ms" if len(modes) == 1 else f"kernels_ms_{m}"] = breakdown(fn, top)
    model.set_residual_dtype(None)
    return out


RESID = {"fp32": None, "bf16": torch.bfloat16}


def breakdown(fn, top=8):
    _lib.profile_begin()
    fn()
    prof = _lib.profile_end()
    return {k: round(v[1], 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["extract", "variations"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--variations", type=int, default=1000)
    ap.add_argument("--var-batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--residual", choices=["fp32", "bf16", "both"], default="fp32")
    ap.add_argument("--rounds", type=int, default=5, help="--residual both: alternating blocks per mode")
    ap.add_argument("--meta-valid", type=float, default=1.0,
                    help="variations: valid length of a metadata row ~ U{1..meta_valid * L} (right-padded); below 1 the run is repeated with "
                         "unpadded execution (model.unpad_inputs = True)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = CM3PConfig(beatmap_config=dict(cls_embed=False), metadata_config=dict(cls_embed=False))
    torch.manual_seed(0)
    model = CM3PModel(cfg).to(dev).eval()
    S, L = 4096, 256
    modes = ["fp32", "bf16"] if args.residual == "both" else [args.residual]
    if "extract" in args.what:
        b = {k: v.to(dev) for k, v in synthetic_batch(cfg, args.batch, S, L, seed=1234).items()}

        def run():
            with torch.no_grad():
                return model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], return_loss=False).beatmap_embeds

        mss = timed_modes(model, run, modes, args.iters, args.rounds)
        ms = mss[modes[-1]]
        fl = tower_flops_fwd(cfg.beatmap_config, args.batch * S, S)
        print(json.dumps({"path": "extract", "batch": args.batch, "seq": S, "beatmaps_per_s": args.batch / ms * 1e3,
                          "tokens_per_s": args.batch * S / ms * 1e3, "tflops": fl / ms / 1e9, **mode_fields(model, run, modes, mss, 8)}))
    if "variations" in args.what:
        B, V = args.var_batch, args.variations
        b = {k: v.to(dev) for k, v in synthetic_batch(cfg, B, S, L, seed=99).items()}
        g = torch.Generator().manual_seed(7)
        mids = torch.randint(3, cfg.metadata_config.vocab_size - 3, (B, V, L), generator=g).to(dev)
        mmask = torch.ones(B, V, L, dtype=torch.int64, device=dev)
        classes = torch.randint(1, 4, (B, V), generator=g)
        classes[:, 0] = 0  # one original per row
        classes = classes.to(dev)
        with torch.no_grad():
            bm = model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], return_loss=False).beatmap_embeds

        def run():
            with torch.no_grad():  # the metadata side of the evaluation step (the beatmap side is the `extract` path above)
                return model.get_metadata_features(metadata_ids=mids.view(B * V, L), metadata_attention_mask=mmask.view(B * V, L)) \
                    if hasattr(model, "get_metadata_features") else None

        def run_full():
            with torch.no_grad():
                return model(input_ids=b["input_ids"], attention_mask=b["attention_mask"], metadata_ids=mids, metadata_attention_mask=mmask,
                             metadata_variation_classes=classes, return_loss=True).loss

        if args.meta_valid < 1.0:
            lens = torch.randint(1, max(2, int(args.meta_valid * L)) + 1, (B, V), generator=g).to(dev)
            mmask = (torch.arange(L, device=dev)[None, None, :] < lens[..., None]).to(torch.int64)
            ms_pad = timed(run_full, args.iters)
            model.unpad_inputs = True
            ms_unp = timed(run_full, args.iters)
            model.unpad_inputs = None
            print(json.dumps({"path": "variations, right-padded metadata", "valid_fraction": float(mmask.float().mean()), "ms_padded_execution": ms_pad,
                              "ms_unpadded_execution": ms_unp}))
            mmask = torch.ones(B, V, L, dtype=torch.int64, device=dev)
        mss = timed_modes(model, run_full, modes, args.iters, args.rounds)
        ms = mss[modes[-1]]
        fl_m = tower_flops_fwd(cfg.metadata_config, B * V * L, L)
        fl_b = tower_flops_fwd(cfg.beatmap_config, B * S, S)
        print(json.dumps({"path": "variations", "batch": B, "variations": V, "metadata_seq": L,
                          "metadata_sequences_per_s": B * V / ms * 1e3, "metadata_tokens_per_s": B * V * L / ms * 1e3,
                          "tflops": (fl_m + fl_b) / ms / 1e9, "metadata_tower_tflop": fl_m / 1e12, **mode_fields(model, run_full, modes, mss, 10)}))
        del bm


if __name__ == "__main__":
    main()
