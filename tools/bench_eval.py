#!/usr/bin/env python3
"""Forward-only throughput of the two evaluation consumers of the hot-path kernels (development aid,
the judged number comes from bench.py):

  extract     ref:extract_beatmap_embeddings.py:217-234 - model(input_ids, attention_mask, return_loss=False) under no_grad,
              default config, B x 4096 beatmap tokens -> beatmap_embeds
  variations  evaluation with V metadata variations per row (ref:configs/train/default.yaml:147 test_metadata_variations: 1000):
              a (B, V, 256) metadata batch through the metadata tower + logits + loss
  packed-pool mean pooling of the valid rows of the variation-evaluation shape (--pool-seqs 8000 sequences, L = 256, H = 256, valid
              lengths ~ U{1..128}), forward + backward, two ways on the same rows, alternating in one process: the packed pooling
              node (_PoolPackedFn on the [total, H] rows) against re-padding them (cm3p_scatter_rows_f32) and pooling the padded
              batch (_PoolFn).  Only when named; no model is built.  The two times and the bytes each way moves go to --pool-out.

    python tools/bench_eval.py [extract] [variations] [packed-pool] [--batch 32] [--variations 1000] [--var-batch 8] [--iters 5]
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


def packed_pool(args, dev):
    """_PoolPackedFn against scatter + _PoolFn on the same valid rows: ms per forward + backward and the algorithmic bytes of each."""
    from cm3p_amd.encoder import _PadRowsFn
    from cm3p_amd.modeling_cm3p import _PoolFn, _PoolPackedFn

    Bn, L, H = args.pool_seqs, 256, 256
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(1, 129, (Bn,), generator=g)
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64).to(dev)
    idx = torch.nonzero(mask.flatten()).flatten()
    cu = torch.nn.functional.pad(torch.cumsum(lens, 0), (1, 0)).to(torch.int32).to(dev)
    total, max_s = int(lens.sum()), int(lens.max())
    rows = torch.randn(total, H, generator=g).to(dev).requires_grad_(True)
    dp = torch.randn(Bn, H, generator=g).to(dev)

    def packed():
        rows.grad = None
        _PoolPackedFn.apply(rows, cu, max_s, False).backward(dp)

    def padded():
        rows.grad = None
        _PoolFn.apply(_PadRowsFn.apply(rows, idx, total, Bn * L).view(Bn, L, H), mask, False).backward(dp)

    ms = {"packed": [], "padded": []}
    for _ in range(args.rounds):
        for name, fn in (("packed", packed), ("padded", padded)):
            ms[name].append(timed(fn, args.iters))
    ms = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    row, chunks = H * 4, -(-max_s // 128)
    small = Bn * row * 2 + Bn * 4  # pooled, dpooled, count
    nbytes = {
        # rows read once; the chunk sums written and read; every row of the gradient written once
        "packed": 2 * total * row + 2 * Bn * chunks * row + small + (Bn + 1) * 4 * 3,
        # zero fill + scatter (read, write) of the rows; the padded batch and its mask read (twice: chunk sums, count); the padded
        # gradient written, then its valid rows gathered (read, write); the row indices read twice
        "padded": Bn * L * row + 2 * total * row + Bn * L * row + 3 * Bn * L * 8 + 2 * Bn * (-(-L // 128)) * row + Bn * L * row
                  + 2 * total * row + 2 * total * 8 + small,
    }
    out = {"path": "packed-pool", "sequences": Bn, "L": L, "H": H, "valid_rows": total, "max_seqlen": max_s, "iters": args.iters,
           "rounds": args.rounds, "ms_packed": round(ms["packed"], 4), "ms_scatter_then_padded": round(ms["padded"], 4),
           "ratio_packed_over_padded": round(ms["packed"] / ms["padded"], 4), "bytes_packed": nbytes["packed"], "bytes_scatter_then_padded": nbytes["padded"],
           "GBps_packed": round(nbytes["packed"] / ms["packed"] / 1e6, 1), "GBps_scatter_then_padded": round(nbytes["padded"] / ms["padded"] / 1e6, 1)}
    print(json.dumps(out))
    if args.pool_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.pool_out)), exist_ok=True)
        with open(args.pool_out, "w") as f:
            f.write("Mean pooling of the valid rows of the variation-evaluation shape, forward + backward, fp32 rows (tools/bench_eval.py packed-pool).\n"
                    "packed: _PoolPackedFn on the [total, H] rows.  scatter_then_padded: cm3p_scatter_rows_f32 to [Bn, L, H], then _PoolFn.\n"
                    "ms: median over the rounds of the mean of `iters` calls, the two variants alternating in one process; bytes: algorithmic.\n")
            for k, v in out.items():
                f.write(f"{k:28s} {v}\n")


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
    ap.add_argument("--pool-seqs", type=int, default=8000, help="packed-pool: number of sequences")
    ap.add_argument("--pool-out", default=None, help="packed-pool: also write the result to this text file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if "packed-pool" in args.what:
        packed_pool(args, dev)
        if set(args.what) == {"packed-pool"}:
            return
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
