#!/usr/bin/env python3
"""Generate the wide-head fixture by running the REFERENCE itself (CPU, fp32, attn_implementation="sdpa") on cases_hd.CASE: a beatmap
tower at head_dim 128 (one global, one sliding layer) and a metadata tower at head_dim 96, a padded batch of S = 203.

Needs a checkout of the reference, named by CM3P_REFERENCE (the tests only read the stored file):

    CM3P_REFERENCE=/path/to/OliBomby-CM3P python tests/golden/make_golden_hd.py      # writes tests/golden/hd_mean_pad.safetensors

Data only: the inputs ("in.*"), loss, logits_per_metadata, both embeddings, both pooler outputs and "grad.<name><slice>" for the
parameters make_golden_bf16_train.py classifies, cut by its stored_slice (a tensor of more than 512 elements as its first rows, the
embedding tables as the rows of the first tokens).  No weights: cases_hd.draw_weights makes them on both sides.
"""
from __future__ import annotations

import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cases_hd  # noqa: E402
from make_golden import build_model  # noqa: E402  (exits unless CM3P_REFERENCE is set; imports the reference package)
from make_golden_bf16_train import class_of, stored_slice  # noqa: E402

OUT = os.path.join(HERE, f"{cases_hd.NAME}.safetensors")


def main():
    torch.set_num_threads(8)
    model = build_model(cases_hd.CASE["cfg"])
    cases_hd.draw_weights(model)
    inputs = cases_hd.inputs()
    model.zero_grad(set_to_none=True)
    out = model(**inputs)
    out.loss.backward()

    blob = {f"in.{k}": v.contiguous() for k, v in inputs.items()}
    blob["loss"] = out.loss.detach().reshape(1)
    blob["logits_per_metadata"] = out.logits_per_metadata.detach().contiguous()
    blob["metadata_embeds"] = out.metadata_embeds.detach().contiguous()
    blob["beatmap_embeds"] = out.beatmap_embeds.detach().contiguous()
    blob["beatmap_pooler_output"] = out.beatmap_model_output.pooler_output.detach().contiguous()
    blob["metadata_pooler_output"] = out.metadata_model_output.pooler_output.detach().contiguous()
    n = 0
    for name, p in sorted(model.named_parameters()):
        if p.grad is None or not class_of(name):
            continue
        suffix, cut = stored_slice(name, p, inputs)
        blob[f"grad.{name}{suffix}"] = cut(p.grad.detach()).clone().contiguous()
        n += 1
    save_file(blob, OUT)
    print(f"{cases_hd.NAME}: loss={out.loss.item():.7f}  {n} gradients  {os.path.getsize(OUT) / 1e6:.3f} MB")


if __name__ == "__main__":
    main()
