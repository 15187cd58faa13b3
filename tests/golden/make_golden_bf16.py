#!/usr/bin/env python3
"""Generate the bf16-inference fixture by running the REFERENCE itself the way its README runs inference: the model in bf16
(`.to(torch.bfloat16)`, ref:README.md:26-29), eval mode, `torch.no_grad()`, float inputs cast to bf16 (ref:README.md:29),
attn_implementation="sdpa", on the CPU.  In that setting ModernBERT's residual stream is bf16 - what the HIP encoder computes
with `set_residual_dtype(torch.bfloat16)`.

Needs a checkout of the reference, named by CM3P_REFERENCE (the tests only read the stored file):

    CM3P_REFERENCE=/path/to/OliBomby-CM3P python tests/golden/make_golden_bf16.py     # writes tests/golden/d64_bf16.safetensors

The weights are the d64 fixture weights (weights_d64.safetensors plus the MLM head of d64_mlm.safetensors), the inputs those
of the fp32 fixtures (cases.make_inputs), so only outputs are stored, in the reference's own dtype (bf16), keyed "<case>.<name>":
  beatmap_last_hidden_state, metadata_last_hidden_state, beatmap_embeds, metadata_embeds, logits_per_metadata,
  and for d64_mlm the MLM head's logits (the forward of a call without labels) instead of its beatmap last_hidden_state.
To keep the file under 1 MiB, the beatmap last_hidden_state of d64_mean_pad and d64_variations holds batch rows 0 and 1 only
(row 0 unpadded, row 1 padded; the key names the rows: "beatmap_last_hidden_state[:2]").
"""
from __future__ import annotations

import os
import sys

import torch
from safetensors.torch import load_file, save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import build_model  # noqa: E402  (exits unless CM3P_REFERENCE is set; imports the reference package)

from cases import make_inputs  # noqa: E402

CASE_NAMES = ["d64_mean_pad", "d64_variations", "d64_audio", "d64_mlm"]
OUT = os.path.join(HERE, "d64_bf16.safetensors")


def main():
    torch.set_num_threads(8)
    from cases import CASES

    shared = load_file(os.path.join(HERE, "weights_d64.safetensors"))
    blob = {}
    for name in CASE_NAMES:
        model = build_model(CASES[name]["cfg"])
        sd = dict(shared)
        sd.update({k[2:]: v for k, v in load_file(os.path.join(HERE, f"{name}.safetensors")).items() if k.startswith("w.")})
        model.load_state_dict(sd, strict=True)  # the weights the GPU tests load (same seed, so equal; loaded to be sure)
        model = model.to(torch.bfloat16).eval()
        inputs = make_inputs(name)
        inputs.pop("labels", None)  # forward logits only
        inputs = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in inputs.items()}
        with torch.no_grad():
            out = model(**inputs, return_loss=False)
        res = {
            "metadata_last_hidden_state": out.metadata_model_output.last_hidden_state,
            "beatmap_embeds": out.beatmap_embeds,
            "metadata_embeds": out.metadata_embeds,
            "logits_per_metadata": out.logits_per_metadata,
        }
        h = out.beatmap_model_output.last_hidden_state
        if out.logits is not None:
            res["mlm_logits"] = out.logits
        elif name in ("d64_mean_pad", "d64_variations"):
            res["beatmap_last_hidden_state[:2]"] = h[:2]
        else:
            res["beatmap_last_hidden_state"] = h
        for k, v in res.items():
            assert v.dtype == torch.bfloat16, (name, k, v.dtype)
            blob[f"{name}.{k}"] = v.detach().contiguous()
        print(f"{name:16s} " + "  ".join(f"{k}={tuple(v.shape)}/{v.dtype}" for k, v in res.items()))
    save_file(blob, OUT)
    print(f"{OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
