#!/usr/bin/env python3
"""Generate the bf16-training fixture by running the REFERENCE itself: one loss + backward per case, twice - the fp32 model (the
yardstick: the existing fp32 fixtures hold the gradients of a fixed subset of parameters only) and the same model after
`model.to(torch.bfloat16).train()` (float inputs cast to bf16), dropout 0 (the d64 configurations), attn_implementation="sdpa", on the
CPU.  An all-bf16 ModernBERT keeps its residual stream and its residual gradient in bf16 - what the HIP encoder computes with
`set_residual_dtype(torch.bfloat16, training=True)`, except that this project keeps fp32 master weights and fp32 statistics and rounds
the LayerNorm backward's sum once where torch rounds twice.

Needs a checkout of the reference, named by CM3P_REFERENCE (the tests only read the stored file):

    CM3P_REFERENCE=/path/to/OliBomby-CM3P python tests/golden/make_golden_bf16_train.py   # writes tests/golden/d64_bf16_train.safetensors

Data only, keyed "<case>.<what>": loss_f32, loss_bf16 ([1] fp32 / bf16) and, for every parameter of PARAMS(case),
"grad_f32.<name><slice>" (fp32) and "grad_bf16.<name><slice>" (bf16, the reference's own dtype).  PARAMS: the embedding table, every
norm weight, Wqkv, Wo, Wi and the MLP Wo of EVERY layer of every tower (the d64 towers are small: first, middle and last, global and
local layers are all in), both projections and the logit scale, the MLM head and decoder, the audio convolutions and the projector.  A tensor of more
than 512 elements is stored as its first rows (at least 256 elements; the key names the slice: "[:4]"), the embedding tables as the
rows of the first tokens of the case's input (named "[ids]": a leading slice would hold mostly rows without a gradient), so that the
file stays under 1 MiB.

CLASSES groups the parameters; tests/test_bf16_train_gpu.py compares per class and case, tensors of a class concatenated:
e_ref = relL2(reference bf16 gradient, reference fp32 gradient) - printed by this script, the table below - against
e_hip = relL2(this project's gradient on the bf16 training stream, reference fp32 gradient).

e_ref as printed by this script (CPU, torch 2.x, sdpa):

    d64_mean_pad    loss 1.490479 / bf16 1.492188  rel 1.15e-03
        embedding    e_ref 1.807e-02   (2 tensors)
        norm         e_ref 2.196e-02   (14 tensors)
        Wqkv         e_ref 2.181e-02   (6 tensors)
        attn_Wo      e_ref 2.071e-02   (6 tensors)
        Wi           e_ref 2.433e-02   (6 tensors)
        mlp_Wo       e_ref 2.087e-02   (6 tensors)
        projection   e_ref 1.287e-02   (2 tensors)
        logit_scale  e_ref 9.214e-03   (1 tensors)
    d64_variations  loss 2.550601 / bf16 2.546875  rel 1.46e-03
        embedding    e_ref 1.677e-02   (2 tensors)
        norm         e_ref 2.239e-02   (14 tensors)
        Wqkv         e_ref 2.947e-02   (6 tensors)
        attn_Wo      e_ref 1.474e-02   (6 tensors)
        Wi           e_ref 2.165e-02   (6 tensors)
        mlp_Wo       e_ref 2.829e-02   (6 tensors)
        projection   e_ref 1.635e-02   (2 tensors)
        logit_scale  e_ref 7.131e-03   (1 tensors)
    d64_audio       loss 2.450577 / bf16 2.437500  rel 5.34e-03
        embedding    e_ref 2.216e-02   (2 tensors)
        audio_conv   e_ref 3.550e-02   (4 tensors)
        projector    e_ref 2.295e-02   (2 tensors)
        norm         e_ref 2.480e-02   (19 tensors)
        Wqkv         e_ref 2.908e-02   (8 tensors)
        attn_Wo      e_ref 2.136e-02   (8 tensors)
        Wi           e_ref 1.775e-02   (8 tensors)
        mlp_Wo       e_ref 1.612e-02   (8 tensors)
        projection   e_ref 2.254e-02   (2 tensors)
        logit_scale  e_ref 3.272e-03   (1 tensors)
    d64_mlm         loss 6.965461 / bf16 6.937500  rel 4.01e-03
        embedding    e_ref 2.042e-02   (2 tensors)
        mlm_head     e_ref 1.339e-02   (4 tensors)
        norm         e_ref 1.939e-02   (14 tensors)
        Wqkv         e_ref 2.191e-02   (6 tensors)
        attn_Wo      e_ref 2.008e-02   (6 tensors)
        Wi           e_ref 1.474e-02   (6 tensors)
        mlp_Wo       e_ref 1.925e-02   (6 tensors)
        projection   e_ref 1.640e-02   (2 tensors)
        logit_scale  e_ref 6.984e-03   (1 tensors)
"""
from __future__ import annotations

import os
import re
import sys

import torch
from safetensors.torch import load_file, save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CASE_NAMES = ["d64_mean_pad", "d64_variations", "d64_audio", "d64_mlm"]
OUT = os.path.join(HERE, "d64_bf16_train.safetensors")

# class -> pattern of the parameter names in it (first match wins, in this order)
CLASSES = [
    ("embedding", r"tok_embeddings\.weight$"),
    ("audio_conv", r"audio_encoder\.conv[12]\.(weight|bias)$"),
    ("projector", r"multi_modal_projector\.linear_[12]\.weight$"),
    ("mlm_head", r"^(head\.dense\.(weight|bias)|head\.norm\.weight|decoder\.(weight|bias))$"),
    ("norm", r"norm\.weight$"),
    ("Wqkv", r"attn\.Wqkv\.weight$"),
    ("attn_Wo", r"attn\.Wo\.weight$"),
    ("Wi", r"mlp\.Wi\.weight$"),
    ("mlp_Wo", r"mlp\.Wo\.weight$"),
    ("projection", r"^(beatmap_projection|metadata_projection)\.weight$"),
    ("logit_scale", r"^logit_scale$"),
]


def class_of(name: str):
    for cls, pat in CLASSES:
        if re.search(pat, name):
            return cls
    return None


def table_rows(name: str, inputs: dict) -> torch.Tensor:
    """The embedding-table rows a case stores: the ids of the first 16 tokens of its first input row (sorted, unique)."""
    ids = inputs["metadata_ids" if name.startswith("metadata_model.") else "input_ids"]
    return torch.unique(ids.reshape(-1, ids.shape[-1])[0, :16])


def stored_slice(name: str, p: torch.Tensor, inputs: dict):
    """-> (key suffix, function that cuts the stored part out of a gradient of p's shape)."""
    if name.endswith("tok_embeddings.weight"):
        rows = table_rows(name, inputs)
        return "[ids]", lambda g: g[rows]
    if p.numel() <= 512 or p.dim() < 2:
        return "", lambda g: g
    r = max(1, -(-256 // p[0].numel()))
    return f"[:{r}]", lambda g: g[:r]


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def main():
    from make_golden import build_model  # (exits unless CM3P_REFERENCE is set; imports the reference package)

    from cases import CASES, make_inputs

    torch.set_num_threads(8)
    shared = load_file(os.path.join(HERE, "weights_d64.safetensors"))
    blob, table = {}, []
    for name in CASE_NAMES:
        inputs = make_inputs(name)
        runs = {}
        for tag, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            model = build_model(CASES[name]["cfg"])
            sd = dict(shared)
            sd.update({k[2:]: v for k, v in load_file(os.path.join(HERE, f"{name}.safetensors")).items() if k.startswith("w.")})
            model.load_state_dict(sd, strict=True)
            for sub in (model.config.metadata_config, model.config.beatmap_config, model.config.beatmap_config.audio_config):
                for p in ("embedding_dropout", "attention_dropout", "mlp_dropout", "classifier_dropout"):
                    assert not getattr(sub, p, 0.0), (name, p)  # dropout 0: one deterministic step
            model = model.to(dtype).train()
            inp = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inputs.items()}
            model.zero_grad(set_to_none=True)
            out = model(**inp)
            out.loss.backward()
            runs[tag] = (out.loss.detach(), {n: p.grad.detach() for n, p in model.named_parameters() if p.grad is not None and class_of(n)})
        (l32, g32), (l16, g16) = runs["f32"], runs["bf16"]
        assert g32.keys() == g16.keys() and l16.dtype == torch.bfloat16
        blob[f"{name}.loss_f32"] = l32.reshape(1).float().contiguous()
        blob[f"{name}.loss_bf16"] = l16.reshape(1).contiguous()
        per_class = {}
        for n in sorted(g32):
            suffix, cut = stored_slice(n, g32[n], inputs)
            a, b = cut(g32[n]).contiguous(), cut(g16[n]).contiguous()
            assert b.dtype == torch.bfloat16 and a.dtype == torch.float32
            blob[f"{name}.grad_f32.{n}{suffix}"] = a
            blob[f"{name}.grad_bf16.{n}{suffix}"] = b
            per_class.setdefault(class_of(n), []).append((a, b))
        line = f"{name:15s} loss {l32.item():.6f} / bf16 {l16.float().item():.6f}  rel {abs(l16.float().item() - l32.item()) / abs(l32.item()):.2e}"
        print(line)
        table.append(line)
        for cls, _ in CLASSES:
            if cls in per_class:
                e = rel_l2(torch.cat([b.float().reshape(-1) for _, b in per_class[cls]]), torch.cat([a.reshape(-1) for a, _ in per_class[cls]]))
                line = f"    {cls:12s} e_ref {e:.3e}   ({len(per_class[cls])} tensors)"
                print(line)
                table.append(line)
    save_file(blob, OUT)
    print(f"{OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB, {len(blob)} tensors")


if __name__ == "__main__":
    main()
