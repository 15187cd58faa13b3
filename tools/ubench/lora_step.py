"""One 12-layer, 768-wide tower at B x S = 32 x 4096, forward + backward, in three modes alternated inside ONE process:
    full      every parameter trains (the four weight-gradient GEMMs per layer run)
    lora      frozen base + adapters r = 16 on all four projections (merged cast + adapter gradients instead)
    frozen    frozen base alone, gradient flowing to the embedding output only (neither)
Prints per-mode milliseconds per step with the A/A spread (the same mode timed in every round), then from one profiled step per mode
the adapter kernels' times per layer next to the weight-gradient GEMMs they replace.  python tools/ubench/lora_step.py [--rounds 4]
[--steps 3] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

L, H, I, NH, B, S = 12, 768, 1152, 12, 32, 4096


def build(mode):
    from transformers import ModernBertConfig

    from cm3p_amd import lora
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    types = ["full_attention" if i % 3 == 0 else "sliding_attention" for i in range(L)]
    cfg = ModernBertConfig(vocab_size=3200, hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=NH,
                           max_position_embeddings=S, layer_types=types, local_attention=128, pad_token_id=0)
    torch.manual_seed(0)
    m = FusedModernBertModel(cfg).cuda().train()
    if mode == "lora":
        lora.add_lora(m, r=16, alpha=32)
        with torch.no_grad():
            for k, v in lora.lora_state_dict(m).items():
                if k.endswith("lora_B"):
                    v.normal_(std=0.02)
    elif mode == "frozen":
        for p in m.parameters():
            p.requires_grad_(False)
    return m


def step(m, ids, emb_grad):
    if emb_grad:  # frozen base alone: something must ask for a backward
        x = m.embeddings.tok_embeddings.weight[ids].detach().requires_grad_(True)
        y = m(inputs_embeds=x).last_hidden_state
    else:
        y = m(input_ids=ids).last_hidden_state
    y.float().square().mean().backward()
    for p in m.parameters():
        p.grad = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cm3p_amd import _lib

    modes = ("full", "lora", "frozen")
    models = {k: build(k) for k in modes}
    ids = torch.randint(3, 3200, (B, S), device="cuda")
    for k in modes:
        step(models[k], ids, k == "frozen")
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    for _ in range(a.rounds):
        for k in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(models[k], ids, k == "frozen")
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.steps)
    lines = [f"tower L={L} H={H} I={I} heads={NH} B={B} S={S}; {a.rounds} rounds x {a.steps} steps per mode, modes alternated in one process"]
    for k in modes:
        t = sorted(times[k])
        lines.append(f"{k:7s} median {t[len(t) // 2]:8.2f} ms/step   min {t[0]:8.2f}   max {t[-1]:8.2f}   A/A spread {(t[-1] - t[0]) / t[len(t) // 2]:.2%}")
    for k in ("full", "lora"):
        _lib.profile_begin()
        step(models[k], ids, False)
        tags = _lib.profile_end()
        lines.append(f"-- one profiled step, mode {k} (event pairs around every launch; per layer = total / {L})")
        for t, (n, ms, _) in sorted(tags.items()):
            if "<false, false," in t or "lora" in t or t == "cm3p_cast_f32_bf16_t_multi":
                lines.append(f"   {t:55s} launches {n:3d}  total {ms:8.3f} ms  per layer {ms / L:7.3f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
