"""Low-rank adapters (LoRA) on the fused encoder stack.

The nn.Linear members of an encoder layer are parameter containers whose torch forward never runs, so a wrapper that hooks
`Linear.forward` adds parameters that never reach the output.  `add_lora` registers `lora_A` [r, in] and `lora_B` [out, r] on the
container itself; `CM3PEncoder` hands them to its layer nodes, which

  * fold them into the bf16 copy every call makes of the weight anyway: W_eff = bf16(W + s B A), s = alpha / r, the sum formed in fp32
    and rounded once (K.lora_merge_cast_many), so every GEMM - Wqkv with RoPE, Wi with GeGLU, the residual epilogues, the input-gradient
    GEMMs, a checkpointed recompute - runs unchanged on the merged copies, and
  * compute dA = s (dY B)^T X and dB = s dY^T (X A^T) from the operands the projection's weight-gradient GEMM reads (K.lora_grad).  A
    frozen base weight's own weight-gradient GEMM is not launched.

DESIGN section 4.9 has the numerics (what one rounding of the sum means while s B A is small), INTEGRATION the calls.  No lora_dropout:
the merged form has no place for it.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import torch
from torch import nn

from .encoder import CM3PEncoder
from .kernels import LORA_RANKS

TARGETS = ("attn.Wqkv", "attn.Wo", "mlp.Wi", "mlp.Wo")
_KEYS = ("lora_A", "lora_B")


def find_encoders(model: nn.Module) -> list:
    """Every CM3PEncoder inside `model`: registered children (the CM3P* towers) and the ones a module exposes as an `encoder` property
    without registering it (FusedModernBertModel keeps the encoder's members under ModernBertModel's names), also inside fuse()'d models.
    The stack inside a CM3PAudioEncoder is left out."""
    # (the audio encoder's stack is out of scope: its inputs are mel frames and its fine-tuning recipes differ)
    seen, out = {id(m.encoder) for m in model.modules() if type(m).__name__ == "CM3PAudioEncoder"}, []
    for m in model.modules():
        for cand in (m, m.encoder if isinstance(getattr(type(m), "encoder", None), property) else None):
            if isinstance(cand, CM3PEncoder) and id(cand) not in seen:
                seen.add(id(cand))
                out.append(cand)
    return out


def _adapted(enc: CM3PEncoder):
    for i, layer in enumerate(enc.layers):
        for t in TARGETS:
            lin = layer.get_submodule(t)
            if getattr(lin, "lora_A", None) is not None:
                yield i, t, lin


def add_lora(model: nn.Module, r: int = 16, alpha: float = 32, targets: Iterable[str] = TARGETS, layers: Optional[Iterable[int]] = None,
             freeze_base: bool = True) -> nn.Module:
    """Attach adapters to the projections named in `targets` (of "attn.Wqkv", "attn.Wo", "mlp.Wi", "mlp.Wo") of the encoder layers in
    `layers` (indices; None: all) of every encoder stack in `model`.  lora_A is kaiming_uniform_(a = sqrt 5), lora_B zeros, so the
    model's outputs are unchanged in bits until a step is taken; both are fp32 parameters of the container nn.Linear (they appear in
    parameters(), state_dict() and DDP).  freeze_base: requires_grad = False on the encoders' own parameters (embeddings, norms and
    projection weights of the stacks; heads, pooling and the audio encoder are left as they are); merge_lora / remove_lora restore the
    flags.  Everything is checked before anything is registered.  Returns the model."""
    targets = tuple(targets)
    if r not in LORA_RANKS:
        raise ValueError(f"add_lora: r must be one of {LORA_RANKS} (the adapter kernels' sizes), got {r!r}")
    if not alpha == alpha or math.isinf(float(alpha)):
        raise ValueError(f"add_lora: alpha must be finite, got {alpha!r}")
    bad = [t for t in targets if t not in TARGETS]
    if bad or not targets:
        raise ValueError(f"add_lora: targets must be a non-empty selection of {TARGETS}, got {targets!r}")
    encoders = find_encoders(model)
    if not encoders:
        raise ValueError("add_lora: no CM3PEncoder stack inside this model")
    want = None if layers is None else sorted({int(i) for i in layers})
    plan = []
    for enc in encoders:
        n = len(enc.layers)
        if want is not None and any(i < 0 or i >= n for i in want):
            raise ValueError(f"add_lora: layers {want} outside a stack of {n} layers")
        if enc.train_residual_dtype is torch.bfloat16:
            raise NotImplementedError("add_lora: the bf16 residual stream of training steps (train_residual_dtype = torch.bfloat16) is not supported "
                                      "with adapters; set it back to None first")
        for i in (range(n) if want is None else want):
            for t in targets:
                lin = enc.layers[i].get_submodule(t)
                w = lin.weight
                if getattr(lin, "lora_A", None) is not None:
                    raise ValueError(f"add_lora: layers.{i}.{t} already carries an adapter (merge_lora or remove_lora first)")
                if w.dtype != torch.float32:
                    raise NotImplementedError(f"add_lora: layers.{i}.{t}.weight is {w.dtype}; adapters need fp32 master weights (the merged cast "
                                              "adds s B A to the fp32 master before its one bf16 rounding)")
                if w.shape[0] % 8 or w.shape[1] % 8:
                    raise NotImplementedError(f"add_lora: layers.{i}.{t}.weight is {tuple(w.shape)}; adapted weights need extents that are multiples of 8")
                plan.append(lin)
    for enc in encoders:
        if freeze_base and getattr(enc, "_lora_base_flags", None) is None:
            enc._lora_base_flags = {n: p.requires_grad for n, p in enc.named_parameters() if n.rsplit(".", 1)[-1] not in _KEYS}
        if freeze_base:
            for n, p in enc.named_parameters():
                if n.rsplit(".", 1)[-1] not in _KEYS:
                    p.requires_grad_(False)
    for lin in plan:
        w = lin.weight
        A = torch.empty((r, w.shape[1]), dtype=torch.float32, device=w.device)
        nn.init.kaiming_uniform_(A, a=math.sqrt(5))
        lin.register_parameter("lora_A", nn.Parameter(A))
        lin.register_parameter("lora_B", nn.Parameter(torch.zeros((w.shape[0], r), dtype=torch.float32, device=w.device)))
        lin.lora_r, lin.lora_alpha, lin.lora_scale = r, float(alpha), float(alpha) / r
    return model


def _strip(model: nn.Module, fold: bool) -> nn.Module:
    for enc in find_encoders(model):
        for _, _, lin in list(_adapted(enc)):
            if fold:
                with torch.no_grad():
                    w = lin.weight
                    w += (lin.lora_scale * (lin.lora_B.to(torch.float32) @ lin.lora_A.to(torch.float32))).to(w.dtype)
            del lin._parameters["lora_A"], lin._parameters["lora_B"]
            for k in ("lora_r", "lora_alpha", "lora_scale"):
                lin.__dict__.pop(k, None)
        flags = getattr(enc, "_lora_base_flags", None)
        if flags is not None:
            for n, p in enc.named_parameters():
                if n in flags:
                    p.requires_grad_(flags[n])
            enc._lora_base_flags = None
    return model


def merge_lora(model: nn.Module) -> nn.Module:
    """Fold every adapter into its fp32 master weight, W += s B A (plain torch, off the hot path), remove the adapter parameters and
    restore the requires_grad flags add_lora(freeze_base=True) changed.  The model's keys are the base model's again.  Its outputs
    differ from the adapted model's by one re-rounding of the weights: bf16(fp32(W + s B A)) against bf16 of the fp32 sum formed
    inside the merged cast (the same values up to the fp32 summation order)."""
    return _strip(model, True)


def remove_lora(model: nn.Module) -> nn.Module:
    """Remove every adapter without folding it in, and restore the requires_grad flags add_lora changed."""
    return _strip(model, False)


def lora_state_dict(model: nn.Module) -> dict:
    """The adapter tensors alone, under their state_dict() names (detached, not copied)."""
    return {k: v for k, v in model.state_dict().items() if k.rsplit(".", 1)[-1] in _KEYS}


def load_lora_state_dict(model: nn.Module, sd: dict) -> nn.Module:
    """Copy adapter tensors saved by lora_state_dict into a model that carries the same adapters (add_lora with the same arguments
    first).  The key sets and shapes must match exactly."""
    own = lora_state_dict(model)
    missing, extra = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    if missing or extra:
        raise KeyError(f"load_lora_state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
    with torch.no_grad():
        for k, dst in own.items():
            if tuple(dst.shape) != tuple(sd[k].shape):
                raise ValueError(f"load_lora_state_dict: {k} is {tuple(sd[k].shape)}, the model's is {tuple(dst.shape)}")
            dst.copy_(sd[k])
    return model


__all__ = ["TARGETS", "add_lora", "merge_lora", "remove_lora", "lora_state_dict", "load_lora_state_dict", "find_encoders"]
