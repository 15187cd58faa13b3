#!/usr/bin/env python3
"""Launches, bits and peak memory of encoder steps on every route of cm3p_amd/encoder.py (the full layer, `cls_only_last_layer`,
`last_layer_rows`, and their fallbacks): a rearrangement of the host code must leave every line unchanged - a peak may only drop.

    python tools/encoder_step_digest.py > profiles/encoder_step_digest.txt

Only the public model API is used (CM3PEncoder on a ModernBertConfig, cm3p_amd.lora.add_lora) plus a wrapper around
cm3p_amd._lib._launch, so the same file runs on any commit.  One line per case:

    <case>: launches fwd <n> <sha> bwd <n> <sha> | out <shape> <sha> | grads <sha> | peak <bytes>

launches: SHA-256 of the ordered C entry-point names with their scalar arguments (pointers as present / absent), forward and backward;
out: of the output's bytes; grads: of every parameter's gradient in name order ("-" on a forward-only call); peak:
torch.cuda.max_memory_allocated() of the step.  Every case builds its model afresh after torch.manual_seed(0).
"""
import ctypes
import gc
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cm3p_amd import _lib  # noqa: E402
from cm3p_amd import kernels as K  # noqa: E402
from cm3p_amd.encoder import CM3PEncoder  # noqa: E402
from cm3p_amd.hf_modernbert import FusedEncoderConfig, encoder_config  # noqa: E402
from cm3p_amd.lora import add_lora  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
FULL, SLIDE = "full_attention", "sliding_attention"
VOCAB, S, LENS = 200, 200, (200, 137, 1)  # the tower of tests/test_cls_last_layer_gpu.py: S > 2 * 64, so a sliding layer slides
ROUTES, LAYOUTS = ("off", "cls", "rows"), ("padded", "unpad", "packed")
TYPES = {1: [FULL], 3: [FULL, SLIDE, SLIDE], 4: [FULL, SLIDE, SLIDE, FULL]}  # 3: the last layer slides; 4: it is global

_log = None
_real_launch = _lib._launch


def _logged_launch(name, args):
    if _log is not None:  # (an address - device or host - is logged as present / absent: its value differs from process to process)
        kinds = getattr(_lib.load(), name).argtypes
        _log.append(name + "(" + ",".join(("0" if a is None else "p") if k is ctypes.c_void_p else repr(a) for k, a in zip(kinds, args)) + ")")
    return _real_launch(name, args)


_lib._launch = _logged_launch


def _sha(data) -> str:
    return hashlib.sha256(data).hexdigest()[:16]


def _bytes(t: torch.Tensor) -> bytes:
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()


def encoder(layers=3, hidden=128, heads=2, inter=192, **kw) -> CM3PEncoder:
    from transformers import ModernBertConfig

    made = max(layers, 3)  # (ModernBertConfig wants both layer types present: the one-layer tower is cut from the 3-layer description)
    cfg = encoder_config(ModernBertConfig(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=made,
                                          num_attention_heads=heads, max_position_embeddings=512, layer_types=TYPES[made], local_attention=128,
                                          pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2, **kw))
    if made != layers:
        cfg = FusedEncoderConfig(**dict(cfg.__dict__, num_hidden_layers=layers, layer_types=TYPES[layers]))
    torch.manual_seed(0)
    enc = CM3PEncoder(cfg)
    with torch.no_grad():  # (the containers' default initialisation, widened so that no gradient is tiny)
        for n, p in enc.named_parameters():
            if p.dim() == 2:
                p.normal_(0.0, 0.05)
    return enc.to(DEV).eval()


def batch(lens=LENS, seq=S):
    g = torch.Generator().manual_seed(0)
    mask = (torch.arange(seq)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(3, VOCAB, (len(lens), seq), generator=g) * mask
    return ids.to(DEV), mask.to(DEV)


def every_7th(lens=LENS, seq=S, packed=False):
    """Row 0 of each sequence plus every 7th valid row, numbered b * seq + position or on the packed axis."""
    rows, start = [], 0
    for b, n in enumerate(lens):
        rows += [(start if packed else b * seq) + p for p in range(0, n, 7)]
        start += n
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def call_of(enc, layout, route, lens=LENS, seq=S, rows=None):
    """-> a function that runs the encoder once on the given layout and route."""
    ids, mask = batch(lens, seq)
    enc.cls_only_last_layer = route == "cls"
    kw = {}
    if route == "rows":
        kw["last_layer_rows"] = every_7th(lens, seq, packed=layout == "packed") if rows is None else rows
    if layout == "packed":
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        flat = ids.flatten()[mask.bool().flatten()]
        return lambda: enc(input_ids=flat, cu_seqlens=cu, max_seqlen=max(lens), **kw)
    if all(n == seq for n in lens):
        return lambda: enc(input_ids=ids, **kw)
    return lambda: enc(input_ids=ids, attention_mask=mask, unpad=layout == "unpad", **kw)


def run(tag, enc, fn, train):
    """One step: forward-only under no_grad, or forward + the loss sum(y * w) + backward."""
    global _log
    g = torch.Generator(device=DEV).manual_seed(1)
    enc.zero_grad(set_to_none=True)
    K.release_workspaces()
    gc.collect()
    torch.manual_seed(0)  # (a dropout plan draws its seed from the default CPU generator)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fwd, bwd = [], []
    try:
        _log = fwd
        if train:
            y = fn()
            loss = (y.float() * torch.randn(y.shape, device=DEV, generator=g)).sum()
            _log = bwd
            loss.backward()
        else:
            with torch.no_grad():
                y = fn()
    except (NotImplementedError, ValueError) as e:  # a combination the code refuses: no line
        print(f"# {tag}: refused ({type(e).__name__})", file=sys.stderr)
        return
    finally:
        _log = None
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    grads = "-"
    if train:
        h = hashlib.sha256()
        for n, p in sorted(enc.named_parameters()):
            h.update(n.encode())
            h.update(b"none" if p.grad is None else _bytes(p.grad))
        grads = h.hexdigest()[:16]
    print(f"{tag}: launches fwd {len(fwd)} {_sha(chr(10).join(fwd).encode())} bwd {len(bwd)} {_sha(chr(10).join(bwd).encode())} | "
          f"out {tuple(y.shape)} {str(y.dtype)[6:]} {_sha(_bytes(y))} | grads {grads} | peak {peak}", flush=True)


def nonzero_lora_B(enc):
    g = torch.Generator(device=DEV).manual_seed(4)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("lora_B"):
                p.normal_(0.0, 0.02, generator=g)


def smallest_shape(supported):
    """The (rows, I, H) with the least rows * I * H that the library's routing rule accepts, on head-64 extents."""
    best = None
    for H in range(64, 769, 64):
        for I in range(64, 1153, 64):
            for T in range(64, 16385, 64):
                if best is not None and T * I * H >= best[0]:
                    break
                if supported(T, I, H):
                    best = (T * I * H, T, I, H)
                    break
    if best is None:
        raise SystemExit(f"{supported.__name__}: no shape found")
    return best[1:]


def split_rows(T):
    """T rows as (sequences, length) with 128 < length <= 512."""
    for seq in range(512, 128, -1):
        if T % seq == 0:
            return T // seq, seq
    raise SystemExit(f"no sequence length divides {T}")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/encoder_step_digest.py runs on the GPU; there is no CPU path")
    # ---- main tower: depth x layout x route x call kind
    for layers in (3, 4):
        for layout in LAYOUTS:
            for route in ROUTES:
                for train in (False, True):
                    enc = encoder(layers)
                    enc.train(train)
                    run(f"L{layers} {layout} {route} {'train' if train else 'fwd'}", enc, call_of(enc, layout, route), train)
    # ---- forward-only bf16 stream
    for route in ROUTES:
        enc = encoder(3)
        enc.residual_dtype = BF
        run(f"bf16 forward-only stream {route}", enc, call_of(enc, "padded", route), False)
    # ---- fallbacks of the two row routes (and what the issue adds on the full route)
    for how in ("dropout", "checkpointing", "adapter on the last Wo", "bf16 training stream"):
        for route in ("cls", "rows"):
            enc = encoder(3, **(dict(attention_dropout=0.1, mlp_dropout=0.1) if how == "dropout" else {})).train()
            if how == "checkpointing":
                enc.gradient_checkpointing = True
            elif how.startswith("adapter"):
                add_lora(enc, r=8, alpha=16, targets=["attn.Wo"], layers=[2], freeze_base=False)
                nonzero_lora_B(enc)
            elif how.startswith("bf16"):
                enc.train_residual_dtype = BF
            run(f"fallback {how} {route} train", enc, call_of(enc, "padded", route), True)
    enc = encoder(3).train()
    add_lora(enc, r=8, alpha=16, layers=[1], freeze_base=False)
    nonzero_lora_B(enc)
    run("full route, adapters on the four projections of layer 1, train", enc, call_of(enc, "padded", "off"), True)
    enc = encoder(3, attention_dropout=0.1, mlp_dropout=0.1, embedding_dropout=0.1).train()
    run("full route, dropout on all three sites, train", enc, call_of(enc, "padded", "off"), True)
    # ---- head size 32 (the generic kernels; the row route falls back)
    for route in ("off", "cls"):
        for train in (False, True):
            enc = encoder(3, hidden=64, heads=2, inter=128)
            enc.train(train)
            run(f"head 32 {route} {'train' if train else 'fwd'}", enc, call_of(enc, "padded", route), train)
    # ---- one layer: the last layer is layer 0; frozen below: the chain ends in the last layer
    for route in ROUTES:
        enc = encoder(1).train()
        run(f"one layer {route} train", enc, call_of(enc, "padded", route), True)
    for route in ROUTES:
        enc = encoder(3).train()
        for n, p in enc.named_parameters():
            if n.startswith("embeddings.") or n.startswith("layers.0.") or n.startswith("layers.1."):
                p.requires_grad_(False)
        run(f"frozen below the last layer {route} train", enc, call_of(enc, "padded", route), True)
    # ---- the two sides of the rows route's fill seam, and the empty list
    for n in (8, 9, 0):
        for train in (False, True):
            enc = encoder(3)
            enc.train(train)
            run(f"rows list of {n} {'train' if train else 'fwd'}", enc, call_of(enc, "padded", "rows", rows=every_7th()[:n].contiguous()), train)
    # ---- fused GeGLU at the smallest shapes the library takes it
    T, I, H = smallest_shape(K.mlp_geglu_fused_supported)
    nseq, seq = split_rows(T)
    for route in ("off", "rows"):
        enc = encoder(3, hidden=H, heads=H // 64, inter=I).train()
        run(f"fused GeGLU training pair rows={T} I={I} H={H} {route} train", enc, call_of(enc, "padded", route, lens=(seq,) * nseq, seq=seq), True)
    T, I, H = smallest_shape(K.gemm_geglu_supported)
    nseq, seq = split_rows(T)
    enc = encoder(3, hidden=H, heads=H // 64, inter=I)
    run(f"fused GeGLU forward-only rows={T} I={I} H={H} off fwd", enc, call_of(enc, "padded", "off", lens=(seq,) * nseq, seq=seq), False)


if __name__ == "__main__":
    main()
