"""The ModernBERT-shaped encoder tower of CM3P on HIP kernels.

`CM3PEncoder` stands where the reference instantiates `transformers.ModernBertModel`
(ref:cm3p/modeling_cm3p.py:305,491,537) and keeps its parameter names, so `state_dict()` keys are unchanged:
    embeddings.tok_embeddings.weight, embeddings.norm.weight, layers.N.{attn_norm,mlp_norm}.weight,
    layers.N.attn.{Wqkv,Wo}.weight, layers.N.mlp.{Wi,Wo}.weight, final_norm.weight
The nn.Linear / nn.LayerNorm / nn.Embedding members are parameter containers only; their torch forward is never
called.  Every encoder layer is ONE autograd node (`_EncoderLayerFn`; `_FinalNormFn` closes the stack) whose forward and
backward are sequences of C-ABI launches (cm3p_amd/kernels.py), restating
TF:models/modernbert/modeling_modernbert.py:262-333,434-478; a last layer of which only some rows are consumed runs as
`_LastLayerRowsFn`, the same layer body (`_pre_attn_*`, `_post_attn_*`: written once, both nodes call them) with attention and what
follows it on those rows:

    per layer:  xn = LN(x) [identity for layer 0] -> qkv = xn Wqkv^T -> RoPE(q,k) -> flash attention (global, or
                |i-j| <= 64 band; key padding) -> x += o Wo^T -> xn = LN(x) -> h = xn Wi^T -> g = gelu(h[:I]) * h[I:]
                -> x += g Wo^T;   after the last layer: final LN.

Numerics: the residual stream, LayerNorm statistics, softmax and all accumulations are fp32; GEMM operands and saved
activations are bf16 (what HF Trainer's bf16 autocast gives the reference's nn.Linear calls).

GeGLU of a training step: where the library's route names the ring GEMM for both calls (the beatmap tower's shapes), no MLP dropout is
planned and CM3P_GEGLU_FUSED is not "0", `h = xn Wi^T` and `g = gelu(h[:I]) * h[I:]` are one launch (K.linear_geglu_fwd: h is kept with
interleaved columns) and the backward's `dg = dy Wo` never exists (K.linear_dgrad_geglu_bwd turns it into the canonical dh in the GEMM's
store phase); loss, output and gradients are those of the two-kernel path bit for bit.

Dropout (training mode, p > 0): embedding output, attention probabilities (inside the attention kernels), attention output before
the residual add, and gelu(h[:I]) * h[I:] before Wo - the masks follow csrc/dropout_rng.h from one seed per stack forward.

bf16 residual stream (opt-in, `CM3PEncoder.residual_dtype = torch.bfloat16`): a forward-only call (nothing recorded for a backward,
no dropout plan) keeps the stream in bf16 the way a bf16 ModernBERT does (TF:...modeling_modernbert.py:68-70,331-332,476): every
LayerNorm reads and writes bf16, `x + o Wo^T` and `x + g Wo^T` are bf16 adds of the bf16-rounded projection (CM3P_EPI_BF16_RESID),
last_hidden_state and hidden_states are bf16.  Every other call runs the fp32 stream whatever that switch says.

bf16 residual stream of a training step (opt-in, its own switch: `CM3PEncoder.train_residual_dtype = torch.bfloat16`, or
`model.set_residual_dtype(torch.bfloat16, training=True)`): a call that records a backward and has no dropout plan runs the forward
above (the same kernels; LayerNorm also writes its fp32 mean / rstd, and a layer keeps x and x_mid as bf16) and a backward whose
residual-stream gradient is ONE bf16 tensor: LayerNorm backward (both streams' one kernel, in its all-bf16 form) reads dy, x and the
incoming gradient g in bf16 and writes bf16(g + LN'(dy)), the sum formed in fp32 and rounded once (8 B per element, not 16 and more).
Statistics, dw partial sums, softmax and GEMM accumulation stay fp32; weight gradients come out of the wgrad GEMMs in fp32 and are cast to
the parameter's dtype as on the fp32 stream.  With a dropout plan (train mode, any p > 0) the fp32 stream runs: the dropout sites have
no bf16 form.

Low-rank adapters (cm3p_amd.lora.add_lora puts `lora_A` / `lora_B` on the container nn.Linear of a projection): the bf16 operand of an
adapted weight is bf16(W + s B A), made in the stack's one cast launch (K.lora_merge_cast_many; kept across forward-only calls like the
plain copies), so every GEMM above runs unchanged; the adapter tensors are extra inputs of _EncoderLayerFn and get their gradients from
K.lora_grad on the operands of the projection's weight-gradient GEMM.  Not on the bf16 stream of training steps.
"""
from __future__ import annotations

import os
import weakref
from typing import Optional

import torch
from torch import nn

from . import kernels as K

Tensor = torch.Tensor


def _check_supported(cfg):
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    problems = []
    if H % nh or H // nh not in (16, 32, 64, 96, 128):
        # 64: the MFMA kernels every default tower runs on; 16 / 32: csrc/attention_generic.hip (plain fp32 kernels, so that the
        # reference's small test configurations run as well); 96 / 128: csrc/attention_hd.hip (MFMA kernels for widened towers:
        # padded execution, no attention dropout)
        problems.append(f"head_dim must be 64 (or 16 / 32 on the generic kernels, or 96 / 128 on the wide-head MFMA kernels); hidden_size={H}, heads={nh}")
    if getattr(cfg, "hidden_activation", "gelu") != "gelu":
        problems.append("hidden_activation must be 'gelu'")
    for flag in ("norm_bias", "attention_bias", "mlp_bias"):
        if getattr(cfg, flag, False):
            problems.append(f"{flag}=True is not supported (the reference configs never set it)")
    for p in ("attention_dropout", "embedding_dropout", "mlp_dropout"):
        v = getattr(cfg, p, 0.0) or 0.0
        if not 0.0 <= float(v) <= 1.0:  # nn.Dropout's own rule
            raise ValueError(f"{p} has to be between 0 and 1, but got {v}")
    if cfg.intermediate_size % 8 or H % 8:
        problems.append("hidden_size and intermediate_size must be multiples of 8")
    if problems:
        raise NotImplementedError("cm3p_amd HIP encoder: " + "; ".join(problems))


class CM3PAttentionParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.Wqkv = nn.Linear(cfg.hidden_size, 3 * cfg.hidden_size, bias=False)
        self.Wo = nn.Linear(cfg.hidden_size, cfg.hidden_size, bias=False)


class CM3PMLPParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.Wi = nn.Linear(cfg.hidden_size, 2 * cfg.intermediate_size, bias=False)
        self.Wo = nn.Linear(cfg.intermediate_size, cfg.hidden_size, bias=False)


class CM3PEncoderLayerParams(nn.Module):
    def __init__(self, cfg, layer_idx: int):
        super().__init__()
        # layer 0 has no attn_norm (TF:...modeling_modernbert.py:309-310)
        self.attn_norm = nn.Identity() if layer_idx == 0 else nn.LayerNorm(cfg.hidden_size, eps=cfg.norm_eps, bias=False)
        self.attn = CM3PAttentionParams(cfg)
        self.mlp_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.norm_eps, bias=False)
        self.mlp = CM3PMLPParams(cfg)


class CM3PEmbeddingParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.tok_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden_size, padding_idx=getattr(cfg, "pad_token_id", None))
        self.norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.norm_eps, bias=False)


def _f32(w: Tensor) -> Tensor:
    return w if w.dtype == torch.float32 else w.float()


def _bf16_weight(w: Tensor) -> Tensor:
    """bf16 GEMM operand of a master weight (what autocast's per-call cast produces)."""
    w = w.detach()
    if w.dtype == torch.bfloat16:
        return w
    if w.dtype != torch.float32:  # fp16 / fp64 checkpoints: widen first (dtype plumbing; the cast kernel reads fp32)
        w = w.float()
    return K.cast_bf16(w.contiguous())


_eval_weights: dict = {}  # id(parameter) -> (weakref to it, its _version, its data_ptr, bf16 copy): forward-only calls
K._other_caches.append(_eval_weights)  # (kernels.release_workspaces() empties it)


def invalidate_weight_cache() -> None:
    """Drop the bf16 weight copies kept across forward-only calls.  Called by every forward that will be followed by a backward (a
    training step means an optimizer is about to rewrite the weights, whatever it is and however it writes them) and by
    `module.train()` / `module.eval()` mode flips of an encoder; call it by hand after writing weights in a way that leaves no trace
    on the parameter (`p.data.copy_(...)`, an EMA swap through `.data`, a kernel that takes `p.data_ptr()`) between two
    forward-only calls."""
    _eval_weights.clear()


def _bf16_weight_cached(w: Tensor, geglu_rows: bool = False) -> Tensor:
    """Forward-only calls (no backward will follow: evaluation, embedding extraction) reuse the bf16 copy of a master weight for
    as long as the weight is the same object with the same version counter and storage - every in-place torch op (torch optimizers,
    load_state_dict) bumps the counter, `p.data = ...` changes the address, and writers that go through raw addresses bump it by hand
    (cm3p_amd.Muon.step does).  Writes through `p.data` bump nothing: see invalidate_weight_cache().  A training step re-casts every
    weight once anyway and empties the cache.
    geglu_rows: the copy of a Wi weight with its rows in the order cm3p_gemm_geglu reads (kernels.geglu_interleave_index)."""
    key = (id(w), geglu_rows)
    hit = _eval_weights.get(key)
    if hit is not None and hit[0]() is w and hit[1] == w._version and hit[2] == w.data_ptr():
        return hit[3]
    wb = _bf16_weight(w)
    if geglu_rows:
        wb = wb.index_select(0, K.geglu_interleave_index(w.shape[0] // 2, wb.device)).contiguous()
    if wb.data_ptr() != w.data_ptr():  # (a bf16 master weight is its own operand: nothing to keep)
        if len(_eval_weights) > 4096:  # dead entries of models that are gone
            for k in [k for k, v in _eval_weights.items() if v[0]() is None]:
                del _eval_weights[k]
        _eval_weights[key] = (weakref.ref(w), w._version, w.data_ptr(), wb)
    return wb


def _bf16_weight_pair(w: Tensor, want_t: bool):
    """-> (bf16 W [out, in], bf16 W^T [in, out] or None).  The transpose feeds the input-gradient GEMM (dx = dy W) with the
    contraction index contiguous in both operands; it is made in the same pass as the cast when a backward will follow and the
    extents allow it (multiples of 8), otherwise dgrad reads W itself (k-strided operand, same result)."""
    if not want_t:
        return _bf16_weight_cached(w), None
    w = w.detach()
    if w.dtype == torch.float32 and w.dim() == 2 and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0:
        return K.cast_bf16_with_transpose(w.contiguous())
    return _bf16_weight(w), None


def lora_of(lin):
    """-> (A [r, in], B [out, r], s) of a container nn.Linear that carries a low-rank adapter (cm3p_amd.lora.add_lora), or None."""
    A = getattr(lin, "lora_A", None)
    return None if A is None else (A, lin.lora_B, float(lin.lora_scale))


def _check_lora_operands(w: Tensor, A: Tensor, B: Tensor) -> None:
    """What the merged cast reads through raw addresses; add_lora refuses the same before it registers anything, this is for edits since."""
    r = A.shape[0]
    if w.dtype != torch.float32 or A.dtype != torch.float32 or B.dtype != torch.float32:
        raise NotImplementedError(f"cm3p_amd LoRA: master weights and adapters must be fp32 (weight {w.dtype}, lora_A {A.dtype}, lora_B {B.dtype})")
    if r not in K.LORA_RANKS or tuple(A.shape) != (r, w.shape[1]) or tuple(B.shape) != (w.shape[0], r) or w.shape[0] % 8 or w.shape[1] % 8:
        raise NotImplementedError(f"cm3p_amd LoRA: weight {tuple(w.shape)} with lora_A {tuple(A.shape)}, lora_B {tuple(B.shape)}: r must be one of "
                                  f"{K.LORA_RANKS} and the weight's extents multiples of 8")


def _lora_merged_cached(entries: list) -> list:
    """Forward-only calls: [(W, A, B, s, geglu_rows)] -> [bf16(W + s B A)] (rows interleaved for a flagged Wi), kept like the copies of
    _bf16_weight_cached for as long as W, A AND B are the same objects with the same version counters and storage; the misses of one call
    are merged in one launch."""
    out, miss = [None] * len(entries), []
    for n, (w, A, B, s, il) in enumerate(entries):
        hit = _eval_weights.get((id(w), il, "lora"))
        if hit is not None and hit[4][0] == s and all(r() is t and v == t._version and p == t.data_ptr()
                                                      for (r, v, p), t in zip((hit[:3], *hit[4][1:]), (w, A, B))):
            out[n] = hit[3]
        else:
            miss.append(n)
    if miss:
        made = K.lora_merge_cast_many([(entries[n][0].detach().contiguous(), entries[n][1].detach().contiguous(), entries[n][2].detach().contiguous(),
                                        entries[n][3], entries[n][4]) for n in miss])
        for n, (y, _) in zip(miss, made):
            w, A, B, s, il = entries[n]
            y = y.clone()  # (the launch's one allocation also holds the transposes, which no forward-only call reads)
            stamp = [(weakref.ref(t), t._version, t.data_ptr()) for t in (w, A, B)]
            _eval_weights[(id(w), il, "lora")] = (*stamp[0], y, (s, stamp[1], stamp[2]))  # (the layout of _bf16_weight_cached's entries, and more)
            out[n] = y
    return out


def _geglu_fwd_fused(plan, rows: int, Wi: Tensor) -> bool:
    """Forward-only call on a shape of the ring kernel: the Wi GEMM stores gelu(h) * g itself (CM3P_GEGLU_FUSED=0: the two-kernel path)."""
    return not (plan is not None and plan.mlp) and Wi.dim() == 2 and K.gemm_geglu_supported(rows, Wi.shape[0] // 2, Wi.shape[1]) \
        and os.environ.get("CM3P_GEGLU_FUSED", "1") != "0"


class _Geometry:
    """Static description of one forward call of the stack (no tensors that need grad)."""

    __slots__ = ("B", "S", "H", "I", "nh", "L", "eps", "windows", "key_mask", "rope", "per_batch_pos", "save", "cu", "max_s", "checkpoint",
                 "handoff", "attn_out", "wcast", "hd", "drop", "bf16", "fused_mlp", "lora", "wcast_geglu")


def _hand_upstream(geo: _Geometry, gx32: Tensor, gx16: Optional[Tensor]) -> None:
    """(bf16 residual stream: the ONE bf16 gradient is handed up in both places, (g, g); _take_bf16_from_downstream reads the first.)
    A node's backward leaves the bf16 twin of the fp32 gradient it returns here; the node below (the next one the autograd
    engine runs on this chain) picks it up instead of re-reading 4 bytes per element to cast it again."""
    geo.handoff = (gx32, gx16)


def _take_from_downstream(geo: _Geometry, dy: Tensor):
    """-> (fp32 gradient this node may update in place, its bf16 twin).  The fast path applies when `dy` is exactly the tensor
    the node above handed up (nothing else consumed that activation, so autograd passed it through untouched); the handoff
    keeps that tensor alive, so an equal address cannot be a recycled allocation.  Anything else (a hook, a second consumer)
    gets a private copy and a fresh cast."""
    h, geo.handoff = geo.handoff, None
    if h is not None and h[1] is not None and h[0].data_ptr() == dy.data_ptr() and h[0].shape == dy.shape and dy.dtype == torch.float32 \
            and dy.is_contiguous():
        return h[0], h[1]
    g = dy.float().contiguous()
    if g.data_ptr() == dy.data_ptr():
        g = g.clone()
    return g, K.cast_bf16(g)


def _take_bf16_from_downstream(geo: _Geometry, dy: Tensor) -> Tensor:
    """bf16 residual stream: -> the ONE bf16 gradient tensor this node may update in place.  The rule of _take_from_downstream: `dy`
    is used as it is only when it is exactly the tensor the node above handed up; anything else (the gradient that enters the stack
    from pooling or a head, a sum autograd formed for two consumers, a hook) gets a private copy."""
    h, geo.handoff = geo.handoff, None
    if h is not None and h[0].data_ptr() == dy.data_ptr() and h[0].shape == dy.shape and dy.dtype == torch.bfloat16 and dy.is_contiguous():
        return h[0]
    g = dy.to(torch.bfloat16).contiguous()
    if g.data_ptr() == dy.data_ptr():
        g = g.clone()
    return g


# ---- the layer body, written once for both layer nodes (_EncoderLayerFn: every row; _LastLayerRowsFn: attention and what follows it on
# a block of query rows): the operands, and a forward and a backward each of the part in front of attention and the part behind it
def _layer_operands(geo: _Geometry, i: int, weights, mlp_rows: Optional[int]):
    """A layer node's `weights` (in the order of CM3PEncoder._stack_weights, then its adapter tensors) -> (wb, wt, adapters):
    wb = (w_an, Wqkv, Wo, w_mn, Wi, Wo2 as bf16 GEMM operands - the norm weights fp32 -, Wi with GeGLU-interleaved rows for the
    forward-only fused kernel or None, whether this Wi is the fused training pair's), wt the four W^T copies the input-gradient GEMMs
    read (None where there is none), adapters (A, B, s) or None per projection in the order Wqkv, Wo, Wi, Wo2.
    mlp_rows: the rows the MLP runs on, which the forward-only fused Wi + GeGLU kernel's shape rule is asked about; None: a row block,
    whose MLP is the plain chain (as _run_stack keeps the fused training pair away from it)."""
    it = iter(weights)
    w_an = None if i == 0 else _f32(next(it))
    Wqkv, Wo, w_mn, Wi, Wo2 = next(it), next(it), _f32(next(it)), next(it), next(it)
    # low-rank adapters (cm3p_amd.lora): (A, B, s) per projection in the order Wqkv, Wo, Wi, Wo2; their tensors follow the weights
    spec = geo.lora[i] if geo.lora is not None else (None,) * 4
    adapters = [None if sc is None else (next(it).detach(), next(it).detach(), sc) for sc in spec]
    # forward-only and a shape of the ring kernel: the Wi GEMM stores gelu(h) * g itself (CM3P_GEGLU_FUSED=0: the two-kernel path)
    fuse_geglu = (not geo.save) and mlp_rows is not None and _geglu_fwd_fused(geo.drop, mlp_rows, Wi)
    # (training: the casts of every layer were made in one launch at the top of the stack, _run_stack; adapted weights: their merged
    # copies bf16(W + s B A) were made there on every kind of call)
    pre = geo.wcast if geo.wcast is not None else {}
    pairs = [pre.get(id(w)) or _bf16_weight_pair(w, geo.save) if not (fuse_geglu and w is Wi) else (None, None) for w in (Wqkv, Wo, Wi, Wo2)]
    # training step, fused pair (_run_stack decided; CM3P_GEGLU_FUSED=0: the two-kernel path): this Wi's copy has interleaved rows
    fused_train = geo.save and id(Wi) in geo.fused_mlp
    Wi_geglu = None
    if fuse_geglu:
        Wi_geglu = geo.wcast_geglu[id(Wi)] if adapters[2] is not None else _bf16_weight_cached(Wi, True)
    wb = (w_an, pairs[0][0], pairs[1][0], w_mn, pairs[2][0], pairs[3][0], Wi_geglu, fused_train)
    return wb, tuple(p[1] for p in pairs), adapters


def _backward_needs(i: int, need, adapters):
    """need: a layer node's needs_input_grad behind x -> ((n_an, n_qkv, n_o, n_mn, n_i, n_o2), lora_grads).  lora_grads(p, dy_p, x_p): the
    adapter gradients (dA, dB) of projection p from the operands its weight-gradient GEMM reads; () when it carries no adapter."""
    n_base = 5 if i == 0 else 6
    need_w = list(need[:n_base])
    if i == 0:
        need_w.insert(0, False)  # (no attn_norm in layer 0)
    need_l = iter(need[n_base:])
    want_l = [None if a is None else (next(need_l), next(need_l)) for a in adapters]

    def lora_grads(p: int, dy_p: Tensor, x_p: Tensor):
        if adapters[p] is None:
            return ()
        if not any(want_l[p]):
            return (None, None)
        dA, dB = K.lora_grad(x_p, dy_p, *adapters[p])
        return (dA if want_l[p][0] else None, dB if want_l[p][1] else None)

    return need_w, lora_grads


def _weight_grads(i: int, dw_an, grads: list, dtypes, need) -> list:
    """What a layer node returns behind x: the gradients in the order of its weights (and adapter tensors), in their dtypes."""
    grads = grads if i == 0 else [dw_an, *grads]
    return [(gw if gw.dtype == dt else gw.to(dt)) if (nd and gw is not None) else None for gw, dt, nd in zip(grads, dtypes, need)]


def _attn_drop(geo: _Geometry, i: int) -> Optional[tuple]:
    """Layer i's attention dropout (probabilities and out_drop, TF:...modeling_modernbert.py:292,300): (thr, seed, layer), or None."""
    return (geo.drop.attn, geo.drop.seed, i) if geo.drop is not None and geo.drop.attn else None


def _pre_attn_forward(geo: _Geometry, i: int, x: Tensor, wb, want_stats: bool):
    """attn_norm (the cast in layer 0) and the Wqkv + RoPE projection on every row: -> (xn, mean_a, rstd_a, qkv)."""
    cos, sin = geo.rope[i]
    if i == 0:  # (bf16 stream: the embedding output is layer 0's GEMM operand as it is)
        xn, mean_a, rstd_a = (x if x.dtype == torch.bfloat16 else K.cast_bf16(x)), None, None
    else:
        _, xn, mean_a, rstd_a = K.layernorm_fwd(x, wb[0], geo.eps, False, True, want_stats)
    if geo.hd != 64:
        # head sizes 16 / 32: plain projection, rotary embedding as its own pass (fp32 on the bf16 projection, one rounding: the
        # reference's order), attention on the generic kernels (csrc/attention_generic.hip); padded execution only
        qkv = K.linear_fwd(xn, wb[1])
        K.rope_apply_generic_(qkv, cos, sin, geo.B, geo.S, geo.nh, geo.hd, geo.per_batch_pos)
    else:
        # projection + RoPE in one kernel; the q third also takes the softmax's scale * log2(e) before its one bf16 rounding, so the
        # attention kernels exponentiate the MFMA's scores as they come (prescaled=True everywhere behind it)
        qkv = K.qkv_linear_rope(xn, wb[1], cos, sin, geo.S, geo.per_batch_pos, q_scale=K.SOFTMAX_Q_SCALE)
    return xn, mean_a, rstd_a, qkv


def _pre_attn_backward(geo: _Geometry, i: int, dqkv: Tensor, g32_of, acts, wb, Wqkv_t, need_x: bool, n_an: bool, n_qkv: bool, lora_grads):
    """Backward of _pre_attn_forward: dqkv and the residual stream's own fp32 gradient -> (dWqkv, Wqkv's adapter gradients, dw_an, the
    fp32 gradient of x or None), and the handoff to the node below.  g32_of() gives that incoming gradient; it is called once, behind the
    weight gradient's launches, and only when something goes upstream (need_x) or into attn_norm's weight - the row node scatters its
    block's gradient into zeros there, no sooner and not where the chain ends.  Nothing is handed up when nothing is returned."""
    x, xn, mean_a, rstd_a = acts
    dWqkv = K.linear_wgrad(dqkv, xn) if n_qkv else None
    l_qkv = lora_grads(0, dqkv, xn)
    dw_an = g32 = None
    if need_x or n_an:  # (else: everything below this layer is frozen, the chain ends here; layer 0 has no attn_norm, n_an is False)
        g32 = g32_of()
        dxn = K.linear_dgrad(dqkv, wb[1], Wqkv_t)
        if i == 0:
            g32, _ = K.add_f32(g32, dxn, want_bf16=False)
            _hand_upstream(geo, g32, None)
        else:
            g32, g16, dw_an = K.layernorm_bwd(dxn, x, wb[0], mean_a, rstd_a, g32, True)
            _hand_upstream(geo, g32, g16)
    return dWqkv, l_qkv, dw_an, g32


def _post_attn_forward(geo: _Geometry, i: int, o: Tensor, x: Tensor, wb, want_stats: bool):
    """The part of a layer behind attention, on every row or on a block of rows (o the attention output, x the residual rows):
    -> x_out = x_mid + GeGLU(mlp_norm(x_mid) Wi^T) Wo2^T with x_mid = x + o Wo^T, and (x_mid, xn2, mean_m, rstd_m, h, g) for the backward."""
    Wo_b, w_mn, Wi_b, Wo2_b, Wi_geglu, fused_train = wb[2:]
    ad = _attn_drop(geo, i)
    if ad is not None:  # out_drop: Wo writes fp32 t, then x_mid = x + Z o t
        x_mid = K.dropout_f32(K.linear_fwd_f32(o, Wo_b), ad[0], ad[1], i, K.SITE_ATTN_OUT, geo.S, geo.cu, resid=x)
    else:
        x_mid = K.linear_fwd(o, Wo_b, resid=x)
    _, xn2, mean_m, rstd_m = K.layernorm_fwd(x_mid, w_mn, geo.eps, False, True, want_stats)
    if Wi_geglu is not None:  # forward-only call: Wi and GeGLU in one kernel, h and g never exist (bit-identical a)
        h, g = None, K.gemm_geglu(xn2, Wi_geglu)
    elif fused_train:  # training step, fused pair: Wi_b has interleaved rows and the GEMM stores h' (interleaved columns) and g
        h, g = K.linear_geglu_fwd(xn2, Wi_b)
    else:
        h = K.linear_fwd(xn2, Wi_b)
        if geo.drop is not None and geo.drop.mlp:  # g o Z: what Wo and its weight gradient read (TF:...modeling_modernbert.py:91)
            g = K.geglu_fwd_dropout(h, geo.drop.mlp, geo.drop.seed, i, geo.S, geo.cu)
        else:
            g = K.geglu_fwd(h)
    x_out = K.linear_fwd(g, Wo2_b, resid=x_mid)
    return x_out, (x_mid, xn2, mean_m, rstd_m, h, g)


def _post_attn_backward(geo: _Geometry, i: int, live: list, o: Tensor, wb, wt, need, lora_grads):
    """Backward of _post_attn_forward.  live = [the output's fp32 gradient, its bf16 twin, x_mid, xn2, mean_m, rstd_m, h, g], a list
    this function empties: the caller keeps no reference of its own (an argument would stay alive on its stack for the whole call), so
    each tensor is released where its last reader has run.  o is read, not taken (attention's backward reads it next).
    -> (the fp32 gradient of x, updated in place; do = the gradient of o; dWo, dw_mn, dWi, dWo2 - None where not needed -; the adapter
    gradients of Wo, Wi, Wo2)."""
    gx32, gx16, x_mid, xn2, mean_m, rstd_m, h, g = live
    live.clear()
    Wo_b, w_mn, Wi_b, Wo2_b = wb[2:6]
    _, Wo_t, Wi_t, Wo2_t = wt
    n_o, n_i, n_o2 = need
    # ---- MLP branch: x_out = x_mid + g Wo2^T
    fused = wb[7]  # h is h' (interleaved columns): the Wo2 dgrad's store phase turns dg into the canonical dh
    dg = None if fused else K.linear_dgrad(gx16, Wo2_b, Wo2_t)
    dWo2 = K.linear_wgrad(gx16, g) if n_o2 else None
    l_o2 = lora_grads(3, gx16, g)
    if fused:
        dh = K.linear_dgrad_geglu_bwd(gx16, Wo2_t, h)
    elif geo.drop is not None and geo.drop.mlp:
        dh = K.geglu_bwd_dropout(dg, h, geo.drop.mlp, geo.drop.seed, i, geo.S, geo.cu)
    else:
        dh = K.geglu_bwd(dg, h)
    del dg, g
    dxn2 = K.linear_dgrad(dh, Wi_b, Wi_t)
    dWi = K.linear_wgrad(dh, xn2) if n_i else None
    l_i = lora_grads(2, dh, xn2)
    del dh, h, xn2
    gx32, gx16, dw_mn = K.layernorm_bwd(dxn2, x_mid, w_mn, mean_m, rstd_m, gx32, True)
    del dxn2, x_mid
    # ---- attention branch: x_mid = x + o Wo^T  (with attention dropout: x + Z o (o Wo^T))
    ad = _attn_drop(geo, i)
    gt16 = gx16 if ad is None else K.dropout_f32(gx32, ad[0], ad[1], i, K.SITE_ATTN_OUT, geo.S, geo.cu, bf16_only=True)
    do = K.linear_dgrad(gt16, Wo_b, Wo_t)
    dWo = K.linear_wgrad(gt16, o) if n_o else None
    l_o = lora_grads(1, gt16, o)
    return gx32, do, dWo, dw_mn, dWi, dWo2, l_o, l_i, l_o2


def _layer_forward(geo: _Geometry, i: int, x: Tensor, wb, want_stats: bool):
    """One encoder layer on [T, H] rows: -> (x_out, activations needed by its backward)."""
    xn, mean_a, rstd_a, qkv = _pre_attn_forward(geo, i, x, wb, want_stats)
    B, S, nh, scale, ad = geo.B, geo.S, geo.nh, geo.hd ** -0.5, _attn_drop(geo, i)
    if geo.hd != 64:
        o, lse = K.attn_fwd_generic(qkv, geo.key_mask, B, S, nh, geo.hd, geo.windows[i], scale, drop=ad)
    elif geo.cu is not None:  # unpadded batch: packed rows, per-token rotary tables
        o, lse = K.attn_fwd_varlen(qkv, geo.cu, B, geo.max_s, nh, geo.windows[i], scale, prescaled=True, drop=ad)
    else:
        o, lse = K.attn_fwd(qkv, geo.key_mask, B, S, nh, geo.windows[i], scale, prescaled=True, drop=ad)
        if geo.attn_out is not None and len(geo.attn_out) == i:  # output_attentions (not again when a checkpointed layer is recomputed)
            geo.attn_out.append(K.attn_probs(qkv, lse, geo.key_mask, B, S, nh, geo.windows[i], scale, prescaled=True))
    x_out, post = _post_attn_forward(geo, i, o, x, wb, want_stats)
    return x_out, (x, xn, mean_a, rstd_a, qkv, o, lse, *post)


def _attn_backward(geo: _Geometry, i: int, qkv: Tensor, o: Tensor, do: Tensor, lse: Tensor, ad: Optional[tuple]) -> Tensor:
    """Layer i's attention backward -> dqkv; the inverse rotary rotation of dq / dk is applied in the kernels' epilogue (head_dim 64)
    or as its own pass (the generic kernels).  ad: the layer's attention dropout (thr, seed, layer), or None."""
    B, S, nh, window, scale = geo.B, geo.S, geo.nh, geo.windows[i], geo.hd ** -0.5
    if geo.hd != 64:
        dqkv = K.attn_bwd_generic(qkv, o, do, lse, geo.key_mask, B, S, nh, geo.hd, window, scale, drop=ad)
        return K.rope_apply_generic_(dqkv, geo.rope[i][0], geo.rope[i][1], B, S, nh, geo.hd, geo.per_batch_pos, inverse=True)
    if geo.cu is not None:
        return K.attn_bwd_varlen(qkv, o, do, lse, geo.cu, B, geo.max_s, nh, window, scale, geo.rope[i], prescaled=True, drop=ad)
    return K.attn_bwd(qkv, o, do, lse, geo.key_mask, B, S, nh, window, scale, geo.rope[i], geo.per_batch_pos, prescaled=True, drop=ad)


class _EncoderLayerFn(torch.autograd.Function):
    """One ModernBERT encoder layer (TF:...modeling_modernbert.py:318-333): x [T,H] fp32 + its weights -> x_out [T,H] fp32
    (bf16 -> bf16 on the bf16 residual stream: the residual GEMMs take x's dtype; its backward is _backward_bf16).

    One autograd node per layer, so a layer's weight gradients reach their parameters (and a DistributedDataParallel
    bucket's all-reduce starts) while the layers below are still in backward.  The fp32 residual-stream gradient travels
    through autograd; its bf16 twin - what the next dgrad / wgrad GEMMs read - travels beside it (_hand_upstream)."""

    @staticmethod
    def forward(ctx, geo: _Geometry, i: int, x: Tensor, *weights: Tensor):
        wb, wt, adapters = _layer_operands(geo, i, weights, x.shape[0])
        x_out, acts = _layer_forward(geo, i, x, wb, geo.save)
        if geo.save:
            # gradient checkpointing (ref: supports_gradient_checkpointing, TF GradientCheckpointingLayer): keep only the
            # layer input; its activations are recomputed by the same kernels (bit-identical) in the backward pass
            ctx.saved = (x,) if geo.checkpoint else acts
            ctx.geo, ctx.i, ctx.wb, ctx.wt, ctx.lora = geo, i, wb, wt, adapters
            ctx.wdtypes = [w.dtype for w in weights]
        return x_out

    @staticmethod
    def _backward_bf16(ctx, dy: Tensor):
        """The backward on the bf16 residual stream (train_residual_dtype; never with a dropout plan): the launch sequence of
        backward() below with ONE bf16 gradient tensor g where that one carries an fp32 tensor and its bf16 twin.  g is what the
        dgrad / wgrad GEMMs read, and each LayerNorm backward replaces it by bf16(g + LN'(dy)) - fp32 sum, one rounding (torch's bf16
        LayerNorm backward rounds LN'(dy) first and the sum again; the single rounding is the more accurate of the two)."""
        geo, i = ctx.geo, ctx.i
        need = ctx.needs_input_grad  # (geo, i, x, *weights)
        assert not any(a is not None for a in ctx.lora)  # (refused before the forward ran: CM3PEncoder._bf16_stream)
        (n_an, n_qkv, n_o, n_mn, n_i, n_o2), _ = _backward_needs(i, need[3:], ctx.lora)
        g = _take_bf16_from_downstream(geo, dy)
        if geo.checkpoint:
            _, acts = _layer_forward(geo, i, ctx.saved[0], ctx.wb, True)
        else:
            acts = ctx.saved
        x, xn, mean_a, rstd_a, qkv, o, lse, x_mid, xn2, mean_m, rstd_m, h, ga = acts
        del acts
        ctx_wb = ctx.wb
        w_an, Wqkv_b, Wo_b, w_mn, Wi_b, Wo2_b = ctx_wb[:6]
        Wqkv_t, Wo_t, Wi_t, Wo2_t = ctx.wt
        ctx.saved = ctx.wb = ctx.wt = None  # release activations as we go
        # ---- MLP branch: x_out = x_mid + g Wo2^T
        fused = len(ctx_wb) > 7 and ctx_wb[7]  # h is h' (interleaved columns): the Wo2 dgrad's store phase turns dg into the canonical dh
        dg = None if fused else K.linear_dgrad(g, Wo2_b, Wo2_t)
        dWo2 = K.linear_wgrad(g, ga) if n_o2 else None
        dh = K.linear_dgrad_geglu_bwd(g, Wo2_t, h) if fused else K.geglu_bwd(dg, h)
        del dg, ga
        dxn2 = K.linear_dgrad(dh, Wi_b, Wi_t)
        dWi = K.linear_wgrad(dh, xn2) if n_i else None
        del dh, h, xn2
        _, g, dw_mn = K.layernorm_bwd(dxn2, x_mid, w_mn, mean_m, rstd_m, g, False, bf16_only=True)
        del dxn2, x_mid
        # ---- attention branch: x_mid = x + o Wo^T
        do = K.linear_dgrad(g, Wo_b, Wo_t)
        dWo = K.linear_wgrad(g, o) if n_o else None
        dqkv = _attn_backward(geo, i, qkv, o, do, lse, None)
        del do, o, qkv
        dWqkv = K.linear_wgrad(dqkv, xn) if n_qkv else None
        dw_an = None
        if i == 0:
            if need[2]:  # layer 0 has no attn_norm: bf16(g + dxn) of two bf16 operands, one rounding
                _, g = K.add_f32(g, K.linear_dgrad(dqkv, Wqkv_b, Wqkv_t))
            _hand_upstream(geo, g, g)
        elif need[2] or n_an:
            dxn = K.linear_dgrad(dqkv, Wqkv_b, Wqkv_t)
            _, g, dw_an = K.layernorm_bwd(dxn, x, w_an, mean_a, rstd_a, g, False, bf16_only=True)
            _hand_upstream(geo, g, g)
        # (else: everything below this layer is frozen: the chain ends here)
        out = _weight_grads(i, dw_an, [dWqkv, dWo, dw_mn, dWi, dWo2], ctx.wdtypes, need[3:])
        return (None, None, g if need[2] else None, *out)

    @staticmethod
    def backward(ctx, dy: Tensor):
        if ctx.geo.bf16:
            return _EncoderLayerFn._backward_bf16(ctx, dy)
        geo, i = ctx.geo, ctx.i
        need = ctx.needs_input_grad  # (geo, i, x, *weights, *adapter tensors)
        (n_an, n_qkv, n_o, n_mn, n_i, n_o2), lora_grads = _backward_needs(i, need[3:], ctx.lora)
        live = list(_take_from_downstream(geo, dy))
        acts = _layer_forward(geo, i, ctx.saved[0], ctx.wb, True)[1] if geo.checkpoint else ctx.saved
        x, xn, mean_a, rstd_a, qkv, o, lse = acts[:7]
        live += acts[7:]
        del acts
        wb, wt = ctx.wb, ctx.wt
        ctx.saved = ctx.wb = ctx.wt = None  # release activations as we go
        gx32, do, dWo, dw_mn, dWi, dWo2, l_o, l_i, l_o2 = _post_attn_backward(geo, i, live, o, wb, wt, (n_o, n_i, n_o2), lora_grads)
        dqkv = _attn_backward(geo, i, qkv, o, do, lse, _attn_drop(geo, i))
        del do, o, qkv
        dWqkv, l_qkv, dw_an, gx = _pre_attn_backward(geo, i, dqkv, lambda: gx32, (x, xn, mean_a, rstd_a), wb, wt[0], need[2], n_an, n_qkv, lora_grads)
        out = _weight_grads(i, dw_an, [dWqkv, dWo, dw_mn, dWi, dWo2, *l_qkv, *l_o, *l_i, *l_o2], ctx.wdtypes, need[3:])
        return (None, None, gx if need[2] else None, *out)


class _FinalNormFn(torch.autograd.Function):
    """final_norm of the stack (TF:...modeling_modernbert.py:472): x [T,H] fp32 -> LayerNorm(x) fp32 (bf16 -> bf16 on the bf16
    residual stream); its backward starts the chain of bf16 gradient twins."""

    @staticmethod
    def forward(ctx, geo: _Geometry, x: Tensor, norm_w: Tensor):
        w = _f32(norm_w.detach())
        if geo.bf16:
            _, y, mean, rstd = K.layernorm_fwd(x, w, geo.eps, False, True, geo.save)
            if geo.save:  # (a training step on the bf16 stream, train_residual_dtype)
                ctx.geo, ctx.pack, ctx.wdtype = geo, (x, w, mean, rstd), norm_w.dtype
            return y
        y, _, mean, rstd = K.layernorm_fwd(x, w, geo.eps, True, False, geo.save)
        if geo.save:
            ctx.geo, ctx.pack, ctx.wdtype = geo, (x, w, mean, rstd), norm_w.dtype
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, w, mean, rstd = ctx.pack
        if ctx.geo.bf16:  # the chain's single bf16 gradient starts here: bf16(LN'(dy)), one rounding
            _, g, dw = K.layernorm_bwd(dy.to(torch.bfloat16).contiguous(), x, w, mean, rstd, None, False, inplace=False, bf16_only=True)
            ctx.pack = None
            _hand_upstream(ctx.geo, g, g)
            return None, g if ctx.needs_input_grad[1] else None, dw.to(ctx.wdtype) if ctx.needs_input_grad[2] else None
        gx32, gx16, dw = K.layernorm_bwd(dy.contiguous(), x, w, mean, rstd, None, True, inplace=False)
        ctx.pack = None
        _hand_upstream(ctx.geo, gx32, gx16)
        return None, gx32 if ctx.needs_input_grad[1] else None, dw.to(ctx.wdtype) if ctx.needs_input_grad[2] else None


def _zero_padded_rows(t: Tensor, rows: int) -> Tensor:
    """t [n, C] -> [rows, C] with zero rows behind (a copy, no arithmetic): a row block whose row count is not a multiple of 8 is filled
    up for the GEMMs; zero rows change no sum."""
    if t.shape[0] == rows:
        return t
    out = t.new_zeros((rows, t.shape[1]))
    out[:t.shape[0]].copy_(t)
    return out


class _TakeRowsFn(torch.autograd.Function):
    """x [R, H] fp32 or bf16 -> x[idx]; backward scatters into zeros (rows of x's dtype both ways)."""

    @staticmethod
    def forward(ctx, x: Tensor, idx: Tensor):
        ctx.idx, ctx.rows = idx, x.shape[0]
        return K.gather_rows(x.contiguous(), idx)

    @staticmethod
    def backward(ctx, dy: Tensor):
        return K.scatter_rows(dy.contiguous(), ctx.idx, ctx.rows), None


class _RowSel:
    """The query rows of the last layer's row node (_LastLayerRowsFn), and what differs between its two kinds as data: idx int64 [n] -
    the rows in the numbering of the stack's row axis (the packed rows on unpadded execution) -, n their count, attn_fwd / attn_bwd the
    attention pair with q, the arguments that describe the queries to it, and pad_rows(n, H, I), the rows the block is filled up to."""

    __slots__ = ("idx", "n", "q", "attn_fwd", "attn_bwd", "pad_rows")

    def __init__(self, idx: Tensor, q: tuple, attn_fwd, attn_bwd, pad_rows):
        self.idx, self.n, self.q, self.attn_fwd, self.attn_bwd, self.pad_rows = idx, idx.numel(), q, attn_fwd, attn_bwd, pad_rows

    @classmethod
    def listed(cls, idx: Tensor, qcu: Tensor, qmax: int) -> "_RowSel":
        """A validated list (CM3PEncoder.forward's last_layer_rows): qcu int32 [sequences + 1] its split by sequence, qmax the largest
        per-sequence count; attention for the listed queries on the matrix cores (csrc/attention_qrows.hip), the block filled up to
        K.row_block_rows."""
        return cls(idx, (idx.to(torch.int32), qcu, int(qmax)), K.attn_qrows_fwd, K.attn_qrows_bwd, K.row_block_rows)

    @classmethod
    def first_rows(cls, qidx: Tensor) -> "_RowSel":
        """Row 0 of every sequence (cls_only_last_layer; qidx: their row numbers): one query per (sequence, head)
        (csrc/attention_row.hip), the block filled up to a multiple of 8."""
        return cls(qidx, (), K.attn_row_fwd, K.attn_row_bwd, lambda n, H, I: (n + 7) // 8 * 8)


class _LastLayerRowsFn(torch.autograd.Function):
    """The LAST encoder layer where only some rows are consumed - row 0 of every sequence (CM3PEncoder.cls_only_last_layer) or a list
    (CM3PEncoder.forward's last_layer_rows: the CLS rows and the rows that carry a masked-LM label); `sel` says which and carries what
    the two differ in: x [T, H] + the layer's weights -> the layer's output on those rows alone, [n, H] (fp32; bf16 on the bf16 residual
    stream of a forward-only call).

    attn_norm and the Wqkv + RoPE projection run on all T rows - K and V come from every token - (_pre_attn_forward); attention runs
    for the query rows against all keys (sel.attn_fwd); the residual rows of the queries are gathered and Wo + residual, mlp_norm, Wi,
    GeGLU and Wo2 + residual run on n rows (_post_attn_forward; zero rows fill the block up to sel.pad_rows).  The same function of the
    same weights as _EncoderLayerFn followed by a row selection.  The backward mirrors it: the block's chain, sel.attn_bwd (dqkv in the
    full layout, its q third zero off the query rows, dk / dv summed over the queries) into the Wqkv weight and input gradients
    unchanged, and a residual-stream gradient that is zero except on the query rows into attn_norm's backward.
    No dropout, no adapters on this layer, no checkpointing, fp32 stream when a backward is recorded: _run_stack sends every other
    call through the full layer."""

    @staticmethod
    def forward(ctx, geo: _Geometry, i: int, x: Tensor, sel: _RowSel, *weights: Tensor):
        wb, wt, adapters = _layer_operands(geo, i, weights, None)
        xn, mean_a, rstd_a, qkv = _pre_attn_forward(geo, i, x, wb, geo.save)
        o, lse = sel.attn_fwd(qkv, *sel.q, geo.key_mask, geo.cu, geo.B, geo.max_s, geo.nh, geo.windows[i], geo.hd ** -0.5, prescaled=True)
        n, Np = sel.n, sel.pad_rows(sel.n, geo.H, geo.I)
        o_p = _zero_padded_rows(o, Np)
        x_out, post = _post_attn_forward(geo, i, o_p, _zero_padded_rows(K.gather_rows(x, sel.idx), Np), wb, geo.save)
        if geo.save:
            ctx.saved = (x, xn, mean_a, rstd_a, qkv, o, lse, o_p, *post)
            ctx.geo, ctx.i, ctx.sel, ctx.wb, ctx.wt, ctx.lora = geo, i, sel, wb, wt, adapters
            ctx.wdtypes = [w.dtype for w in weights]
        return x_out[:n] if Np != n else x_out

    @staticmethod
    def backward(ctx, dy: Tensor):
        geo, i, sel, n = ctx.geo, ctx.i, ctx.sel, ctx.sel.n
        need = ctx.needs_input_grad  # (geo, i, x, sel, *weights)
        (n_an, n_qkv, n_o, n_mn, n_i, n_o2), lora_grads = _backward_needs(i, need[4:], ctx.lora)
        gx32, gx16 = _take_from_downstream(geo, dy)
        x, xn, mean_a, rstd_a, qkv, o, lse, o_p = ctx.saved[:8]
        # ---- the row block: x_out = x_mid + g Wo2^T, x_mid = x[idx] + o Wo^T; its output gradient is filled up with zero rows like it
        live = [_zero_padded_rows(gx32, o_p.shape[0]), _zero_padded_rows(gx16, o_p.shape[0]), *ctx.saved[8:]]
        del gx32, gx16
        wb, wt = ctx.wb, ctx.wt
        ctx.saved = ctx.wb = ctx.wt = None
        gblock, do, dWo, dw_mn, dWi, dWo2 = _post_attn_backward(geo, i, live, o_p, wb, wt, (n_o, n_i, n_o2), lora_grads)[:6]
        del o_p
        # ---- all rows: dqkv in the full layout (q third zero off the query rows), then what every layer does with it; the residual
        # stream's own gradient is zero except on the query rows
        dqkv = sel.attn_bwd(qkv, o, do[:n].contiguous(), lse, *sel.q, geo.key_mask, geo.cu, geo.B, geo.max_s, geo.nh, geo.windows[i], geo.hd ** -0.5,
                            geo.rope[i], geo.per_batch_pos, prescaled=True)
        del do, o, qkv
        dWqkv, _, dw_an, gfull = _pre_attn_backward(geo, i, dqkv, lambda: K.scatter_rows(gblock[:n].contiguous(), sel.idx, x.shape[0]),
                                                    (x, xn, mean_a, rstd_a), wb, wt[0], need[2], n_an, n_qkv, lora_grads)
        out = _weight_grads(i, dw_an, [dWqkv, dWo, dw_mn, dWi, dWo2], ctx.wdtypes, need[4:])
        return (None, None, gfull if need[2] else None, None, *out)


class _EmbedLNFn(torch.autograd.Function):
    """LayerNorm(tok_embeddings[ids]) with optional audio rows scattered over the placeholder tokens
    (TF:...modeling_modernbert.py:64-71, ref:cm3p/modeling_cm3p.py:592,603-605).  bf16: the bf16 output alone (the bf16 residual
    stream; no fp32 rows are written).  The backward takes the stream's gradient in its dtype (fp32 or bf16); its results are fp32."""

    @staticmethod
    def forward(ctx, ids: Tensor, table: Tensor, norm_w: Tensor, eps: float, padding_idx: int, slot: Optional[Tensor],
                audio_rows: Optional[Tensor], bf16: bool = False):
        w = _f32(norm_w.detach())
        tab = table.detach()
        ar = audio_rows.detach().contiguous() if audio_rows is not None else None
        if bf16:  # (the statistics are written either way; a training step on the bf16 stream keeps them for the backward)
            _, y, mean, rstd = K.embed_ln_fwd(ids, tab, w, eps, slot, ar, want_bf16=True, want_f32=False)
        else:
            y, _, mean, rstd = K.embed_ln_fwd(ids, tab, w, eps, slot, ar)
        ctx.pack = (ids, tab, w, mean, rstd, slot, ar, padding_idx)
        ctx.dtypes = (table.dtype, norm_w.dtype, audio_rows.dtype if audio_rows is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        ids, tab, w, mean, rstd, slot, ar, padding_idx = ctx.pack
        d_table, d_audio, dw = K.embed_ln_bwd(dy.contiguous(), ids, tab, w, mean, rstd, padding_idx, slot, ar,
                                              want_table_grad=ctx.needs_input_grad[1])
        td, wd, ad = ctx.dtypes
        if d_table is not None and d_table.dtype != td:
            d_table = d_table.to(td)
        if d_audio is not None and d_audio.dtype != ad:
            d_audio = d_audio.to(ad)
        return None, d_table, dw.to(wd), None, None, None, d_audio, None


class _DropPlan:
    """The dropout of one stack forward in training mode: one seed (regenerates every mask in the backward and in a checkpointed
    recompute) and the thresholds round(p * 65536) of the live sites (0: site off)."""

    __slots__ = ("seed", "embedding", "attn", "mlp")

    def __init__(self, seed: int, embedding: int, attn: int, mlp: int):
        self.seed, self.embedding, self.attn, self.mlp = seed, embedding, attn, mlp


class _EmbedDropFn(torch.autograd.Function):
    """ModernBertEmbeddings.drop (TF:...modeling_modernbert.py:70) on [rows, H] fp32: x o Z; backward dy o Z (same mask)."""

    @staticmethod
    def forward(ctx, x: Tensor, plan: _DropPlan, S: int, cu: Optional[Tensor]):
        ctx.args = (plan.embedding, plan.seed, S, cu)
        return K.dropout_f32(x.contiguous(), plan.embedding, plan.seed, 0, K.SITE_EMBED, S, cu)

    @staticmethod
    def backward(ctx, dy: Tensor):
        thr, seed, S, cu = ctx.args
        return K.dropout_f32(dy.float().contiguous(), thr, seed, 0, K.SITE_EMBED, S, cu), None, None, None


class _PadRowsFn(torch.autograd.Function):
    """Packed rows -> padded [rows, H] with zeros at the padding positions (ref:cm3p/modeling_cm3p.py:106-134 _pad_cm3p_output);
    backward gathers the rows back."""

    @staticmethod
    def forward(ctx, y: Tensor, idx: Tensor, n_valid: int, rows: int):
        ctx.idx, ctx.n_valid, ctx.packed_rows = idx, n_valid, y.shape[0]
        return K.scatter_rows(y[:n_valid].contiguous() if n_valid != y.shape[0] else y.contiguous(), idx, rows)

    @staticmethod
    def backward(ctx, dy: Tensor):
        g = K.gather_rows(dy.contiguous(), ctx.idx)
        if ctx.packed_rows != ctx.n_valid:  # alignment rows of the packed layout take no gradient
            g = torch.cat((g, torch.zeros((ctx.packed_rows - ctx.n_valid, g.shape[1]), dtype=g.dtype, device=g.device)))
        return g, None, None, None


class _LayerNormFn(torch.autograd.Function):
    """Plain LayerNorm of given rows (the `inputs_embeds` entry of ModernBertEmbeddings, TF:...modeling_modernbert.py:67-68).
    bf16: the bf16 output alone (the bf16 residual stream of a forward-only call)."""

    @staticmethod
    def forward(ctx, x: Tensor, norm_w: Tensor, eps: float, bf16: bool = False):
        w = _f32(norm_w.detach())
        xd = x.detach().contiguous()
        if bf16:
            want = any(ctx.needs_input_grad[:2])  # (a training step on the bf16 stream: the statistics its backward reads)
            _, y, mean, rstd = K.layernorm_fwd(xd, w, eps, False, True, want)
        else:
            y, _, mean, rstd = K.layernorm_fwd(xd, w, eps, True, False)
        ctx.pack = (xd, w, mean, rstd)
        ctx.dtypes = (x.dtype, norm_w.dtype)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        xd, w, mean, rstd = ctx.pack
        x32 = xd if xd.dtype == torch.float32 else xd.float()
        dx, _, dw = K.layernorm_bwd(dy.contiguous(), x32, w, mean, rstd, None, False, inplace=False)
        return (dx if ctx.dtypes[0] == torch.float32 else dx.to(ctx.dtypes[0])), dw.to(ctx.dtypes[1]), None, None


class CM3PEncoder(nn.Module):
    """Drop-in for the `ModernBertModel` member of the reference towers (same submodule / parameter names)."""

    def __init__(self, config):
        super().__init__()
        _check_supported(config)
        self.config = config
        self.embeddings = CM3PEmbeddingParams(config)
        self.layers = nn.ModuleList([CM3PEncoderLayerParams(config, i) for i in range(config.num_hidden_layers)])
        self.final_norm = nn.LayerNorm(config.hidden_size, eps=config.norm_eps, bias=False)
        self.gradient_checkpointing = False  # set by PreTrainedModel.gradient_checkpointing_enable()
        self.residual_dtype = None  # None / torch.float32: fp32 residual stream; torch.bfloat16: bf16 on forward-only calls
        self.train_residual_dtype = None  # the same choice for calls that record a backward (training steps)
        self.cls_only_last_layer = False  # opt-in: the last layer (and the final norm) on row 0 of every sequence only
        self._inv_freq_cache = {}
        # init roles (TF:...modeling_modernbert.py:372-386): 'in'/'embedding' std = initializer_range,
        # 'out' std = initializer_range / sqrt(2 L); consumed by CM3PPreTrainedModel._init_weights
        cutoff = config.initializer_cutoff_factor or 3
        std_in = config.initializer_range
        std_out = config.initializer_range / (2.0 * config.num_hidden_layers) ** 0.5
        self.embeddings.tok_embeddings._cm3p_init = (std_in, cutoff)
        for layer in self.layers:
            layer.attn.Wqkv._cm3p_init = (std_in, cutoff)
            layer.attn.Wo._cm3p_init = (std_out, cutoff)
            layer.mlp.Wi._cm3p_init = (std_in, cutoff)
            layer.mlp.Wo._cm3p_init = (std_out, cutoff)

    @property
    def residual_dtype(self) -> Optional[torch.dtype]:
        """dtype of the residual stream on forward-only calls: None or torch.float32 (the default) keep it fp32; torch.bfloat16 runs
        it in bf16 as a bf16 model of the reference does under no_grad (every LayerNorm reads and writes bf16, the residual adds are
        bf16 adds of the bf16-rounded projections, last_hidden_state and hidden_states are bf16).  Applies only to calls that record
        nothing for a backward and have no dropout plan; training steps and calls with grad enabled on trainable parameters or inputs
        (those follow `train_residual_dtype`) and train-mode calls with dropout p > 0 run the fp32 stream bit for bit as with None.
        Not part of the state dict or config."""
        return self._residual_dtype

    @residual_dtype.setter
    def residual_dtype(self, dtype) -> None:
        if dtype is not None and dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"residual_dtype must be None, torch.float32 or torch.bfloat16, got {dtype!r}")
        self._residual_dtype = dtype

    @property
    def train_residual_dtype(self) -> Optional[torch.dtype]:
        """dtype of the residual stream on calls that record a backward (training steps, fine-tuning with part of the tower frozen):
        None or torch.float32 (the default) keep it fp32; torch.bfloat16 runs the forward of `residual_dtype` and a backward whose
        residual-stream gradient is one bf16 tensor (see the module docstring).  Master weights keep their dtype (fp32 masters with a
        bf16 stream is the expected use); weight gradients have the parameter's dtype.  Limitation: a call with a dropout plan (train
        mode, any dropout p > 0) runs the fp32 stream bit for bit as with None - the dropout sites have no bf16 form.  Calls that
        record nothing follow `residual_dtype`, not this attribute.  Not part of the state dict or config."""
        return self._train_residual_dtype

    @train_residual_dtype.setter
    def train_residual_dtype(self, dtype) -> None:
        if dtype is not None and dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"train_residual_dtype must be None, torch.float32 or torch.bfloat16, got {dtype!r}")
        self._train_residual_dtype = dtype

    @property
    def cls_only_last_layer(self) -> bool:
        """Opt-in for callers whose only consumer of this encoder is the pooled CLS row h[:, 0] (`cls_embed: true` towers, a
        `classifier_pooling == "cls"` head): the last layer and the final norm are computed for row 0 of every sequence only.
        The encoder then returns `(B, 1, H)` for padded and `unpad` calls and `(Bn, H)` - one row per sequence of `cu_seqlens` - for
        caller-packed rows; with `output_hidden_states` the last entry is that short tensor and the others are unchanged.  The rows are
        the same function of the same weights as row 0 of the full result: attn_norm and the Wqkv + RoPE projection still run on
        every token (K and V come from all of them), attention is one query per (sequence, head) (csrc/attention_row.hip), and
        Wo, mlp_norm, the GeGLU MLP and the final norm run on B rows (_LastLayerRowsFn on _RowSel.first_rows).  Supported on that route: the fp32 stream
        (forward-only and training), the bf16 stream of forward-only calls, padded execution, `unpad`, caller-packed rows.
        Where the row route has no form - an active dropout plan, adapters on the last layer, the bf16 stream of a training step,
        head_dim other than 64, gradient checkpointing - the full layer runs and its row 0 is taken, so the output SHAPE does not
        depend on the route (and the values are those of the switch-off call, bit for bit).  `output_attentions` raises
        NotImplementedError.  Consumers of all rows (mean pooling, an MLM or decoder head) must leave the switch off; the model classes
        refuse such calls.  Not part of the state dict or config; off by default, and off changes nothing."""
        return self._cls_only_last_layer

    @cls_only_last_layer.setter
    def cls_only_last_layer(self, value) -> None:
        self._cls_only_last_layer = bool(value)

    def _bf16_stream(self, plan: Optional[_DropPlan], *inputs: Optional[Tensor]) -> bool:
        """Whether this call runs the bf16 residual stream: there is no dropout plan, and the switch of the call's kind is set -
        `residual_dtype` when nothing will be recorded for a backward (the rule _run_stack applies to geo.save, decided before the
        embedding runs), `train_residual_dtype` when something will."""
        if plan is not None:
            return False
        records = torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters()))
        if records and self._train_residual_dtype is torch.bfloat16 and self.has_lora():
            raise NotImplementedError("cm3p_amd LoRA: a training call on the bf16 residual stream (train_residual_dtype = torch.bfloat16) is not "
                                      "supported with adapters attached; set train_residual_dtype back to None, or merge_lora() / remove_lora() first")
        return (self._train_residual_dtype if records else self._residual_dtype) is torch.bfloat16

    def train(self, mode: bool = True):
        if mode != self.training:
            invalidate_weight_cache()  # HF Trainer flips the mode around every evaluation: copies never cross a train/eval boundary
        return super().train(mode)

    def _dropout_plan(self) -> Optional[_DropPlan]:
        """-> the dropout of this call, or None: eval mode or every p = 0 (then the launch sequence is exactly the dropout-free one).
        The seed comes from torch's default CPU generator (torch.manual_seed / transformers' set_seed make runs reproducible): a
        host draw, no device sync."""
        cfg = self.config
        p_emb, p_attn, p_mlp = (float(getattr(cfg, n, 0.0) or 0.0) for n in ("embedding_dropout", "attention_dropout", "mlp_dropout"))
        if not self.training or (p_emb == 0.0 and p_attn == 0.0 and p_mlp == 0.0):
            return None
        _check_supported(cfg)  # (the fields are read per call: a value set after construction is held to the same rules)
        hd = cfg.hidden_size // cfg.num_attention_heads
        if p_attn > 0.0 and hd in K.HD_MFMA_SIZES:
            raise NotImplementedError(f"attention_dropout > 0 in training mode at head_dim {hd}: the head_dim 96 / 128 attention kernels have no "
                                      "dropout form (embedding and MLP dropout work)")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("dropout in training mode inside a CUDA-graph capture: the host-drawn seed would be frozen into the graph")
        seed = int(torch.randint(-(2 ** 63), 2 ** 63 - 1, (), dtype=torch.int64)) & (2 ** 64 - 1)
        thr = [K.dropout_threshold(p) if p > 0.0 else 0 for p in (p_emb, p_attn, p_mlp)]
        return _DropPlan(seed, *thr)

    @staticmethod
    def _embed_dropout(x0: Tensor, plan: Optional[_DropPlan], S: int, cu: Optional[Tensor]) -> Tensor:
        if plan is None or not plan.embedding:
            return x0
        return _EmbedDropFn.apply(x0, plan, S, cu)

    def get_input_embeddings(self):
        return self.embeddings.tok_embeddings

    def set_input_embeddings(self, value):
        self.embeddings.tok_embeddings = value

    def _inv_freq(self, theta: float, device) -> Tensor:
        key = (float(theta), str(device))
        if key not in self._inv_freq_cache:
            # TF:...modeling_modernbert.py:141, evaluated on the host exactly as the reference does
            hd = self.config.hidden_size // self.config.num_attention_heads
            inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))
            self._inv_freq_cache[key] = inv.to(device)
        return self._inv_freq_cache[key]

    def _stack_weights(self):
        """Per layer: [attn_norm (layers > 0)], Wqkv, Wo, mlp_norm, Wi, Wo(mlp) - the argument order of _EncoderLayerFn."""
        ws = []
        for i, layer in enumerate(self.layers):
            w = [layer.attn_norm.weight] if i > 0 else []
            ws.append(w + [layer.attn.Wqkv.weight, layer.attn.Wo.weight, layer.mlp_norm.weight, layer.mlp.Wi.weight, layer.mlp.Wo.weight])
        return ws

    def _stack_lora(self):
        """Per layer: the adapters (A, B, s) or None of Wqkv, Wo, Wi, Wo(mlp); None when the stack carries no adapter at all."""
        ad = [[lora_of(lin) for lin in (layer.attn.Wqkv, layer.attn.Wo, layer.mlp.Wi, layer.mlp.Wo)] for layer in self.layers]
        return ad if any(a is not None for row in ad for a in row) else None

    def has_lora(self) -> bool:
        return self._stack_lora() is not None

    def forward(self, input_ids: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None,
                position_ids: Optional[Tensor] = None, inputs_embeds: Optional[Tensor] = None,
                audio_slot: Optional[Tensor] = None, audio_rows: Optional[Tensor] = None, unpad: bool = False,
                output_hidden_states: bool = False, cu_seqlens: Optional[Tensor] = None, max_seqlen: Optional[int] = None,
                output_attentions: bool = False, last_layer_rows: Optional[Tensor] = None):
        """-> last_hidden_state (B, S, H) fp32 (bf16 on the bf16 residual stream, see residual_dtype) [, tuple of L+1 detached hidden states (the stack's input and every layer's output,
        TF:...modeling_modernbert.py:457-470) when output_hidden_states].  Exactly one of input_ids / inputs_embeds.
        output_attentions: -> (last_hidden_state, hidden states or None, tuple of L attention-probability tensors (B, nh, S, S) fp32,
        detached): what the reference returns as `attentions` (TF runs its eager attention for such a call); padded execution only.

        unpad: run the stack on the valid tokens only, packed back to back (what the reference's flash_attention_2 path does,
        ref:cm3p/modeling_cm3p.py:911-931); padding positions of the result are zero.  Used when the mask is a right-padded
        one with at least one padded position; otherwise the padded path runs (same values on the valid positions).

        last_layer_rows: an int64 device tensor [n] of strictly ascending GLOBAL row numbers (b * S + position of a (B, S) batch, with
        or without `unpad`; the packed row with `cu_seqlens`) for callers that consume only those rows of the result - the CLS rows and
        the rows that carry a masked-LM label.  The last layer and the final norm are computed for them alone and the output is
        (n, H), in list order; with `output_hidden_states` the last entry is that short tensor.  The same function of the same
        weights as those rows of the full result: attn_norm and the Wqkv + RoPE projection still run on every token, attention
        runs for the listed queries against all keys (csrc/attention_qrows.hip), Wo, mlp_norm, the GeGLU MLP and the final norm on n
        rows (_LastLayerRowsFn on _RowSel.listed).  ONE host read validates the list (ascending, in range, with `unpad` every row on a valid token)
        and gives the grid its size; a wrong list raises ValueError.  Where the row route has no form - the cases cls_only_last_layer
        names - the full layer runs and the rows are gathered: the output shape does not depend on the route.  Wins over
        cls_only_last_layer when both are given.  `output_attentions` with it raises NotImplementedError."""
        cfg = self.config
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        if cfg.hidden_size // cfg.num_attention_heads != 64:
            # the generic attention kernels (head_dim 16 / 32) and the wide-head ones (96 / 128) know the padded layout only
            if cu_seqlens is not None:
                raise NotImplementedError("unpadded inputs need head_dim 64 (the generic attention kernels run padded batches)")
            if output_attentions:
                raise NotImplementedError("output_attentions needs head_dim 64")
            unpad = False
        cls_only = self._cls_only_last_layer and last_layer_rows is None  # (the explicit argument wins)
        if last_layer_rows is not None and output_attentions:
            raise NotImplementedError("output_attentions with last_layer_rows: the last layer computes the listed queries only, there is no "
                                      "(B, nh, S, S) probability tensor for it")
        if cls_only and output_attentions:
            raise NotImplementedError("output_attentions with cls_only_last_layer: the last layer computes one query per sequence, there is no "
                                      "(B, nh, S, S) probability tensor for it; switch cls_only_last_layer off for such a call")
        plan = self._dropout_plan()  # (before any launch: a refused graph capture has captured nothing)
        if output_attentions and plan is not None and plan.attn:
            raise NotImplementedError("output_attentions with attention dropout in training mode (the kernels return undropped probabilities)")
        bf16 = self._bf16_stream(plan, inputs_embeds, audio_rows)
        if cu_seqlens is not None:
            if output_attentions:
                raise NotImplementedError("output_attentions with unpadded inputs: attention probabilities are (B, nh, S, S) tensors of a padded batch")
            return self._forward_prepacked(input_ids, position_ids, audio_slot, audio_rows, cu_seqlens, max_seqlen, output_hidden_states, plan, bf16,
                                           cls_only, last_layer_rows)
        if output_attentions:
            unpad = False  # the probabilities are laid out per padded (batch, head, query, key)
        if input_ids is not None and input_ids.dtype != torch.int64:
            input_ids = input_ids.to(torch.int64)  # nn.Embedding takes IntTensor or LongTensor; the kernels index with int64
        ref = input_ids if input_ids is not None else inputs_embeds
        if not ref.is_cuda:
            raise RuntimeError("cm3p_amd runs on MI355X only: inputs must be CUDA/HIP tensors (no CPU fallback)")
        B, S = ref.shape[0], ref.shape[1]
        H = cfg.hidden_size
        dev = ref.device

        packed = None
        if unpad and attention_mask is not None and input_ids is not None:
            packed = self._plan_unpadded(attention_mask.reshape(B, S), position_ids)

        sel = None
        if last_layer_rows is not None:  # (before any launch of the stack: a wrong list has computed nothing)
            sel = self._plan_last_layer_rows(last_layer_rows, B, S, B * S, packed[1] if packed is not None else None, repack=packed is not None)
        if packed is not None:
            idx, cu, max_s, n_valid, n_rows, pos = packed
            ids = input_ids.contiguous().view(-1)[idx]  # integer row selection (the reference's _unpad_cm3p_input)
            slot_p = None
            if audio_slot is not None:  # audio placeholders are valid tokens: their slot numbers travel with them
                slot_p = audio_slot.view(-1)[idx]
            if n_rows != n_valid:  # alignment rows: one extra pseudo-sequence of pad tokens, no gradient flows into it
                ids = torch.cat((ids, ids.new_zeros(n_rows - n_valid)))
                if slot_p is not None:
                    slot_p = torch.cat((slot_p, slot_p.new_full((n_rows - n_valid,), -1)))
            pad = self.embeddings.tok_embeddings.padding_idx
            x0 = _EmbedLNFn.apply(ids, self.embeddings.tok_embeddings.weight, self.embeddings.norm.weight, cfg.norm_eps,
                                  -1 if pad is None else pad, None if slot_p is None else slot_p.contiguous(), audio_rows, bf16)
        elif input_ids is not None:
            pad = self.embeddings.tok_embeddings.padding_idx
            x0 = _EmbedLNFn.apply(input_ids.contiguous().view(-1), self.embeddings.tok_embeddings.weight,
                                  self.embeddings.norm.weight, cfg.norm_eps, -1 if pad is None else pad, audio_slot, audio_rows, bf16)
        else:
            x0 = _LayerNormFn.apply(inputs_embeds.reshape(B * S, H), self.embeddings.norm.weight, cfg.norm_eps, bf16)

        x0 = self._embed_dropout(x0, plan, S, packed[1] if packed is not None else None)
        y, hiddens, attns = self._run_stack(x0, B, S, attention_mask, position_ids, packed, output_hidden_states, dev, output_attentions, plan, bf16,
                                            cls_only, sel)
        short = [hiddens.pop()] if ((cls_only or sel is not None) and hiddens is not None) else []  # (the last layer's output: short already)
        if hiddens is not None:
            if packed is not None:
                hiddens = [K.scatter_rows(h[:n_valid].contiguous(), idx, B * S) for h in hiddens]
            hiddens = tuple(h.view(B, S, H) for h in hiddens) + tuple(h if sel is not None else h.view(B, 1, H) for h in short)
        if cls_only:
            y = y.view(B, 1, H)
        elif sel is None:  # (with last_layer_rows y is (n, H), in list order, as it is)
            if packed is not None:
                y = _PadRowsFn.apply(y, idx, n_valid, B * S)
            y = y.view(B, S, H)
        if output_attentions:
            return y, hiddens, attns
        return (y, hiddens) if output_hidden_states else y

    def _run_stack(self, x0: Tensor, B: int, S: int, attention_mask, position_ids, packed, output_hidden_states: bool, dev,
                   output_attentions: bool = False, plan: Optional[_DropPlan] = None, bf16: bool = False, cls_only: bool = False,
                   sel: Optional[_RowSel] = None):
        """The L encoder layers + final norm on [rows, H]; `packed` = (idx, cu, max_s, n_valid, n_rows, pos) for unpadded execution;
        `plan`: the call's dropout (None: none); `bf16`: x0 is bf16 and the stream stays bf16 (_bf16_stream); `cls_only`: y and the last
        hidden state are the rows of query position 0 alone, [sequences, H] (cls_only_last_layer); `sel`: they are the listed rows alone, [n, H]
        (last_layer_rows; never together with cls_only)."""
        cfg = self.config
        H = cfg.hidden_size
        geo = _Geometry()
        geo.B, geo.S, geo.H, geo.I, geo.nh, geo.L = B, S, H, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers
        geo.hd = H // cfg.num_attention_heads
        geo.eps = cfg.norm_eps
        geo.windows = [-1 if cfg.is_global_layer(i) else cfg.half_window for i in range(geo.L)]
        geo.key_mask = None
        geo.cu = None
        geo.checkpoint = bool(self.gradient_checkpointing and self.training)
        geo.drop = plan
        geo.max_s = S
        if packed is not None:
            idx, cu, max_s, n_valid, n_rows, pos = packed
            geo.B = cu.numel() - 1  # (+1 when alignment rows form a pseudo-sequence)
            geo.S = max_s
            geo.cu, geo.max_s = cu, max_s
            geo.per_batch_pos = True  # rotary tables are per packed token
            pos_tok = pos
        else:
            if attention_mask is not None:
                # padding term of the reference mask depends on the key only (TF:masking_utils.py:168-179)
                geo.key_mask = (attention_mask.reshape(B, S) != 0).to(torch.uint8).contiguous()
            if position_ids is None:
                position_ids = torch.arange(S, device=dev).unsqueeze(0)
            geo.per_batch_pos = position_ids.shape[0] != 1
            if geo.per_batch_pos and position_ids.shape[0] != B:
                raise ValueError("position_ids must be (1, S) or (B, S)")
            pos_tok = position_ids.contiguous().to(torch.int64)
        tables = {}
        for is_global, theta in ((True, cfg.global_rope_theta), (False, cfg.local_rope_theta)):
            if any(cfg.is_global_layer(i) == is_global for i in range(geo.L)):
                tables[is_global] = K.rope_table(pos_tok, self._inv_freq(theta, dev))
        geo.rope = [tables[cfg.is_global_layer(i)] for i in range(geo.L)]
        weights = self._stack_weights()
        lora = self._stack_lora()
        geo.save = torch.is_grad_enabled() and (x0.requires_grad or self.final_norm.weight.requires_grad
                                                or any(w.requires_grad for ws in weights for w in ws)
                                                or (lora is not None and any(t.requires_grad for row in lora for a in row if a is not None for t in a[:2])))
        if bf16 and geo.save and (self._train_residual_dtype is not torch.bfloat16 or plan is not None):
            # (_bf16_stream applies the same rules before the embedding ran)
            raise RuntimeError("cm3p_amd: bf16 residual stream on a call that records a backward without train_residual_dtype, or with dropout")
        geo.bf16 = bf16
        # cls_only_last_layer: the row route where it has a form, else the full layer and a row selection behind the final norm
        has_route = geo.hd == 64 and plan is None and not geo.checkpoint and not (bf16 and geo.save) \
            and (lora is None or all(a is None for a in lora[geo.L - 1]))
        row_route = (cls_only or (sel is not None and sel.n > 0)) and has_route  # (an empty list: the full layer and an empty gather)
        if geo.save and _eval_weights:
            invalidate_weight_cache()  # a backward will follow, so an optimizer will: no copy made before this step may outlive it
        geo.wcast = None
        geo.fused_mlp = frozenset()
        geo.lora = geo.wcast_geglu = None
        adapted = {}  # id(weight) -> (weight, A, B, s) of the projections that carry an adapter
        if lora is not None:
            if bf16 and geo.save:
                raise NotImplementedError("cm3p_amd LoRA: a training call on the bf16 residual stream is not supported with adapters attached")
            geo.lora = [tuple(None if a is None else a[2] for a in row) for row in lora]
            for ws, row in zip(weights, lora):
                for w, a in zip((ws[-5], ws[-4], ws[-2], ws[-1]), row):
                    if a is not None:
                        _check_lora_operands(w, a[0], a[1])
                        adapted[id(w)] = (w, a[0], a[1], a[2])
        if adapted and not geo.save:
            # forward-only: the merged copies are kept across calls (keyed on W, A and B); a Wi whose GEMM stores GeGLU itself gets the
            # interleaved row order instead of the canonical one
            ents = [(w, A, B, s, False) for w, A, B, s in adapted.values()]
            for n, ws in enumerate(weights):
                if id(ws[-2]) in adapted and _geglu_fwd_fused(plan, x0.shape[0], ws[-2]):
                    k = [e[0] is ws[-2] for e in ents].index(True)
                    ents[k] = (*ents[k][:4], True)
            copies = _lora_merged_cached(ents)
            geo.wcast = {id(e[0]): (y, None) for e, y in zip(ents, copies) if not e[4]}
            geo.wcast_geglu = {id(e[0]): y for e, y in zip(ents, copies) if e[4]}
        if geo.save and (adapted or os.environ.get("CM3P_CAST_BATCHED", "1") != "0"):
            # bf16 copies + transposes of every projection weight of the stack in ONE launch (r03: 4 launches per layer); adapted weights
            # go through the merged form of that launch (K.lora_merge_cast_many) whatever CM3P_CAST_BATCHED says
            elig = [w for ws in weights for w in ws
                    if w.dim() == 2 and w.dtype == torch.float32 and w.shape[0] % 8 == 0 and w.shape[1] % 8 == 0 and w.is_contiguous()
                    and (id(w) in adapted or os.environ.get("CM3P_CAST_BATCHED", "1") != "0")]
            if adapted and any(id(w) not in {id(e) for e in elig} for w, *_ in adapted.values()):
                raise NotImplementedError("cm3p_amd LoRA: an adapted weight must be a contiguous fp32 matrix")
            if elig:
                # GeGLU in the store phases of the Wi GEMM and the Wo2 dgrad (K.linear_geglu_fwd / K.linear_dgrad_geglu_bwd): taken by the
                # layers whose Wi and Wo2 are cast here - the same launch then writes Wi's copy with interleaved rows; the canonical
                # copy is not needed, the Wi dgrad reads Wi^T - when no MLP dropout is planned and the library's route names the ring
                # for both calls.  CM3P_GEGLU_FUSED=0: the two-kernel path everywhere.
                if not (plan is not None and plan.mlp) and os.environ.get("CM3P_GEGLU_FUSED", "1") != "0" \
                        and K.mlp_geglu_fused_supported(x0.shape[0], cfg.intermediate_size, H):
                    cast = {id(w) for w in elig}
                    # (not the last layer on the row route: its Wi is a plain GEMM on B rows and reads the canonical copy)
                    geo.fused_mlp = frozenset(id(ws[-2]) for n, ws in enumerate(weights)
                                              if id(ws[-2]) in cast and id(ws[-1]) in cast and not (row_route and n == geo.L - 1))
                plain = [w for w in elig if id(w) not in adapted]
                pairs = K.cast_bf16_with_transpose_many([w.detach() for w in plain], [id(w) in geo.fused_mlp for w in plain])
                geo.wcast = {id(w): pair for w, pair in zip(plain, pairs)}
                merged = [adapted[id(w)] for w in elig if id(w) in adapted]
                pairs = K.lora_merge_cast_many([(w.detach(), A.detach().contiguous(), B.detach().contiguous(), s, id(w) in geo.fused_mlp) for w, A, B, s in merged])
                geo.wcast.update({id(e[0]): pair for e, pair in zip(merged, pairs)})
        n_seq = geo.B - (1 if (packed is not None and packed[4] != packed[3]) else 0)  # (without the pseudo-sequence of alignment rows)
        if cls_only:  # the row of query position 0 of every sequence (never together with a list: the explicit argument wins)
            sel = _RowSel.first_rows(geo.cu[:-1].to(torch.int64) if geo.cu is not None else torch.arange(B, device=dev, dtype=torch.int64) * S)
        geo.handoff = None
        geo.attn_out = [] if output_attentions else None
        # output_hidden_states: the stack's input and every layer's output (TF:...modeling_modernbert.py:457-470), detached
        hiddens = [x0.detach()] if output_hidden_states else None
        x = x0
        for i in range(geo.L):
            extra = () if lora is None else tuple(t for a in lora[i] if a is not None for t in a[:2])
            if row_route and i == geo.L - 1:
                x = _LastLayerRowsFn.apply(geo, i, x, sel, *weights[i])  # [sel.n, H]
            else:
                x = _EncoderLayerFn.apply(geo, i, x, *weights[i], *extra)
            if hiddens is not None:
                if sel is not None and i == geo.L - 1:  # the last layer's output on the query rows alone, whichever route made it
                    last = x.detach() if row_route else K.gather_rows(x.detach(), sel.idx)
                    hiddens.append(last[:n_seq] if cls_only else last)
                else:
                    hiddens.append(x.detach())
        y = _FinalNormFn.apply(geo, x, self.final_norm.weight)
        if sel is not None and not row_route:
            y = _TakeRowsFn.apply(y, sel.idx)
        if cls_only and n_seq != y.shape[0]:
            y = y[:n_seq]
        attns = tuple(geo.attn_out) if geo.attn_out is not None else None
        geo.attn_out = None
        return y, hiddens, attns

    def _forward_prepacked(self, input_ids: Tensor, position_ids: Optional[Tensor], audio_slot, audio_rows, cu_seqlens: Tensor,
                           max_seqlen: Optional[int], output_hidden_states: bool, plan: Optional[_DropPlan] = None, bf16: bool = False,
                           cls_only: bool = False, last_layer_rows: Optional[Tensor] = None):
        """Caller-supplied unpadded inputs (ref:cm3p/modeling_cm3p.py:911-931 when `indices` / `cu_seqlens` / `max_seqlen` are given;
        the layout of _unpad_cm3p_input, :65-104): input_ids (total,), cu_seqlens (batch + 1,) -> last_hidden_state (total, H),
        NOT re-padded (the reference's encoder leaves caller-packed rows packed as well)."""
        cfg = self.config
        if input_ids is None or input_ids.dim() != 1:
            raise ValueError("with cu_seqlens, input_ids must be the 1-D unpadded token tensor (total_nnz,)")
        if not input_ids.is_cuda:
            raise RuntimeError("cm3p_amd runs on MI355X only: inputs must be CUDA/HIP tensors (no CPU fallback)")
        dev = input_ids.device
        ids = input_ids.to(torch.int64).contiguous()
        total = ids.numel()
        cu = cu_seqlens.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if cu.numel() < 2:
            raise ValueError("cu_seqlens needs at least two entries (batch + 1)")
        lens = cu[1:] - cu[:-1]
        # ONE host read validates the description (a wrong cu_seqlens would send the kernels past the rows)
        first, last, mx, mn = torch.stack((cu[0], cu[-1], lens.max(), lens.min())).tolist()
        if first != 0 or last != total or mn <= 0:
            raise ValueError(f"cu_seqlens must start at 0, increase strictly and end at the token count ({total}); got end {last}, min length {mn}")
        max_s = int(mx) if max_seqlen is None else int(max_seqlen)
        if max_s < mx:
            raise ValueError(f"max_seqlen {max_s} is smaller than the longest sequence ({mx})")
        sel = None
        if last_layer_rows is not None:  # (rows of the packed axis; the pseudo-sequence of alignment rows added below owns none)
            sel = self._plan_last_layer_rows(last_layer_rows, cu.numel() - 1, max_s, total, cu, repack=False, n_seq=cu.numel() - 1 + (total % 64 != 0))
        n_rows = (total + 63) // 64 * 64  # alignment rows: one pseudo-sequence of pad tokens, no gradient flows into it
        if position_ids is None:
            pos = torch.arange(total, device=dev) - torch.repeat_interleave(cu[:-1].to(torch.int64), lens.to(torch.int64))
        else:
            pos = position_ids.reshape(-1).to(torch.int64)
            if pos.numel() != total:
                raise ValueError("position_ids must be unpadded like input_ids")
        slot_p = audio_slot
        if n_rows != total:
            ids = torch.cat((ids, ids.new_zeros(n_rows - total)))
            pos = torch.cat((pos, torch.arange(n_rows - total, device=dev)))
            cu = torch.cat((cu, cu.new_full((1,), n_rows)))
            if slot_p is not None:
                slot_p = torch.cat((slot_p, slot_p.new_full((n_rows - total,), -1)))
        pad = self.embeddings.tok_embeddings.padding_idx
        x0 = _EmbedLNFn.apply(ids, self.embeddings.tok_embeddings.weight, self.embeddings.norm.weight, cfg.norm_eps,
                              -1 if pad is None else pad, None if slot_p is None else slot_p.contiguous(), audio_rows, bf16)
        packed = (None, cu, max(max_s, n_rows - total), total, n_rows, pos.contiguous())
        x0 = self._embed_dropout(x0, plan, max_s, cu)
        y, hiddens, _ = self._run_stack(x0, cu.numel() - 1, max_s, None, None, packed, output_hidden_states, dev, plan=plan, bf16=bf16,
                                        cls_only=cls_only, sel=sel)
        if n_rows != total:
            short = cls_only or sel is not None
            if not short:
                y = y[:total]
            if hiddens is not None:
                hiddens = [h[:total] for h in hiddens[:-1]] + [hiddens[-1]] if short else [h[:total] for h in hiddens]
        return (y, tuple(hiddens)) if output_hidden_states else y

    @staticmethod
    def _plan_last_layer_rows(rows: Tensor, B: int, S: int, total: int, cu: Optional[Tensor], repack: bool, n_seq: Optional[int] = None) -> _RowSel:
        """Validates `last_layer_rows` and splits it by sequence, on the device plus ONE host read (validity and the largest per-sequence
        count).  rows number the (B, S) batch (cu None, or `repack`: the stack then runs on the packed rows of `cu` and the list is
        renumbered; every row must sit on a valid token) or the caller's packed axis of `total` rows (cu given, not repack).
        n_seq: the sequences the stack will see (with the pseudo-sequence of alignment rows), default cu's or B."""
        if not isinstance(rows, Tensor) or rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_cuda:
            raise ValueError("last_layer_rows must be a 1-D int64 CUDA/HIP tensor of ascending global row numbers")
        if n_seq is None:
            n_seq = B if cu is None else cu.numel() - 1
        n = rows.numel()
        if n == 0:
            return _RowSel.listed(rows.contiguous(), torch.zeros(n_seq + 1, dtype=torch.int32, device=rows.device), 0)
        rows = rows.contiguous()
        limit = B * S if (cu is None or repack) else total
        ok = (rows[0] >= 0) & (rows[-1] < limit)
        if n > 1:
            ok = ok & (rows[1:] > rows[:-1]).all()
        rc = rows.clamp(0, limit - 1)  # (a wrong list is refused below, before anything reads through it)
        if cu is None or repack:
            seq = rc // S
            idx = rc
            if repack:
                pos = rc - seq * S
                cu64 = cu.to(torch.int64)
                ok = ok & (pos < (cu64[1:] - cu64[:-1])[seq]).all()
                idx = cu64[seq] + pos
        else:
            seq = torch.searchsorted(cu[1:].to(torch.int64).contiguous(), rc, right=True).clamp(max=B - 1)
            idx = rc
        counts = torch.bincount(seq, minlength=n_seq)
        good, qmax = torch.stack((ok.to(torch.int64), counts.max())).tolist()
        if not good:
            raise ValueError(f"last_layer_rows must be strictly ascending row numbers in [0, {limit})" + (" on valid (unmasked) tokens" if repack else ""))
        qcu = torch.zeros(n_seq + 1, dtype=torch.int32, device=rows.device)
        qcu[1:] = torch.cumsum(counts, 0)
        return _RowSel.listed(idx.contiguous(), qcu, qmax)

    @staticmethod
    def _plan_unpadded(mask: Tensor, position_ids: Optional[Tensor]):
        """Index bookkeeping of _unpad_cm3p_input (ref:cm3p/modeling_cm3p.py:88-104) on the device plus ONE host read (the
        reference reads max_seqlen the same way).  -> (indices, cu_seqlens, max_seqlen, n_valid, n_rows, positions) or None
        when unpadding does not apply: nothing padded, an empty row, or a mask that is not right-padded (then the padded path
        keeps the reference's sdpa semantics exactly)."""
        B, S = mask.shape
        m = mask != 0
        lens = m.sum(dim=1, dtype=torch.int32)
        last = (m * torch.arange(1, S + 1, device=mask.device)).amax(dim=1).to(torch.int32)  # 1 + index of the last valid key
        total, max_s, min_s, prefix = torch.stack((lens.sum(), lens.max(), lens.min(), (last == lens).all().to(torch.int32))).tolist()
        if total == B * S or min_s == 0 or not prefix:
            return None
        idx = torch.nonzero(m.flatten()).flatten()
        n_rows = (total + 63) // 64 * 64  # keeps the token-contraction GEMMs (weight gradients) on the 256 x 256 kernel
        seq = lens if n_rows == total else torch.cat((lens, lens.new_full((1,), n_rows - total)))
        cu = torch.zeros(seq.numel() + 1, dtype=torch.int32, device=mask.device)
        cu[1:] = torch.cumsum(seq, 0)
        if position_ids is None:
            pos = idx % S
        else:
            pos = position_ids.expand(B, S).reshape(-1)[idx]
        if n_rows != total:
            pos = torch.cat((pos, torch.arange(n_rows - total, device=mask.device)))
        return idx, cu, max(int(max_s), n_rows - total), int(total), int(n_rows), pos.contiguous().to(torch.int64)
