"""CM3P model classes on the MI355X kernels, behind the reference's HuggingFace surface.

Drop-in for `cm3p.modeling_cm3p` on the contrastive training path (ref:cm3p/modeling_cm3p.py): same class names,
`forward` signature (incl. `return_loss=True` and `labels`, which HF Trainer introspects), `CM3POutput` field order,
submodule / state-dict names and Auto* registration, so `train.py` drives it unchanged.
All arithmetic runs in libcm3p_hip.so through autograd nodes defined here and in encoder.py; there is no PyTorch-op
fallback and inputs must live on the GPU.

Scope: CM3PModel's contrastive branch with both towers and the audio front end, plus the "next" rows:
CM3PModel's MLM head (`has_decoder_head`, loss_type "ForMaskedLM": `loss += 0.5 * mlm_loss`, the v7 recipe), padded AND
unpadded ("varlen") execution of the towers, and the stand-alone variants the reference's train.py imports
(`CM3PForMaskedLM`, `CM3PForBeatmapClassification`, `CM3PBeatmapModelWithProjection`, `CM3PMetadataModelWithProjection`),
all implemented on the same kernels below.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Optional

import torch
from torch import nn
from transformers import AutoModel
from transformers.modeling_outputs import BaseModelOutput, BaseModelOutputWithPooling
from transformers.modeling_utils import PreTrainedModel
from transformers.utils import ModelOutput

from . import kernels as K
from .configuration_cm3p import CM3PAudioConfig, CM3PBeatmapConfig, CM3PConfig, CM3PMetadataConfig
from .encoder import CM3PEncoder, _f32, _PadRowsFn

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------- outputs
@dataclass
class CM3PAudioModelOutput(BaseModelOutput):
    audio_embeds: Optional[torch.FloatTensor] = None


@dataclass
class CM3PBeatmapModelOutput(BaseModelOutputWithPooling):
    beatmap_embeds: Optional[torch.FloatTensor] = None
    audio_model_output: Optional[CM3PAudioModelOutput] = None
    selected_rows: Optional[Tensor] = None  # the rows last_hidden_state holds when the tower ran with last_layer_rows (else None)


@dataclass
class CM3PMetadataModelOutput(BaseModelOutput):
    metadata_embeds: Optional[torch.FloatTensor] = None


@dataclass
class CM3POutput(ModelOutput):
    """Field ORDER is part of the interface: Trainer drops `loss` and passes the rest positionally, and the reference's
    compute_metrics indexes [0] and [4] (ref:cm3p/modeling_cm3p.py:237-244, ref:train.py:77,101)."""

    loss: Optional[torch.FloatTensor] = None
    logits_per_beatmap: Optional[Tensor] = None
    logits_per_metadata: Optional[Tensor] = None
    metadata_embeds: Optional[torch.FloatTensor] = None
    beatmap_embeds: Optional[torch.FloatTensor] = None
    logits: Optional[torch.FloatTensor] = None
    metadata_model_output: BaseModelOutputWithPooling = None
    beatmap_model_output: BaseModelOutputWithPooling = None

    def to_tuple(self) -> tuple[Any]:
        nested = ("metadata_model_output", "beatmap_model_output")
        return tuple(self[k] if k not in nested else getattr(self, k).to_tuple() for k in self.keys())


@dataclass
class MaskedTokenPredictions(ModelOutput):
    """What `predict_tokens` returns: for each of the n selected positions the k most likely tokens, best first (equal logits: the
    lower token id first, torch.argmax's rule).  When the vocabulary has fewer than k tokens the slots past it hold id -1, logit and
    logprob -inf."""

    rows: Optional[Tensor] = None       # int64 [n]: global row b * S + s of the (B, S) batch, ascending
    token_ids: Optional[Tensor] = None  # int64 [n, k]
    logits: Optional[Tensor] = None     # fp32 [n, k]
    logprobs: Optional[Tensor] = None   # fp32 [n, k] = logits - log sum exp of the row's logits


# ----------------------------------------------------------------------------------------------- autograd nodes
class _PoolFn(torch.autograd.Function):
    """cls: h[:, 0]; else masked mean in fp32 (ref:cm3p/modeling_cm3p.py:385-396,631-642).  The gradient is written in h's dtype
    (bf16 rows of a bf16 residual stream get a bf16 gradient, one rounding of the fp32 value)."""

    @staticmethod
    def forward(ctx, h: Tensor, mask: Optional[Tensor], cls: bool):
        Bn, S, H = h.shape
        m = mask.contiguous().to(torch.int64) if mask is not None else None
        pooled, count = K.pool_fwd(h.detach().contiguous(), m, Bn, S, cls)
        ctx.pack = (m, count, Bn, S, cls)
        ctx.hdtype = h.dtype
        return pooled

    @staticmethod
    def backward(ctx, dp: Tensor):
        m, count, Bn, S, cls = ctx.pack
        dh = K.pool_bwd(dp.contiguous(), m, count, Bn, S, cls, dtype=torch.bfloat16 if ctx.hdtype == torch.bfloat16 else torch.float32)
        return dh.view(Bn, S, -1), None, None


class _PoolPackedFn(torch.autograd.Function):
    """_PoolFn for rows the caller packed: h [total, H] fp32 or bf16, cu int32 [Bn + 1] (sequence b owns rows cu[b] .. cu[b+1]-1),
    max_seqlen -> pooled [Bn, H] fp32.  cls: row cu[b]; else the mean of the sequence's rows, summed in the order of the padded
    kernels, so the result has the bits _PoolFn gives on a right-padded batch of the same rows.  The gradient
    is [total, H] in h's dtype, every row written once (zeros at and past cu[Bn]).  One host read checks that cu describes rows of h:
    the kernels index h with it."""

    @staticmethod
    def forward(ctx, h: Tensor, cu: Tensor, max_seqlen: int, cls: bool):
        if h.dim() != 2:
            raise ValueError("packed pooling takes the (total_nnz, H) rows of an unpadded batch")
        total = h.shape[0]
        cu = cu.to(device=h.device, dtype=torch.int32).reshape(-1).contiguous()
        if cu.numel() < 2:
            raise ValueError("cu_seqlens needs at least two entries (batch + 1)")
        lens = cu[1:] - cu[:-1]
        first, last, mx, mn = torch.stack((cu[0], cu[-1], lens.max(), lens.min())).tolist()
        if first != 0 or last > total or mn < 0:
            raise ValueError(f"cu_seqlens must start at 0, not decrease and end within the {total} rows; got start {first}, end {last}, min length {mn}")
        if int(max_seqlen) < mx:
            raise ValueError(f"max_seqlen {max_seqlen} is smaller than the longest sequence ({mx})")
        Bn, S = cu.numel() - 1, max(int(max_seqlen), 1)
        pooled, _ = K.pool_fwd(h.detach().contiguous(), None, Bn, S, cls, cu=cu, total=total)  # (.contiguous() of a y[:total] slice: no copy)
        ctx.pack = (cu, Bn, S, total, cls)
        ctx.hdtype = h.dtype
        return pooled

    @staticmethod
    def backward(ctx, dp: Tensor):
        cu, Bn, S, total, cls = ctx.pack
        dh = K.pool_bwd(dp.contiguous(), None, None, Bn, S, cls, dtype=torch.bfloat16 if ctx.hdtype == torch.bfloat16 else torch.float32,
                        cu=cu, total=total)
        return dh, None, None, None


class _ProjectFn(torch.autograd.Function):
    """y = x W^T in fp32: the bias-free projection heads (ref:cm3p/modeling_cm3p.py:761-762,959,971)."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor):
        x32, w32 = x.detach().contiguous(), _f32(w.detach()).contiguous()
        R, Hin = x32.shape
        P = w32.shape[0]
        y = K.gemm_f32(x32, w32, R, P, Hin, (Hin, 1), (Hin, 1))
        ctx.pack = (x32, w32, w.dtype)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x32, w32, wd = ctx.pack
        dy = dy.contiguous()
        R, Hin = x32.shape
        P = w32.shape[0]
        dx = K.gemm_f32(dy, w32, R, Hin, P, (P, 1), (1, Hin)) if ctx.needs_input_grad[0] else None  # dy W
        dw = K.gemm_f32(dy, x32, P, Hin, R, (1, P), (1, Hin)) if ctx.needs_input_grad[1] else None  # dy^T x
        if dw is not None and dw.dtype != wd:
            dw = dw.to(wd)
        return dx, dw


class _L2NormFn(torch.autograd.Function):
    """x / sqrt(sum x^2), no eps (ref:cm3p/modeling_cm3p.py:54-62,960,972)."""

    @staticmethod
    def forward(ctx, x: Tensor):
        y, norm = K.l2norm_fwd(x.detach().contiguous())
        ctx.pack = (y, norm)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        y, norm = ctx.pack
        return K.l2norm_bwd(dy.contiguous(), y, norm)


class _LogitsFn(torch.autograd.Function):
    """logits = (A B^T) * exp(logit_scale) (ref:cm3p/modeling_cm3p.py:976-977).  A [M,P], B [N,P] fp32."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, log_scale: Tensor):
        a32, b32 = a.detach().contiguous(), b.detach().contiguous()
        s32 = _f32(log_scale.detach()).reshape(1).contiguous()
        M, P = a32.shape
        N = b32.shape[0]
        raw = K.gemm_f32(a32, b32, M, N, P, (P, 1), (P, 1))
        logits = K.scale_exp(raw, s32)
        ctx.pack = (a32, b32, s32, logits, log_scale.dtype)
        return logits

    @staticmethod
    def backward(ctx, dl: Tensor):
        a32, b32, s32, logits, sd = ctx.pack
        dl = dl.contiguous()
        M, P = a32.shape
        N = b32.shape[0]
        draw = K.scale_exp(dl, s32)
        da = K.gemm_f32(draw, b32, M, P, N, (N, 1), (1, P)) if ctx.needs_input_grad[0] else None  # draw B
        db = K.gemm_f32(draw, a32, N, P, M, (1, N), (1, P)) if ctx.needs_input_grad[1] else None  # draw^T A
        ds = None
        if ctx.needs_input_grad[2]:
            ds = K.dot_f32(dl, logits).reshape(()).to(sd)  # d/ds [raw * e^s] = logits
        return da, db, ds


class _CrossEntropySumFn(torch.autograd.Function):
    """loss = sum_k coef_k * mean_rows CE_k over strided views of the given logits tensors: the pieces of cm3p_loss
    (ref:cm3p/modeling_cm3p.py:33-51) without materialising `.t()` / `.permute().reshape()` / gathered rows.
    spec = (tensor index, rows, cols, row_stride, col_stride, row_offset|None, target, coef)."""

    @staticmethod
    def forward(ctx, specs, *logits: Tensor):
        ls = [l.detach().contiguous() for l in logits]
        grads = [torch.zeros_like(l) for l in ls]
        loss = None
        for (ti, rows, cols, rs, cs, roff, target, coef) in specs:
            lr = K.cross_entropy(ls[ti], rows, cols, rs, cs, target, roff, coef / rows, grads[ti])
            loss = K.sum_f32(lr, coef / rows, out=loss, accumulate=loss is not None)
        ctx.grads = grads
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        g = g.reshape(1).contiguous()
        return (None, *[K.scale_by(d, g) for d in ctx.grads])


def cm3p_loss_hip(logits_per_metadata: Tensor, metadata_variation_classes: Optional[Tensor] = None) -> Tensor:
    """cm3p_loss on the GPU (ref:cm3p/modeling_cm3p.py:33-51), both directions from one logits tensor."""
    L = logits_per_metadata
    dev = L.device
    if L.dim() == 3:
        Bm, V, Bb = L.shape
        if Bm != Bb:
            raise AssertionError("metadata and beatmap batch sizes differ")
        idx = K.first_zero_index(metadata_variation_classes.contiguous().to(torch.int64))  # (classes == 0).argmax(1)
        rows_b = torch.arange(Bm, device=dev, dtype=torch.int64)
        # metadata loss: rows L[b, idx[b], :]  -> row offset (b*V + idx[b]) * Bb          (integer index arithmetic only)
        roff = (rows_b * V + idx) * Bb
        # beatmap loss over L.permute(2,0,1).reshape(Bb, Bm*V): element (bm, m*V+v) = L[m, v, bm]; target m*V + idx[m]
        tgt_b = rows_b * V + idx
        specs = [(0, Bm, Bb, 0, 1, roff, rows_b, 0.5), (0, Bb, Bm * V, 1, Bb, None, tgt_b, 0.5)]
    else:
        Bm, Bb = L.shape
        t = torch.arange(Bm, device=dev, dtype=torch.int64)
        specs = [(0, Bm, Bb, Bb, 1, None, t, 0.5), (0, Bb, Bm, 1, Bb, None, t, 0.5)]
    return _CrossEntropySumFn.apply(specs, L)


def _mlm_head_trunk(h: Tensor, Wd: Tensor, bd: Optional[Tensor], norm_w: Tensor, Wdec: Tensor, bdec: Optional[Tensor], eps: float):
    """norm(gelu(dense(h))) and the decoder's operands: what _mlm_head_forward and the logit-free node share -> (what the backward
    needs, the decoder bias padded to Vp in fp32 | None, parameter dtypes); Vp = vocab rounded up to a multiple of 64."""
    from ._lib import EPI_F32
    from .encoder import _bf16_weight

    T, H = h.shape
    V = Wdec.shape[0]
    Vp = (V + 63) // 64 * 64
    hb = h.detach().contiguous()
    if hb.dtype != torch.bfloat16:  # (rows of the bf16 residual stream are the GEMM operand as they are)
        hb = K.cast_bf16(hb)
    Wd_b = _bf16_weight(Wd)
    Wdec_b = _bf16_weight(Wdec)
    if Vp != V:
        pad = torch.zeros((Vp, H), dtype=torch.bfloat16, device=h.device)
        pad[:V].copy_(Wdec_b)  # layout only: pad the vocabulary to the GEMM's column granularity
        Wdec_b = pad
    bd32 = _f32(bd.detach()).contiguous() if bd is not None else torch.zeros((H,), dtype=torch.float32, device=h.device)
    w32 = _f32(norm_w.detach()).contiguous()
    z = K.gemm(hb, Wd_b, T, H, H, True, True, EPI_F32)
    _, a32 = K.bias_gelu_fwd(z, bd32, False, True)
    _, y, mean, rstd = K.layernorm_fwd(a32, w32, eps, False, True)
    bp = None
    if bdec is not None:
        bp = torch.zeros((Vp,), dtype=torch.float32, device=h.device)
        bp[:V].copy_(_f32(bdec.detach()))
    pack = (hb, Wd_b, Wdec_b, bd32, w32, z, a32, y, mean, rstd, V)
    meta = (Wd.dtype, bd.dtype if bd is not None else None, norm_w.dtype, Wdec.dtype, bdec.dtype if bdec is not None else None, h.dtype)
    return pack, bp, meta


def _mlm_head_forward(h: Tensor, Wd: Tensor, bd: Optional[Tensor], norm_w: Tensor, Wdec: Tensor, bdec: Optional[Tensor], eps: float):
    """decoder(norm(gelu(dense(h)))) (CM3PPredictionHead + decoder, ref:cm3p/modeling_cm3p.py:991,1229-1238) -> (fp32 logits
    [T, Vp], what the backward needs, parameter dtypes); Vp = vocab rounded up to a multiple of 64, so that the decoder's input-
    gradient GEMM, which contracts over Vp, runs on the 256 x 256 kernel (pad columns hold the zero pad weights' product;
    callers slice)."""
    from ._lib import EPI_F32, EPI_F32_BIAS

    pack, bp, meta = _mlm_head_trunk(h, Wd, bd, norm_w, Wdec, bdec, eps)
    Wdec_b, y = pack[2], pack[7]
    T, H = y.shape
    Vp = Wdec_b.shape[0]
    if bp is not None:  # the decoder bias is added while the GEMM stores its tiles (no extra pass over [T, Vp])
        logits = K.gemm(y, Wdec_b, T, Vp, H, True, True, EPI_F32_BIAS, resid=bp)
    else:
        logits = K.gemm(y, Wdec_b, T, Vp, H, True, True, EPI_F32)
    return logits, pack, meta


def _mlm_head_backward(pack, meta, need_dh: bool, dlb: Tensor, dbdec_full: Optional[Tensor]):
    """dlb: bf16 [T, Vp] gradient of the padded logits; dbdec_full: its fp32 column sums.  -> gradients of
    (h, Wd, bd, norm_w, Wdec, bdec); dh has the dtype of h (bf16 rows of a bf16 residual stream: the dgrad GEMM stores bf16)."""
    Wdec_b, y = pack[2], pack[7]
    dy = K.linear_dgrad(dlb, Wdec_b)
    dWdec_full = K.linear_wgrad(dlb, y)
    return _mlm_head_backward_below(pack, meta, need_dh, dy, dWdec_full, dbdec_full)


def _mlm_head_backward_below(pack, meta, need_dh: bool, dy: Tensor, dWdec_full: Tensor, dbdec_full: Optional[Tensor]):
    """Everything below the decoder: dy bf16 [T, H] (the decoder's input gradient), dWdec_full fp32 [Vp, H], dbdec_full fp32 [Vp]."""
    from ._lib import EPI_BF16, EPI_F32

    hb, Wd_b, Wdec_b, bd32, w32, z, a32, y, mean, rstd, V = pack
    dWd_t, dbd_t, dnw_t, dWdec_t, dbdec_t, h_t = meta
    T, H = hb.shape
    dWdec = dWdec_full[:V]
    dbdec = dbdec_full[:V] if dbdec_t is not None else None
    da, _, dnw = K.layernorm_bwd(dy, a32, w32, mean, rstd, None, False, inplace=False)
    dz, dbd = K.bias_gelu_bwd(da, z, bd32)
    dh = K.gemm(dz, Wd_b, T, H, H, True, False, EPI_BF16 if h_t == torch.bfloat16 else EPI_F32) if need_dh else None
    dWd = K.linear_wgrad(dz, hb)
    return (dh, dWd.to(dWd_t), dbd.to(dbd_t) if dbd_t is not None else None, dnw.to(dnw_t), dWdec.to(dWdec_t),
            dbdec.to(dbdec_t) if dbdec is not None else None)


class _MLMHeadFn(torch.autograd.Function):
    """The MLM head alone (logits wanted, no labels): see _mlm_head_forward."""

    @staticmethod
    def forward(ctx, h: Tensor, Wd: Tensor, bd: Optional[Tensor], norm_w: Tensor, Wdec: Tensor, bdec: Optional[Tensor], eps: float):
        logits, ctx.pack, ctx.meta = _mlm_head_forward(h, Wd, bd, norm_w, Wdec, bdec, eps)
        return logits

    @staticmethod
    def backward(ctx, dl: Tensor):
        dl = dl.contiguous()
        dbdec_full = K.colsum_f32(dl) if ctx.meta[4] is not None else None
        return (*_mlm_head_backward(ctx.pack, ctx.meta, ctx.needs_input_grad[0], K.cast_bf16(dl), dbdec_full), None)


class _MLMHeadLossFn(torch.autograd.Function):
    """MLM head + ForMaskedLMLoss in one node (ref:cm3p/modeling_cm3p.py:987-996; TF:loss/loss_utils.py:32-46,74-91: mean cross
    entropy over labels != -100, or the sum divided by `num_items_in_batch` when the Trainer supplies it) -> (fp32 logits
    [T, Vp], loss).  Keeping both in one node lets the backward write the logits' gradient once, in bf16, straight into the
    layout the decoder's dgrad / wgrad GEMMs read, together with the decoder-bias gradient: no [T, Vp] fp32 gradient tensor,
    no scale / cast / column-sum passes over it, and the 85 % of rows without a label are never read."""

    @staticmethod
    def forward(ctx, h: Tensor, Wd: Tensor, bd: Optional[Tensor], norm_w: Tensor, Wdec: Tensor, bdec: Optional[Tensor], eps: float,
                labels: Tensor, num_items: Optional[Tensor]):
        logits, ctx.pack, ctx.meta = _mlm_head_forward(h, Wd, bd, norm_w, Wdec, bdec, eps)
        V = Wdec.shape[0]
        lab = labels.reshape(-1).contiguous().to(torch.int64)
        if lab.numel() != logits.shape[0]:
            raise ValueError(f"labels have {lab.numel()} entries, the logits {logits.shape[0]} rows")
        if num_items is None:
            inv = K.inv_valid_count(lab, -100)
        else:
            n = num_items if torch.is_tensor(num_items) else torch.tensor(float(num_items))
            inv = (1.0 / n.to(device=logits.device, dtype=torch.float32)).reshape(1).contiguous()  # scalar plumbing
        loss_rows, lse_rows = K.ce_masked_stats(logits, V, lab, -100)
        loss = K.scale_by(K.sum_f32(loss_rows, 1.0), inv)
        ctx.ce = (logits, lab, lse_rows, inv, V)
        ctx.set_materialize_grads(False)
        return logits, loss.reshape(())

    @staticmethod
    def backward(ctx, dl_ext: Optional[Tensor], dloss: Optional[Tensor]):
        logits, lab, lse_rows, inv, V = ctx.ce
        dlb = colsum = None
        if dloss is not None:
            dlb, colsum = K.ce_masked_dlogits_bf16(logits, V, lab, -100, lse_rows, dloss.reshape(1).contiguous().float(), inv)
        if dl_ext is not None:  # the logits were also used outside the loss: add that gradient (not the Trainer's path)
            dl_ext = dl_ext.contiguous().float()
            cs = K.colsum_f32(dl_ext)
            if dlb is None:
                dlb, colsum = K.cast_bf16(dl_ext), cs
            else:
                _, dlb = K.add_f32(dl_ext, dlb, want_bf16=True, inplace=False)
                colsum, _ = K.add_f32(colsum, cs, want_bf16=False, inplace=False)
        if dlb is None:
            return (None,) * 9
        return (*_mlm_head_backward(ctx.pack, ctx.meta, ctx.needs_input_grad[0], dlb, colsum), None, None, None)


# Bytes of the bf16 logit gradient _MLMHeadLogitFreeLossFn.backward holds at a time: it works in chunks of the largest multiple of 128
# rows whose [rows, Vp] bf16 block fits (at least 128 rows).  Tests set MLM_LOGIT_FREE_CHUNK_ROWS to force several chunks.
MLM_LOGIT_FREE_CHUNK_BYTES = 256 << 20
MLM_LOGIT_FREE_CHUNK_ROWS: Optional[int] = None


def _mlm_logit_free_chunk_rows(Vp: int) -> int:
    if MLM_LOGIT_FREE_CHUNK_ROWS is not None:
        rows = int(MLM_LOGIT_FREE_CHUNK_ROWS)
        if rows < 128 or rows % 128:
            raise ValueError(f"MLM_LOGIT_FREE_CHUNK_ROWS must be a positive multiple of 128, got {rows}")
        return rows
    return max(128, MLM_LOGIT_FREE_CHUNK_BYTES // (Vp * 2) // 128 * 128)


class _MLMHeadLogitFreeLossFn(torch.autograd.Function):
    """_MLMHeadLossFn without the logits (`logit_free_mlm_loss`): same arguments, returns the loss only.  The forward runs the head's
    trunk and cm3p_mlm_lse, which consumes the decoder's logit tiles where they are computed; the backward recomputes them in
    cm3p_mlm_dlogits, a chunk of rows at a time, so that the largest [rows, Vp] tensor of the step is one bf16 chunk
    (MLM_LOGIT_FREE_CHUNK_BYTES).  Per chunk: the decoder's dgrad rows, its weight gradient (summed in fp32 over the chunks) and the
    bias gradient (summed by the kernel's accumulate flag); everything below the decoder then runs once on the full dy."""

    @staticmethod
    def forward(ctx, h: Tensor, Wd: Tensor, bd: Optional[Tensor], norm_w: Tensor, Wdec: Tensor, bdec: Optional[Tensor], eps: float,
                labels: Tensor, num_items: Optional[Tensor]):
        ctx.pack, bp, ctx.meta = _mlm_head_trunk(h, Wd, bd, norm_w, Wdec, bdec, eps)
        Wdec_b, y = ctx.pack[2], ctx.pack[7]
        V = Wdec.shape[0]
        lab = labels.reshape(-1).contiguous().to(torch.int64)
        if lab.numel() != y.shape[0]:
            raise ValueError(f"labels have {lab.numel()} entries, the head {y.shape[0]} rows")
        if num_items is None:
            inv = K.inv_valid_count(lab, -100)
        else:
            n = num_items if torch.is_tensor(num_items) else torch.tensor(float(num_items))
            inv = (1.0 / n.to(device=y.device, dtype=torch.float32)).reshape(1).contiguous()  # scalar plumbing
        loss_rows, lse_rows = K.mlm_lse(y, Wdec_b, bp, V, lab, -100)
        loss = K.scale_by(K.sum_f32(loss_rows, 1.0), inv)
        ctx.ce = (bp, lab, lse_rows, inv)
        ctx.set_materialize_grads(False)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss: Optional[Tensor]):
        from ._lib import EPI_BF16

        if dloss is None:
            return (None,) * 9
        bp, lab, lse_rows, inv = ctx.ce
        Wdec_b, y, V = ctx.pack[2], ctx.pack[7], ctx.pack[10]
        T, H = y.shape
        Vp = Wdec_b.shape[0]
        g = dloss.reshape(1).contiguous().float()
        rows = min(_mlm_logit_free_chunk_rows(Vp), max(T + 127, 128) // 128 * 128)
        buf = torch.empty((rows, Vp), dtype=torch.bfloat16, device=y.device)
        dy = torch.empty((T, H), dtype=torch.bfloat16, device=y.device)
        colsum = torch.empty((Vp,), dtype=torch.float32, device=y.device)
        dWdec = None
        for r0 in range(0, T, rows):
            r1 = min(r0 + rows, T)
            dlb, _ = K.mlm_dlogits(y[r0:r1], Wdec_b, bp, V, lab[r0:r1], -100, lse_rows[r0:r1], g, inv, colsum=colsum, accumulate=r0 > 0, out=buf)
            K.gemm(dlb, Wdec_b, r1 - r0, H, Vp, True, False, EPI_BF16, out=dy[r0:r1])
            dW = K.linear_wgrad(dlb, y[r0:r1])
            dWdec = dW if dWdec is None else K.add_f32(dWdec, dW)[0]
        return (*_mlm_head_backward_below(ctx.pack, ctx.meta, ctx.needs_input_grad[0], dy, dWdec, colsum), None, None, None)


# ----------------------------------------------------------------------------------------------- predictions without the logits
def _mlm_topk_chunk_rows(Vp: int, k: int) -> int:
    """Rows per cm3p_mlm_topk call: the largest multiple of 128 whose workspace - (k + 1) pairs of 8 bytes per (128-column tile, row) -
    stays within MLM_LOGIT_FREE_CHUNK_BYTES, at least 128 (_mlm_logit_free_chunk_rows' rule)."""
    return max(128, MLM_LOGIT_FREE_CHUNK_BYTES // (-(-Vp // 128) * (k + 1) * 8) // 128 * 128)


def _prediction_rows(positions, attention_mask: Optional[Tensor], B: int, S: int, device) -> Tensor:
    """`positions` of predict_tokens -> int64 [n] ascending global rows on `device`.  A (B, S) mask (nonzero = predict) and None (every
    position whose attention_mask is nonzero) cost one host read for the count; a list is taken as it is (the encoder validates it)."""
    if positions is None:
        if attention_mask is None:
            return torch.arange(B * S, dtype=torch.int64, device=device)
        positions = attention_mask.reshape(B, S)
    if not torch.is_tensor(positions):
        positions = torch.as_tensor(positions, dtype=torch.int64)
    positions = positions.to(device)
    if positions.dim() == 2:
        if tuple(positions.shape) != (B, S):
            raise ValueError(f"positions as a mask must have the inputs' shape ({B}, {S}), got {tuple(positions.shape)}")
        return torch.nonzero(positions.reshape(-1) != 0).flatten()
    if positions.dim() != 1 or positions.dtype != torch.int64:
        raise ValueError("positions must be a (B, S) mask, a 1-D int64 list of strictly ascending global rows b * S + s, or None")
    return positions.contiguous()


def _empty_predictions(k: int, device) -> MaskedTokenPredictions:
    z = torch.empty((0, k), dtype=torch.float32, device=device)
    return MaskedTokenPredictions(rows=torch.empty((0,), dtype=torch.int64, device=device), token_ids=torch.empty((0, k), dtype=torch.int64, device=device),
                                  logits=z, logprobs=z.clone())


def _check_prediction_call(model, k: int) -> int:
    if model.training:
        raise ValueError("predict_tokens on a model in training mode: predictions have evaluation semantics (no dropout); call model.eval() first")
    if not 1 <= int(k) <= 8:
        raise ValueError(f"predict_tokens: k must lie in 1..8, got {k}")
    return int(k)


def _predict_rows(h: Tensor, rows: Tensor, head, decoder, eps: float, k: int) -> MaskedTokenPredictions:
    """The MLM head's trunk on the n selected rows h [n, H], then cm3p_mlm_topk on chunks of them: no [n, vocab] tensor exists."""
    pack, bp, _ = _mlm_head_trunk(h, head.dense.weight, head.dense.bias, head.norm.weight, decoder.weight, decoder.bias, eps)
    Wdec_b, y, V = pack[2], pack[7], pack[10]
    n = y.shape[0]
    step = _mlm_topk_chunk_rows(Wdec_b.shape[0], k)
    parts = [K.mlm_topk(y[r0:r0 + step], Wdec_b, bp, V, k) for r0 in range(0, n, step)]
    idx, val, lse = (torch.cat(p) if len(parts) > 1 else p[0] for p in zip(*parts))
    return MaskedTokenPredictions(rows=rows, token_ids=idx.to(torch.int64), logits=val, logprobs=val - lse[:, None])


def masked_lm_accuracy(pred: MaskedTokenPredictions, labels: Tensor, ignore_index: int = -100) -> dict:
    """The masked-LM accuracy counts of the reference's compute_metrics (ref:train.py:75-90) from `predict_tokens`' output instead of
    the logits -> dict(total, correct, top5_correct) of int64 scalars on the device (no host read; add them up over the batches and
    read once).  labels: the batch's (B, S) labels - the entries at pred.rows are taken - or the n labels of pred.rows themselves.
    A row counts when its label differs from ignore_index; `correct`: its first id is the label; `top5_correct`: the label is among its
    first min(5, k) ids (with fewer than 5 tokens in the vocabulary the slots past it hold -1 and match no label)."""
    ids = pred.token_ids
    lab = labels.to(ids.device).reshape(-1)
    if lab.numel() != ids.shape[0]:
        lab = lab[pred.rows]
    live = lab != ignore_index
    hit = (ids[:, :5] == lab[:, None]) & live[:, None]
    return dict(total=live.sum(), correct=hit[:, 0].sum(), top5_correct=hit.any(dim=-1).sum())


class _AddScaledFn(torch.autograd.Function):
    """a + c * b for 0-dim fp32 tensors on the device (`loss += 0.5 * mlm_loss`, ref:cm3p/modeling_cm3p.py:996)."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, c: float):
        ctx.c = c
        out = a.detach().reshape(1).clone()
        K.sum_f32(b.detach().reshape(1).contiguous(), c, out=out, accumulate=True)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        gc = torch.empty((1,), dtype=torch.float32, device=g.device)
        K.sum_f32(g.reshape(1).contiguous(), ctx.c, out=gc)
        return g, gc.reshape(()), None


# ----------------------------------------------------------------------------------------------- base class
class CM3PPreTrainedModel(PreTrainedModel):
    config_class = CM3PConfig
    base_model_prefix = "cm3p"
    supports_gradient_checkpointing = True  # per-layer recompute inside encoder._EncoderLayerFn
    _supports_flash_attn_2 = True
    _supports_flash_attn = True
    _supports_sdpa = True
    _supports_flex_attn = False

    def _pooled_towers(self):
        return [t for t in (getattr(self, "beatmap_model", None), getattr(self, "metadata_model", None)) if t is not None]

    @property
    def cls_only_last_layer(self) -> bool:
        """Opt-in for `cls_embed: true` towers (CM3PEncoder.cls_only_last_layer): the last encoder layer and the final norm of the
        beatmap and metadata towers run on the pooled CLS row of every sequence only; `last_hidden_state` is then (B, 1, H) (with
        (B, V, L) metadata: (B, V, 1, H); caller-packed rows: (Bn, H)) and the pooled outputs, embeddings, logits, loss and gradients
        are those of the full layer.  Set on every pooled tower this model owns (the audio encoder has no pooling and no switch), True
        when all of them have it.  A call whose consumer needs all rows - mean pooling (`cls_embed` false) with a pooled output, the
        MLM / decoder head (`has_decoder_head`, `output_logits`, CM3PForMaskedLM) - raises ValueError before any launch, and
        `output_attentions` NotImplementedError.  Off by default; not part of the state dict or config."""
        towers = self._pooled_towers()
        return bool(towers) and all(t.cls_only_last_layer for t in towers)

    @cls_only_last_layer.setter
    def cls_only_last_layer(self, value: bool):
        for t in self._pooled_towers():
            t.cls_only_last_layer = bool(value)

    def set_residual_dtype(self, dtype: Optional[torch.dtype], training: bool = False):
        """Set `residual_dtype` on every encoder this model owns (beatmap, metadata and audio towers): torch.bfloat16 runs the
        residual stream of forward-only calls in bf16, the reference's inference recipe (a bf16 model called under no_grad);
        None / torch.float32 keep the fp32 stream.  With the default training=False, training steps always run fp32
        (CM3PEncoder.residual_dtype).  training=True sets `train_residual_dtype` as well: calls that record a backward then run the
        bf16 stream too, with a bf16 residual-stream gradient (CM3PEncoder.train_residual_dtype; master weights and weight
        gradients keep their dtype).  Calls with dropout (train mode, any p > 0) run fp32 either way.
        Returns the model; the state dict and the config are unchanged."""
        from .encoder import CM3PEncoder

        if dtype is not None and dtype not in (torch.float32, torch.bfloat16):  # (before anything is changed; the setters' rule)
            raise ValueError(f"residual_dtype must be None, torch.float32 or torch.bfloat16, got {dtype!r}")
        encoders = [m for m in self.modules() if isinstance(m, CM3PEncoder)]
        for enc in encoders:
            enc.residual_dtype = dtype
            if training:
                enc.train_residual_dtype = dtype
        return self

    def _check_and_adjust_attn_implementation(self, attn_implementation, *args, **kwargs):
        # Attention always runs in the HIP flash kernels; the configured string ("sdpa", "flash_attention_2", "eager", as
        # `train.py` copies it from the Hydra config, ref:train.py:275) selects nothing and needs no extra package.
        return attn_implementation if attn_implementation is not None else "sdpa"

    @torch.no_grad()
    def _init_weights(self, module):
        """Initialisation rules of the reference wrapper (ref:cm3p/modeling_cm3p.py:262-297) and of the encoder it
        wraps (TF:models/modernbert/modeling_modernbert.py:353-408: truncated normal, 'in' std 0.02, 'out' 0.02/sqrt(2L)).
        HF only visits modules that own parameters, so the encoder's role-dependent stds ride on leaf tags."""
        cfg = self.config
        tag = getattr(module, "_cm3p_init", None)
        if tag is not None:  # encoder leaves, tagged with their role's std by CM3PEncoder.__init__
            std, cutoff = tag
            nn.init.trunc_normal_(module.weight, mean=0.0, std=std, a=-cutoff * std, b=cutoff * std)
        elif isinstance(module, nn.LayerNorm):
            module.weight.fill_(1.0)
        elif isinstance(module, (nn.Linear, nn.Conv1d)):
            nn.init.normal_(module.weight, std=cfg.initializer_range)
            if module.bias is not None:
                module.bias.zero_()
        elif isinstance(module, CM3PModel):
            nn.init.normal_(module.metadata_projection.weight, std=module.metadata_embed_dim ** -0.5 * cfg.initializer_factor)
            nn.init.normal_(module.beatmap_projection.weight, std=module.beatmap_embed_dim ** -0.5 * cfg.initializer_factor)
            module.logit_scale.fill_(cfg.logit_scale_init_value)


def _pool_packed(h: Tensor, cu_seqlens: Tensor, max_seqlen: Optional[int], cls: bool) -> Tensor:
    """Pooled rows [Bn, H] fp32 of caller-packed rows h (total_nnz, H); max_seqlen None: the longest sequence (one host read)."""
    if max_seqlen is None:
        max_seqlen = int((cu_seqlens[1:] - cu_seqlens[:-1]).max().item())
    return _PoolPackedFn.apply(h, cu_seqlens, int(max_seqlen), cls)


def _cls_only_call(tower, output_attentions, output_pooler: bool) -> bool:
    """Whether this tower call runs with cls_only_last_layer; the calls the switch has no form for are refused here, before any launch."""
    if not tower.encoder.cls_only_last_layer:
        return False
    if output_attentions:
        raise NotImplementedError("output_attentions with cls_only_last_layer: the last layer computes one query per sequence; switch "
                                  "cls_only_last_layer off for such a call")
    if output_pooler and not tower.config.cls_embed:
        raise ValueError("cls_only_last_layer with mean pooling (cls_embed = False): the pooled output reads every row of the last layer; "
                         "switch cls_only_last_layer off on this tower")
    return True


def _pool_cls_rows(h: Tensor) -> Tensor:
    """Pooled output of a tower that ran with cls_only_last_layer: its rows as they are, (B, 1, H) or (Bn, H) -> [B, H] fp32."""
    if h.dim() == 3:
        return _PoolFn.apply(h, None, True)
    return h if h.dtype == torch.float32 else _WidenRowsFn.apply(h)


class _TowerSwitches:
    @property
    def cls_only_last_layer(self) -> bool:
        """CM3PEncoder.cls_only_last_layer of this tower's encoder."""
        return self.encoder.cls_only_last_layer

    @cls_only_last_layer.setter
    def cls_only_last_layer(self, value: bool):
        self.encoder.cls_only_last_layer = bool(value)


def _require_gpu(t: Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"cm3p_amd: {what} must be on the GPU; this build has no CPU path (use the reference package on CPU)")


# ----------------------------------------------------------------------------------------------- towers
class CM3PMetadataTransformer(_TowerSwitches, nn.Module):
    """ref:cm3p/modeling_cm3p.py:300-403."""

    def __init__(self, config: CM3PMetadataConfig):
        super().__init__()
        self.config = config
        self.encoder = CM3PEncoder(config)
        self.unpad_inputs = None  # as CM3PBeatmapTransformer.unpad_inputs: run padded (B, L) batches on their valid tokens only
        self.pool_unpadded = False  # opt-in: pool caller-packed rows (CLS and mean), which the reference does not implement

    def get_input_embeddings(self):
        return self.encoder.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.encoder.set_input_embeddings(value)

    def forward(self, input_ids: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None, indices=None, cu_seqlens=None,
                max_seqlen=None, batch_size=None, seq_len=None, output_attentions=None, output_hidden_states=None,
                output_pooler: bool = True) -> BaseModelOutputWithPooling:
        """Caller-packed rows (`cu_seqlens` given) are pooled only with `self.pool_unpadded = True`; otherwise the call raises the
        reference's NotImplementedError.  A caller-packed batch has no variation axis, so its `pooler_output` is 2-D, [Bn, H] in
        fp32 (one row per sequence of `cu_seqlens`), while `last_hidden_state` stays (total_nnz, H)."""
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        cls_only = _cls_only_call(self, output_attentions, output_pooler)
        if indices is not None or cu_seqlens is not None:
            # caller-supplied unpadded rows (ref:cm3p/modeling_cm3p.py:359-372): the encoder runs packed; the reference has no pooling
            # for them in this tower (ref:cm3p/modeling_cm3p.py:383-384)
            if cu_seqlens is None:
                raise ValueError("unpadded inputs need cu_seqlens (and max_seqlen)")
            if output_attentions:
                raise NotImplementedError("output_attentions with unpadded inputs: attention probabilities are (B, nh, S, S) tensors of a padded batch")
            if output_pooler and not self.pool_unpadded:  # (before the encoder runs: the reference's own message, ref:cm3p/modeling_cm3p.py:383-384)
                raise NotImplementedError("Pooling with unpadded input is not implemented yet.")
            _require_gpu(input_ids, "input_ids")
            h = self.encoder(input_ids=input_ids, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen, output_hidden_states=bool(output_hidden_states))
            hiddens = None
            if output_hidden_states:
                h, hiddens = h
            if cls_only:
                pooled = _pool_cls_rows(h) if output_pooler else None
            else:
                pooled = _pool_packed(h, cu_seqlens, max_seqlen, bool(self.config.cls_embed)) if output_pooler else None
            return BaseModelOutputWithPooling(last_hidden_state=h, pooler_output=pooled, hidden_states=hiddens, attentions=None)
        _require_gpu(input_ids, "input_ids")
        is_3d = input_ids.dim() == 3
        B0 = input_ids.size(0)
        ids2, am2 = input_ids, attention_mask
        if is_3d:  # (B, V, L) -> (B*V, L), ref:cm3p/modeling_cm3p.py:351-357
            ids2 = input_ids.reshape(-1, input_ids.size(-1))
            am2 = attention_mask.reshape(-1, attention_mask.size(-1)) if attention_mask is not None else None
        # output_attentions: the probabilities of every layer, (B[*V], nh, L, L) fp32 (a separate inspection kernel: the flash
        # kernels never materialise them; the reference switches to eager attention for such a call)
        # unpadded execution of a padded batch (metadata rows are usually much shorter than the padded length - the 1000-variation
        # evaluation is mostly padding): asked for explicitly or, like the reference, by attn_implementation == flash_attention_2;
        # the encoder re-pads its output and keeps the padded path where packing does not apply
        unpad = self.unpad_inputs if self.unpad_inputs is not None else getattr(self.config, "_attn_implementation", None) == "flash_attention_2"
        h = self.encoder(input_ids=ids2, attention_mask=am2, output_hidden_states=bool(output_hidden_states),
                         output_attentions=bool(output_attentions), unpad=bool(unpad) and not output_attentions)
        hiddens = attns = None
        if output_attentions:
            h, hiddens, attns = h
        elif output_hidden_states:
            h, hiddens = h
        if cls_only:
            pooled = _pool_cls_rows(h) if output_pooler else None
        else:
            pooled = _PoolFn.apply(h, am2, bool(self.config.cls_embed)) if output_pooler else None
        if is_3d:
            h = h.view(B0, -1, h.size(-2), h.size(-1))
            if pooled is not None:
                pooled = pooled.view(B0, -1, pooled.size(-1))
            if hiddens is not None:
                hiddens = tuple(t.view(B0, -1, t.size(-2), t.size(-1)) for t in hiddens)
        return BaseModelOutputWithPooling(last_hidden_state=h, pooler_output=pooled, hidden_states=hiddens, attentions=attns)


class CM3PMultiModalProjector(nn.Module):
    """Parameter container for linear_1 / linear_2 (ref:cm3p/modeling_cm3p.py:470-481)."""

    def __init__(self, config: CM3PAudioConfig):
        super().__init__()
        if config.projector_hidden_act != "gelu":
            raise NotImplementedError("projector_hidden_act must be 'gelu'")
        self.linear_1 = nn.Linear(config.projector_intermediate_size, config.projector_dim, bias=False)
        self.linear_2 = nn.Linear(config.projector_dim, config.projector_dim, bias=False)


class CM3PAudioEncoder(nn.Module):
    """ref:cm3p/modeling_cm3p.py:484-528: conv1d x2 + GELU -> encoder -> 4-frame concat -> projector."""

    def __init__(self, config: CM3PAudioConfig):
        super().__init__()
        self.config = config
        self.conv1 = nn.Conv1d(config.n_mels, config.hidden_size, kernel_size=3, padding=1)
        self.conv2 = nn.Conv1d(config.hidden_size, config.hidden_size, kernel_size=3, stride=2, padding=1)
        self.encoder = CM3PEncoder(config)
        self.multi_modal_projector = CM3PMultiModalProjector(config)

    def forward(self, input_features: Tensor, output_attentions=None, output_hidden_states=None) -> CM3PAudioModelOutput:
        from .audio import audio_frontend, audio_projector

        _require_gpu(input_features, "input_features")
        x = audio_frontend(input_features, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias)  # (B, T/2, H)
        B, T2, _ = x.shape
        pos = torch.arange(T2, device=x.device).unsqueeze(0).repeat(B, 1)  # explicit per-row positions, :506-507
        attns = None
        if output_attentions:
            h, _, attns = self.encoder(inputs_embeds=x, position_ids=pos, output_attentions=True)
        else:
            h = self.encoder(inputs_embeds=x, position_ids=pos)
        audio_embeds = audio_projector(h.reshape(-1, self.config.projector_intermediate_size),
                                       self.multi_modal_projector.linear_1.weight, self.multi_modal_projector.linear_2.weight)
        return CM3PAudioModelOutput(audio_embeds=audio_embeds, last_hidden_state=h, hidden_states=None, attentions=attns)


class CM3PBeatmapTransformer(_TowerSwitches, nn.Module):
    """ref:cm3p/modeling_cm3p.py:531-650."""

    def __init__(self, config: CM3PBeatmapConfig):
        super().__init__()
        self.config = config
        self.audio_encoder = CM3PAudioEncoder(config.audio_config)
        self.encoder = CM3PEncoder(config)
        self.unpad_inputs = None  # None: follow config._attn_implementation == 'flash_attention_2' (the reference's rule)
        self.pool_unpadded = False  # opt-in: mean pooling of caller-packed rows, which the reference does not implement

    def get_input_embeddings(self):
        return self.encoder.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.encoder.set_input_embeddings(value)

    def forward(self, input_ids: Optional[Tensor] = None, input_features: Optional[Tensor] = None,
                attention_mask: Optional[Tensor] = None, sliding_window_mask=None, position_ids: Optional[Tensor] = None,
                inputs_embeds: Optional[Tensor] = None, indices=None, cu_seqlens=None, max_seqlen=None, batch_size=None,
                seq_len=None, output_attentions=None, output_hidden_states=None, output_pooler: bool = True,
                last_layer_rows: Optional[Tensor] = None) -> CM3PBeatmapModelOutput:
        """last_layer_rows (CM3PEncoder.forward): the last layer, the final norm and last_hidden_state - then (n, H) - on the listed
        rows only, returned as `selected_rows`; padded (B, S) batches, with or without unpad_inputs.  With output_pooler the tower must
        pool the CLS row (`cls_embed`) and the list must hold row b * S of every sequence b: pooling takes those entries."""
        audio_out = None
        ohs = bool(output_hidden_states)
        oat = bool(output_attentions)
        if last_layer_rows is not None:  # (before the audio encoder runs)
            if oat:
                raise NotImplementedError("output_attentions with last_layer_rows: the last layer computes the listed queries only")
            if indices is not None or cu_seqlens is not None:
                raise NotImplementedError("last_layer_rows with caller-packed rows is not supported on the tower; call the encoder")
            if output_pooler and not self.config.cls_embed:
                raise ValueError("last_layer_rows with mean pooling (cls_embed = False): the pooled output reads every row of the last layer")
        cls_only = last_layer_rows is None and _cls_only_call(self, oat, output_pooler)  # (before the audio encoder runs)
        if oat and (indices is not None or cu_seqlens is not None):
            raise NotImplementedError("output_attentions with unpadded inputs: attention probabilities are (B, nh, S, S) tensors of a padded batch")
        if indices is not None or cu_seqlens is not None:
            # Caller-supplied unpadded rows (ref:cm3p/modeling_cm3p.py:911-931 with indices / cu_seqlens / max_seqlen given, layout of
            # _unpad_cm3p_input :65-104): input_ids (total_nnz,), last_hidden_state stays (total_nnz, H), CLS pooling reads row
            # cu_seqlens[:-1] of it (:624-627); mean pooling of unpadded rows is not implemented in the reference (:628-629) and here
            # only behind pool_unpadded: pooler_output [B, H] fp32 from the packed pooling kernels.
            if cu_seqlens is None:
                raise ValueError("unpadded inputs need cu_seqlens (and max_seqlen)")
            if inputs_embeds is not None:
                raise NotImplementedError("unpadded inputs_embeds are not supported; pass unpadded input_ids")
            _require_gpu(input_ids, "input_ids")
            slot = rows = None
            if input_features is not None:
                audio_out = self.audio_encoder(input_features)
                rows = audio_out.audio_embeds
                slot, count = K.audio_slots(input_ids.contiguous().view(-1).to(torch.int64), int(self.config.audio_token_id))
                n = int(count.item())
                if n != rows.shape[0]:
                    raise RuntimeError(f"shape mismatch: {n} audio placeholder tokens but {rows.shape[0]} audio embeddings")
            if output_pooler and not self.config.cls_embed and not self.pool_unpadded:  # before the encoder runs (ref:cm3p/modeling_cm3p.py:628-629)
                raise NotImplementedError("Pooling with unpadded input is not implemented yet.")
            h = self.encoder(input_ids=input_ids, position_ids=position_ids, audio_slot=slot, audio_rows=rows, cu_seqlens=cu_seqlens,
                             max_seqlen=max_seqlen, output_hidden_states=ohs)
            hiddens = None
            if ohs:
                h, hiddens = h
            pooled = None
            if output_pooler and cls_only:
                pooled = _pool_cls_rows(h)
            elif output_pooler and not self.config.cls_embed:
                pooled = _pool_packed(h, cu_seqlens, max_seqlen, False)
            elif output_pooler:
                first = cu_seqlens[:-1].to(device=h.device, dtype=torch.int64).contiguous()
                pooled = _TakeRowsFn.apply(h, first)
                if pooled.dtype != torch.float32:  # bf16 residual stream: the pooled rows widened exactly, as _PoolFn returns them
                    pooled = _WidenRowsFn.apply(pooled)
            return CM3PBeatmapModelOutput(last_hidden_state=h, pooler_output=pooled, hidden_states=hiddens, attentions=None,
                                          audio_model_output=audio_out)
        if inputs_embeds is not None:
            if input_features is not None:
                raise NotImplementedError("input_features together with inputs_embeds is not supported")
            _require_gpu(inputs_embeds, "inputs_embeds")
            h = self.encoder(inputs_embeds=inputs_embeds, attention_mask=attention_mask, position_ids=position_ids,
                             output_hidden_states=ohs, output_attentions=oat, last_layer_rows=last_layer_rows)
        else:
            _require_gpu(input_ids, "input_ids")
            slot = rows = None
            if input_features is not None:
                audio_out = self.audio_encoder(input_features)
                rows = audio_out.audio_embeds
                slot, count = K.audio_slots(input_ids.contiguous().view(-1).to(torch.int64), int(self.config.audio_token_id))
                # the reference's masked assignment raises on a count mismatch (ref:cm3p/modeling_cm3p.py:603-605)
                n = int(count.item())
                if n != rows.shape[0]:
                    raise RuntimeError(f"shape mismatch: {n} audio placeholder tokens but {rows.shape[0]} audio embeddings")
            # unpadded execution when asked for explicitly (unpad_inputs) or, like the reference, when the configuration says
            # flash_attention_2 (ref:cm3p/modeling_cm3p.py:911-931); the encoder falls back to the padded path where it does not apply
            unpad = self.unpad_inputs if self.unpad_inputs is not None else \
                getattr(self.config, "_attn_implementation", None) == "flash_attention_2"
            h = self.encoder(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, audio_slot=slot,
                             audio_rows=rows, unpad=bool(unpad), output_hidden_states=ohs, output_attentions=oat,
                             last_layer_rows=last_layer_rows)
        hiddens = attns = None
        if oat:
            h, hiddens, attns = h
        elif ohs:
            h, hiddens = h
        if last_layer_rows is not None:
            pooled = None
            if output_pooler:  # the list's entries b * S (ascending list: a search, no host read)
                ref = input_ids if input_ids is not None else inputs_embeds
                first = torch.arange(ref.shape[0], device=h.device, dtype=torch.int64) * ref.shape[1]
                pooled = _TakeRowsFn.apply(h, torch.searchsorted(last_layer_rows, first).clamp(max=h.shape[0] - 1))
                if pooled.dtype != torch.float32:
                    pooled = _WidenRowsFn.apply(pooled)
        elif cls_only:
            pooled = _pool_cls_rows(h) if output_pooler else None
        else:
            pooled = _PoolFn.apply(h, attention_mask, bool(self.config.cls_embed)) if output_pooler else None
        return CM3PBeatmapModelOutput(last_hidden_state=h, pooler_output=pooled, hidden_states=hiddens, attentions=attns,
                                      audio_model_output=audio_out, selected_rows=last_layer_rows)


class CM3PPredictionHead(nn.Module):
    """Parameter container of the MLM head (ref:cm3p/modeling_cm3p.py:1229-1238): dense -> GELU -> LayerNorm."""

    def __init__(self, config: CM3PBeatmapConfig):
        super().__init__()
        if config.classifier_activation != "gelu" or config.norm_bias:
            raise NotImplementedError("MLM head: classifier_activation must be 'gelu' and norm_bias False")
        self.dense = nn.Linear(config.hidden_size, config.hidden_size, config.classifier_bias)
        self.norm = nn.LayerNorm(config.hidden_size, eps=config.norm_eps, bias=False)


class CM3PMetadataModel(CM3PPreTrainedModel):
    config_class = CM3PMetadataConfig

    def __init__(self, config: CM3PMetadataConfig):
        super().__init__(config)
        self.metadata_model = CM3PMetadataTransformer(config)
        self.post_init()

    def get_input_embeddings(self) -> nn.Module:
        return self.metadata_model.encoder.embeddings.tok_embeddings

    def set_input_embeddings(self, value):
        self.metadata_model.encoder.embeddings.tok_embeddings = value

    def forward(self, *args, **kwargs):
        return self.metadata_model(*args, **kwargs)


class CM3PBeatmapModel(CM3PPreTrainedModel):
    config_class = CM3PBeatmapConfig
    main_input_name = "input_ids"

    def __init__(self, config: CM3PBeatmapConfig):
        super().__init__(config)
        self.beatmap_model = CM3PBeatmapTransformer(config)
        self.post_init()

    def get_input_embeddings(self) -> nn.Module:
        return self.beatmap_model.encoder.embeddings.tok_embeddings

    def set_input_embeddings(self, value):
        self.beatmap_model.encoder.embeddings.tok_embeddings = value

    def forward(self, *args, **kwargs):
        return self.beatmap_model(*args, **kwargs)


# ----------------------------------------------------------------------------------------------- the dual tower
_tower_streams: dict = {}  # device -> the stream the metadata tower runs on beside the beatmap tower


def _tower_stream(device) -> "torch.cuda.Stream":
    st = _tower_streams.get(device)
    if st is None:
        st = _tower_streams[device] = torch.cuda.Stream(device)
    return st


def _tensors_of(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from _tensors_of(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _tensors_of(o)


class CM3PModel(CM3PPreTrainedModel):
    config_class = CM3PConfig

    def __init__(self, config: CM3PConfig):
        super().__init__(config)
        if not isinstance(config.metadata_config, CM3PMetadataConfig):
            raise TypeError(f"config.metadata_config is expected to be of type CM3PMetadataConfig but is of type {type(config.metadata_config)}.")
        if not isinstance(config.beatmap_config, CM3PBeatmapConfig):
            raise TypeError(f"config.beatmap_config is expected to be of type CM3PBeatmapConfig but is of type {type(config.beatmap_config)}.")
        if config.has_decoder_head and config.loss_type != "ForMaskedLM":
            # the reference silently falls back to a shifted causal-LM loss for any other value (TF:modeling_utils.py:4655-4667)
            raise NotImplementedError('has_decoder_head needs loss_type="ForMaskedLM" (the published v7 recipe)')
        self.loss_type = config.loss_type
        self.projection_dim = config.projection_dim
        self.metadata_embed_dim = config.metadata_config.hidden_size
        self.beatmap_embed_dim = config.beatmap_config.hidden_size
        self.metadata_model = CM3PMetadataTransformer(config.metadata_config)
        self.beatmap_model = CM3PBeatmapTransformer(config.beatmap_config)
        self.beatmap_projection = nn.Linear(self.beatmap_embed_dim, self.projection_dim, bias=False)
        self.metadata_projection = nn.Linear(self.metadata_embed_dim, self.projection_dim, bias=False)
        self.logit_scale = nn.Parameter(torch.tensor(float(config.logit_scale_init_value)))
        if config.has_decoder_head:  # MLM head on the beatmap tower (ref:cm3p/modeling_cm3p.py:765-767)
            bc = config.beatmap_config
            self.head = CM3PPredictionHead(bc)
            self.decoder = nn.Linear(bc.hidden_size, bc.vocab_size, bias=bc.decoder_bias)
        # Opt-in: in-batch negatives across all ranks of the default process group (new behaviour): (B, L)
        # metadata always, (B, V, L) metadata variations in training mode (eval scores them rank-locally; cm3p_amd/dist.py).
        self.gather_negatives = False
        self.unpad_inputs = None  # True / False overrides the reference's rule (unpad iff attn_implementation is flash_attention_2)
        self._labelled_rows_last_layer = False
        # Opt-in (not in config or state dict): a training-mode call with labels and return_loss takes the masked-LM loss from the
        # decoder's logit tiles without storing them (_MLMHeadLogitFreeLossFn); the output's `logits` is then None.  Every other call -
        # evaluation, no labels - returns logits as without it.
        self.logit_free_mlm_loss = False
        self.post_init()

    @property
    def labelled_rows_last_layer(self) -> bool:
        """Opt-in for training steps of the recipe with CLS pooling and the decoder head: the beatmap tower's last layer, its final
        norm and the MLM head run on the rows that are consumed - row 0 of every sequence (pooling) and every position with a label
        (the loss) - instead of all B x S rows (CM3PEncoder.forward's last_layer_rows).  Takes effect only on calls in training mode
        with `labels`, `return_loss` and the logits of a model with `has_decoder_head` on a padded (B, S) batch (with or without
        unpad_inputs) of a `cls_embed` beatmap tower; every other call - evaluation, no labels, caller-packed rows - runs as without it.
        On such a call `logits` is (n, vocab) and `beatmap_model_output.last_hidden_state` (n, H) in the order of
        `beatmap_model_output.selected_rows`; loss, embeddings and every gradient are those of the full call.  Setting it on a model
        whose beatmap tower pools the mean raises ValueError.  Not part of the state dict or config; off by default."""
        return self._labelled_rows_last_layer

    @labelled_rows_last_layer.setter
    def labelled_rows_last_layer(self, value: bool):
        if value and not self.config.beatmap_config.cls_embed:
            raise ValueError("labelled_rows_last_layer with mean pooling (beatmap_config.cls_embed = False): the pooled output reads every row "
                             "of the last layer")
        self._labelled_rows_last_layer = bool(value)

    @property
    def pool_unpadded(self) -> bool:
        """Opt-in pooling of caller-packed rows (`cu_seqlens` given), which the reference does not implement: set on both towers,
        True when both have it.  Off by default: such a call then raises the reference's NotImplementedError."""
        return bool(self.beatmap_model.pool_unpadded) and bool(self.metadata_model.pool_unpadded)

    @pool_unpadded.setter
    def pool_unpadded(self, value: bool):
        self.beatmap_model.pool_unpadded = self.metadata_model.pool_unpadded = bool(value)

    def _overlap_towers(self, input_ids, metadata_ids) -> bool:
        """Run the metadata tower on a second stream beside the beatmap tower?  (CM3P_TOWER_OVERLAP=0 switches it off.)"""
        if input_ids is None or metadata_ids is None or not metadata_ids.is_cuda or self.gather_negatives:
            return False
        if os.environ.get("CM3P_TOWER_OVERLAP", "1") == "0":
            return False
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            return False
        return True

    def get_metadata_features(self, input_ids=None, output_attentions=None, output_hidden_states=None) -> Tensor:
        out = self.metadata_model(input_ids=input_ids)
        p = out.pooler_output
        return _ProjectFn.apply(p.reshape(-1, p.size(-1)), self.metadata_projection.weight).view(*p.shape[:-1], -1)

    def get_beatmap_features(self, input_ids=None, input_features=None, attention_mask=None, position_ids=None, inputs_embeds=None,
                             output_attentions=None, output_hidden_states=None) -> Tensor:
        out = self.beatmap_model(input_ids=input_ids, input_features=input_features, attention_mask=attention_mask,
                                 position_ids=position_ids, inputs_embeds=inputs_embeds)
        return _ProjectFn.apply(out.pooler_output, self.beatmap_projection.weight)

    def forward(
        self,
        input_ids: Optional[torch.LongTensor] = None,
        input_features: Optional[torch.FloatTensor] = None,
        metadata_ids: Optional[torch.LongTensor] = None,
        attention_mask: Optional[Tensor] = None,
        metadata_attention_mask: Optional[Tensor] = None,
        position_ids: Optional[torch.LongTensor] = None,
        inputs_embeds: Optional[torch.FloatTensor] = None,
        metadata_variation_classes: Optional[torch.LongTensor] = None,
        labels: Optional[Tensor] = None,
        indices: Optional[Tensor] = None,
        cu_seqlens: Optional[Tensor] = None,
        max_seqlen: Optional[int] = None,
        batch_size: Optional[int] = None,
        seq_len: Optional[int] = None,
        return_loss: Optional[bool] = True,
        output_attentions: Optional[bool] = None,
        output_hidden_states: Optional[bool] = None,
        output_logits: Optional[bool] = None,
        **kwargs,
    ) -> CM3POutput:
        """Contrastive forward (ref:cm3p/modeling_cm3p.py:849-1012).  Whatever `attn_implementation` says, attention runs in the
        HIP flash kernels, which take the key-padding mask as it is: padded batches need no host-side unpadding.  Unpadded
        execution is supported as well - `self.unpad_inputs = True` packs the valid tokens of a padded batch, and a caller may hand
        over rows it has unpadded itself (`indices` / `cu_seqlens` / `max_seqlen` / `batch_size` / `seq_len`, the arguments of the
        reference's flash_attention_2 branch, ref:cm3p/modeling_cm3p.py:911-931) - with the same results."""
        output_logits = output_logits if output_logits is not None else self.config.has_decoder_head
        if metadata_ids is not None and metadata_ids.dim() == 3 and return_loss and metadata_variation_classes is None:
            raise ValueError("When providing multiple metadata variations, metadata_variation_classes must be provided in order to compute loss correctly.")
        if output_logits and not self.config.has_decoder_head:
            raise ValueError("Cannot return logits when the model is not configured with a decoder head.")
        # cls_only_last_layer: every consumer of all rows is refused before either tower launches anything
        if output_logits and self.beatmap_model.cls_only_last_layer:
            raise ValueError("cls_only_last_layer with the MLM head (has_decoder_head / output_logits): the head reads every row of the beatmap "
                             "tower's last layer; switch cls_only_last_layer off on the beatmap tower")
        if input_ids is not None:
            _cls_only_call(self.beatmap_model, output_attentions, True)
        if metadata_ids is not None:
            _cls_only_call(self.metadata_model, output_attentions, True)

        beatmap_embeds = beatmap_outputs = metadata_embeds = metadata_outputs = beatmap_pending = None
        logits_per_beatmap = logits_per_metadata = None
        loss = 0 if return_loss else None

        def run_metadata():
            mo = self.metadata_model(input_ids=metadata_ids, attention_mask=metadata_attention_mask,
                                     output_attentions=output_attentions, output_hidden_states=output_hidden_states)
            p = mo.pooler_output
            me = _L2NormFn.apply(_ProjectFn.apply(p.reshape(-1, p.size(-1)), self.metadata_projection.weight))
            return mo, me.view(*p.shape[:-1], -1)

        # The two towers do not meet before the logits.  On one GPU the metadata tower (a few hundred launches of a few workgroups:
        # 8192 tokens at C2) runs on a second stream BESIDE the beatmap tower instead of after it; autograd runs each node's
        # backward on its forward stream and orders the gradients across streams, so the backward overlaps the same way.
        # Not with gathered negatives / more than one rank (DDP's bucket hooks take the stream of the last gradient of a bucket).
        # (both towers learn the unpadding rule before either is launched: with the towers overlapped the metadata tower goes first)
        if self.unpad_inputs is not None or getattr(self.config, "_attn_implementation", None) == "flash_attention_2":
            self.beatmap_model.unpad_inputs = True if self.unpad_inputs is None else bool(self.unpad_inputs)
            self.metadata_model.unpad_inputs = self.beatmap_model.unpad_inputs
        side = None
        if self._overlap_towers(input_ids, metadata_ids):
            main = torch.cuda.current_stream(metadata_ids.device)
            side = _tower_stream(metadata_ids.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                metadata_outputs, metadata_embeds = run_metadata()

        # labelled_rows_last_layer: the rows this training step consumes - every sequence's row 0 and the labelled positions
        sel_rows = sel_labels = None
        if (self._labelled_rows_last_layer and self.training and labels is not None and return_loss and output_logits and self.config.has_decoder_head
                and self.config.beatmap_config.cls_embed and input_ids is not None and input_ids.dim() == 2 and indices is None and cu_seqlens is None
                and labels.numel() == input_ids.numel()):
            want = labels.reshape(input_ids.shape) != -100
            want[:, 0] = True
            sel_rows = torch.nonzero(want.flatten()).flatten()  # ascending, deduplicated by construction
            sel_labels = labels.reshape(-1)[sel_rows]           # (an unlabelled CLS row keeps its -100)
        if input_ids is not None:
            try:
                beatmap_outputs = self.beatmap_model(input_ids=input_ids, last_layer_rows=sel_rows, input_features=input_features, attention_mask=attention_mask,
                                                     position_ids=position_ids, inputs_embeds=inputs_embeds, indices=indices,
                                                     cu_seqlens=cu_seqlens, max_seqlen=max_seqlen, batch_size=batch_size, seq_len=seq_len,
                                                     output_attentions=output_attentions, output_hidden_states=output_hidden_states)
                beatmap_embeds = _L2NormFn.apply(_ProjectFn.apply(beatmap_outputs.pooler_output, self.beatmap_projection.weight))
            except BaseException:
                if side is not None:  # the metadata tower is in flight on the other stream: join it before its tensors are dropped
                    main.wait_stream(side)
                raise
            if self.gather_negatives and metadata_ids is not None:
                if metadata_ids.dim() == 2 or self.training:
                    # start the all-gather now: it runs on the process group's side stream under the whole metadata tower and is
                    # joined just before the logits (cm3p_amd/dist.py)
                    from .dist import start_gather

                    beatmap_pending = start_gather(beatmap_embeds)
                else:
                    from .dist import warn_variations_stay_local

                    warn_variations_stay_local()

        if side is not None:
            # join: everything the caller (and the logits) will read was produced on `side`; its memory belongs to that stream's pool
            main.wait_stream(side)
            for t in _tensors_of((metadata_embeds, dict(metadata_outputs))):
                t.record_stream(main)
        elif metadata_ids is not None:
            try:
                metadata_outputs, metadata_embeds = run_metadata()
            except BaseException:
                if beatmap_pending is not None:  # never leave a collective un-joined behind an exception
                    beatmap_pending.wait()
                raise

        if metadata_embeds is not None and beatmap_embeds is not None:
            me2 = metadata_embeds.reshape(-1, metadata_embeds.size(-1))
            if self.gather_negatives and metadata_embeds.dim() == 2:
                from .dist import gathered_contrastive

                logits_per_metadata, logits_per_beatmap, gl = gathered_contrastive(me2, beatmap_embeds, self.logit_scale,
                                                                                   beatmap_pending=beatmap_pending)
                if return_loss:
                    loss = gl
            elif self.gather_negatives and self.training:
                # (B, V, L) variations, training: (b, V, N*b) / (b, N*b, V) logits against every rank's rows; both pending gathers
                # are joined inside, also behind an exception
                from .dist import gathered_contrastive_variations

                logits_per_metadata, logits_per_beatmap, gl = gathered_contrastive_variations(
                    metadata_embeds, beatmap_embeds, metadata_variation_classes if return_loss else None, self.logit_scale,
                    beatmap_pending=beatmap_pending)
                if return_loss:
                    loss = gl
            else:
                lpm = _LogitsFn.apply(me2, beatmap_embeds, self.logit_scale)
                if metadata_embeds.dim() == 3:
                    logits_per_metadata = lpm.view(metadata_embeds.size(0), metadata_embeds.size(1), -1)
                    logits_per_beatmap = logits_per_metadata.permute(2, 0, 1)
                else:
                    logits_per_metadata = lpm
                    logits_per_beatmap = lpm.t()
                if return_loss:
                    loss = cm3p_loss_hip(logits_per_metadata, metadata_variation_classes)

        logits = None
        if output_logits:  # MLM head; with labels, loss += 0.5 * masked-LM loss (ref:cm3p/modeling_cm3p.py:987-996)
            if beatmap_outputs is None:
                raise ValueError("output_logits needs input_ids")
            hs = beatmap_outputs.last_hidden_state
            V = self.config.beatmap_config.vocab_size
            n_sel = None
            if sel_rows is not None:  # the head on the row block: zero rows (label -100) fill it up as in the last layer
                n_sel = hs.shape[0]
                bc = self.config.beatmap_config
                n_pad = K.row_block_rows(n_sel, bc.hidden_size, bc.intermediate_size)
                if n_pad != n_sel:
                    hs = _ZeroPadRowsFn.apply(hs, n_pad)
                    sel_labels = torch.cat((sel_labels, sel_labels.new_full((n_pad - n_sel,), -100)))
                labels = sel_labels
            head_args = (hs.reshape(-1, hs.size(-1)), self.head.dense.weight, self.head.dense.bias, self.head.norm.weight,
                         self.decoder.weight, self.decoder.bias, self.config.beatmap_config.norm_eps)
            mlm = lp = None
            if labels is not None and return_loss and self.logit_free_mlm_loss and self.training:
                mlm = _MLMHeadLogitFreeLossFn.apply(*head_args, labels, kwargs.get("num_items_in_batch"))  # (logits stays None)
            elif labels is not None and return_loss:
                lp, mlm = _MLMHeadLossFn.apply(*head_args, labels, kwargs.get("num_items_in_batch"))
            else:
                lp = _MLMHeadFn.apply(*head_args)
            if lp is not None and hs.dim() == 3:
                logits = lp.view(hs.size(0), hs.size(1), -1)[..., :V]
            elif lp is not None:
                # caller-supplied unpadded rows: logits (total_nnz, V), re-padded like the reference's flash_attention_2 branch
                # (_pad_cm3p_output, ref:cm3p/modeling_cm3p.py:999-1001) when the padded geometry was given
                logits = lp[:, :V] if n_sel is None else lp[:n_sel, :V]  # (labelled_rows_last_layer: the selected rows, in their order)
                if indices is not None and batch_size is not None and seq_len is not None:
                    idx64 = indices.to(device=lp.device, dtype=torch.int64).reshape(-1).contiguous()
                    rows = int(batch_size) * int(seq_len)
                    # the scatter kernel writes row indices[i] of a [batch_size * seq_len] buffer for every packed row i: a wrong
                    # `indices` would be an out-of-bounds write on the GPU, not an exception - checked on the host (one read)
                    if idx64.numel() != lp.shape[0]:
                        raise ValueError(f"indices has {idx64.numel()} entries but there are {lp.shape[0]} unpadded rows")
                    if idx64.numel():
                        lo, hi = torch.stack((idx64.min(), idx64.max())).tolist()
                        if lo < 0 or hi >= rows:
                            raise ValueError(f"indices must lie in [0, batch_size * seq_len = {rows}); got [{lo}, {hi}]")
                    # the reference re-pads under no_grad only when labels are given and repad_logits_with_grad is off
                    # (ref:cm3p/modeling_cm3p.py:1000-1001); otherwise the padded logits stay differentiable
                    keep_grad = labels is None or bool(getattr(self.config.beatmap_config, "repad_logits_with_grad", False))
                    if keep_grad and lp.requires_grad:
                        padded = _PadRowsFn.apply(lp, idx64, lp.shape[0], rows)
                    else:
                        padded = K.scatter_rows(lp.detach().contiguous(), idx64, rows)
                    logits = padded.view(int(batch_size), int(seq_len), -1)[..., :V]
            if mlm is not None:
                if torch.is_tensor(loss):
                    loss = _AddScaledFn.apply(loss, mlm, 0.5)
                else:
                    loss = _AddScaledFn.apply(torch.zeros((), dtype=torch.float32, device=mlm.device), mlm, 0.5)

        return CM3POutput(loss=loss, logits_per_beatmap=logits_per_beatmap, logits_per_metadata=logits_per_metadata,
                          metadata_embeds=metadata_embeds, beatmap_embeds=beatmap_embeds, logits=logits,
                          metadata_model_output=metadata_outputs, beatmap_model_output=beatmap_outputs)

    @torch.no_grad()
    def predict_tokens(self, input_ids: Tensor, input_features: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None,
                       position_ids: Optional[Tensor] = None, positions=None, k: int = 5) -> MaskedTokenPredictions:
        """CM3PForMaskedLM.predict_tokens on this model's decoder head (`has_decoder_head`): the k most likely tokens at the selected
        positions - `forward(...).logits` followed by torch.topk there - without the (B, S, vocab) logits.  Only the beatmap tower
        runs, its last layer on the selected rows; `unpad_inputs` is honoured as in forward."""
        k = _check_prediction_call(self, k)
        if not self.config.has_decoder_head:
            raise ValueError("Cannot return logits when the model is not configured with a decoder head.")
        if self.beatmap_model.cls_only_last_layer:
            raise ValueError("cls_only_last_layer with the MLM head (has_decoder_head / output_logits): the head reads every row of the beatmap "
                             "tower's last layer; switch cls_only_last_layer off on the beatmap tower")
        rows = _prediction_rows(positions, attention_mask, input_ids.shape[0], input_ids.shape[1], input_ids.device)
        if rows.numel() == 0:
            return _empty_predictions(k, input_ids.device)
        if self.unpad_inputs is not None or getattr(self.config, "_attn_implementation", None) == "flash_attention_2":
            self.beatmap_model.unpad_inputs = True if self.unpad_inputs is None else bool(self.unpad_inputs)
        out = self.beatmap_model(input_ids=input_ids, input_features=input_features, attention_mask=attention_mask, position_ids=position_ids,
                                 output_pooler=False, last_layer_rows=rows)
        return _predict_rows(out.last_hidden_state, rows, self.head, self.decoder, self.config.beatmap_config.norm_eps, k)


# ----------------------------------------------------------------------------------------------- stand-alone variants
class CM3PMetadataModelWithProjection(CM3PPreTrainedModel):
    """Metadata tower + projection, un-normalised (ref:cm3p/modeling_cm3p.py:1015-1065)."""

    config_class = CM3PMetadataConfig

    def __init__(self, config: CM3PMetadataConfig):
        super().__init__(config)
        self.metadata_model = CM3PMetadataTransformer(config)
        self.metadata_projection = nn.Linear(config.hidden_size, config.projection_dim, bias=False)
        self.post_init()

    def get_input_embeddings(self) -> nn.Module:
        return self.metadata_model.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.metadata_model.set_input_embeddings(value)

    def forward(self, input_ids: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None, output_attentions=None,
                output_hidden_states=None) -> CM3PMetadataModelOutput:
        out = self.metadata_model(input_ids=input_ids, attention_mask=attention_mask, output_attentions=output_attentions,
                                  output_hidden_states=output_hidden_states)
        p = out.pooler_output
        emb = _ProjectFn.apply(p.reshape(-1, p.size(-1)), self.metadata_projection.weight).view(*p.shape[:-1], -1)
        return CM3PMetadataModelOutput(metadata_embeds=emb, last_hidden_state=out.last_hidden_state, hidden_states=out.hidden_states,
                                       attentions=out.attentions)


class CM3PBeatmapModelWithProjection(CM3PPreTrainedModel):
    """Beatmap tower + projection, un-normalised (ref:cm3p/modeling_cm3p.py:1068-1128)."""

    config_class = CM3PBeatmapConfig

    def __init__(self, config: CM3PBeatmapConfig):
        super().__init__(config)
        self.beatmap_model = CM3PBeatmapTransformer(config)
        self.beatmap_projection = nn.Linear(config.hidden_size, config.projection_dim, bias=False)
        self.post_init()

    def get_input_embeddings(self) -> nn.Module:
        return self.beatmap_model.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.beatmap_model.set_input_embeddings(value)

    def forward(self, input_ids: Optional[Tensor] = None, input_features: Optional[Tensor] = None,
                attention_mask: Optional[Tensor] = None, position_ids: Optional[Tensor] = None,
                inputs_embeds: Optional[Tensor] = None, output_attentions=None, output_hidden_states=None) -> CM3PBeatmapModelOutput:
        out = self.beatmap_model(input_ids=input_ids, input_features=input_features, attention_mask=attention_mask,
                                 position_ids=position_ids, inputs_embeds=inputs_embeds, output_attentions=output_attentions,
                                 output_hidden_states=output_hidden_states)
        emb = _ProjectFn.apply(out.pooler_output, self.beatmap_projection.weight)
        return CM3PBeatmapModelOutput(beatmap_embeds=emb, pooler_output=out.pooler_output, last_hidden_state=out.last_hidden_state,
                                      hidden_states=out.hidden_states, attentions=out.attentions, audio_model_output=out.audio_model_output)


class _TakeRowsFn(torch.autograd.Function):
    """x [R, H] fp32 or bf16 -> x[idx] (boolean-mask row selection of the sparse MLM head); backward scatters into zeros (rows of
    x's dtype both ways: bf16 rows move through the half-width copies)."""

    @staticmethod
    def forward(ctx, x: Tensor, idx: Tensor):
        ctx.idx, ctx.rows = idx, x.shape[0]
        return K.gather_rows(x.contiguous(), idx)

    @staticmethod
    def backward(ctx, dy: Tensor):
        return K.scatter_rows(dy.contiguous(), ctx.idx, ctx.rows), None


class _ZeroPadRowsFn(torch.autograd.Function):
    """x [n, H] -> [rows, H] with zero rows behind (a copy); backward: the first n rows of the gradient."""

    @staticmethod
    def forward(ctx, x: Tensor, rows: int):
        ctx.n = x.shape[0]
        out = x.new_zeros((rows, x.shape[1]))
        out[:ctx.n].copy_(x)
        return out

    @staticmethod
    def backward(ctx, dy: Tensor):
        return dy[:ctx.n].contiguous(), None


class _WidenRowsFn(torch.autograd.Function):
    """bf16 rows -> the same values as fp32 (exact; dtype plumbing of the pooled CLS rows of caller-packed inputs); backward: the
    fp32 gradient rounded once to bf16 by cm3p_cast_f32_bf16, the dtype the bf16 residual stream takes its gradient in."""

    @staticmethod
    def forward(ctx, x: Tensor):
        return x.float()

    @staticmethod
    def backward(ctx, dy: Tensor):
        return K.cast_bf16(dy.float().contiguous())


class CM3PForMaskedLM(CM3PPreTrainedModel):
    """Beatmap tower + MLM head + ForMaskedLM loss (ref:cm3p/modeling_cm3p.py:1241-1377), including `sparse_prediction`
    (head and decoder on the labelled positions only, :1349-1357)."""

    config_class = CM3PBeatmapConfig
    _tied_weights_keys = {"decoder.weight": "beatmap_model.encoder.embeddings.tok_embeddings.weight"}

    def __init__(self, config: CM3PBeatmapConfig):
        super().__init__(config)
        self.beatmap_model = CM3PBeatmapTransformer(config)
        self.head = CM3PPredictionHead(config)
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size, bias=config.decoder_bias)
        self.sparse_prediction = bool(getattr(config, "sparse_prediction", False))
        self.sparse_pred_ignore_index = int(getattr(config, "sparse_pred_ignore_index", -100))
        # opt-in (not in config or state dict): with sparse_prediction, in training mode with labels, the tower's last layer runs on the
        # labelled rows only (CM3PEncoder.forward's last_layer_rows) instead of on all rows followed by the row selection
        self.labelled_rows_last_layer = False
        # opt-in (not in config or state dict): in training mode with labels the loss comes from _MLMHeadLogitFreeLossFn, which never
        # stores the [rows, vocab] logits, and the output's `logits` is None; evaluation and calls without labels return logits as ever
        self.logit_free_mlm_loss = False
        self.post_init()

    def get_output_embeddings(self):
        return self.decoder

    def set_output_embeddings(self, new_embeddings: nn.Linear):
        self.decoder = new_embeddings

    def get_input_embeddings(self) -> nn.Module:
        return self.beatmap_model.get_input_embeddings()

    def forward(self, input_ids: Optional[Tensor] = None, input_features: Optional[Tensor] = None,
                attention_mask: Optional[Tensor] = None, sliding_window_mask=None, position_ids: Optional[Tensor] = None,
                inputs_embeds: Optional[Tensor] = None, labels: Optional[Tensor] = None, indices=None, cu_seqlens=None,
                max_seqlen=None, batch_size=None, seq_len=None, output_attentions=None, output_hidden_states=None, **kwargs):
        from transformers.modeling_outputs import MaskedLMOutput

        if self.beatmap_model.cls_only_last_layer:
            raise ValueError("CM3PForMaskedLM with cls_only_last_layer: the MLM head reads every row of the last layer; switch it off")
        sparse = self.sparse_prediction and labels is not None
        idx = None
        if sparse:  # keep the labelled tokens only (row selection by index; the count needs one host read, as in the reference)
            labels = labels.reshape(-1)
            idx = torch.nonzero(labels != self.sparse_pred_ignore_index).flatten()
            labels = labels[idx]
        on_rows = sparse and self.labelled_rows_last_layer and self.training and indices is None and cu_seqlens is None and not output_attentions
        out = self.beatmap_model(input_ids=input_ids, input_features=input_features, attention_mask=attention_mask,
                                 position_ids=position_ids, inputs_embeds=inputs_embeds, indices=indices, cu_seqlens=cu_seqlens,
                                 output_attentions=output_attentions, output_hidden_states=output_hidden_states, output_pooler=False,
                                 last_layer_rows=idx if on_rows else None)
        hs = out.last_hidden_state
        V = self.config.vocab_size
        if on_rows:
            rows = hs  # (n, H): the labelled rows already
        else:
            Bq, Sq, Hq = hs.shape
            rows = hs.reshape(Bq * Sq, Hq)
            if sparse:
                rows = _TakeRowsFn.apply(rows, idx)
        head_args = (rows, self.head.dense.weight, self.head.dense.bias, self.head.norm.weight, self.decoder.weight, self.decoder.bias,
                     self.config.norm_eps)
        loss = None
        if labels is not None and self.logit_free_mlm_loss and self.training:
            loss = _MLMHeadLogitFreeLossFn.apply(*head_args, labels, kwargs.get("num_items_in_batch"))
            return MaskedLMOutput(loss=loss, logits=None, hidden_states=out.hidden_states, attentions=out.attentions)
        if labels is not None:
            lp, loss = _MLMHeadLossFn.apply(*head_args, labels, kwargs.get("num_items_in_batch"))
        else:
            lp = _MLMHeadFn.apply(*head_args)
        logits = lp[..., :V] if sparse else lp.view(Bq, Sq, -1)[..., :V]
        return MaskedLMOutput(loss=loss, logits=logits, hidden_states=out.hidden_states, attentions=out.attentions)

    @torch.no_grad()
    def predict_tokens(self, input_ids: Tensor, input_features: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None,
                       position_ids: Optional[Tensor] = None, positions=None, k: int = 5) -> MaskedTokenPredictions:
        """The k most likely tokens at the selected positions of a padded (B, S) batch without the (B, S, vocab) logits: what
        `forward(...).logits` followed by torch.topk at those positions gives (argmax for k = 1), from cm3p_mlm_topk.
        positions: a (B, S) mask (nonzero = predict), a 1-D int64 list of strictly ascending global rows b * S + s, or None for every
        position whose attention_mask is nonzero; with `unpad_inputs` every selected position must be an unmasked one.  The tower's
        last layer, its final norm and the head run on the selected rows only (CM3PEncoder.forward's last_layer_rows).  An empty
        selection returns empty tensors and launches nothing.  Evaluation semantics: a model in training mode raises ValueError."""
        k = _check_prediction_call(self, k)
        if self.beatmap_model.cls_only_last_layer:
            raise ValueError("CM3PForMaskedLM with cls_only_last_layer: the MLM head reads every row of the last layer; switch it off")
        rows = _prediction_rows(positions, attention_mask, input_ids.shape[0], input_ids.shape[1], input_ids.device)
        if rows.numel() == 0:
            return _empty_predictions(k, input_ids.device)
        out = self.beatmap_model(input_ids=input_ids, input_features=input_features, attention_mask=attention_mask, position_ids=position_ids,
                                 output_pooler=False, last_layer_rows=rows)
        return _predict_rows(out.last_hidden_state, rows, self.head, self.decoder, self.config.norm_eps, k)


class _AddBiasFn(torch.autograd.Function):
    """x [rows, n] fp32 + bias [n]; backward: db = column sums."""

    @staticmethod
    def forward(ctx, x: Tensor, bias: Tensor):
        ctx.bdtype = bias.dtype
        return K.add_bias_(x.detach().clone().contiguous(), _f32(bias.detach()).contiguous())

    @staticmethod
    def backward(ctx, dy: Tensor):
        dy = dy.contiguous()
        return dy, K.colsum_f32(dy).to(ctx.bdtype)


class _PointwiseLossFn(torch.autograd.Function):
    """Mean MSELoss (kind 0) / BCEWithLogitsLoss (kind 1)."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, kind: int):
        loss, dx = K.pointwise_loss(x.detach().contiguous(), y.detach().to(torch.float32).contiguous(), kind)
        ctx.dx = dx
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        return K.scale_by(ctx.dx, g.reshape(1).contiguous()), None, None


class _MaskedCrossEntropyFn(torch.autograd.Function):
    """CrossEntropyLoss() of the single-label classifier (ref:cm3p/modeling_cm3p.py:1214-1216): rows labelled -100 (the default
    ignore_index) get no loss and no gradient, and the mean is over the labelled rows only.  A batch without a labelled row gives
    loss 0 and a zero gradient (torch returns NaN there; the masked-LM loss makes the same choice, inv_valid_count's max(n, 1))."""

    @staticmethod
    def forward(ctx, logits: Tensor, target: Tensor):
        x = logits.detach().contiguous()
        inv = K.inv_valid_count(target, -100)
        loss_rows, dx = K.cross_entropy_masked(x, x.shape[1], target, -100, 1.0, inv, True)
        ctx.dx = dx
        return K.scale_by(K.sum_f32(loss_rows, 1.0), inv).reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        return K.scale_by(ctx.dx, g.reshape(1).contiguous()), None


@dataclass
class BeatmapClassifierOutput(ModelOutput):
    loss: Optional[torch.FloatTensor] = None
    logits: Optional[torch.FloatTensor] = None
    hidden_states: Optional[tuple] = None
    attentions: Optional[tuple] = None


class CM3PForBeatmapClassification(CM3PPreTrainedModel):
    """Beatmap tower + linear classifier on the pooled output with the three HF loss flavours
    (ref:cm3p/modeling_cm3p.py:1137-1225)."""

    config_class = CM3PBeatmapConfig
    base_model_prefix = "beatmap_model"

    def __init__(self, config: CM3PBeatmapConfig):
        super().__init__(config)
        self.num_labels = config.num_labels
        self.beatmap_model = CM3PBeatmapTransformer(config)
        self.classifier = nn.Linear(config.hidden_size, config.num_labels) if config.num_labels > 0 else nn.Identity()
        self.post_init()

    def forward(self, input_ids: Optional[Tensor] = None, input_features: Optional[Tensor] = None,
                attention_mask: Optional[Tensor] = None, position_ids: Optional[Tensor] = None,
                inputs_embeds: Optional[Tensor] = None, labels: Optional[Tensor] = None, output_attentions=None,
                output_hidden_states=None) -> BeatmapClassifierOutput:
        out = self.beatmap_model(input_ids=input_ids, input_features=input_features, attention_mask=attention_mask,
                                 position_ids=position_ids, inputs_embeds=inputs_embeds, output_attentions=output_attentions,
                                 output_hidden_states=output_hidden_states)
        logits = out.pooler_output
        if self.num_labels > 0:
            logits = _AddBiasFn.apply(_ProjectFn.apply(out.pooler_output, self.classifier.weight), self.classifier.bias)
        loss = None
        if labels is not None:
            labels = labels.to(logits.device)
            if self.config.problem_type is None:  # the reference's (HF's) inference rule, :1198-1204
                if self.num_labels == 1:
                    self.config.problem_type = "regression"
                elif self.num_labels > 1 and labels.dtype in (torch.long, torch.int):
                    self.config.problem_type = "single_label_classification"
                else:
                    self.config.problem_type = "multi_label_classification"
            want = logits.shape[0] if self.config.problem_type == "single_label_classification" else logits.numel()
            if labels.numel() != want:  # (the torch losses raise on a size mismatch; the kernels would read past the labels)
                raise ValueError(f"labels have {labels.numel()} entries, expected {want}")
            if self.config.problem_type == "regression":
                loss = _PointwiseLossFn.apply(logits.reshape(-1), labels.reshape(-1), 0)
            elif self.config.problem_type == "single_label_classification":
                loss = _MaskedCrossEntropyFn.apply(logits, labels.reshape(-1).to(torch.int64).contiguous())
            else:
                loss = _PointwiseLossFn.apply(logits.reshape(-1), labels.reshape(-1), 1)
        return BeatmapClassifierOutput(loss=loss, logits=logits, hidden_states=out.hidden_states, attentions=out.attentions)



def _register():
    for cfg, cls in ((CM3PMetadataConfig, CM3PMetadataModel), (CM3PBeatmapConfig, CM3PBeatmapModel), (CM3PConfig, CM3PModel)):
        try:
            AutoModel.register(cfg, cls)
        except ValueError:
            pass
    try:
        from transformers import AutoModelForMaskedLM, AutoModelForSequenceClassification

        AutoModelForMaskedLM.register(CM3PBeatmapConfig, CM3PForMaskedLM)
        AutoModelForSequenceClassification.register(CM3PBeatmapConfig, CM3PForBeatmapClassification)
    except ValueError:
        pass


_register()

__all__ = [
    "CM3PModel", "CM3PPreTrainedModel", "CM3PMetadataModel", "CM3PBeatmapModel", "CM3PMetadataTransformer",
    "CM3PBeatmapTransformer", "CM3PAudioEncoder", "CM3POutput", "CM3PForMaskedLM", "CM3PForBeatmapClassification",
    "CM3PMetadataModelWithProjection", "CM3PBeatmapModelWithProjection", "cm3p_loss_hip",
]
