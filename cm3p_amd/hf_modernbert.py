"""Seam 2b of SURVEY.md section 8(b): a whole Hugging Face ModernBERT on the fused encoder stack.

`cm3p_amd.hf_attention` (seam 2) hands only the attention function to the HIP kernels.  This module replaces the MODEL: a
`ModernBertModel` of the installed `transformers` is architecturally what `CM3PEncoder` runs (same submodule and parameter names, same
layer: LN -> Wqkv + RoPE -> attention (global, or the |i - j| <= sliding_window band; key padding) -> Wo + residual -> LN -> Wi -> GeGLU ->
Wo + residual; final LN), so the fused stack - Wqkv + RoPE in the GEMM epilogue, the pipelined forward with pre-scaled q, the
five-product backward, GeGLU in the store phases, the bf16 residual streams, unpadded execution, per-layer recompute - serves any
ModernBERT checkpoint whose configuration passes `encoder_config`.

    from cm3p_amd.hf_modernbert import FusedModernBertModel, FusedModernBertForMaskedLM, fuse, unfuse
    model = FusedModernBertModel.from_pretrained(local_dir).cuda()          # an ordinary HF checkpoint directory
    model = fuse(ModernBertForSequenceClassification.from_pretrained(...))  # swap the tower of a model that already exists

Refused at construction (NotImplementedError naming the field and its value): a `rope_type` other than "default", `norm_bias` /
`attention_bias` / `mlp_bias`, `hidden_activation != "gelu"`, and the head sizes / extents `encoder._check_supported` refuses.

All arithmetic of the tower runs on libcm3p_hip.so through the encoder's autograd nodes; there is no torch-op fallback and inputs must
live on the GPU.  Nothing here adds a kernel or a C-ABI symbol.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn
from transformers import ModernBertConfig, ModernBertModel
from transformers.modeling_outputs import BaseModelOutput, MaskedLMOutput
from transformers.models.modernbert.modeling_modernbert import (
    ModernBertForMaskedLM,
    ModernBertForSequenceClassification,
    ModernBertForTokenClassification,
    ModernBertPredictionHead,
    ModernBertPreTrainedModel,
)

from . import kernels as K
from .encoder import CM3PEncoder, _check_supported

Tensor = torch.Tensor
_WRAPPERS = (ModernBertForMaskedLM, ModernBertForSequenceClassification, ModernBertForTokenClassification)


# ----------------------------------------------------------------------------------------------- config translation
class FusedEncoderConfig:
    """What `CM3PEncoder` reads, filled from a `ModernBertConfig` by `encoder_config` (a snapshot: later edits of the HF config do
    not reach it).  `is_global_layer(i)` follows `layer_types[i]`, so any pattern of full / sliding layers works, not only "every n"."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def is_global_layer(self, i: int) -> bool:
        return self.layer_types[i] == "full_attention"

    @property
    def half_window(self) -> int:
        """|q - kv| <= half_window in sliding layers: `ModernBertConfig.sliding_window` (= local_attention // 2) as it is."""
        return self.sliding_window

    def __repr__(self):
        return f"FusedEncoderConfig({self.__dict__})"


def encoder_config(hf_config: ModernBertConfig) -> FusedEncoderConfig:
    """`ModernBertConfig` of the installed `transformers` -> the configuration `CM3PEncoder` runs.  The caller's object is only read.
    Raises NotImplementedError (naming the field and its value) for what the kernels do not implement."""
    c = hf_config
    layer_types = list(c.layer_types)
    if len(layer_types) != c.num_hidden_layers:
        raise ValueError(f"layer_types has {len(layer_types)} entries for num_hidden_layers={c.num_hidden_layers}")
    for i, t in enumerate(layer_types):
        if t not in ("full_attention", "sliding_attention"):
            raise NotImplementedError(f"cm3p_amd fused ModernBERT: layer_types[{i}]={t!r} (full_attention and sliding_attention only)")
    rope = c.rope_parameters or {}
    thetas = {}
    for kind in ("full_attention", "sliding_attention"):
        params = rope.get(kind)
        if params is None:
            if kind in layer_types:
                raise ValueError(f"rope_parameters has no entry for {kind}")
            params = {"rope_type": "default", "rope_theta": ModernBertConfig.default_theta["global" if kind == "full_attention" else "local"]}
        rope_type = params.get("rope_type", "default")
        if rope_type != "default":
            raise NotImplementedError(f"cm3p_amd fused ModernBERT: rope_parameters[{kind!r}]['rope_type']={rope_type!r}: "
                                      "only rope_type 'default' (the rotary tables are theta ** (-2 i / head_dim))")
        thetas[kind] = float(params["rope_theta"])
    for flag in ("norm_bias", "attention_bias", "mlp_bias"):
        if getattr(c, flag, False):
            raise NotImplementedError(f"cm3p_amd fused ModernBERT: {flag}={getattr(c, flag)!r} is not supported (the kernels have no bias terms)")
    if c.hidden_activation != "gelu":
        raise NotImplementedError(f"cm3p_amd fused ModernBERT: hidden_activation={c.hidden_activation!r}; the GeGLU kernels implement 'gelu'")
    out = FusedEncoderConfig(
        vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
        num_attention_heads=c.num_attention_heads, hidden_activation=c.hidden_activation, norm_eps=c.norm_eps, norm_bias=False,
        attention_bias=False, mlp_bias=False, pad_token_id=c.pad_token_id, layer_types=layer_types, sliding_window=int(c.sliding_window),
        global_rope_theta=thetas["full_attention"], local_rope_theta=thetas["sliding_attention"],
        attention_dropout=float(c.attention_dropout or 0.0), embedding_dropout=float(c.embedding_dropout or 0.0),
        mlp_dropout=float(c.mlp_dropout or 0.0), initializer_range=c.initializer_range, initializer_cutoff_factor=c.initializer_cutoff_factor)
    try:
        _check_supported(out)  # head size, hidden_size / intermediate_size multiples of 8, dropout ranges
    except NotImplementedError as e:
        raise NotImplementedError(f"{e} (num_attention_heads={c.num_attention_heads}, hidden_size={c.hidden_size}, "
                                  f"intermediate_size={c.intermediate_size})") from None
    return out


class _ToDtypeFn(torch.autograd.Function):
    """fp32 rows -> the parameters' dtype (one rounding; bf16 through cm3p_cast_f32_bf16); backward widens the gradient exactly."""

    @staticmethod
    def forward(ctx, x: Tensor, dtype: torch.dtype):
        return K.cast_bf16(x.contiguous()) if dtype == torch.bfloat16 else x.to(dtype)

    @staticmethod
    def backward(ctx, dy: Tensor):
        return dy.float(), None


def _init_encoder_leaf(module) -> bool:
    """ModernBERT's initialisation of the tower (truncated normal: 'in' / embedding std = initializer_range, 'out' std =
    initializer_range / sqrt(2 L)): the leaves carry their role's std as a tag (HF visits a
    module that owns no parameter itself only to skip it).  -> whether `module` was one of them
    (everything else is the parent class's business)."""
    from transformers import initialization as init

    tag = getattr(module, "_cm3p_init", None)
    if tag is None:
        return False
    std, cutoff = tag
    init.trunc_normal_(module.weight, mean=0.0, std=std, a=-cutoff * std, b=cutoff * std)
    if getattr(module, "bias", None) is not None:
        init.zeros_(module.bias)
    return True


# ----------------------------------------------------------------------------------------------- the tower
class FusedModernBertModel(ModernBertPreTrainedModel):
    """`ModernBertModel` on the fused HIP encoder stack.  Submodule and parameter names are `ModernBertModel`'s (`embeddings.
    tok_embeddings`, `embeddings.norm`, `layers.N.attn.Wqkv`, ...), so `from_pretrained` / `save_pretrained` of an ordinary checkpoint
    directory and `load_state_dict(hf_model.state_dict())` work; the nn.Linear / nn.LayerNorm / nn.Embedding members are parameter
    containers whose torch forward is never called.

    dtype: the output follows the parameters.  An fp32 model runs the fp32 residual stream and returns fp32.  A model moved
    `.to(torch.bfloat16)` returns bf16, and its forward-only calls run the bf16 residual stream (every LayerNorm reads and writes bf16,
    bf16 residual adds: what a bf16 HF model computes); calls that record a backward keep the fp32 stream unless
    `set_residual_dtype(torch.bfloat16, training=True)` asked for the bf16 one, and their output is rounded to bf16 once.
    `set_residual_dtype` overrides the rule for fp32 masters too.

    Dropout: `embedding_dropout`, `attention_dropout` and `mlp_dropout` are honoured in `train()` mode, with the masks of the kernels'
    own counter-based generator (csrc/dropout_rng.h; one seed per forward drawn from torch's default CPU generator),
    NOT torch's device RNG stream: a run is reproducible under `torch.manual_seed`, but its masks are not those the torch model draws.

    `unpad_inputs = True` runs right-padded batches on their valid tokens only (padding positions of the outputs are zeros);
    `gradient_checkpointing_enable()` maps to the encoder's per-layer recompute (bit-identical loss and gradients)."""

    def __init__(self, config: ModernBertConfig):
        super().__init__(config)
        self.config = config
        enc = CM3PEncoder(encoder_config(config))
        self.__dict__["_encoder"] = enc  # not a registered child: its three members are this model's, under ModernBertModel's names
        self.embeddings = enc.embeddings
        self.layers = enc.layers
        self.final_norm = enc.final_norm
        self.unpad_inputs = False
        self._residual_follows_params = True
        self.__dict__["_unfused"] = None  # the ModernBertModel this tower was made from by fuse(), for unfuse()
        self.post_init()

    # -- plumbing shared with the encoder
    @property
    def encoder(self) -> CM3PEncoder:
        return self.__dict__["_encoder"]

    @property
    def gradient_checkpointing(self) -> bool:
        return self.encoder.gradient_checkpointing

    @gradient_checkpointing.setter
    def gradient_checkpointing(self, value: bool) -> None:  # (what gradient_checkpointing_enable / _disable set)
        self.encoder.gradient_checkpointing = bool(value)

    @property
    def cls_only_last_layer(self) -> bool:
        """`CM3PEncoder.cls_only_last_layer` of this tower's encoder (opt-in, off by default): the last layer and the final norm run
        on row 0 of every sequence only and `last_hidden_state` is (B, 1, H) - with `output_hidden_states` so is the last entry.  A
        sequence-classification model returned by `fuse()` with `classifier_pooling == "cls"` reads `last_hidden_state[:, 0]` and runs
        unchanged on it.  Heads that read every row must leave the switch off: `classifier_pooling == "mean"` (the HF head would
        broadcast the one row against the mask without an error), token classification, question answering;
        `FusedModernBertForMaskedLM` refuses the call itself."""
        return self.encoder.cls_only_last_layer

    @cls_only_last_layer.setter
    def cls_only_last_layer(self, value: bool) -> None:
        self.encoder.cls_only_last_layer = bool(value)

    def train(self, mode: bool = True):
        self.encoder.train(mode)  # dropout and per-layer recompute follow the encoder's own flag
        return super().train(mode)

    def set_residual_dtype(self, dtype: Optional[torch.dtype], training: bool = False):
        """As `CM3PPreTrainedModel.set_residual_dtype`: torch.bfloat16 runs forward-only calls on the bf16 residual stream (with
        training=True also the calls that record a backward); None / torch.float32 keep the fp32 stream.  After this call the stream no
        longer follows the parameters' dtype.  Returns the model."""
        if dtype is not None and dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"residual_dtype must be None, torch.float32 or torch.bfloat16, got {dtype!r}")
        self._residual_follows_params = False
        self.encoder.residual_dtype = dtype
        if training:
            self.encoder.train_residual_dtype = dtype
        return self

    def get_input_embeddings(self):
        return self.embeddings.tok_embeddings

    def set_input_embeddings(self, value):
        self.embeddings.tok_embeddings = value

    def _check_and_adjust_attn_implementation(self, attn_implementation, *args, **kwargs):
        # attention always runs in the HIP flash kernels: the configured name selects nothing
        return attn_implementation if attn_implementation is not None else "sdpa"

    @torch.no_grad()
    def _init_weights(self, module):
        if not _init_encoder_leaf(module):
            super()._init_weights(module)

    def forward(self, input_ids: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None, position_ids: Optional[Tensor] = None,
                inputs_embeds: Optional[Tensor] = None, output_attentions: Optional[bool] = None, output_hidden_states: Optional[bool] = None,
                return_dict: Optional[bool] = None, last_layer_rows: Optional[Tensor] = None, **kwargs) -> BaseModelOutput:
        """last_layer_rows: CM3PEncoder.forward's argument, passed through - last_hidden_state (and the last hidden state) are then (n, H).
        -> BaseModelOutput(last_hidden_state (B, S, H), hidden_states: L + 1 tensors when asked for - the stack's input, the output of
        layers 0 .. L-2 (detached) and, as the installed ModernBertModel reports it, last_hidden_state itself in the last place -,
        attentions: the L eager-semantics probability tensors (B, nh, S, S) fp32 when asked for).  CPU inputs raise."""
        cfg = self.config
        output_attentions = bool(cfg.output_attentions if output_attentions is None else output_attentions)
        output_hidden_states = bool(cfg.output_hidden_states if output_hidden_states is None else output_hidden_states)
        return_dict = bool(getattr(cfg, "return_dict", True) if return_dict is None else return_dict)
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        if isinstance(attention_mask, dict) or (attention_mask is not None and attention_mask.dim() != 2):
            raise NotImplementedError("cm3p_amd fused ModernBERT: attention_mask must be the 2-D (batch, key) padding mask; the kernels "
                                      "build the sliding window themselves")
        enc = self.encoder
        pdtype = self.final_norm.weight.dtype
        if self._residual_follows_params:
            enc.residual_dtype = torch.bfloat16 if pdtype == torch.bfloat16 else None
        out = enc(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, inputs_embeds=inputs_embeds,
                  unpad=bool(self.unpad_inputs) and not output_attentions, output_hidden_states=output_hidden_states,
                  output_attentions=output_attentions, last_layer_rows=last_layer_rows)
        hiddens = attns = None
        if output_attentions:
            y, hiddens, attns = out
            if not output_hidden_states:
                hiddens = None
        elif output_hidden_states:
            y, hiddens = out
        else:
            y = out
        if y.dtype != pdtype and pdtype != torch.float32:
            y = _ToDtypeFn.apply(y, pdtype)
            if hiddens is not None:
                hiddens = tuple(_ToDtypeFn.apply(h, pdtype) for h in hiddens)
        if hiddens is not None:
            # the installed ModernBertModel reports last_hidden_state (after the final norm) as the last entry, not the last layer's
            # raw output; the entries before it are the encoder's detached copies
            hiddens = tuple(hiddens[:-1]) + (y,)
        if not return_dict:
            return tuple(v for v in (y, hiddens, attns) if v is not None)
        return BaseModelOutput(last_hidden_state=y, hidden_states=hiddens, attentions=attns)


# ----------------------------------------------------------------------------------------------- masked LM
class FusedModernBertForMaskedLM(ModernBertPreTrainedModel):
    """`ModernBertForMaskedLM` with the fused tower AND the fused head / loss of `CM3PForMaskedLM` (`_mlm_head_forward` /
    `_MLMHeadLossFn`: dense -> GELU -> LayerNorm -> decoder with the vocabulary padded to a multiple of 64 internally, masked cross
    entropy with the device-side denominator, the logits' gradient written once in bf16).  Parameter names are the HF class's, so the
    same checkpoints load; `decoder.weight` stays tied to the embedding table, whose gradient is then the sum of the embedding backward
    and the decoder's weight gradient.  `sparse_prediction` runs head and decoder on the labelled positions only.  Logits are fp32."""

    _tied_weights_keys = {"decoder.weight": "model.embeddings.tok_embeddings.weight"}

    def __init__(self, config: ModernBertConfig):
        super().__init__(config)
        self.config = config
        if config.classifier_activation != "gelu":
            raise NotImplementedError(f"cm3p_amd fused ModernBERT: classifier_activation={config.classifier_activation!r}; the MLM head kernels implement 'gelu'")
        self.model = FusedModernBertModel(config)
        self.head = ModernBertPredictionHead(config)  # parameter container (dense, norm): its torch forward is never called
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size, bias=config.decoder_bias)
        # the parent's rule for the head's dense and the decoder ('out' std), as leaf tags like the tower's
        cutoff = config.initializer_cutoff_factor or 3
        self.head.dense._cm3p_init = self.decoder._cm3p_init = (config.initializer_range / (2.0 * config.num_hidden_layers) ** 0.5, cutoff)
        self.sparse_prediction = bool(config.sparse_prediction)
        self.sparse_pred_ignore_index = int(config.sparse_pred_ignore_index)
        # opt-in (not in config or state dict): with sparse_prediction, in training mode with labels, the tower's last layer runs on the
        # labelled rows only (CM3PEncoder.forward's last_layer_rows) instead of on all rows followed by the row selection
        self.labelled_rows_last_layer = False
        # opt-in (not in config or state dict): in training mode with labels the loss comes from _MLMHeadLogitFreeLossFn, which never
        # stores the [rows, vocab] logits (13.2 GB at 8 x 8192 tokens of the default vocabulary), and the output's `logits` is None;
        # evaluation and calls without labels return logits as ever
        self.logit_free_mlm_loss = False
        self.post_init()

    def get_output_embeddings(self):
        return self.decoder

    def set_output_embeddings(self, new_embeddings: nn.Linear):
        self.decoder = new_embeddings

    def set_residual_dtype(self, dtype: Optional[torch.dtype], training: bool = False):
        self.model.set_residual_dtype(dtype, training)
        return self

    def _check_and_adjust_attn_implementation(self, attn_implementation, *args, **kwargs):
        return attn_implementation if attn_implementation is not None else "sdpa"

    @torch.no_grad()
    def _init_weights(self, module):
        if not _init_encoder_leaf(module):
            super()._init_weights(module)

    def forward(self, input_ids: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None, position_ids: Optional[Tensor] = None,
                inputs_embeds: Optional[Tensor] = None, labels: Optional[Tensor] = None, output_attentions: Optional[bool] = None,
                output_hidden_states: Optional[bool] = None, return_dict: Optional[bool] = None, **kwargs) -> MaskedLMOutput:
        from .modeling_cm3p import _MLMHeadFn, _MLMHeadLogitFreeLossFn, _MLMHeadLossFn, _TakeRowsFn

        if self.model.cls_only_last_layer:
            raise ValueError("FusedModernBertForMaskedLM with cls_only_last_layer: the MLM head reads every row of the last layer; switch it off")
        sparse = self.sparse_prediction and labels is not None
        idx = None
        if sparse:  # keep the labelled tokens only (row selection by index; the count needs one host read, as in the HF model)
            labels = labels.reshape(-1)
            idx = torch.nonzero(labels != self.sparse_pred_ignore_index).flatten()
            labels = labels[idx]
        oat = bool(self.config.output_attentions if output_attentions is None else output_attentions)
        on_rows = sparse and self.labelled_rows_last_layer and self.training and not oat
        out = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, inputs_embeds=inputs_embeds,
                         output_attentions=output_attentions, output_hidden_states=output_hidden_states, return_dict=True,
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
            logits = None  # (never formed: the Trainer reads `loss`)
        else:
            if labels is not None:
                lp, loss = _MLMHeadLossFn.apply(*head_args, labels, kwargs.get("num_items_in_batch"))
            else:
                lp = _MLMHeadFn.apply(*head_args)
            logits = lp[..., :V] if sparse else lp.view(Bq, Sq, -1)[..., :V]
        ret_dict = bool(getattr(self.config, "return_dict", True) if return_dict is None else return_dict)
        if not ret_dict:
            return tuple(v for v in (loss, logits, out.hidden_states, out.attentions) if v is not None)
        return MaskedLMOutput(loss=loss, logits=logits, hidden_states=out.hidden_states, attentions=out.attentions)

    @torch.no_grad()
    def predict_tokens(self, input_ids: Tensor, attention_mask: Optional[Tensor] = None, position_ids: Optional[Tensor] = None, positions=None,
                       k: int = 5):
        """Fill-mask without the (B, S, vocab) logits: the k most likely tokens at the selected positions of a padded (B, S) batch, what
        `forward(...).logits` followed by torch.topk there gives (13.2 GB of fp32 logits at 8 x 8192 tokens of a 50368-token vocabulary),
        as `CM3PForMaskedLM.predict_tokens` -> MaskedTokenPredictions.  positions: a (B, S) mask (e.g. input_ids == mask_token_id), a
        1-D int64 list of strictly ascending global rows b * S + s, or None for every unmasked position."""
        from .modeling_cm3p import _check_prediction_call, _empty_predictions, _predict_rows, _prediction_rows

        k = _check_prediction_call(self, k)
        if self.model.cls_only_last_layer:
            raise ValueError("FusedModernBertForMaskedLM with cls_only_last_layer: the MLM head reads every row of the last layer; switch it off")
        rows = _prediction_rows(positions, attention_mask, input_ids.shape[0], input_ids.shape[1], input_ids.device)
        if rows.numel() == 0:
            return _empty_predictions(k, input_ids.device)
        out = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, output_attentions=False,
                         output_hidden_states=False, return_dict=True, last_layer_rows=rows)
        return _predict_rows(out.last_hidden_state, rows, self.head, self.decoder, self.config.norm_eps, k)


# ----------------------------------------------------------------------------------------------- fuse / unfuse
def _share_parameters(src: nn.Module, dst: nn.Module) -> None:
    """Make every parameter of `dst` the nn.Parameter OBJECT `src` holds under the same name (no copy)."""
    have, want = dict(src.named_parameters()), dict(dst.named_parameters())
    if set(have) != set(want):
        raise ValueError(f"parameter names differ: {sorted(set(have) ^ set(want))}")
    for name, p in have.items():
        parent, _, leaf = name.rpartition(".")
        setattr(dst.get_submodule(parent) if parent else dst, leaf, p)


def _fuse_tower(tower: ModernBertModel) -> FusedModernBertModel:
    with torch.device("meta"):  # the fresh parameters are placeholders: nothing is allocated or initialised
        fused = FusedModernBertModel(tower.config)
    _share_parameters(tower, fused)
    fused.__dict__["_unfused"] = tower
    fused.train(tower.training)
    fused.gradient_checkpointing = bool(getattr(tower, "gradient_checkpointing", False))
    return fused


def fuse(model):
    """Put a ModernBERT that already exists on the fused stack.  A bare `ModernBertModel` -> a `FusedModernBertModel` holding the SAME
    nn.Parameter objects (identity, no copy), so an optimizer built on the original keeps training the result.  A
    `ModernBertForMaskedLM` / `ForSequenceClassification` / `ForTokenClassification`: its `.model` is swapped in place and the same
    object comes back; its head stays the torch module it was, and tied weights stay tied.  Idempotent; `unfuse` undoes it."""
    if isinstance(model, (FusedModernBertModel, FusedModernBertForMaskedLM)):
        return model
    if isinstance(model, ModernBertModel):
        return _fuse_tower(model)
    if isinstance(model, _WRAPPERS):
        if not isinstance(model.model, FusedModernBertModel):
            model.model = _fuse_tower(model.model)
        return model
    raise TypeError(f"fuse() takes a ModernBertModel or a ModernBertFor{{MaskedLM,SequenceClassification,TokenClassification}}, got {type(model).__name__}")


def _unfuse_tower(fused: FusedModernBertModel) -> ModernBertModel:
    tower = fused.__dict__.get("_unfused")
    if tower is None:  # made by the constructor / from_pretrained: build the torch tower around the same parameters
        tower = ModernBertModel(fused.config)
    _share_parameters(fused, tower)  # (a no-op after fuse(); load_state_dict and .to() keep parameter identity)
    tower.rotary_emb.to(fused.final_norm.weight.device)  # its buffers did not travel with a .to() of the fused model
    tower.train(fused.training)
    return tower


def unfuse(model):
    """Undo `fuse`: the original `ModernBertModel` (same parameters), or the wrapper with its torch tower back in place."""
    if isinstance(model, FusedModernBertModel):
        return _unfuse_tower(model)
    if isinstance(model, _WRAPPERS):
        if isinstance(model.model, FusedModernBertModel):
            model.model = _unfuse_tower(model.model)
        return model
    if isinstance(model, ModernBertModel):
        return model
    raise TypeError(f"unfuse() takes what fuse() returns, got {type(model).__name__}")


__all__ = ["FusedEncoderConfig", "FusedModernBertModel", "FusedModernBertForMaskedLM", "encoder_config", "fuse", "unfuse"]
