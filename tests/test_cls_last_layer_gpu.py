"""`cls_only_last_layer` (CM3PEncoder / the model classes / the fused ModernBERT tower), `-m gpu`: with the switch on, the last encoder
layer and the final norm run on the pooled CLS row of every sequence only (cm3p_amd/encoder.py _LastLayerRowsFn on csrc/attention_row.hip).

  - the reference-made fixtures whose towers pool by CLS, within the class bounds of tests/test_model_gpu.py (FIX_TOL);
  - a 3-layer head-64 tower whose LAST layer is a sliding one, padded / `unpad` / caller-packed, against the float64 oracle on the CPU;
  - the launch ledger: L - 1 full attention forwards and one row launch, no fused or band backward for the last layer;
  - the fallbacks (head_dim 16, attention dropout in train() mode, checkpointing): (B, 1, H), the bits of row 0 of the switch-off run;
  - the bf16 forward-only stream within the bounds of tests/golden/d64_bf16.safetensors; the refusals; switch off = never set, in bits;
  - a fused ModernBertForSequenceClassification (classifier_pooling "cls") against the installed model on sdpa.
Every measured figure is printed before it is held (`pytest -s`)."""
import functools
import os

import pytest
import torch
from safetensors.torch import load_file

import transformers  # noqa: F401  (a missing transformers is an error here, not a skip)

import test_bf16_residual_gpu as TB
import test_model_gpu as TM
from cases import CASES, make_inputs

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIX_TOL = TM.FIX_TOL
FULL, SLIDE = "full_attention", "sliding_attention"
HIDDEN_TOL, GRAD_TOL = 2e-2, 6e-2  # the class bounds tests/test_hf_modernbert_gpu.py and tests/test_lora_model_gpu.py state
VOCAB, HID, S, LENS = 200, 128, 200, (200, 137, 1)


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm().clamp_min(1e-12)).item()


def _hold(what: str, value: float, bound: float):
    print(f"{what} = {value:.3e} (bound {bound:.0e})")
    assert value <= bound, f"{what} = {value:.3e} > {bound:.0e}"


# ---- reference-made fixtures ---------------------------------------------------------------------------------------------------------
def _fixture_step(name, model, blob, tag):
    out = model(**TM._inputs(blob))
    _hold(f"{tag}: loss", abs(out.loss.item() - blob["loss"].item()), FIX_TOL["loss"])
    _hold(f"{tag}: logits", _rel(out.logits_per_metadata, blob["logits_per_metadata"]), FIX_TOL["logits"])
    _hold(f"{tag}: metadata_embeds", _rel(out.metadata_embeds, blob["metadata_embeds"]), FIX_TOL["embeds"])
    _hold(f"{tag}: beatmap_embeds", _rel(out.beatmap_embeds, blob["beatmap_embeds"]), FIX_TOL["embeds"])
    _hold(f"{tag}: beatmap_pooled", _rel(out.beatmap_model_output.pooler_output, blob["beatmap_pooler_output"]), FIX_TOL["pooled"])
    _hold(f"{tag}: metadata_pooled", _rel(out.metadata_model_output.pooler_output, blob["metadata_pooler_output"]), FIX_TOL["pooled"])
    out.loss.backward()
    params = dict(model.named_parameters())
    checked = 0
    for k, v in blob.items():
        if not k.startswith("grad."):
            continue
        g = params[k[5:]].grad
        assert g is not None, k
        if v.norm() < 1e-8:
            assert g.float().norm().item() < 1e-5, k
        else:
            _hold(f"{tag}: {k}", _rel(g, v), FIX_TOL["grad"])
        checked += 1
    assert checked >= 10
    return out


@pytest.mark.parametrize("name", ["d64_cls_nopad", "d64_short_seq", "d64_audio"])
def test_cls_fixtures_with_the_switch_on_both_towers(name):
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    model = TM._build(name)
    assert model.cls_only_last_layer is False
    model.cls_only_last_layer = True
    assert model.cls_only_last_layer and model.beatmap_model.encoder.cls_only_last_layer and model.metadata_model.encoder.cls_only_last_layer
    assert not model.beatmap_model.audio_encoder.encoder.cls_only_last_layer  # (no pooling there, no switch)
    assert not any("cls_only" in k for k in model.state_dict())
    out = _fixture_step(name, model, blob, f"{name} cls_only")
    c = CASES[name]
    bc, mc = model.config.beatmap_config, model.config.metadata_config
    assert out.beatmap_model_output.last_hidden_state.shape == (c["B"], 1, bc.hidden_size)
    assert out.metadata_model_output.last_hidden_state.shape == (c["B"], 1, mc.hidden_size)


def test_variations_fixture_mean_pooled_metadata_tower_refuses_the_switch_and_the_beatmap_tower_alone_takes_it():
    name = "d64_variations"
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    model = TM._build(name)
    model.cls_only_last_layer = True
    with pytest.raises(ValueError, match="mean pooling"):
        model(**TM._inputs(blob))
    model.cls_only_last_layer = False
    model.beatmap_model.cls_only_last_layer = True
    assert not model.cls_only_last_layer  # (True only when every pooled tower has it)
    out = _fixture_step(name, model, blob, f"{name} cls_only on the beatmap tower")
    c = CASES[name]
    assert out.beatmap_model_output.last_hidden_state.shape == (c["B"], 1, model.config.beatmap_config.hidden_size)
    mh = out.metadata_model_output.last_hidden_state
    assert mh.dim() == 4 and mh.shape[-2] == blob["in.metadata_ids"].shape[-1]  # (B, V, L, H): the metadata tower ran every row


# ---- a sliding last layer against the float64 oracle ---------------------------------------------------------------------------------
def _config(**kw):
    from transformers import ModernBertConfig

    cfg = dict(vocab_size=VOCAB, hidden_size=HID, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2, max_position_embeddings=512,
               layer_types=[FULL, SLIDE, SLIDE], local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2)
    cfg.update(kw)
    return ModernBertConfig(**cfg)


@functools.lru_cache(maxsize=None)
def _state():
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    torch.manual_seed(0)
    return {k: v.clone() for k, v in FusedModernBertModel(_config()).state_dict().items()}


def _model(cls_only=True, **kw):
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    m = FusedModernBertModel(_config(**kw))
    m.load_state_dict(_state(), strict=True)
    m.cls_only_last_layer = cls_only
    return m.cuda().eval()


def _batch():
    g = torch.Generator().manual_seed(0)
    mask = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(3, VOCAB, (len(LENS), S), generator=g) * mask
    w = torch.randn(len(LENS), HID, generator=g)
    return ids, mask, w


@functools.lru_cache(maxsize=None)
def _oracle():
    """The float64 oracle on the CPU, once: the pooled rows h[:, 0] and the gradients of sum(pooled * w)."""
    from oracle import cm3p_oracle as O

    enc = _model().encoder.config
    assert [enc.is_global_layer(i) for i in range(3)] == [True, False, False] and enc.half_window == 64 and S > 2 * 64  # the last layer slides
    cfg = dict(num_attention_heads=enc.num_attention_heads, hidden_size=enc.hidden_size, norm_eps=enc.norm_eps, num_hidden_layers=3,
               local_attention=2 * enc.half_window, global_rope_theta=enc.global_rope_theta, local_rope_theta=enc.local_rope_theta,
               global_attn_every_n_layers=3)
    sd = {k: v.detach().double().cpu().requires_grad_(v.is_floating_point()) for k, v in _state().items()}
    ids, mask, w = _batch()
    collect = []
    y = O.encoder(sd, "", cfg, input_ids=ids, attention_mask=mask, collect=collect)
    pooled = y[:, 0]
    (pooled * w.double()).sum().backward()
    return dict(pooled=pooled.detach(), last_layer=collect[-1][:, 0].detach(), grads={k: v.grad for k, v in sd.items() if v.grad is not None})


@pytest.mark.parametrize("route", ["padded", "unpad", "packed"])
def test_sliding_last_layer_against_the_float64_oracle(route):
    ref = _oracle()
    ids, mask, w = (t.cuda() for t in _batch())
    m = _model().train()  # (no dropout configured: train() only records the backward)
    B = len(LENS)
    if route == "packed":
        keep = mask.bool().flatten()
        cu = torch.tensor([0] + list(torch.tensor(LENS).cumsum(0)), dtype=torch.int32, device="cuda")
        y, hiddens = m.encoder(input_ids=ids.flatten()[keep], cu_seqlens=cu, max_seqlen=max(LENS), output_hidden_states=True)
        assert y.shape == (B, HID) and hiddens[-1].shape == (B, HID) and hiddens[-2].shape == (sum(LENS), HID)
        pooled, last_layer = y, hiddens[-1]
    else:
        m.unpad_inputs = route == "unpad"
        out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        y = out.last_hidden_state
        assert y.shape == (B, 1, HID) and out.hidden_states[-1].shape == (B, 1, HID) and out.hidden_states[-2].shape == (B, S, HID)
        pooled = y[:, 0]
        last_layer = m.encoder(input_ids=ids, attention_mask=mask, unpad=m.unpad_inputs, output_hidden_states=True)[1][-1][:, 0]
    assert pooled.dtype == torch.float32 and pooled.requires_grad
    _hold(f"{route}: pooled rows", _rel(pooled, ref["pooled"]), HIDDEN_TOL)
    _hold(f"{route}: last layer's rows", _rel(last_layer, ref["last_layer"]), HIDDEN_TOL)
    (pooled * w).sum().backward()
    worst = []
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        worst.append((_rel(p.grad, ref["grads"][n]), n))
    for e, n in sorted(worst, reverse=True)[:4]:
        print(f"{route}: grad.{n} = {e:.3e} (bound {GRAD_TOL:.0e})")
    assert max(worst)[0] <= GRAD_TOL, max(worst)
    assert len(worst) == len(ref["grads"])


# ---- launch ledger -------------------------------------------------------------------------------------------------------------------
def _ledger(fn):
    from cm3p_amd import _lib

    _lib.profile_begin()
    try:
        ret = fn()
    finally:
        rec = _lib.profile_end()
    return ret, {k: v[0] for k, v in rec.items()}


def _count(rec, prefix):
    return sum(n for tag, n in rec.items() if tag.startswith(prefix))


@pytest.mark.parametrize("cls_only", [False, True])
def test_launch_ledger_of_a_stack_forward_and_backward(cls_only):
    ids, mask, w = (t.cuda() for t in _batch())
    m = _model(cls_only=cls_only).train()
    L = 3
    y, fwd = _ledger(lambda: m(input_ids=ids, attention_mask=mask).last_hidden_state)
    print("forward:", {k: v for k, v in fwd.items() if k.startswith("attn")})
    assert _count(fwd, "attn_fwd") == (L - 1 if cls_only else L)
    assert _count(fwd, "attn_row_fwd_kernel") == (1 if cls_only else 0)
    _, bwd = _ledger(lambda: (y[:, 0] * w).sum().backward())
    print("backward:", {k: v for k, v in bwd.items() if k.startswith("attn")})
    # layer 0 is global (the fused backward), layers 1 and 2 slide (the band backward's dq and dkv kernels)
    assert _count(bwd, "attn_bwd_prep_kernel") == 1
    assert _count(bwd, "attn_bwd_dq_kernel") == _count(bwd, "attn_bwd_dkv_kernel") == (1 if cls_only else 2)
    assert _count(bwd, "attn_row_bwd_kernel") == (1 if cls_only else 0)
    assert _count(bwd, "attn_row") + _count(fwd, "attn_row") == (2 if cls_only else 0)


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
def test_fallback_head_dim_16_gives_the_bits_of_row_0():
    name = "c1_tiny_nopad"
    inp = {k: v.to("cuda") for k, v in make_inputs(name).items() if k != "labels"}
    off, on = TB._model(name), TB._model(name)
    assert off.config.beatmap_config.hidden_size // off.config.beatmap_config.num_attention_heads == 16
    on.cls_only_last_layer = True
    with torch.no_grad():
        a, b = off(**inp, return_loss=False), on(**inp, return_loss=False)
    for t in ("beatmap_model_output", "metadata_model_output"):
        full, short = a[t].last_hidden_state, b[t].last_hidden_state
        assert short.shape == (full.shape[0], 1, full.shape[2]) and torch.equal(short, full[:, :1])
        assert torch.equal(a[t].pooler_output, b[t].pooler_output)
    assert torch.equal(a.logits_per_metadata, b.logits_per_metadata)


@pytest.mark.parametrize("how", ["attention_dropout", "checkpointing"])
def test_fallback_in_training_gives_the_bits_of_row_0(how):
    ids, mask, w = (t.cuda() for t in _batch())
    kw = dict(attention_dropout=0.25) if how == "attention_dropout" else {}
    runs = []
    for cls_only in (False, True):
        m = _model(cls_only=cls_only, **kw).train()
        if how == "checkpointing":
            m.gradient_checkpointing = True
        torch.manual_seed(5)
        _, rec = _ledger(lambda: runs.append(m(input_ids=ids, attention_mask=mask).last_hidden_state))
        assert _count(rec, "attn_row") == 0 and _count(rec, "attn_fwd") == 3  # the full layer ran
    full, short = runs
    assert short.shape == (len(LENS), 1, HID) and torch.equal(short, full[:, :1])
    (short[:, 0] * w).sum().backward()  # (and the selection carries the gradient back into the full layer)
    if how == "attention_dropout":
        torch.manual_seed(6)
        m = _model(cls_only=True, **kw).train()
        assert not torch.equal(m(input_ids=ids, attention_mask=mask).last_hidden_state, short)  # (the dropout really is on)


# ---- the bf16 forward-only stream ----------------------------------------------------------------------------------------------------
def test_bf16_forward_only_stream_within_the_bounds_of_the_bf16_fixture():
    name, BF = "d64_audio", torch.bfloat16
    ref = {k.split(".", 1)[1]: v for k, v in load_file(TB.FIX).items() if k.startswith(name + ".")}
    model = TB._model(name, BF).set_residual_dtype(BF)
    model.cls_only_last_layer = True
    inp = {k: (v.to(BF) if v.is_floating_point() else v).to("cuda") for k, v in make_inputs(name).items() if k != "labels"}
    with torch.no_grad():
        out, rec = _ledger(lambda: model(**inp, return_loss=False))
    assert _count(rec, "attn_row_fwd_kernel") == 2  # (both towers took the row route on the bf16 stream)
    bo, mo = out.beatmap_model_output, out.metadata_model_output
    assert bo.last_hidden_state.dtype == BF and bo.last_hidden_state.shape[1] == 1 and mo.last_hidden_state.shape[1] == 1
    assert bo.pooler_output.dtype == torch.float32
    _hold("bf16 stream: beatmap_embeds", _rel(out.beatmap_embeds, ref["beatmap_embeds"]), TB.BF16_TOL["embeds"])
    _hold("bf16 stream: metadata_embeds", _rel(out.metadata_embeds, ref["metadata_embeds"]), TB.BF16_TOL["embeds"])
    _hold("bf16 stream: logits_per_metadata", _rel(out.logits_per_metadata, ref["logits_per_metadata"]), TB.BF16_TOL["logits"])
    if "beatmap_last_hidden_state" in ref:
        _hold("bf16 stream: beatmap CLS rows", _rel(bo.last_hidden_state[:, 0], ref["beatmap_last_hidden_state"][:, 0]), TB.BF16_TOL["hidden"])
    _hold("bf16 stream: metadata CLS rows", _rel(mo.last_hidden_state[:, 0], ref["metadata_last_hidden_state"][:, 0]), TB.BF16_TOL["hidden"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_before_any_launch():
    from cm3p_amd import CM3PConfig, CM3PModel
    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM
    from cm3p_amd.modeling_cm3p import CM3PForMaskedLM

    ids, mask, _ = (t.cuda() for t in _batch())
    m = _model()
    with pytest.raises(NotImplementedError, match="output_attentions"):
        m(input_ids=ids, attention_mask=mask, output_attentions=True)
    name = "d64_cls_nopad"
    model = TM._build(name)
    model.cls_only_last_layer = True
    inp = TM._inputs(load_file(os.path.join(GOLD, f"{name}.safetensors")))
    with pytest.raises(NotImplementedError, match="output_attentions"):
        model(**inp, output_attentions=True)
    # the MLM head of CM3PModel (has_decoder_head) and CM3PForMaskedLM read every row
    mlm = CM3PModel(CM3PConfig(**CASES["d64_mlm"]["cfg"])).cuda()
    mlm.cls_only_last_layer = True
    blob = TM._inputs(load_file(os.path.join(GOLD, "d64_mlm.safetensors")))
    from cm3p_amd import _lib

    _lib.profile_begin()
    try:
        with pytest.raises(ValueError, match="MLM head"):
            mlm(**blob)
        fm = CM3PForMaskedLM(mlm.config.beatmap_config).cuda()
        fm.cls_only_last_layer = True
        with pytest.raises(ValueError, match="MLM head"):
            fm(input_ids=blob["input_ids"], attention_mask=blob.get("attention_mask"))
        hf = FusedModernBertForMaskedLM(_config()).cuda()
        hf.model.cls_only_last_layer = True
        with pytest.raises(ValueError, match="MLM head"):
            hf(input_ids=ids, attention_mask=mask)
    finally:
        rec = _lib.profile_end()
    assert not rec, f"a refused call launched {sorted(rec)}"


# ---- switch off ----------------------------------------------------------------------------------------------------------------------
def test_switch_off_is_bit_identical_to_a_model_that_never_had_it_set():
    name = "d64_cls_nopad"
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    never, toggled = TM._build(name), TM._build(name)
    toggled.cls_only_last_layer = True
    toggled.cls_only_last_layer = False
    a, b = never(**TM._inputs(blob)), toggled(**TM._inputs(blob))
    assert torch.equal(a.loss, b.loss) and torch.equal(a.logits_per_metadata, b.logits_per_metadata)
    assert torch.equal(a.beatmap_model_output.last_hidden_state, b.beatmap_model_output.last_hidden_state)
    assert a.beatmap_model_output.last_hidden_state.shape[1] == CASES[name]["S"]
    a.loss.backward(), b.loss.backward()
    pb = dict(toggled.named_parameters())
    assert all(torch.equal(p.grad, pb[n].grad) for n, p in never.named_parameters() if p.grad is not None)


# ---- the HF seam ---------------------------------------------------------------------------------------------------------------------
def test_fused_sequence_classification_with_cls_pooling_against_the_installed_model_on_sdpa():
    from cm3p_amd.hf_modernbert import FusedModernBertModel, fuse
    from transformers import ModernBertForSequenceClassification

    cfg = dict(num_labels=3, num_hidden_layers=2, layer_types=[FULL, SLIDE], classifier_pooling="cls")
    ids, mask, _ = (t.cuda() for t in _batch())
    labels = torch.tensor([0, 1, 2], device="cuda")
    torch.manual_seed(6)
    ref = ModernBertForSequenceClassification._from_config(_config(**cfg), attn_implementation="sdpa").cuda().eval()
    assert ref.config._attn_implementation == "sdpa" and ref.config.classifier_pooling == "cls"
    m = ModernBertForSequenceClassification._from_config(_config(**cfg), attn_implementation="sdpa")
    m.load_state_dict(ref.state_dict())
    m = m.cuda().eval()
    assert fuse(m) is m and isinstance(m.model, FusedModernBertModel)
    m.model.cls_only_last_layer = True
    want = ref(input_ids=ids, attention_mask=mask, labels=labels)
    want.loss.backward()
    out, rec = _ledger(lambda: m(input_ids=ids, attention_mask=mask, labels=labels))
    assert _count(rec, "attn_row_fwd_kernel") == 1 and _count(rec, "attn_fwd") == 1
    assert out.logits.shape == (3, 3)
    _hold("sequence classification: logits", _rel(out.logits, want.logits), HIDDEN_TOL)
    _hold("sequence classification: loss abs diff", abs(out.loss.item() - want.loss.item()), FIX_TOL["loss"])
    out.loss.backward()
    got = dict(m.named_parameters())
    worst = []
    for n, p in ref.named_parameters():
        assert got[n].grad is not None, n
        worst.append((_rel(got[n].grad, p.grad), n))
    for e, n in sorted(worst, reverse=True)[:4]:
        print(f"sequence classification: grad.{n} = {e:.3e} (bound {GRAD_TOL:.0e})")
    assert max(worst)[0] <= GRAD_TOL, max(worst)
