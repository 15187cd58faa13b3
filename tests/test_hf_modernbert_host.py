"""Seam 2b on the CPU (cm3p_amd/hf_modernbert.py): the translation of a `ModernBertConfig` into what `CM3PEncoder` reads, the refusals,
state-dict key identity with the installed `transformers` classes, parameter identity through `fuse` / `unfuse`, checkpoint round trips
in both directions, and the refusal of CPU inputs.  (The kernels behind it: tests/test_hf_modernbert_gpu.py, `-m gpu`.)"""
import copy

import pytest
import torch

import transformers  # (a missing transformers is an error here, not a skip)

FULL, SLIDE = "full_attention", "sliding_attention"


def _config(**kw):
    from transformers import ModernBertConfig

    cfg = dict(vocab_size=200, hidden_size=128, intermediate_size=192, num_hidden_layers=4, num_attention_heads=2, max_position_embeddings=512,
               layer_types=[FULL, SLIDE, SLIDE, FULL], local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1,
               sep_token_id=2)
    cfg.update(kw)
    return ModernBertConfig(**cfg)


def _is_in(p, params):
    return any(p is q for q in params)


# ---- translation ------------------------------------------------------------------------------------------------------------------------
def test_translation_follows_layer_types_window_and_thetas_and_leaves_the_input_alone():
    from cm3p_amd.hf_modernbert import encoder_config

    cfg = _config(num_hidden_layers=5, layer_types=[FULL, SLIDE, SLIDE, FULL, FULL], local_attention=96, norm_eps=3e-6, embedding_dropout=0.1,
                  attention_dropout=0.2, mlp_dropout=0.3, initializer_range=0.03, initializer_cutoff_factor=2.5,
                  rope_parameters={FULL: {"rope_type": "default", "rope_theta": 123456.0}, SLIDE: {"rope_type": "default", "rope_theta": 7777.0}})
    before = copy.deepcopy(cfg.to_dict())
    ec = encoder_config(cfg)
    assert [ec.is_global_layer(i) for i in range(5)] == [True, False, False, True, True]  # not an "every n" pattern
    assert ec.half_window == cfg.sliding_window == 48
    assert (ec.global_rope_theta, ec.local_rope_theta) == (123456.0, 7777.0)
    assert (ec.norm_eps, ec.embedding_dropout, ec.attention_dropout, ec.mlp_dropout) == (3e-6, 0.1, 0.2, 0.3)
    assert (ec.vocab_size, ec.pad_token_id, ec.initializer_range, ec.initializer_cutoff_factor) == (200, 0, 0.03, 2.5)
    assert (ec.hidden_size, ec.intermediate_size, ec.num_hidden_layers, ec.num_attention_heads) == (128, 192, 5, 2)
    assert cfg.to_dict() == before
    ec.layer_types[0] = SLIDE  # the translation owns its list
    assert cfg.layer_types[0] == FULL


def test_default_config_is_modernbert_base_and_translates():
    from cm3p_amd.hf_modernbert import encoder_config
    from transformers import ModernBertConfig

    ec = encoder_config(ModernBertConfig())
    assert [ec.is_global_layer(i) for i in range(6)] == [True, False, False, True, False, False]
    assert (ec.half_window, ec.global_rope_theta, ec.local_rope_theta) == (64, 160000.0, 10000.0)


def _with_rope_type(cfg):
    cfg.rope_parameters[FULL] = {"rope_type": "linear", "factor": 2.0, "rope_theta": 160000.0}
    return cfg


@pytest.mark.parametrize("field,make", [
    ("rope_type", lambda: _with_rope_type(_config())),
    ("norm_bias", lambda: _config(norm_bias=True)),
    ("attention_bias", lambda: _config(attention_bias=True)),
    ("mlp_bias", lambda: _config(mlp_bias=True)),
    ("hidden_activation", lambda: _config(hidden_activation="relu")),
    ("num_attention_heads", lambda: _config(hidden_size=120, num_attention_heads=3)),  # head_dim 40
    ("intermediate_size", lambda: _config(intermediate_size=196)),
])
def test_unsupported_configs_are_refused_by_name_before_anything_runs(field, make):
    from cm3p_amd.hf_modernbert import FusedModernBertModel, encoder_config

    cfg = make()
    with pytest.raises(NotImplementedError, match=field):
        encoder_config(cfg)
    with pytest.raises(NotImplementedError, match=field):
        FusedModernBertModel(cfg)  # at construction


def test_refusals_name_the_value_too():
    from cm3p_amd.hf_modernbert import encoder_config

    with pytest.raises(NotImplementedError, match="'relu'"):
        encoder_config(_config(hidden_activation="relu"))
    with pytest.raises(NotImplementedError, match="'linear'"):
        encoder_config(_with_rope_type(_config()))
    with pytest.raises(NotImplementedError, match="num_attention_heads=3"):
        encoder_config(_config(hidden_size=120, num_attention_heads=3))


# ---- names and parameter identity ------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_equal_the_installed_classes():
    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM, FusedModernBertModel
    from transformers import ModernBertForMaskedLM, ModernBertModel

    cfg = _config()
    assert set(FusedModernBertModel(cfg).state_dict()) == set(ModernBertModel(cfg).state_dict())
    assert set(FusedModernBertForMaskedLM(cfg).state_dict()) == set(ModernBertForMaskedLM(cfg).state_dict())
    a, b = dict(FusedModernBertForMaskedLM(cfg).named_parameters()), dict(ModernBertForMaskedLM(cfg).named_parameters())
    assert set(a) == set(b) and all(a[k].shape == b[k].shape for k in a)
    # every bias the heads may carry
    cfg = _config(classifier_bias=True, decoder_bias=False)
    assert set(FusedModernBertForMaskedLM(cfg).state_dict()) == set(ModernBertForMaskedLM(cfg).state_dict())


def test_load_state_dict_of_the_hf_model():
    from cm3p_amd.hf_modernbert import FusedModernBertModel
    from transformers import ModernBertModel

    torch.manual_seed(0)
    hf = ModernBertModel(_config())
    fused = FusedModernBertModel(_config())
    res = fused.load_state_dict(hf.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, hf.state_dict()[k]) for k, v in fused.state_dict().items())


def test_fuse_shares_the_parameter_objects_is_idempotent_and_unfuse_restores():
    from cm3p_amd.hf_modernbert import FusedModernBertModel, fuse, unfuse
    from transformers import ModernBertModel

    m = ModernBertModel(_config()).eval()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    orig = list(m.parameters())
    f = fuse(m)
    assert isinstance(f, FusedModernBertModel) and not f.training and not f.encoder.training
    fp = list(f.parameters())
    assert len(fp) == len(orig) and all(_is_in(p, orig) for p in fp)
    assert all(_is_in(p, opt.param_groups[0]["params"]) for p in fp)  # the optimizer built before fuse() trains the fused model
    assert dict(f.named_parameters()).keys() == dict(m.named_parameters()).keys()
    assert fuse(f) is f and len(list(fuse(f).parameters())) == len(orig)
    back = unfuse(f)
    assert back is m and type(back) is ModernBertModel and all(_is_in(p, orig) for p in back.parameters())
    with pytest.raises(TypeError):
        fuse(torch.nn.Linear(2, 2))


def test_unfuse_of_a_model_that_was_never_fused_builds_the_torch_tower_around_the_same_parameters():
    from cm3p_amd.hf_modernbert import FusedModernBertModel, unfuse
    from transformers import ModernBertModel

    f = FusedModernBertModel(_config())
    t = unfuse(f)
    assert type(t) is ModernBertModel and all(_is_in(p, list(f.parameters())) for p in t.parameters())
    ids = torch.randint(3, 200, (2, 24))
    with torch.no_grad():
        assert torch.isfinite(t(input_ids=ids).last_hidden_state).all()  # a working torch model (CPU)


@pytest.mark.parametrize("cls_name", ["ModernBertForMaskedLM", "ModernBertForSequenceClassification", "ModernBertForTokenClassification"])
def test_fuse_swaps_the_tower_of_a_task_model_in_place(cls_name):
    from cm3p_amd.hf_modernbert import FusedModernBertModel, fuse, unfuse

    cls = getattr(transformers, cls_name)
    m = cls(_config(num_labels=3))
    tower = m.model
    orig = list(m.parameters())
    names = set(m.state_dict())
    out = fuse(m)
    assert out is m and isinstance(m.model, FusedModernBertModel)
    assert set(m.state_dict()) == names
    now = list(m.parameters())
    assert len(now) == len(orig) and all(_is_in(p, orig) for p in now)
    if cls_name == "ModernBertForMaskedLM":
        assert m.decoder.weight is m.model.embeddings.tok_embeddings.weight  # tied weights stay tied
    fused_tower = m.model
    assert fuse(m) is m and m.model is fused_tower  # idempotent
    assert unfuse(m) is m and m.model is tower
    if cls_name == "ModernBertForMaskedLM":
        assert m.decoder.weight is m.model.embeddings.tok_embeddings.weight


def test_fused_masked_lm_ties_the_decoder_to_the_embedding_table():
    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM

    m = FusedModernBertForMaskedLM(_config())
    assert m.decoder.weight is m.model.embeddings.tok_embeddings.weight
    assert m.get_output_embeddings() is m.decoder and m.get_input_embeddings() is m.model.embeddings.tok_embeddings


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------------
def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_checkpoint_round_trip_both_directions(tmp_path):
    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM, FusedModernBertModel
    from transformers import ModernBertForMaskedLM, ModernBertModel

    torch.manual_seed(1)
    hf = ModernBertModel(_config())
    hf.save_pretrained(tmp_path / "hf")
    fused = FusedModernBertModel.from_pretrained(tmp_path / "hf")
    assert _same_state(fused, hf)
    assert [fused.encoder.config.is_global_layer(i) for i in range(4)] == [True, False, False, True]
    fused.save_pretrained(tmp_path / "fused")
    assert _same_state(ModernBertModel.from_pretrained(tmp_path / "fused"), hf)
    # the MaskedLM pair, and a base checkpoint from a MaskedLM directory (HF's own prefix rule)
    mlm = ModernBertForMaskedLM(_config())
    mlm.save_pretrained(tmp_path / "mlm")
    fmlm = FusedModernBertForMaskedLM.from_pretrained(tmp_path / "mlm")
    assert _same_state(fmlm, mlm) and fmlm.decoder.weight is fmlm.model.embeddings.tok_embeddings.weight
    fmlm.save_pretrained(tmp_path / "fmlm")
    assert _same_state(ModernBertForMaskedLM.from_pretrained(tmp_path / "fmlm"), mlm)
    assert _same_state(FusedModernBertModel.from_pretrained(tmp_path / "mlm"), mlm.model)


# ---- switches and the CPU refusal ----------------------------------------------------------------------------------------------------------
def test_mode_checkpointing_and_residual_switches_reach_the_encoder():
    from cm3p_amd.hf_modernbert import FusedModernBertModel, fuse
    from transformers import ModernBertForSequenceClassification

    f = FusedModernBertModel(_config())
    assert f.unpad_inputs is False
    f.train()
    assert f.encoder.training
    f.eval()
    assert not f.encoder.training
    f.gradient_checkpointing_enable()
    assert f.encoder.gradient_checkpointing and f.is_gradient_checkpointing
    f.gradient_checkpointing_disable()
    assert not f.encoder.gradient_checkpointing
    assert f.set_residual_dtype(torch.bfloat16) is f and f.encoder.residual_dtype is torch.bfloat16 and f.encoder.train_residual_dtype is None
    f.set_residual_dtype(torch.bfloat16, training=True)
    assert f.encoder.train_residual_dtype is torch.bfloat16
    with pytest.raises(ValueError):
        f.set_residual_dtype(torch.float16)
    # through a third-party wrapper: train() and gradient_checkpointing_enable() of the OUTER model arrive
    w = fuse(ModernBertForSequenceClassification(_config(num_labels=3)))
    w.train()
    w.gradient_checkpointing_enable()
    assert w.model.encoder.training and w.model.encoder.gradient_checkpointing
    w.eval()
    assert not w.model.encoder.training


def test_cpu_inputs_raise_the_no_cpu_path_error():
    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM, FusedModernBertModel

    ids = torch.randint(3, 200, (2, 16))
    with pytest.raises(RuntimeError, match="no CPU"):
        FusedModernBertModel(_config())(input_ids=ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(RuntimeError, match="no CPU"):
        FusedModernBertForMaskedLM(_config())(input_ids=ids, labels=ids)
    with pytest.raises(ValueError):
        FusedModernBertModel(_config())()
    with pytest.raises(NotImplementedError, match="attention_mask"):
        FusedModernBertModel(_config())(input_ids=ids, attention_mask=torch.ones(2, 1, 16, 16))
