"""`labelled_rows_last_layer` (CM3PModel, CM3PForMaskedLM, FusedModernBertForMaskedLM) and `last_layer_rows` (CM3PEncoder.forward), `-m gpu`:
the beatmap tower's last layer, its final norm and the MLM head run on the rows a training step consumes - the CLS row of every
sequence and the labelled positions - (cm3p_amd/encoder.py _LastLayerRowsFn on csrc/attention_qrows.hip).

  - the d64 geometry of tests/golden/cases.py with `cls_embed` towers and the decoder head, weights of tests/golden/weights_d64.safetensors,
    B = 4, S = 128, right-padded rows, ~15 % labels (a sequence without a label, a labelled CLS, a label on a row's last valid token):
    loss, both embeddings, the logits on the selected rows and every parameter's gradient against the float64 CPU oracle
    (oracle/cm3p_oracle.py), within the d64 class tolerances of tests/test_model_gpu.py (FIX_TOL) - switch on AND off, a global and a
    sliding last layer, padded and `unpad_inputs`;
  - the GEMM ledger: the last layer's Wo / Wi / Wo2 and the head on the padded n rows, attn_qrows in place of the full attention;
  - the fallbacks (dropout, checkpointing, an adapter on the last layer, the bf16 training stream): same output shape, same tolerances;
  - eval-mode and no-labels calls: the bits of the switch-off call; mean pooling raises; the sparse_prediction classes; the refusals.
Every measured figure is printed before it is held (`pytest -s`)."""
import copy
import functools
import os

import pytest
import torch
from safetensors.torch import load_file

import transformers  # noqa: F401  (a missing transformers is an error here, not a skip)

import test_model_gpu as TM
from cases import _BEATMAP_D64, _METADATA_D64, _cfg

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIX_TOL = TM.FIX_TOL
B, S, L_META, LENS = 4, 128, 16, (128, 100, 77, 128)


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm().clamp_min(1e-12)).item()


def _hold(what: str, value: float, bound: float):
    print(f"{what} = {value:.3e} (bound {bound:.0e})")
    assert value <= bound, f"{what} = {value:.3e} > {bound:.0e}"


def _config(layers=4, **beatmap):
    """layers = 4: the last layer is global (layers 0 and 3); layers = 3: it slides (half window 64 < S)."""
    c = dict(_cfg(_BEATMAP_D64, _METADATA_D64), has_decoder_head=True, loss_type="ForMaskedLM")
    c = copy.deepcopy(c)
    c["beatmap_config"].update(num_hidden_layers=layers, **beatmap)
    return c


@functools.lru_cache(maxsize=None)
def _state(layers=4):
    sd = load_file(os.path.join(GOLD, "weights_d64.safetensors"))
    sd.update({k[2:]: v for k, v in load_file(os.path.join(GOLD, "d64_mlm.safetensors")).items() if k.startswith("w.")})  # the MLM head
    return {k: v for k, v in sd.items() if not any(k.startswith(f"beatmap_model.encoder.layers.{i}.") for i in range(layers, 4))}


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(77)
    mask = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(3, 194, (B, S), generator=g) * mask
    pick = (torch.rand(B, S, generator=g) < 0.15) & mask.bool()
    pick[:, 0] = False
    pick[1, 0] = True             # a labelled CLS
    pick[1, LENS[1] - 1] = True   # a label on a row's last valid token
    pick[2] = False               # a sequence with no label
    labels = torch.where(pick, ids, torch.full_like(ids, -100))
    mids = torch.randint(3, 97, (B, L_META), generator=g)
    return dict(input_ids=ids, attention_mask=mask, labels=labels, metadata_ids=mids, metadata_attention_mask=torch.ones_like(mids))


def _rows():
    want = _batch()["labels"] != -100
    want = want.clone()
    want[:, 0] = True
    return torch.nonzero(want.flatten()).flatten()


def test_the_batch_holds_what_the_issue_asks_for():
    lab, rows = _batch()["labels"], _rows()
    frac = (lab != -100).float().mean().item()
    assert 0.08 < frac < 0.2 and not bool((lab[2] != -100).any()) and lab[1, 0] != -100 and lab[1, LENS[1] - 1] != -100
    assert all(int(b * S) in rows.tolist() for b in range(B)) and rows.numel() == int((lab != -100).sum()) + B - 1


@functools.lru_cache(maxsize=None)
def _oracle(layers):
    """The float64 restatement on the CPU, once per depth: loss, embeddings, (B, S, V) logits and every parameter's gradient."""
    from oracle import cm3p_oracle as O

    sd = {k: v.detach().double().requires_grad_(v.is_floating_point()) for k, v in _state(layers).items()}
    out = O.forward(sd, _config(layers), **_batch())
    out["loss"].backward()
    return dict(loss=out["loss"].detach(), metadata_embeds=out["metadata_embeds"].detach(), beatmap_embeds=out["beatmap_embeds"].detach(),
                logits=out["logits"].detach(), grads={k: v.grad for k, v in sd.items() if v.grad is not None})


def _model(layers=4, switch=True, dtype=torch.float32, **beatmap):
    from cm3p_amd import CM3PConfig, CM3PModel

    model = CM3PModel(CM3PConfig(**_config(layers, **beatmap)))
    model.load_state_dict(_state(layers), strict=True)
    model.labelled_rows_last_layer = switch
    return model.to("cuda").to(dtype).train()


def _inputs(**drop):
    return {k: v.cuda() for k, v in _batch().items() if k not in drop}


def _against_oracle(tag, model, out, layers, selected):
    ref = _oracle(layers)
    n, V = _rows().numel(), 200
    _hold(f"{tag}: loss", abs(out.loss.item() - ref["loss"].item()), FIX_TOL["loss"])
    _hold(f"{tag}: metadata_embeds", _rel(out.metadata_embeds, ref["metadata_embeds"]), FIX_TOL["embeds"])
    _hold(f"{tag}: beatmap_embeds", _rel(out.beatmap_embeds, ref["beatmap_embeds"]), FIX_TOL["embeds"])
    want = ref["logits"].reshape(B * S, V)[_rows()]
    if selected:
        assert out.logits.shape == (n, V) and out.beatmap_model_output.last_hidden_state.shape == (n, 128)
        assert torch.equal(out.beatmap_model_output.selected_rows.cpu(), _rows())
        got = out.logits
    else:
        assert out.logits.shape == (B, S, V) and out.beatmap_model_output.selected_rows is None
        got = out.logits.reshape(B * S, V)[_rows().cuda()]
    _hold(f"{tag}: mlm logits on the selected rows", _rel(got, want), FIX_TOL["mlm_logits"])
    out.loss.backward()
    worst = []
    for name, p in model.named_parameters():
        if name not in ref["grads"]:  # (the audio encoder: no input_features in this batch, so no gradient on either side)
            assert name.startswith("beatmap_model.audio_encoder.") and (p.grad is None or p.grad.float().norm().item() == 0.0), name
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        g = ref["grads"][name]
        if g.norm() < 1e-8:
            assert p.grad.float().norm().item() < 1e-5, name
        else:
            worst.append((_rel(p.grad, g), name))
    for e, name in sorted(worst, reverse=True)[:4]:
        print(f"{tag}: grad.{name} = {e:.3e} (bound {FIX_TOL['grad']:.0e})")
    assert max(worst)[0] <= FIX_TOL["grad"], max(worst)
    assert len(worst) == sum(1 for g in ref["grads"].values() if g.norm() >= 1e-8) >= 10


@pytest.mark.parametrize("layers,switch,unpad", [(4, True, False), (4, False, False), (3, True, False), (3, False, False), (4, True, True), (3, True, True)],
                         ids=lambda v: str(v))
def test_training_step_against_the_float64_oracle(layers, switch, unpad):
    model = _model(layers, switch)
    assert not any("labelled_rows" in k for k in model.state_dict()) and "labelled_rows_last_layer" not in model.config.to_dict()
    model.unpad_inputs = unpad
    out = model(**_inputs())
    _against_oracle(f"L{layers} {'on' if switch else 'off'}{' unpad' if unpad else ''}", model, out, layers, switch)


# ---- ledger --------------------------------------------------------------------------------------------------------------------------
def _ledger(fn, monkeypatch):
    """-> (result, kernel tags with launch counts, the (M, N, K) of every K.gemm call)."""
    from cm3p_amd import _lib
    from cm3p_amd import kernels as K

    shapes, real = [], K.gemm

    def gemm(a, b, M, N, Kd, *args, **kw):
        shapes.append((M, N, Kd))
        return real(a, b, M, N, Kd, *args, **kw)

    monkeypatch.setattr(K, "gemm", gemm)
    _lib.profile_begin()
    try:
        ret = fn()
    finally:
        rec = _lib.profile_end()
        monkeypatch.setattr(K, "gemm", real)
    return ret, {k: v[0] for k, v in rec.items()}, shapes


def _count(rec, prefix):
    return sum(n for tag, n in rec.items() if tag.startswith(prefix))


@pytest.mark.parametrize("layers", [4, 3])
def test_launch_ledger_of_a_training_step(layers, monkeypatch):
    from cm3p_amd import kernels as K

    monkeypatch.setenv("CM3P_TOWER_OVERLAP", "0")
    H, I, V, T = 128, 192, 200, B * S
    n = _rows().numel()
    Np = K.row_block_rows(n, H, I)
    assert Np % 8 == 0 and n <= Np < n + 64
    led = {}
    for switch in (False, True):
        model = _model(layers, switch)
        out, fwd, gf = _ledger(lambda: model(**_inputs()), monkeypatch)
        _, bwd, gb = _ledger(lambda: out.loss.backward(), monkeypatch)
        led[switch] = (fwd, gf, bwd, gb)
    (f0, gf0, b0, gb0), (f1, gf1, b1, gb1) = led[False], led[True]
    print("forward, switch on:", {k: v for k, v in f1.items() if k.startswith("attn")})
    print("backward, switch on:", {k: v for k, v in b1.items() if k.startswith("attn")})
    # attention: one full forward less, attn_qrows in its place; nothing of it in a switch-off step
    assert _count(f0, "attn_qrows") == _count(b0, "attn_qrows") == 0
    assert _count(f1, "attn_qrows_fwd_kernel") == 1 and _count(b1, "attn_qrows_bwd_kernel") == 1
    assert _count(f1, "attn_fwd") == _count(f0, "attn_fwd") - 1
    assert _count(b1, "attn_bwd") < _count(b0, "attn_bwd")
    # GEMMs of the beatmap tower (H = 128; the metadata tower's are 64 wide): Wo, Wi, Wo2 of the last layer and the head's two on Np rows
    rows_of = lambda g, N, Kd: sorted(M for M, n_, k_ in g if (n_, k_) == (N, Kd) and M in (T, Np))
    Vp = (V + 63) // 64 * 64
    assert rows_of(gf0, 2 * I, H) == [T] * layers and rows_of(gf1, 2 * I, H) == [Np] + [T] * (layers - 1)            # Wi
    assert rows_of(gf0, H, I) == [T] * layers and rows_of(gf1, H, I) == [Np] + [T] * (layers - 1)                    # Wo2
    assert rows_of(gf0, Vp, H) == [T] and rows_of(gf1, Vp, H) == [Np]                                              # the decoder
    assert rows_of(gf0, H, H) == [T] * (layers + 1) and rows_of(gf1, H, H) == [Np, Np] + [T] * (layers - 1)          # Wo and the head's dense
    # the weight gradients of those five GEMMs contract Np rows (dW [N, K] = dy^T x: M = N, N = K, K = rows)
    assert {(M, N) for M, N, Kd in gb1 if Kd == Np and N in (H, I)} >= {(H, H), (2 * I, H), (H, I), (Vp, H)}
    assert {(M, N) for M, N, Kd in gb0 if Kd == T and N in (H, I)} >= {(H, H), (2 * I, H), (H, I), (Vp, H)}


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------
def _pair(how, layers=4):
    """A switch-off and a switch-on step under one fallback condition, same seed."""
    runs = []
    for switch in (False, True):
        kw = dict(mlp_dropout=0.1, embedding_dropout=0.1) if how == "dropout" else {}
        model = _model(layers, switch, **kw)
        if how == "checkpointing":
            model.gradient_checkpointing_enable()
        elif how == "adapter":
            from cm3p_amd.lora import add_lora

            torch.manual_seed(3)
            add_lora(model.beatmap_model, r=8, alpha=16, layers=[layers - 1], freeze_base=False)
            for name, p in model.named_parameters():
                if name.endswith("lora_B"):
                    torch.nn.init.normal_(p, std=0.02, generator=torch.Generator(device="cuda").manual_seed(4))
        elif how == "bf16_stream":
            model.beatmap_model.encoder.train_residual_dtype = torch.bfloat16
        torch.manual_seed(11)
        out = model(**_inputs())
        out.loss.backward()
        runs.append((model, out))
    return runs


@pytest.mark.parametrize("how", ["dropout", "checkpointing", "adapter", "bf16_stream"])
def test_fallbacks_keep_the_shape_and_the_result(how, monkeypatch):
    from cm3p_amd import _lib

    monkeypatch.setenv("CM3P_TOWER_OVERLAP", "0")
    _lib.profile_begin()
    try:
        (m0, o0), (m1, o1) = _pair(how)
    finally:
        rec = {k: v[0] for k, v in _lib.profile_end().items()}
    assert _count(rec, "attn_qrows") == 0, "the row route ran where it has no form"
    n, V = _rows().numel(), 200
    assert o1.logits.shape == (n, V) and o1.beatmap_model_output.last_hidden_state.shape == (n, 128) and o0.logits.shape == (B, S, V)
    _hold(f"{how}: loss", abs(o1.loss.item() - o0.loss.item()), FIX_TOL["loss"])
    _hold(f"{how}: beatmap_embeds", _rel(o1.beatmap_embeds, o0.beatmap_embeds), FIX_TOL["embeds"])
    _hold(f"{how}: mlm logits on the selected rows", _rel(o1.logits, o0.logits.reshape(B * S, V)[_rows().cuda()]), FIX_TOL["mlm_logits"])
    g0 = dict(m0.named_parameters())
    worst = max((_rel(p.grad, g0[k].grad), k) for k, p in m1.named_parameters() if p.grad is not None and g0[k].grad.norm() > 1e-8)
    _hold(f"{how}: worst gradient ({worst[1]})", worst[0], FIX_TOL["grad"])


# ---- calls the switch does not touch ----------------------------------------------------------------------------------------------------
def test_eval_mode_and_no_labels_calls_are_the_bits_of_the_switch_off_call():
    on, off = _model(4, True), _model(4, False)
    for what, kw, mode in (("eval", _inputs(), "eval"), ("no labels", _inputs(labels=0), "train"), ("return_loss off", dict(_inputs(), return_loss=False), "train")):
        getattr(on, mode)(), getattr(off, mode)()
        with torch.no_grad():
            a, b = on(**kw), off(**kw)
        assert a.logits.shape == (B, S, 200) and a.beatmap_model_output.selected_rows is None, what
        assert torch.equal(a.logits, b.logits) and torch.equal(a.beatmap_embeds, b.beatmap_embeds), what
        assert torch.equal(a.beatmap_model_output.last_hidden_state, b.beatmap_model_output.last_hidden_state), what
        if a.loss is not None and torch.is_tensor(a.loss):
            assert torch.equal(a.loss, b.loss), what


def test_output_field_order_is_unchanged_and_selected_rows_comes_last():
    from cm3p_amd.modeling_cm3p import CM3PBeatmapModelOutput
    import dataclasses

    names = [f.name for f in dataclasses.fields(CM3PBeatmapModelOutput)]
    assert names[-1] == "selected_rows" and names[-3:-1] == ["beatmap_embeds", "audio_model_output"]


def test_mean_pooling_raises():
    from cm3p_amd import CM3PConfig, CM3PModel

    model = CM3PModel(CM3PConfig(**_config(4, cls_embed=False)))
    with pytest.raises(ValueError, match="mean pooling"):
        model.labelled_rows_last_layer = True
    assert model.labelled_rows_last_layer is False


# ---- the sparse_prediction classes ----------------------------------------------------------------------------------------------------------
def _masked_lm(kind):
    if kind == "cm3p":
        from cm3p_amd import CM3PBeatmapConfig
        from cm3p_amd.modeling_cm3p import CM3PForMaskedLM

        torch.manual_seed(0)
        return CM3PForMaskedLM(CM3PBeatmapConfig(**dict(_BEATMAP_D64, sparse_prediction=True)))
    from transformers import ModernBertConfig

    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM

    torch.manual_seed(0)
    return FusedModernBertForMaskedLM(ModernBertConfig(vocab_size=200, hidden_size=128, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2,
                                                       max_position_embeddings=512, local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                                                       cls_token_id=1, sep_token_id=2, sparse_prediction=True))


@pytest.mark.parametrize("kind", ["cm3p", "fused_modernbert"])
def test_sparse_prediction_switch_on_against_switch_off(kind, monkeypatch):
    base = _masked_lm(kind)
    state = {k: v.clone() for k, v in base.state_dict().items()}
    kw = {k: v for k, v in _inputs().items() if k in ("input_ids", "attention_mask", "labels")}
    runs = []
    for switch in (False, True):
        model = _masked_lm(kind)
        model.load_state_dict(state)
        model = model.cuda().train()
        assert model.labelled_rows_last_layer is False
        model.labelled_rows_last_layer = switch
        out, rec, _ = _ledger(lambda: model(**kw), monkeypatch)
        assert _count(rec, "attn_qrows_fwd_kernel") == int(switch)
        out.loss.backward()
        runs.append((model, out))
    (m0, o0), (m1, o1) = runs
    assert o1.logits.shape == o0.logits.shape == (int((_batch()["labels"] != -100).sum()), 200)
    _hold(f"{kind}: loss", abs(o1.loss.item() - o0.loss.item()), FIX_TOL["loss"])
    _hold(f"{kind}: logits", _rel(o1.logits, o0.logits), FIX_TOL["mlm_logits"])
    g0 = dict(m0.named_parameters())
    worst = max((_rel(p.grad, g0[k].grad), k) for k, p in m1.named_parameters() if p.grad is not None and g0[k].grad.norm() > 1e-8)
    _hold(f"{kind}: worst gradient ({worst[1]})", worst[0], FIX_TOL["grad"])
    m1.eval()
    with torch.no_grad():
        assert torch.equal(m1(**kw).logits, m0.eval()(**kw).logits)  # (evaluation runs as without the switch)


# ---- the encoder argument ---------------------------------------------------------------------------------------------------------------
def test_encoder_rows_equal_the_rows_of_the_full_result_within_the_hidden_tolerance_and_refusals():
    enc = _model(3, False).beatmap_model.encoder.eval()
    ids, mask = _inputs()["input_ids"], _inputs()["attention_mask"]
    rows = _rows().cuda()
    with torch.no_grad():
        full = enc(input_ids=ids, attention_mask=mask)
        y, hiddens = enc(input_ids=ids, attention_mask=mask, last_layer_rows=rows, output_hidden_states=True)
        enc.cls_only_last_layer = True  # (the explicit argument wins)
        y2 = enc(input_ids=ids, attention_mask=mask, last_layer_rows=rows)
        enc.cls_only_last_layer = False
        empty = enc(input_ids=ids, attention_mask=mask, last_layer_rows=rows[:0])
    assert y.shape == (rows.numel(), 128) and hiddens[-1].shape == y.shape and hiddens[-2].shape == (B, S, 128) and torch.equal(y, y2)
    assert empty.shape == (0, 128)
    _hold("encoder: listed rows against the full result", _rel(y, full.reshape(B * S, -1)[rows]), FIX_TOL["hidden"])
    bad = [rows.flip(0), torch.cat((rows, rows[-1:])), torch.cat((rows, rows.new_tensor([B * S]))), torch.cat((rows.new_tensor([-1]), rows)),
           rows.to(torch.int32), rows.cpu(), rows.view(1, -1)]
    for r in bad:
        with pytest.raises(ValueError):
            enc(input_ids=ids, attention_mask=mask, last_layer_rows=r)
    with pytest.raises(ValueError, match="valid"):  # unpad: a row on a padding token has no packed row
        enc(input_ids=ids, attention_mask=mask, unpad=True, last_layer_rows=torch.tensor([0, S + LENS[1]], device="cuda"))
    with pytest.raises(NotImplementedError):
        enc(input_ids=ids, attention_mask=mask, last_layer_rows=rows, output_attentions=True)


def test_encoder_rows_on_caller_packed_inputs():
    enc = _model(3, False).beatmap_model.encoder.eval()
    ids, mask = _inputs()["input_ids"], _inputs()["attention_mask"].bool()
    cu = torch.tensor([0] + list(torch.tensor(LENS).cumsum(0)), dtype=torch.int32, device="cuda")
    total = sum(LENS)
    rows = torch.tensor(sorted({0, 5, LENS[0] - 1, LENS[0], LENS[0] + LENS[1] + 3, total - 1}), device="cuda")
    with torch.no_grad():
        full = enc(input_ids=ids[mask], cu_seqlens=cu, max_seqlen=max(LENS))
        y = enc(input_ids=ids[mask], cu_seqlens=cu, max_seqlen=max(LENS), last_layer_rows=rows)
    assert full.shape == (total, 128) and y.shape == (rows.numel(), 128)
    _hold("packed encoder: listed rows against the full result", _rel(y, full[rows]), FIX_TOL["hidden"])
    with pytest.raises(ValueError):
        enc(input_ids=ids[mask], cu_seqlens=cu, max_seqlen=max(LENS), last_layer_rows=torch.tensor([0, total], device="cuda"))
