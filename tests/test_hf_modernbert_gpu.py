"""Seam 2b on the GPU (cm3p_amd/hf_modernbert.py): a whole Hugging Face ModernBERT on the fused encoder stack against the installed
`transformers` model with `attn_implementation="sdpa"` in fp32 on the same GPU, holding the same weights.

Tiny model (hidden 128, 2 heads of 64, intermediate 192, vocab 200, layers [full, sliding, sliding, full], HF default init, fp32 weights)
on the (S, lens) grid of the narrow seam's GPU test: right padding down to one token (late local queries of that row see no key), S < 64,
no padding, lengths that cross the 128- and 256-row tile seams.

Bounds are the project's class bounds, restated: hidden states rel-L2 2e-2 (d64, tests/test_hf_attention.py), gradients 6e-2, MLM loss
3e-2 absolute and logits 3e-2 (tests/test_model_gpu.py FIX_TOL), packed against padded execution 5e-3
(test_unpadded_and_padded_paths_agree_and_full_batches_stay_padded), bf16 residual stream hidden states 5e-2
(tests/test_bf16_residual_gpu.py BF16_TOL).  Every measured value is printed before it is held (`pytest -s`).

CM3P_HF_MODERNBERT_ERRORS_OUT=<file>: write the values this run measured there (profiles/hf_modernbert_err.txt holds one run's)."""
import functools
import os

import pytest
import torch

import transformers  # (a missing transformers is an error here, not a skip)
pytestmark = pytest.mark.gpu

FULL, SLIDE = "full_attention", "sliding_attention"
GRID = [(200, (200, 137, 70, 1)), (48, (48, 20)), (384, (384, 384))]
HIDDEN_TOL, GRAD_TOL, LOSS_TOL, LOGITS_TOL, UNPAD_TOL, BF16_HIDDEN_TOL = 2e-2, 6e-2, 3e-2, 3e-2, 5e-3, 5e-2
VOCAB, HID = 200, 128
_SEEN: list = []


@pytest.fixture(scope="module", autouse=True)
def _gpu_and_record():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    path = os.environ.get("CM3P_HF_MODERNBERT_ERRORS_OUT")
    if _SEEN and path:
        with open(path, "w") as f:
            f.write("\n".join(_SEEN) + "\n")


def _hold(case: str, key: str, value: float, bound: float, lower: float = None):
    line = f"{case}: {key}={value:.3e} (bound {bound:.0e})"
    print(line)
    _SEEN.append(line)
    assert value <= bound, line
    if lower is not None:
        assert value > lower, line


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return ((got - want).norm() / want.norm()).item()


def _config(**kw):
    from transformers import ModernBertConfig

    cfg = dict(vocab_size=VOCAB, hidden_size=HID, intermediate_size=192, num_hidden_layers=4, num_attention_heads=2, max_position_embeddings=512,
               layer_types=[FULL, SLIDE, SLIDE, FULL], local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1,
               sep_token_id=2)
    cfg.update(kw)
    return ModernBertConfig(**cfg)


def _batch(S, lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(3, VOCAB, (B, S), generator=g) * mask
    w = torch.randn(B, S, HID, generator=g)
    return ids.cuda(), mask.cuda(), w.cuda()


def _loss(y, w, mask):
    return (y.float() * w)[mask.bool()].sum()


@functools.lru_cache(maxsize=None)
def _reference(S, lens, gain=1.0):
    """The reference arm, once per case: the installed model on sdpa, fp32, on the GPU -> its weights, hidden states and gradients.
    gain: factor on the four projection weights of every layer after the default init (see
    test_forward_with_projection_weights_of_trained_scale)."""
    from transformers import ModernBertModel

    torch.manual_seed(0)
    ref = ModernBertModel._from_config(_config(), attn_implementation="sdpa").cuda().eval()
    assert ref.config._attn_implementation == "sdpa" and ref.dtype == torch.float32
    if gain != 1.0:
        with torch.no_grad():
            for layer in ref.layers:
                for lin in (layer.attn.Wqkv, layer.attn.Wo, layer.mlp.Wi, layer.mlp.Wo):
                    lin.weight.mul_(gain)
    ids, mask, w = _batch(S, lens)
    out = ref(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    _loss(out.last_hidden_state, w, mask).backward()
    return dict(state={k: v.detach().clone() for k, v in ref.state_dict().items()}, last=out.last_hidden_state.detach(),
                hiddens=tuple(h.detach() for h in out.hidden_states), grads={n: p.grad.detach().clone() for n, p in ref.named_parameters()})


def _fused(state, **kw):
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    m = FusedModernBertModel(_config(**kw))
    m.load_state_dict(state, strict=True)
    return m.cuda().eval()


# ---- the tower ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,lens", GRID)
def test_forward_matches_the_installed_model_on_sdpa(S, lens):
    r = _reference(S, lens)
    ids, mask, _ = _batch(S, lens)
    m = _fused(r["state"])
    with torch.no_grad():
        out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    from transformers.modeling_outputs import BaseModelOutput

    assert isinstance(out, BaseModelOutput) and out.last_hidden_state.dtype == torch.float32 and out.attentions is None
    assert torch.isfinite(out.last_hidden_state).all()
    v = mask.bool()
    case = f"forward S={S} lens={lens}"
    # (a bit-equal result would mean the bf16-operand kernels did not run)
    _hold(case, "last_hidden_state", _rel(out.last_hidden_state[v], r["last"][v]), HIDDEN_TOL, lower=0.0)
    assert len(out.hidden_states) == len(r["hiddens"]) == 5
    for i, (h, want) in enumerate(zip(out.hidden_states, r["hiddens"])):
        assert h.shape == want.shape
        _hold(case, f"hidden_states[{i}]", _rel(h[v], want[v]), HIDDEN_TOL)
    # tuple output and the attention probabilities (eager semantics: rows over the visible keys sum to one)
    with torch.no_grad():
        tup = m(input_ids=ids, attention_mask=mask, return_dict=False)
        att = m(input_ids=ids, attention_mask=mask, output_attentions=True).attentions
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0], out.last_hidden_state)
    assert len(att) == 4 and all(a.shape == (len(lens), 2, S, S) for a in att)
    sums = att[0].sum(-1)[:, 0][v]
    assert (sums - 1).abs().max().item() <= 1e-3
    assert att[1][0, 0, 0, 66:].abs().max().item() == 0.0 if S > 66 else True  # the band of a sliding layer


def test_forward_with_projection_weights_of_trained_scale():
    """With HF's default init (std 0.02, output projections 0.007) a layer adds a few percent to the fp32 residual stream, so the
    forward errors above are those of an almost untouched stream (1e-5).  The same comparison with every projection weight six times
    larger - layers that contribute at the scale of the stream, as in a trained checkpoint - under the same hidden-state bound."""
    S, lens = GRID[0]
    r = _reference(S, lens, 6.0)
    ids, mask, _ = _batch(S, lens)
    m = _fused(r["state"])
    with torch.no_grad():
        out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    v = mask.bool()
    layer_share = _rel(r["hiddens"][1][v], r["hiddens"][0][v])
    print(f"layer 0 changes the stream by {layer_share:.3f} of its norm")
    assert layer_share > 0.1
    case = f"forward, projection weights x 6, S={S} lens={lens}"
    _hold(case, "last_hidden_state", _rel(out.last_hidden_state[v], r["last"][v]), HIDDEN_TOL, lower=0.0)
    for i, (h, want) in enumerate(zip(out.hidden_states, r["hiddens"])):
        _hold(case, f"hidden_states[{i}]", _rel(h[v], want[v]), HIDDEN_TOL)


@pytest.mark.parametrize("S,lens", GRID)
def test_backward_matches_sdpa_autograd_on_every_parameter(S, lens):
    r = _reference(S, lens)
    ids, mask, w = _batch(S, lens)
    m = _fused(r["state"]).train()
    _loss(m(input_ids=ids, attention_mask=mask).last_hidden_state, w, mask).backward()
    case = f"backward S={S} lens={lens}"
    got = dict(m.named_parameters())
    assert set(got) == set(r["grads"])
    worst = []
    for n, want in sorted(r["grads"].items()):
        g = got[n].grad
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), n
        e = _rel(g, want)
        line = f"{case}: grad.{n}={e:.3e} (bound {GRAD_TOL:.0e})"
        print(line)
        _SEEN.append(line)
        worst.append((e, n))
    assert max(worst)[0] <= GRAD_TOL, max(worst)


def test_the_fused_kernels_run_and_torch_sdpa_does_not(monkeypatch):
    from cm3p_amd import _lib
    from cm3p_amd import kernels as K

    S, lens = GRID[0]
    r = _reference(S, lens)
    ids, mask, w = _batch(S, lens)
    m = _fused(r["state"]).train()

    def no_sdpa(*a, **k):
        raise AssertionError("torch sdpa was called on the fused arm")

    monkeypatch.setattr(torch.nn.functional, "scaled_dot_product_attention", no_sdpa)
    names = []
    real_call = K.call

    def recording_call(name, *a, **k):
        names.append(name)
        return real_call(name, *a, **k)

    monkeypatch.setattr(K, "call", recording_call)
    _lib.profile_begin()
    try:
        _loss(m(input_ids=ids, attention_mask=mask).last_hidden_state, w, mask).backward()
    finally:
        tags = _lib.profile_end()
    seen = set(names)
    assert "cm3p_qkv_gemm_rope" in seen and names.count("cm3p_qkv_gemm_rope") == 4  # Wqkv + RoPE in one launch, once per layer
    assert names.count("cm3p_attn_fwd") == 4
    assert {"cm3p_embed_ln_fwd", "cm3p_layernorm_fwd", "cm3p_layernorm_bwd"} <= seen
    # GeGLU: its own kernel, or (shapes the route gives the ring GEMM) the store phase of the Wi GEMM under that epilogue's tag
    assert "cm3p_geglu_fwd" in seen or any(t.endswith(f", {_lib.EPI_BF16_GEGLU_FWD}, true>") or t.endswith(f", {_lib.EPI_BF16_GEGLU_FWD}, false>") for t in tags), (seen, set(tags))
    assert "cm3p_geglu_bwd" in seen or any(t.endswith(f", {_lib.EPI_BF16_GEGLU_BWD}, true>") or t.endswith(f", {_lib.EPI_BF16_GEGLU_BWD}, false>") for t in tags)
    assert any(n.startswith("cm3p_attn_bwd") for n in seen)
    # the profiling window saw the same launches: attention forward kernels of both kinds, and the row kernels under their own names
    assert any(t.startswith("attn_fwd") and "[global]" in t for t in tags) and any(t.startswith("attn_fwd") and "[local]" in t for t in tags), set(tags)
    assert "cm3p_layernorm_fwd" in tags and "cm3p_embed_ln_fwd" in tags


def test_unpad_inputs_agrees_with_the_padded_run_and_zero_fills_the_padding():
    from cm3p_amd import _lib

    S, lens = GRID[0]
    r = _reference(S, lens)
    ids, mask, _ = _batch(S, lens)
    m = _fused(r["state"])
    assert m.unpad_inputs is False
    with torch.no_grad():
        padded = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        m.unpad_inputs = True
        _lib.profile_begin()
        packed = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        tags = set(_lib.profile_end())
    assert any("varlen" in t for t in tags), tags  # the packed kernels really ran
    v = mask.bool()
    _hold("unpad_inputs", "last_hidden_state vs padded", _rel(packed.last_hidden_state[v], padded.last_hidden_state[v]), UNPAD_TOL)
    _hold("unpad_inputs", "last_hidden_state vs sdpa", _rel(packed.last_hidden_state[v], r["last"][v]), HIDDEN_TOL)
    assert (~v).any() and packed.last_hidden_state[~v].abs().max().item() == 0.0
    assert all(h[~v].abs().max().item() == 0.0 for h in packed.hidden_states)
    # a batch without padding is not repacked and still runs
    S2, lens2 = GRID[2]
    ids2, mask2, _ = _batch(S2, lens2)
    with torch.no_grad():
        y2 = m(input_ids=ids2, attention_mask=mask2).last_hidden_state
    _hold("unpad_inputs", "full batch vs sdpa", _rel(y2, _reference(S2, lens2)["last"]), HIDDEN_TOL)


def test_bf16_model_returns_bf16_from_the_bf16_residual_stream():
    from cm3p_amd import _lib

    S, lens = GRID[0]
    r = _reference(S, lens)
    ids, mask, _ = _batch(S, lens)
    m = _fused(r["state"]).to(torch.bfloat16)
    assert m.encoder.residual_dtype is None
    with torch.no_grad():
        _lib.profile_begin()
        out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
        tags = set(_lib.profile_end())
    assert out.last_hidden_state.dtype == torch.bfloat16 and all(h.dtype == torch.bfloat16 for h in out.hidden_states)
    with torch.no_grad():
        assert m.encoder.residual_dtype is torch.bfloat16 and m.encoder._bf16_stream(None)
    assert any("<true, true, 7" in t for t in tags), tags  # CM3P_EPI_BF16_RESID (epilogue 7): the bf16 residual adds
    v = mask.bool()
    _hold("bf16 model", "last_hidden_state vs fp32 sdpa", _rel(out.last_hidden_state[v], r["last"][v]), BF16_HIDDEN_TOL, lower=0.0)
    for i, (h, want) in enumerate(zip(out.hidden_states, r["hiddens"])):
        _hold("bf16 model", f"hidden_states[{i}] vs fp32 sdpa", _rel(h[v], want[v]), BF16_HIDDEN_TOL)
    # back to fp32 parameters: the fp32 stream again
    m = m.to(torch.float32)
    with torch.no_grad():
        y = m(input_ids=ids, attention_mask=mask).last_hidden_state
    assert y.dtype == torch.float32 and m.encoder.residual_dtype is None


def test_gradient_checkpointing_recomputes_bit_identically():
    S, lens = GRID[0]
    r = _reference(S, lens)
    ids, mask, w = _batch(S, lens)
    runs = []
    for ckpt in (False, True):
        m = _fused(r["state"]).train()
        if ckpt:
            m.gradient_checkpointing_enable()
            assert m.encoder.gradient_checkpointing and m.encoder.training
        loss = _loss(m(input_ids=ids, attention_mask=mask).last_hidden_state, w, mask)
        loss.backward()
        runs.append((loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) == 26
    for n, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][n]), n


def test_dropout_fields_are_honoured_in_train_mode_only():
    """The masks are the kernels' own: reproducible under torch.manual_seed, switched off by eval()."""
    S, lens = GRID[1]
    r = _reference(S, lens)
    ids, mask, _ = _batch(S, lens)
    m = _fused(r["state"], embedding_dropout=0.1, attention_dropout=0.1, mlp_dropout=0.1)
    v = mask.bool()
    with torch.no_grad():
        clean = m(input_ids=ids, attention_mask=mask).last_hidden_state
        m.train()
        torch.manual_seed(3)
        a = m(input_ids=ids, attention_mask=mask).last_hidden_state
        torch.manual_seed(3)
        b = m(input_ids=ids, attention_mask=mask).last_hidden_state
        c = m(input_ids=ids, attention_mask=mask).last_hidden_state
    assert _rel(clean[v], r["last"][v]) <= HIDDEN_TOL  # eval mode: no dropout
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.isfinite(a).all() and _rel(a[v], clean[v]) > 1e-2  # (far above the kernels' own rounding: masks were applied)


# ---- masked LM -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mlm_reference():
    from transformers import ModernBertForMaskedLM

    S, lens = GRID[0]
    torch.manual_seed(4)
    ref = ModernBertForMaskedLM._from_config(_config(), attn_implementation="sdpa").cuda().eval()
    assert ref.decoder.weight is ref.model.embeddings.tok_embeddings.weight
    with torch.no_grad():  # (a zero bias would hide a bias that is dropped)
        ref.decoder.bias.normal_(0.0, 0.5)
    ids, mask, _ = _batch(S, lens, seed=4)
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(3, VOCAB, (len(lens), S), generator=g)
    labels[torch.rand(len(lens), S, generator=g) < 0.85] = -100
    labels = labels.cuda()
    labels[mask == 0] = -100
    labels[3] = -100  # a row with no label at all
    assert (labels != -100).any(1).tolist() == [True, True, True, False]
    out = ref(input_ids=ids, attention_mask=mask, labels=labels)
    out.loss.backward()
    return dict(state={k: v.detach().clone() for k, v in ref.state_dict().items()}, ids=ids, mask=mask, labels=labels, loss=out.loss.detach(),
                logits=out.logits.detach(), grads={n: p.grad.detach().clone() for n, p in ref.named_parameters()})


def _fused_mlm(state, sparse=False):
    from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM

    m = FusedModernBertForMaskedLM(_config(sparse_prediction=sparse))
    m.load_state_dict(state, strict=True)
    m = m.cuda().train()
    assert m.decoder.weight is m.model.embeddings.tok_embeddings.weight
    return m


def test_masked_lm_loss_logits_and_the_tied_embedding_gradient():
    r = _mlm_reference()
    m = _fused_mlm(r["state"])
    out = m(input_ids=r["ids"], attention_mask=r["mask"], labels=r["labels"])
    v = r["mask"].bool()
    assert out.logits.shape == r["logits"].shape == (4, 200, VOCAB)
    _hold("masked LM", "loss abs diff", abs(out.loss.item() - r["loss"].item()), LOSS_TOL)
    _hold("masked LM", "logits", _rel(out.logits[v], r["logits"][v]), LOGITS_TOL, lower=0.0)
    out.loss.backward()
    got = dict(m.named_parameters())
    assert set(got) == set(r["grads"])
    table = "model.embeddings.tok_embeddings.weight"
    # embedding backward + decoder weight gradient on ONE parameter: the whole table, rows of ids that never occur included (the
    # decoder's gradient is dense, so no row is exactly zero by construction)
    _hold("masked LM", f"grad.{table}", _rel(got[table].grad, r["grads"][table]), GRAD_TOL)
    for n, want in sorted(r["grads"].items()):
        if n != table:
            _hold("masked LM", f"grad.{n}", _rel(got[n].grad, want), GRAD_TOL)
    # without labels: logits only
    with torch.no_grad():
        plain = m(input_ids=r["ids"], attention_mask=r["mask"])
    assert plain.loss is None and _rel(plain.logits[v], r["logits"][v]) <= LOGITS_TOL


def test_masked_lm_sparse_prediction_gives_the_same_loss():
    r = _mlm_reference()
    m = _fused_mlm(r["state"], sparse=True)
    assert m.sparse_prediction
    out = m(input_ids=r["ids"], attention_mask=r["mask"], labels=r["labels"])
    n = int((r["labels"] != -100).sum())
    assert out.logits.shape == (n, VOCAB)
    _hold("masked LM sparse", "loss abs diff", abs(out.loss.item() - r["loss"].item()), LOSS_TOL)
    _hold("masked LM sparse", "logits", _rel(out.logits, r["logits"][r["labels"] != -100]), LOGITS_TOL)
    out.loss.backward()
    table = "model.embeddings.tok_embeddings.weight"
    _hold("masked LM sparse", f"grad.{table}", _rel(m.model.embeddings.tok_embeddings.weight.grad, r["grads"][table]), GRAD_TOL)


# ---- a third-party head on the fused tower ----------------------------------------------------------------------------------------------------
def test_sequence_classification_head_on_the_fused_tower_trains_through_shared_parameters():
    from cm3p_amd.hf_modernbert import FusedModernBertModel, fuse
    from transformers import ModernBertForSequenceClassification

    S, lens = GRID[0]
    ids, mask, _ = _batch(S, lens, seed=6)
    torch.manual_seed(6)
    ref = ModernBertForSequenceClassification._from_config(_config(num_labels=3), attn_implementation="sdpa").cuda().eval()
    m = ModernBertForSequenceClassification._from_config(_config(num_labels=3), attn_implementation="sdpa")
    m.load_state_dict(ref.state_dict())
    m = m.cuda().eval()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)  # built BEFORE fuse
    assert fuse(m) is m and isinstance(m.model, FusedModernBertModel)
    with torch.no_grad():
        want = ref(input_ids=ids, attention_mask=mask).logits
    out = m(input_ids=ids, attention_mask=mask, labels=torch.tensor([0, 1, 2, 1], device="cuda"))
    assert out.logits.shape == (4, 3)
    _hold("sequence classification", "logits", _rel(out.logits, want), HIDDEN_TOL, lower=0.0)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    out.loss.backward()
    opt.step()
    changed = [n for n, p in m.named_parameters() if not torch.equal(p, before[n])]
    assert "model.layers.0.attn.Wqkv.weight" in changed and "model.embeddings.tok_embeddings.weight" in changed and "classifier.weight" in changed
    assert len(changed) >= 26
