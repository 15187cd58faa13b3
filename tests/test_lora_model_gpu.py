"""Low-rank adapters on a whole tower (cm3p_amd.lora + the encoder's layer nodes), `-m gpu`: a head_dim-64 tower of 3 layers (global,
sliding, global), hidden 128, B = 2, S = 200 with the second sequence right-padded down to ONE token - the smallest model where tile
seams and packing still bite.  The reference is the float64 oracle on the CPU run with W + s B A as its weights; its full weight
gradients dW give dA = s B^T dW and dB = s dW A^T.  Bounds are the project's class bounds as tests/test_hf_modernbert_gpu.py states
them: hidden states rel-L2 2e-2, parameter gradients 6e-2, packed against padded 5e-3; merge_lora against the adapted model 5e-3."""
import functools

import pytest
import torch

import transformers  # noqa: F401  (a missing transformers is an error here, not a skip)

pytestmark = pytest.mark.gpu

FULL, SLIDE = "full_attention", "sliding_attention"
HIDDEN_TOL, GRAD_TOL, UNPAD_TOL, MERGE_TOL = 2e-2, 6e-2, 5e-3, 5e-3
VOCAB, HID, S, LENS = 200, 128, 200, (200, 1)
TARGETS = ("attn.Wqkv", "attn.Wo", "mlp.Wi", "mlp.Wo")


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm()).item()


def _config(**kw):
    from transformers import ModernBertConfig

    cfg = dict(vocab_size=VOCAB, hidden_size=HID, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2, max_position_embeddings=512,
               layer_types=[FULL, SLIDE, FULL], local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2)
    cfg.update(kw)
    return ModernBertConfig(**cfg)


@functools.lru_cache(maxsize=None)
def _state():
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    torch.manual_seed(0)
    return {k: v.clone() for k, v in FusedModernBertModel(_config()).state_dict().items()}


def _model(**kw):
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    m = FusedModernBertModel(_config(**kw))
    m.load_state_dict(_state(), strict=True)
    return m.cuda().eval()


def _batch():
    g = torch.Generator().manual_seed(0)
    mask = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(3, VOCAB, (len(LENS), S), generator=g) * mask
    w = torch.randn(len(LENS), S, HID, generator=g)
    return ids, mask, w


def _loss(y, w, mask):
    return (y.float() * w)[mask.bool()].sum()


def _randomise(m, seed=1):
    """The same A and B on every model (add_lora draws A from torch's global generator): A as kaiming_uniform_(a = sqrt 5) leaves it,
    U(-1 / sqrt(in), 1 / sqrt(in)); B as large as a trained adapter's, so that s B A moves the weights by a few percent."""
    from cm3p_amd import lora

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in sorted(lora.lora_state_dict(m).items()):
            if k.endswith("lora_B"):
                v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.device))
            else:
                v.copy_(((torch.rand(v.shape, generator=g) * 2 - 1) * v.shape[1] ** -0.5).to(v.device))
    return m


def _adapted(r=8, alpha=16, randomise=True, **kw):
    from cm3p_amd import lora

    m = lora.add_lora(_model(), r=r, alpha=alpha, **kw)
    return _randomise(m) if randomise else m


@functools.lru_cache(maxsize=None)
def _reference(r=8, alpha=16):
    """The float64 oracle with W + s B A as its weights, once: hidden states, last_hidden_state, dA and dB by the chain rule."""
    from cm3p_amd import lora
    from oracle import cm3p_oracle as O

    m = _adapted(r, alpha)
    enc = m.encoder.config
    cfg = dict(num_attention_heads=enc.num_attention_heads, hidden_size=enc.hidden_size, norm_eps=enc.norm_eps, num_hidden_layers=3,
               local_attention=2 * enc.half_window, global_rope_theta=enc.global_rope_theta, local_rope_theta=enc.local_rope_theta,
               global_attn_every_n_layers=2)
    assert [enc.is_global_layer(i) for i in range(3)] == [True, False, True] and enc.half_window == 64
    ad = {k: v.detach().double().cpu() for k, v in lora.lora_state_dict(m).items()}
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items() if k not in ad}
    s = alpha / r
    leaves = {}
    for i in range(3):
        for t in TARGETS:
            k = f"layers.{i}.{t}"
            leaves[k] = (sd[k + ".weight"] + s * ad[k + ".lora_B"] @ ad[k + ".lora_A"]).requires_grad_(True)
            sd[k + ".weight"] = leaves[k]
    ids, mask, w = _batch()
    collect = []
    y = O.encoder(sd, "", cfg, input_ids=ids, attention_mask=mask, collect=collect)
    _loss(y, w.double(), mask).backward()
    grads = {}
    for k, leaf in leaves.items():
        grads[k + ".lora_A"] = s * ad[k + ".lora_B"].t() @ leaf.grad
        grads[k + ".lora_B"] = s * leaf.grad @ ad[k + ".lora_A"].t()
    return dict(last=y.detach(), hiddens=[h.detach() for h in collect], grads=grads, adapters=ad)


def test_fresh_adapters_leave_every_output_bit_unchanged():
    ids, mask, w = (t.cuda() for t in _batch())
    plain, fresh = _model(), _adapted(randomise=False)
    with torch.no_grad():
        assert torch.equal(fresh(input_ids=ids, attention_mask=mask).last_hidden_state, plain(input_ids=ids, attention_mask=mask).last_hidden_state)
    plain.train(), fresh.train()
    y0, y1 = plain(input_ids=ids, attention_mask=mask).last_hidden_state, fresh(input_ids=ids, attention_mask=mask).last_hidden_state
    assert y1.requires_grad and torch.equal(y0, y1)
    pd, fd = _model(mlp_dropout=0.25).train(), None
    from cm3p_amd import lora

    fd = lora.add_lora(_model(mlp_dropout=0.25), r=8, alpha=16).train()
    torch.manual_seed(5)
    y0 = pd(input_ids=ids, attention_mask=mask).last_hidden_state
    torch.manual_seed(5)
    y1 = fd(input_ids=ids, attention_mask=mask).last_hidden_state
    assert torch.equal(y0, y1)
    torch.manual_seed(6)
    assert not torch.equal(pd(input_ids=ids, attention_mask=mask).last_hidden_state, y0)  # (the dropout really is on)


def test_forward_and_adapter_gradients_against_the_float64_oracle():
    ref = _reference()
    ids, mask, w = (t.cuda() for t in _batch())
    m = _adapted().train()
    out = m(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    _loss(out.last_hidden_state, w, mask).backward()
    v = mask.bool().cpu()
    e = _rel(out.last_hidden_state.cpu()[v], ref["last"][v])
    print(f"last_hidden_state: {e:.3e} (bound {HIDDEN_TOL:.0e})")
    assert e <= HIDDEN_TOL
    for i, (h, want) in enumerate(zip(out.hidden_states[:-1], ref["hiddens"][:-1])):
        e = _rel(h.cpu()[v], want[v])
        print(f"hidden_states[{i}]: {e:.3e}")
        assert e <= HIDDEN_TOL, i
    worst = []
    params = dict(m.named_parameters())
    for k, want in sorted(ref["grads"].items()):
        g = params[k].grad
        assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
        e = _rel(g, want)
        print(f"grad.{k}: {e:.3e} (bound {GRAD_TOL:.0e})")
        worst.append((e, k))
    assert max(worst)[0] <= GRAD_TOL, max(worst)
    # the adapter is not a no-op at this scale: the plain model sits far further from the reference than the adapted one
    with torch.no_grad():
        away = _rel(_model()(input_ids=ids, attention_mask=mask).last_hidden_state.cpu()[v], ref["last"][v])
    print(f"the model without adapters is {away:.3e} from the reference")
    assert away > 5e-3 and away > 10 * _rel(out.last_hidden_state.cpu()[v], ref["last"][v])


def _is_wgrad(tag):
    return "<false, false," in tag  # the weight-gradient GEMMs are the family's only calls with both operands token-major


def test_frozen_base_launches_no_weight_gradient_gemm_and_unfrozen_base_gets_the_plain_models_bits():
    from cm3p_amd import _lib, lora

    ids, mask, w = (t.cuda() for t in _batch())
    m = _adapted().train()
    _lib.profile_begin()
    try:
        _loss(m(input_ids=ids, attention_mask=mask).last_hidden_state, w, mask).backward()
    finally:
        tags = _lib.profile_end()
    ad = lora.lora_state_dict(m)
    for k, p in m.named_parameters():
        assert (p.grad is not None) == (k in ad), k  # base .grad is None, every adapter tensor has one
    assert not [t for t in tags if _is_wgrad(t)], sorted(tags)
    assert tags["cm3p_lora_grad"][0] == 12 and tags["cm3p_lora_merge_cast_multi"][0] == 1, sorted(tags)
    # freeze_base=False: the base gradients are those of a plain model whose weights are the merged operands (bf16 values, so that
    # its own cast reproduces them in bits); the weight-gradient GEMMs run
    u = _adapted(freeze_base=False).train()
    _lib.profile_begin()
    try:
        _loss(u(input_ids=ids, attention_mask=mask).last_hidden_state, w, mask).backward()
    finally:
        tags_u = _lib.profile_end()
    assert sum(n for t, (n, _, _) in tags_u.items() if _is_wgrad(t)) == 12 and tags_u["cm3p_lora_grad"][0] == 12
    from cm3p_amd import kernels as K

    plain = _model().train()
    with torch.no_grad():
        for i in range(3):
            for t in TARGETS:
                src, dst = u.layers[i].get_submodule(t), plain.layers[i].get_submodule(t)
                (eff, _), = K.lora_merge_cast_many([(src.weight.detach(), src.lora_A.detach(), src.lora_B.detach(), src.lora_scale, False)])
                dst.weight.copy_(eff.float())
    _loss(plain(input_ids=ids, attention_mask=mask).last_hidden_state, w, mask).backward()
    got = dict(u.named_parameters())
    for k, p in plain.named_parameters():
        assert got[k].grad is not None and torch.equal(got[k].grad, p.grad), k
    # adapters of the unfrozen and the frozen model: the same launches on the same operands
    for k in ad:
        assert torch.equal(got[k].grad, dict(m.named_parameters())[k].grad), k


def test_gradient_checkpointing_recomputes_bit_identically():
    ids, mask, w = (t.cuda() for t in _batch())
    a, b = _adapted().train(), _adapted().train()
    b.gradient_checkpointing_enable()
    assert b.encoder.gradient_checkpointing
    ya, yb = a(input_ids=ids, attention_mask=mask).last_hidden_state, b(input_ids=ids, attention_mask=mask).last_hidden_state
    assert torch.equal(ya, yb)
    _loss(ya, w, mask).backward()
    _loss(yb, w, mask).backward()
    pb = dict(b.named_parameters())
    for k, p in a.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, pb[k].grad), k


def test_unpadded_and_caller_packed_rows_agree_with_the_padded_run():
    from cm3p_amd import _lib

    ref = _reference()
    ids, mask, w = (t.cuda() for t in _batch())
    v = mask.bool()
    pad, unp = _adapted().train(), _adapted().train()
    unp.unpad_inputs = True
    yp = pad(input_ids=ids, attention_mask=mask).last_hidden_state
    _lib.profile_begin()
    try:
        yu = unp(input_ids=ids, attention_mask=mask).last_hidden_state
    finally:
        tags = set(_lib.profile_end())
    assert any("varlen" in t for t in tags), tags
    e = _rel(yu[v], yp[v])
    print(f"unpad_inputs last_hidden_state vs padded: {e:.3e} (bound {UNPAD_TOL:.0e})")
    assert e <= UNPAD_TOL and yu[~v].abs().max().item() == 0.0
    _loss(yu, w, mask).backward()
    # caller-packed rows through the encoder's own entry: T = 201 valid tokens, not a multiple of anything
    cp = _adapted().train()
    cu = torch.tensor([0, LENS[0], LENS[0] + LENS[1]], dtype=torch.int32, device="cuda")
    yc = cp.encoder(input_ids=ids[v], cu_seqlens=cu, max_seqlen=S)
    assert yc.shape == (sum(LENS), HID)
    e = _rel(yc, yp[v])
    print(f"caller-packed last_hidden_state vs padded: {e:.3e} (bound {UNPAD_TOL:.0e})")
    assert e <= UNPAD_TOL
    (yc.float() * w[v]).sum().backward()
    for name, model in (("unpad_inputs", unp), ("caller-packed", cp)):
        worst = max((_rel(p.grad, ref["grads"][k]), k) for k, p in model.named_parameters() if k in ref["grads"])
        print(f"{name}: worst adapter gradient against the oracle {worst[0]:.3e} at {worst[1]} (bound {GRAD_TOL:.0e})")
        assert worst[0] <= GRAD_TOL, (name, worst)


def test_an_in_place_edit_of_lora_b_between_two_forward_only_calls_is_seen():
    ids, mask, _ = (t.cuda() for t in _batch())
    m = _adapted()
    with torch.no_grad():
        y0 = m(input_ids=ids, attention_mask=mask).last_hidden_state
        y1 = m(input_ids=ids, attention_mask=mask).last_hidden_state  # (served from the kept copies)
        assert torch.equal(y0, y1)
        m.layers[1].mlp.Wi.lora_B.mul_(-1.0)
        y2 = m(input_ids=ids, attention_mask=mask).last_hidden_state
        assert not torch.equal(y0, y2)
        m.layers[1].mlp.Wi.lora_B.mul_(-1.0)
        m.layers[2].attn.Wo.lora_A.add_(0.01)
        y3 = m(input_ids=ids, attention_mask=mask).last_hidden_state
        assert not torch.equal(y0, y3) and not torch.equal(y2, y3)


def test_merge_lora_keeps_the_outputs_within_one_rerounding_of_the_weights():
    from cm3p_amd import lora

    ids, mask, _ = (t.cuda() for t in _batch())
    m = _adapted(r=16, alpha=32)
    v = mask.bool()
    with torch.no_grad():
        y0 = m(input_ids=ids, attention_mask=mask).last_hidden_state
        lora.merge_lora(m)
        assert lora.lora_state_dict(m) == {} and all(p.requires_grad for p in m.parameters())
        y1 = m(input_ids=ids, attention_mask=mask).last_hidden_state
        base = _model()(input_ids=ids, attention_mask=mask).last_hidden_state
    e = _rel(y1[v], y0[v])
    print(f"merged against adapted: {e:.3e} (bound {MERGE_TOL:.0e}); the base model is {_rel(base[v], y0[v]):.3e} away")
    assert e <= MERGE_TOL and _rel(base[v], y0[v]) > MERGE_TOL  # (the adapter is no no-op at this scale)
