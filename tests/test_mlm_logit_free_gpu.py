"""`logit_free_mlm_loss` (CM3PModel with the decoder head, CM3PForMaskedLM, FusedModernBertForMaskedLM), `-m gpu`: in training mode with
labels the masked-LM loss comes from _MLMHeadLogitFreeLossFn (csrc/mlm_loss.hip), which never stores the [rows, vocab] logits.

Tiny models (hidden 64, 2 layers, head_dim 16 and 64, B = 2, S = 64, one padded row, about a quarter of the positions labelled).  With
the switch on `logits` is None and the loss and every parameter gradient agree with the switch-off step of the same seeded model -
gradients within FIX_TOL["grad"], the class tolerance of tests/test_model_gpu.py, the loss within the 1e-4 tests/loss_head_refs.py
documents for it (ce_stats_ref: "a few 1e-5" at lse = 100) - and the same parameters have a gradient.  Evaluation and calls without
labels return the switch-off bits; so does a step after the switch is turned off again.  The memory test states the sizes the two
nodes hold.  Every measured figure is printed before it is held (`pytest -s`)."""
import copy

import pytest
import torch

import transformers  # noqa: F401  (a missing transformers is an error here, not a skip)

import test_model_gpu as TM
from cases import _BEATMAP_C1, _METADATA_C1, _cfg

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIX_TOL = TM.FIX_TOL
LOSS_TOL = 1e-4
B, S, L_META, LENS = 2, 64, 16, (64, 50)
KINDS = ("masked_lm dense", "masked_lm sparse", "model", "model labelled rows", "model packed rows", "fused modernbert", "fused modernbert sparse")


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm().clamp_min(1e-12)).item()


def _hold(what: str, value: float, bound: float):
    print(f"{what} = {value:.3e} (bound {bound:.0e})")
    assert value <= bound, f"{what} = {value:.3e} > {bound:.0e}"


def _batch():
    g = torch.Generator().manual_seed(91)
    mask = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(3, 194, (B, S), generator=g) * mask
    pick = (torch.rand(B, S, generator=g) < 0.25) & mask.bool()
    pick[0, 0], pick[1, LENS[1] - 1] = True, True  # a labelled CLS, a label on a row's last valid token
    labels = torch.where(pick, ids, torch.full_like(ids, -100))
    mids = torch.randint(3, 97, (B, L_META), generator=g)
    return dict(input_ids=ids, attention_mask=mask, labels=labels, metadata_ids=mids, metadata_attention_mask=torch.ones_like(mids))


def _build(kind, heads):
    """A freshly seeded model of the kind on the device in training mode, and the keyword arguments of a training call."""
    torch.manual_seed(0)
    b = {k: v.to(DEV) for k, v in _batch().items()}
    three = {k: b[k] for k in ("input_ids", "attention_mask", "labels")}
    if kind.startswith("masked_lm"):
        from cm3p_amd import CM3PBeatmapConfig
        from cm3p_amd.modeling_cm3p import CM3PForMaskedLM

        cfg = dict(_BEATMAP_C1, num_hidden_layers=2, num_attention_heads=heads, sparse_prediction=kind.endswith("sparse"))
        return CM3PForMaskedLM(CM3PBeatmapConfig(**cfg)).to(DEV).train(), three
    if kind.startswith("fused modernbert"):
        from transformers import ModernBertConfig

        from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM

        cfg = ModernBertConfig(vocab_size=203, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=heads,
                               max_position_embeddings=512, local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1,
                               sep_token_id=2, sparse_prediction=kind.endswith("sparse"))
        model = FusedModernBertForMaskedLM(cfg).to(DEV).train()
        assert model.decoder.weight is model.model.embeddings.tok_embeddings.weight and cfg.vocab_size % 64 != 0  # tied; the vocabulary is padded
        return model, three
    from cm3p_amd import CM3PConfig, CM3PModel

    c = copy.deepcopy(dict(_cfg(dict(_BEATMAP_C1, num_hidden_layers=2, num_attention_heads=heads), dict(_METADATA_C1, num_hidden_layers=2)),
                           has_decoder_head=True, loss_type="ForMaskedLM"))
    model = CM3PModel(CM3PConfig(**c)).to(DEV).train()
    if kind == "model labelled rows":
        model.labelled_rows_last_layer = True
    if kind == "model packed rows":  # the caller unpads: _unpad_cm3p_input (ref:cm3p/modeling_cm3p.py:88-104) restated
        model.pool_unpadded = True
        mask = b["attention_mask"]
        lens = mask.sum(dim=-1, dtype=torch.int32)
        indices = torch.nonzero(mask.flatten(), as_tuple=False).flatten()
        cu = torch.nn.functional.pad(torch.cumsum(lens, dim=0, dtype=torch.int32), (1, 0))
        b = dict(input_ids=b["input_ids"].flatten()[indices], indices=indices, cu_seqlens=cu, max_seqlen=int(lens.max()), batch_size=B, seq_len=S,
                 labels=b["labels"].flatten()[indices], metadata_ids=b["metadata_ids"], metadata_attention_mask=b["metadata_attention_mask"])
    return model, b


def _step(model, kw):
    model.zero_grad(set_to_none=True)
    out = model(**kw)
    out.loss.backward()
    return out, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


# (caller-packed rows run on the head_dim 64 attention kernels only: the encoder refuses them at head_dim 16, with or without the switch)
CASES = [(k, h) for k in KINDS for h in (4, 1) if not (k == "model packed rows" and h == 4)]


@pytest.mark.parametrize("kind,heads", CASES, ids=[f"{k}-head_dim {64 // h}" for k, h in CASES])
def test_switch_on_against_switch_off(kind, heads, monkeypatch):
    monkeypatch.setenv("CM3P_TOWER_OVERLAP", "0")
    off, kw = _build(kind, heads)
    on, _ = _build(kind, heads)
    assert off.logit_free_mlm_loss is False and "logit_free_mlm_loss" not in off.state_dict() and not hasattr(off.config, "logit_free_mlm_loss")
    on.load_state_dict(off.state_dict())
    on.logit_free_mlm_loss = True
    o0, g0 = _step(off, kw)
    o1, g1 = _step(on, kw)
    assert o0.logits is not None and o1.logits is None, "the switch-on training step still returns logits"
    assert list(o1.keys()) == [k for k in o0.keys() if k != "logits"]  # (field order; a None field is not listed)
    assert o1.loss.shape == () and o1.loss.dtype == o0.loss.dtype
    _hold(f"{kind}: loss", abs(o1.loss.item() - o0.loss.item()), LOSS_TOL)
    assert set(g1) == set(g0), sorted(set(g1) ^ set(g0))
    worst = max((_rel(g1[k], g0[k]), k) for k in g0 if g0[k].norm() > 1e-8)
    _hold(f"{kind}: worst gradient ({worst[1]})", worst[0], FIX_TOL["grad"])
    for k in g0:
        if g0[k].norm() <= 1e-8:
            assert g1[k].norm() <= 1e-8, k
    # a second step with the switch on: the same bits (fixed reduction orders)
    o2, g2 = _step(on, kw)
    assert torch.equal(o2.loss, o1.loss)
    head = [k for k in g1 if k.startswith(("head.", "decoder."))]
    assert head and all(torch.equal(g2[k], g1[k]) for k in head)

    # calls the switch does not touch: evaluation (with labels) and no labels return the switch-off model's bits
    no_labels = {k: v for k, v in kw.items() if k != "labels"}
    with torch.no_grad():
        a, b = on(**no_labels), off(**no_labels)
        assert a.logits is not None and torch.equal(a.logits, b.logits), "training mode without labels"
        on.eval(), off.eval()
        a, b = on(**kw), off(**kw)
        assert a.logits is not None and torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss), "evaluation with labels"
        a, b = on(**no_labels), off(**no_labels)
        assert torch.equal(a.logits, b.logits), "evaluation without labels"
    if kind.startswith("model"):
        with torch.no_grad():
            a = on.train()(**dict(kw, return_loss=False))
        assert a.logits is not None, "return_loss off"

    # switch off after switch on: the original forward bits and head gradients
    on.train(), off.train()
    on.logit_free_mlm_loss = False
    o3, g3 = _step(on, kw)
    assert torch.equal(o3.loss, o0.loss) and torch.equal(o3.logits, o0.logits)
    assert all(torch.equal(g3[k], g0[k]) for k in head)


def test_num_items_in_batch_reaches_the_logit_free_node():
    off, kw = _build("masked_lm dense", 4)
    on, _ = _build("masked_lm dense", 4)
    on.load_state_dict(off.state_dict())
    on.logit_free_mlm_loss = True
    n = torch.tensor(57, device=DEV)
    o0, g0 = _step(off, dict(kw, num_items_in_batch=n))
    o1, g1 = _step(on, dict(kw, num_items_in_batch=n))
    plain, _ = _step(on, kw)
    assert abs(plain.loss.item() - o1.loss.item()) > 1e-2  # (57 is not the number of labels: the two losses differ)
    _hold("num_items_in_batch: loss", abs(o1.loss.item() - o0.loss.item()), LOSS_TOL)
    worst = max((_rel(g1[k], g0[k]), k) for k in g0 if g0[k].norm() > 1e-8)
    _hold(f"num_items_in_batch: worst gradient ({worst[1]})", worst[0], FIX_TOL["grad"])


def test_the_head_node_holds_no_logits_sized_tensor():
    """T = 2048, V = Vp = 8192, H = 64: the fp32 logits are 64 MiB.  Around forward + backward of the head node the peak of allocated
    memory rises by at least that with _MLMHeadLossFn (it holds the logits and, in backward, 32 MiB of bf16 gradient beside them) and
    by less than that with _MLMHeadLogitFreeLossFn, whose largest tensor is one 32 MiB chunk of bf16 dlogits next to its workspaces
    (1 MiB of (M, S) pairs, 0.5 MiB of column sums) and the decoder's 2 MiB weight gradient and its split-K slabs."""
    from cm3p_amd import modeling_cm3p as M

    T, V, H = 2048, 8192, 64
    logits_bytes = T * V * 4
    g = torch.Generator().manual_seed(5)
    p = dict(h=torch.randn(T, H, generator=g), Wd=torch.randn(H, H, generator=g) / 8, bd=torch.zeros(H), nw=torch.ones(H),
             Wdec=torch.randn(V, H, generator=g) / 4, bdec=torch.zeros(V))
    lab = torch.where(torch.rand(T, generator=g) < 0.15, torch.randint(0, V, (T,), generator=g), torch.full((T,), -100)).to(DEV)
    rise, losses = {}, {}
    for name, node in (("off", M._MLMHeadLossFn), ("on", M._MLMHeadLogitFreeLossFn)):
        d = {k: v.to(DEV).requires_grad_(True) for k, v in p.items()}
        for _ in range(2):  # (the first pass also fills the bf16 weight cache and loads the kernels)
            for t in d.values():
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = node.apply(d["h"], d["Wd"], d["bd"], d["nw"], d["Wdec"], d["bdec"], 1e-5, lab, None)
            loss = out[1] if name == "off" else out
            loss.backward()
            torch.cuda.synchronize()
            rise[name] = torch.cuda.max_memory_allocated() - base
            losses[name] = loss.item()
            del out, loss
    print(f"peak rise around the head node: off {rise['off'] / 2 ** 20:.1f} MiB, on {rise['on'] / 2 ** 20:.1f} MiB (logits {logits_bytes / 2 ** 20:.0f} MiB)")
    assert rise["off"] >= logits_bytes
    assert rise["on"] < logits_bytes
    assert abs(losses["on"] - losses["off"]) <= LOSS_TOL
