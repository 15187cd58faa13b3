"""`predict_tokens` and `masked_lm_accuracy` (CM3PForMaskedLM, CM3PModel with the decoder head, FusedModernBertForMaskedLM), `-m gpu`:
the k most likely tokens at selected positions from cm3p_mlm_topk, which never stores the [rows, vocab] logits.

Small models (hidden 128, two heads of 64, one global and one sliding-window layer, B = 3, S = 200, the last row right-padded to 100,
vocabulary 190 and 300: one and three column tiles of 128).  The reference route is `model(...).logits` on the same inputs, the path
every caller had before.  Held per call:
  rows      equal the selected rows (a mask, a list, None = every unmasked position, an empty selection);
  values    `logits` and `logprobs` agree with the full route's values at the returned ids within FIX_TOL["mlm_logits"], the class
            tolerance of tests/test_model_gpu.py for these logits (relative L2);
  ranking   every returned id's full-route logit is no further below the full route's i-th largest logit of the row than that
            tolerance times the row's largest |logit| - a statement that holds through ties and leaves no row out;
  no id twice in a row, every id inside the vocabulary.
`masked_lm_accuracy` equals the three counts of the reference's compute_metrics (ref:train.py:75-90) evaluated with torch on the full
route's logits, on labels placed on rows whose first six full-route logits are further apart than the ranking margin.  The memory
test states what the two routes allocate.  Every measured figure is printed before it is held (`pytest -s`)."""
import copy
import functools

import pytest
import torch

import transformers  # noqa: F401  (a missing transformers is an error here, not a skip)

import test_model_gpu as TM
from cases import _BEATMAP_C1, _METADATA_C1, _cfg

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = TM.FIX_TOL["mlm_logits"]
B, S, LENS = 3, 200, (200, 200, 100)
CLASSES = ("masked_lm", "model", "fused modernbert")
VOCABS = (190, 300)


def _hold(what: str, value: float, bound: float):
    print(f"{what} = {value:.3e} (bound {bound:.0e})")
    assert value <= bound, f"{what} = {value:.3e} > {bound:.0e}"


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def _batch(V):
    g = torch.Generator().manual_seed(17 + V)
    mask = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(3, V - 4, (B, S), generator=g) * mask
    pick = (torch.rand(B, S, generator=g) < 0.15) & mask.bool()
    pick[0, 0], pick[1, S - 1], pick[2, LENS[2] - 1] = True, True, True  # a CLS row, a row's last position, the last valid one of the padded row
    return ids.to(DEV), mask.to(DEV), pick.to(DEV)


def _beatmap_cfg(V, **over):
    return dict(_BEATMAP_C1, vocab_size=V, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                global_attn_every_n_layers=2, local_attention=128, audio_sos_token_id=V - 3, audio_eos_token_id=V - 2, audio_token_id=V - 1, **over)


def _build(kind, V, decoder_head=True):
    torch.manual_seed(0)
    if kind == "masked_lm":
        from cm3p_amd import CM3PBeatmapConfig
        from cm3p_amd.modeling_cm3p import CM3PForMaskedLM

        return CM3PForMaskedLM(CM3PBeatmapConfig(**_beatmap_cfg(V))).to(DEV).eval()
    if kind == "fused modernbert":
        from transformers import ModernBertConfig

        from cm3p_amd.hf_modernbert import FusedModernBertForMaskedLM

        cfg = ModernBertConfig(vocab_size=V, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                               max_position_embeddings=512, global_attn_every_n_layers=2, local_attention=128, pad_token_id=0, bos_token_id=1,
                               eos_token_id=2, cls_token_id=1, sep_token_id=2)
        return FusedModernBertForMaskedLM(cfg).to(DEV).eval()
    from cm3p_amd import CM3PConfig, CM3PModel

    c = copy.deepcopy(dict(_cfg(_beatmap_cfg(V), dict(_METADATA_C1, num_hidden_layers=2)), has_decoder_head=decoder_head, loss_type="ForMaskedLM"))
    return CM3PModel(CM3PConfig(**c)).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _model(kind, V):
    return _build(kind, V)


def _tower(model, kind):
    return model.model if kind == "fused modernbert" else model.beatmap_model


def _set_unpad(model, kind, value):
    (model if kind == "model" else _tower(model, kind)).unpad_inputs = value


def _full(model, kind, ids, mask):
    """The reference route: (B * S, V) fp32 logits of the plain forward."""
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, return_loss=False) if kind == "model" else model(input_ids=ids, attention_mask=mask)
    return out.logits.reshape(B * S, -1).float()


def _check(pred, full, rows, k, V, tag):
    assert torch.equal(pred.rows, rows), f"{tag}: rows"
    n = rows.numel()
    assert pred.token_ids.shape == (n, k) and pred.token_ids.dtype == torch.int64 and pred.logits.shape == (n, k) and pred.logprobs.shape == (n, k)
    assert pred.logits.dtype == pred.logprobs.dtype == torch.float32
    ids = pred.token_ids
    assert bool(((ids >= 0) & (ids < V)).all()), f"{tag}: an id outside the vocabulary"
    srt = ids.sort(1).values
    assert not bool((srt[:, 1:] == srt[:, :-1]).any()), f"{tag}: an id twice in a row"
    sel = full[rows]
    at = sel.gather(1, ids)
    _hold(f"{tag}: logits at the returned ids", _rel(pred.logits, at), TOL)
    _hold(f"{tag}: logprobs at the returned ids", _rel(pred.logprobs, at - torch.logsumexp(sel, 1, keepdim=True)), TOL)
    short = (sel.topk(k, dim=1).values - at).clamp_min(0) / sel.abs().amax(1, keepdim=True)
    _hold(f"{tag}: returned ids below the full route's i-th largest logit / largest |logit|", short.max().item(), TOL)
    hits = (ids == sel.topk(k, dim=1).indices).float().mean().item()
    print(f"{tag}: {100 * hits:.1f} % of the ids equal torch.topk's on the full route")


# ================================================================================================ classes and positions
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("kind", CLASSES)
def test_predictions_against_the_full_route(kind, V):
    model = _model(kind, V)
    ids, mask, pick = _batch(V)
    full = _full(model, kind, ids, mask)
    rows = torch.nonzero(pick.flatten()).flatten()
    for k in (5, 1, 8):
        pred = model.predict_tokens(ids, attention_mask=mask, positions=pick, k=k)
        _check(pred, full, rows, k, V, f"{kind} V={V} mask k={k}")
    listed = model.predict_tokens(ids, attention_mask=mask, positions=rows, k=8)
    for f in ("rows", "token_ids", "logits", "logprobs"):
        assert torch.equal(listed[f], pred[f]), f"a list and a mask of the same positions differ in {f}"
    listed = model.predict_tokens(ids, attention_mask=mask, positions=rows.tolist(), k=8)
    assert torch.equal(listed.token_ids, pred.token_ids)
    every = model.predict_tokens(ids, attention_mask=mask)
    _check(every, full, torch.nonzero(mask.flatten()).flatten(), 5, V, f"{kind} V={V} every unmasked position")
    for empty in (torch.zeros_like(pick), torch.empty(0, dtype=torch.int64, device=DEV)):
        none = model.predict_tokens(ids, attention_mask=mask, positions=empty, k=3)
        assert none.rows.shape == (0,) and none.rows.dtype == torch.int64 and none.token_ids.shape == (0, 3) and none.token_ids.dtype == torch.int64
        assert none.logits.shape == none.logprobs.shape == (0, 3) and none.rows.device.type == "cuda"
    # the plain forward is what it was: the same bits after the prediction calls
    assert torch.equal(_full(model, kind, ids, mask), full)


@pytest.mark.parametrize("kind", CLASSES)
def test_unpadded_execution_and_the_bf16_stream(kind):
    V = 300
    model = _build(kind, V)
    ids, mask, pick = _batch(V)
    rows = torch.nonzero(pick.flatten()).flatten()
    plain = model.predict_tokens(ids, attention_mask=mask, positions=pick)
    _set_unpad(model, kind, True)
    full = _full(model, kind, ids, mask)
    pred = model.predict_tokens(ids, attention_mask=mask, positions=pick)
    _check(pred, full, rows, 5, V, f"{kind} unpad_inputs")
    _hold(f"{kind}: unpad_inputs against padded execution", _rel(pred.logits, plain.logits), TOL)
    with pytest.raises(ValueError):  # a position on a padded token has no row in the packed stack
        model.predict_tokens(ids, attention_mask=mask, positions=torch.tensor([5, 2 * S + LENS[2]], device=DEV))
    _set_unpad(model, kind, False)
    model.set_residual_dtype(torch.bfloat16)
    full = _full(model, kind, ids, mask)
    pred = model.predict_tokens(ids, attention_mask=mask, positions=pick)
    _check(pred, full, rows, 5, V, f"{kind} bf16 stream")


@pytest.mark.parametrize("kind", CLASSES)
def test_several_row_chunks_give_the_single_chunk_bits(kind, monkeypatch):
    """The 500 unmasked rows through cm3p_mlm_topk in one call and, with the workspace limit shrunk to 128 rows' worth, in chunks of
    128, 128, 128 and 116 rows: a row's result does not depend on the rows beside it, so the concatenation has the same bits."""
    from cm3p_amd import kernels as K
    from cm3p_amd import modeling_cm3p as M

    V, k = 300, 5
    model = _model(kind, V)
    ids, mask, _ = _batch(V)
    calls = []
    real = K.mlm_topk
    monkeypatch.setattr(K, "mlm_topk", lambda y, *a: calls.append(y.shape[0]) or real(y, *a))
    one = model.predict_tokens(ids, attention_mask=mask, k=k)
    assert calls == [sum(LENS)]
    del calls[:]
    Vp = -(-V // 64) * 64
    per_row = -(-Vp // 128) * (k + 1) * 8
    monkeypatch.setattr(M, "MLM_LOGIT_FREE_CHUNK_BYTES", 128 * per_row)
    assert M._mlm_topk_chunk_rows(Vp, k) == 128 and M._mlm_topk_chunk_rows(Vp, 8) == 128  # (never below 128 rows)
    many = model.predict_tokens(ids, attention_mask=mask, k=k)
    assert calls == [128, 128, 128, 116]
    for f in ("rows", "token_ids", "logits", "logprobs"):
        assert torch.equal(many[f], one[f]), f"{kind}: chunked and single-call predictions differ in {f}"
    _check(many, _full(model, kind, ids, mask), torch.nonzero(mask.flatten()).flatten(), k, V, f"{kind} four row chunks")


def test_refusals():
    V = 190
    ids, mask, pick = _batch(V)
    for kind in CLASSES:
        model = _build(kind, V)
        model.train()
        with pytest.raises(ValueError, match="training mode"):
            model.predict_tokens(ids, attention_mask=mask, positions=pick)
        assert model.training  # (the mode is the caller's)
        model.eval()
        for k in (0, 9):
            with pytest.raises(ValueError, match="1..8"):
                model.predict_tokens(ids, attention_mask=mask, positions=pick, k=k)
        with pytest.raises(ValueError):
            model.predict_tokens(ids, attention_mask=mask, positions=torch.ones(B, S - 1, device=DEV))
        with pytest.raises(ValueError):
            model.predict_tokens(ids, attention_mask=mask, positions=torch.tensor([7, 7], device=DEV))
        _tower(model, kind).cls_only_last_layer = True
        with pytest.raises(ValueError, match="cls_only_last_layer"):
            model.predict_tokens(ids, attention_mask=mask, positions=pick)
    bare = _build("model", V, decoder_head=False)
    with pytest.raises(ValueError, match="not configured with a decoder head"):
        bare.predict_tokens(ids, attention_mask=mask, positions=pick)


# ================================================================================================ accuracy
def _reference_counts(logits, labels):
    """ref:train.py:75-90 on (N, V) logits and (N,) labels."""
    m = labels != -100
    correct = (logits.argmax(-1)[m] == labels[m]).sum().item()
    total = m.sum().item()
    top5 = torch.topk(logits, k=min(5, logits.size(-1)), dim=-1).indices
    return total, correct, (top5[m] == labels[m].unsqueeze(-1)).any(dim=-1).sum().item()


@pytest.mark.parametrize("kind", CLASSES)
def test_accuracy_counts_equal_the_reference_arithmetic(kind):
    from cm3p_amd.modeling_cm3p import masked_lm_accuracy

    V = 300
    model = _model(kind, V)
    ids, mask, _ = _batch(V)
    full = _full(model, kind, ids, mask)
    # rows whose first six full-route logits are further apart than the ranking margin: both routes rank their first five alike
    top = full.topk(6, dim=1)
    margin = TOL * full.abs().amax(1)
    clear = ((top.values[:, :-1] - top.values[:, 1:]).amin(1) > margin) & mask.flatten().bool()
    rows = torch.nonzero(clear).flatten()
    print(f"{kind}: {rows.numel()} of {int(mask.sum())} rows have clear first six logits")
    assert rows.numel() >= 5  # (one label of each kind below)
    # labels by turns: the best id, the third, the fifth, the sixth (outside the first five), the least likely id
    order = full.argsort(1, descending=True)
    labels = torch.full((B * S,), -100, dtype=torch.int64, device=DEV)
    for j, rank in enumerate((0, 2, 4, 5, V - 1)):
        r = rows[j::5]
        labels[r] = order[r, rank]
    assert bool((((top.values[:, :-1] - top.values[:, 1:]).amin(1) > margin) | (labels == -100)).all())
    want = _reference_counts(full, labels)
    assert want[0] == rows.numel() and 0 < want[1] < want[2] < want[0]
    for k, positions in ((5, labels.view(B, S) != -100), (8, None), (1, labels.view(B, S) != -100)):
        pred = model.predict_tokens(ids, attention_mask=mask, positions=positions, k=k)
        got = masked_lm_accuracy(pred, labels.view(B, S))
        assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.int64 and v.shape == () for v in got.values())
        got = {n: int(v) for n, v in got.items()}
        print(f"{kind} k={k}: {got} (reference {want})")
        assert (got["total"], got["correct"]) == want[:2]
        assert got["top5_correct"] == (want[2] if k >= 5 else want[1])
    # the n labels of the listed rows themselves
    pred = model.predict_tokens(ids, attention_mask=mask, positions=rows, k=5)
    got = masked_lm_accuracy(pred, labels[rows])
    assert (int(got["total"]), int(got["correct"]), int(got["top5_correct"])) == want
    assert int(masked_lm_accuracy(pred, torch.full_like(labels, -100))["total"]) == 0


# ================================================================================================ memory
def test_the_topk_call_holds_no_logits_sized_tensor():
    """T = 2048, H = 64, V = Vp = 4096: the fp32 logits are 32 MiB.  Above the operands and its outputs cm3p_mlm_topk allocates its
    workspace, 9 / 64 of that at k = 8 (4.5 MiB), and the peak is held to less than half of the logits, which leaves room for the
    allocator's rounding; the GEMM + torch.topk route rises by at least the logits."""
    from cm3p_amd import kernels as K
    from cm3p_amd._lib import EPI_F32_BIAS

    T, H, V, k = 2048, 64, 4096, 8
    logits_bytes = T * V * 4
    g = torch.Generator().manual_seed(5)
    y = torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV)
    W = (torch.randn(V, H, generator=g) / 4).to(torch.bfloat16).to(DEV)
    b = torch.randn(V, generator=g).to(DEV)
    out_bytes = T * k * 8 + T * 4
    rise = {}
    for name in ("topk", "gemm + torch.topk"):
        for _ in range(2):  # (the first pass loads the kernels)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            if name == "topk":
                idx, val, lse = K.mlm_topk(y, W, b, V, k)
            else:
                logits = K.gemm(y, W, T, V, H, True, True, EPI_F32_BIAS, resid=b)
                ref = torch.topk(logits, k, dim=1)
                del logits
            torch.cuda.synchronize()
            rise[name] = torch.cuda.max_memory_allocated() - base
    print(f"peak rise: topk {rise['topk'] / 2 ** 20:.2f} MiB of which outputs {out_bytes / 2 ** 20:.2f} MiB, gemm + torch.topk "
          f"{rise['gemm + torch.topk'] / 2 ** 20:.2f} MiB (logits {logits_bytes / 2 ** 20:.0f} MiB)")
    assert rise["topk"] - out_bytes < logits_bytes // 2
    assert rise["gemm + torch.topk"] >= logits_bytes
    print(f"{100 * (idx.long() == ref.indices).float().mean().item():.2f} % of the ids equal torch.topk's")
