"""Pooling of caller-packed rows (`cu_seqlens` layout), opt-in through `pool_unpadded`.

Kernel level (cm3p_pool_fwd / cm3p_pool_bwd with cu_seqlens, reached through cm3p_amd.kernels):
  1. packed equals padded, bit for bit: pooled, count and the gradient of every valid row, fp32 and bf16, mean and CLS;
  2. the packed mean against float64 segment means, inside the bound tests/row_kernel_refs.py gives the padded kernel;
  3. extents: nothing is written past `total`, rows at and past cu[Bn] are zeros;
  4. the autograd node on the y[:total] slice of a row-aligned tensor.
Model level (fixtures that exist: d64_mean_pad, d64_mlm):
  5. a mean-pooled contrastive step on caller-packed rows against the padded step and the fixture's gradients;
  6. the metadata tower alone, mean and CLS;
  7. the MLM head on a mean-pooled configuration, and one step on the bf16 residual stream;
  8. the switch is off by default (the reference's NotImplementedError, before any launch).
"""
import copy
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import row_kernel_refs as R
from cases import CASES
from row_kernel_refs import check, gen

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
BF = torch.bfloat16

LENS = [1, 127, 128, 129, 300]  # below, at and above one 128-row chunk; three chunks with a ragged last one; total 685 = 10 * 64 + 45
TOTAL = sum(LENS)
S_PAD = max(LENS)


@pytest.fixture(scope="module")
def K():
    from cm3p_amd import kernels

    return kernels


def _cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)


_batches: dict = {}


def _batch(H, dtype):
    """-> (packed rows [685, H], the same rows right-padded to [5, 300, H] with finite values behind them, int64 mask, dpooled),
    built once per (H, dtype) and shared by the tests below (nothing writes to them)."""
    if (H, dtype) not in _batches:
        g = gen("packed-pool", H)
        rows = (torch.randn(TOTAL, H, generator=g) + 0.25).to(dtype)
        padded = torch.randn(len(LENS), S_PAD, H, generator=g).to(dtype)  # (finite rows behind the valid ones: h * 0.0f adds nothing)
        mask = torch.zeros(len(LENS), S_PAD, dtype=torch.int64)
        at = 0
        for b, n in enumerate(LENS):
            padded[b, :n] = rows[at:at + n]
            mask[b, :n] = 1
            at += n
        dp = torch.randn(len(LENS), H, generator=g)
        _batches[(H, dtype)] = (rows, padded, mask, dp)
    return _batches[(H, dtype)]


# ------------------------------------------------------------------------------------------------ 1. packed == padded
@pytest.mark.parametrize("cls", [False, True], ids=["mean", "cls"])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [4, 260, 768])
def test_packed_pooling_has_the_bits_of_the_padded_kernels(K, H, dtype, cls):
    rows, padded, mask, dp = _batch(H, dtype)
    Bn = len(LENS)
    cu = _cu(LENS).to(DEV)
    md, dpd = mask.to(DEV), dp.to(DEV)
    want, want_count = K.pool_fwd(padded.to(DEV), md, Bn, S_PAD, cls)
    want_dh = {dd: K.pool_bwd(dpd, md, want_count, Bn, S_PAD, cls, dtype=dd).view(Bn, S_PAD, H)[md.bool()] for dd in (torch.float32, BF)}
    for max_s in (300, 384):  # (max_seqlen sizes the workspace; the result does not depend on it)
        what = f"H {H} {dtype} cls {cls} max_seqlen {max_s}"
        got, count = K.pool_fwd(rows.to(DEV), None, Bn, max_s, cls, cu=cu, total=TOTAL)
        assert got.dtype == torch.float32 and got.shape == (Bn, H)
        assert torch.equal(got, want), what
        if not cls:  # (CLS pooling writes no count, in either layout)
            assert torch.equal(count, want_count) and count.tolist() == [float(n) for n in LENS], what
        for dd in (torch.float32, BF):
            dh = K.pool_bwd(dpd, None, count, Bn, max_s, cls, dtype=dd, cu=cu, total=TOTAL)
            assert dh.dtype == dd and dh.shape == (TOTAL, H)
            assert torch.equal(dh, want_dh[dd]), what + f" backward {dd}"
            if cls:  # row cu[b] holds dpooled[b], every other row is zero
                first = cu[:-1].long()
                rest = torch.ones(TOTAL, dtype=torch.bool, device=DEV)
                rest[first] = False
                assert torch.equal(dh[first], dpd.to(dd)) and (dh[rest] == 0).all(), what


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [4, 260, 768])
def test_packed_mean_against_float64_segment_means(K, H, dtype):
    """The reference is the float64 mean of every sequence's own rows (no padded tensor involved); the bound is R.pool_ref's for a
    padded batch of these rows: the packed kernels round where the padded ones do."""
    rows, padded, mask, dp = _batch(H, dtype)
    cu = _cu(LENS)
    _, cnt, bound = R.pool_ref(padded.double(), mask, False)
    ref = torch.stack([rows[cu[b]:cu[b + 1]].double().mean(0) for b in range(len(LENS))])
    got, count = K.pool_fwd(rows.to(DEV), None, len(LENS), S_PAD, False, cu=cu.to(DEV), total=TOTAL)
    check(got, ref, bound, f"packed mean H {H} {dtype}")
    assert torch.equal(count.cpu().double(), cnt)
    first, _, _ = R.pool_ref(padded.double(), mask, True)
    got, _ = K.pool_fwd(rows.to(DEV), None, len(LENS), S_PAD, True, cu=cu.to(DEV), total=TOTAL)
    check(got, first, 0.0, f"packed cls H {H} {dtype}")
    dh = K.pool_bwd(dp.to(DEV), None, None, len(LENS), S_PAD, False, cu=cu.to(DEV), total=TOTAL)
    ref, bnd = R.pool_bwd_ref(dp.double(), mask, cnt, S_PAD, False)
    check(dh, ref[mask.bool()], bnd[mask.bool()], f"packed mean backward H {H}")


# ------------------------------------------------------------------------------------------------ 3. extents
@pytest.mark.parametrize("cls", [False, True], ids=["mean", "cls"])
@pytest.mark.parametrize("dd", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [4, 260])
def test_backward_writes_rows_below_total_only_and_zeros_past_the_last_sequence(K, H, dd, cls):
    _, _, _, dp = _batch(H, torch.float32)
    Bn = len(LENS)
    dh = torch.full((TOTAL + 7, H), float("nan"), dtype=dd, device=DEV)
    K.pool_bwd(dp.to(DEV), None, None, Bn, S_PAD, cls, cu=_cu(LENS).to(DEV), total=TOTAL, out=dh)
    assert torch.isfinite(dh[:TOTAL]).all() and torch.isnan(dh[TOTAL:]).all()
    full = dh[:TOTAL].clone()
    shorter = LENS[:-1] + [LENS[-1] - 3]  # cu ends three rows before total: alignment rows behind the packed ones
    dh.fill_(float("nan"))
    K.pool_bwd(dp.to(DEV), None, None, Bn, S_PAD, cls, cu=_cu(shorter).to(DEV), total=TOTAL, out=dh)
    assert torch.isnan(dh[TOTAL:]).all() and torch.isfinite(dh[:TOTAL]).all()
    assert (dh[TOTAL - 3:TOTAL] == 0).all()
    assert torch.equal(dh[:TOTAL - LENS[-1]], full[:TOTAL - LENS[-1]])  # the other sequences do not notice
    if not cls:
        assert (dh[TOTAL - LENS[-1]:TOTAL - 3] != 0).any()


def test_forward_reads_no_row_at_or_past_total(K):
    """Rows behind `total` hold NaN: a packed forward that read one of them would return it."""
    rows, padded, mask, _ = _batch(260, torch.float32)
    h = torch.cat((rows, torch.full((7, 260), float("nan")))).to(DEV)
    want, _ = K.pool_fwd(padded.to(DEV), mask.to(DEV), len(LENS), S_PAD, False)
    got, _ = K.pool_fwd(h, None, len(LENS), S_PAD, False, cu=_cu(LENS).to(DEV), total=TOTAL)
    assert torch.equal(got, want)
    # an empty sequence in the middle pools to zero (count 0), as an all-zero mask row does, and gets no gradient row
    lens = [5, 0, 130]
    h = rows[:135].to(DEV)
    got, count = K.pool_fwd(h, None, 3, 130, False, cu=_cu(lens).to(DEV), total=135)
    assert count.tolist() == [5.0, 0.0, 130.0] and (got[1] == 0).all() and torch.isfinite(got).all()
    dp = torch.randn(3, 260, generator=gen("packed-pool", "empty"))
    dh = K.pool_bwd(dp.to(DEV), None, None, 3, 130, False, cu=_cu(lens).to(DEV), total=135)
    scale = torch.tensor(1.0) / torch.tensor([5.0, 1.0, 130.0])  # fp32 divisions, as the kernel's 1 / max(count, 1e-9)
    want = (dp * scale[:, None]).repeat_interleave(torch.tensor(lens), dim=0)  # (the empty sequence owns no row)
    assert torch.equal(dh.cpu(), want)


# ------------------------------------------------------------------------------------------------ 4. the autograd node
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("cls", [False, True], ids=["mean", "cls"])
def test_autograd_node_on_the_slice_of_a_row_aligned_tensor(K, cls, dtype):
    from cm3p_amd.modeling_cm3p import _PoolPackedFn

    H = 260
    rows, _, _, dp = _batch(H, dtype)
    n_rows = (TOTAL + 63) // 64 * 64
    assert n_rows == 704
    base = torch.cat((rows, torch.full((n_rows - TOTAL, H), float("nan"), dtype=dtype))).to(DEV).requires_grad_(True)
    y = base[:TOTAL]
    assert y.is_contiguous() and y.data_ptr() == base.data_ptr()  # (the slice _forward_prepacked returns: pooled in place, no copy)
    cu = _cu(LENS).to(DEV)
    pooled = _PoolPackedFn.apply(y, cu, S_PAD, cls)
    want, _ = K.pool_fwd(rows.to(DEV), None, len(LENS), S_PAD, cls, cu=cu, total=TOTAL)
    assert pooled.dtype == torch.float32 and torch.equal(pooled, want)
    pooled.backward(dp.to(DEV))
    assert base.grad.dtype == dtype and base.grad.shape == (n_rows, H)
    assert torch.equal(base.grad[:TOTAL], K.pool_bwd(dp.to(DEV), None, None, len(LENS), S_PAD, cls, dtype=dtype, cu=cu, total=TOTAL))
    assert (base.grad[TOTAL:] == 0).all()
    # a description that leaves the rows is refused on the host: the kernels index h with it
    with pytest.raises(ValueError, match="cu_seqlens"):
        _PoolPackedFn.apply(y, _cu(LENS[:-1] + [LENS[-1] + 1]).to(DEV), S_PAD + 1, cls)
    with pytest.raises(ValueError, match="max_seqlen"):
        _PoolPackedFn.apply(y, cu, S_PAD - 1, cls)


# ================================================================================================ model level
def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _build(name, cfg=None):
    from cm3p_amd import CM3PConfig, CM3PModel

    model = CM3PModel(CM3PConfig(**(cfg or CASES[name]["cfg"])))
    sd = load_file(os.path.join(GOLD, "weights_d64.safetensors"))
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    sd.update({k[2:]: v for k, v in blob.items() if k.startswith("w.")})  # parameters only this case has (MLM head)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train()


def _inputs(blob):
    return {k[3:]: v.to(DEV) for k, v in blob.items() if k.startswith("in.")}


def _unpad_like_the_reference(ids, mask):
    """_unpad_cm3p_input (ref:cm3p/modeling_cm3p.py:88-104) restated: -> unpadded ids, indices, cu_seqlens, max_seqlen."""
    lens = mask.sum(dim=-1, dtype=torch.int32)
    indices = torch.nonzero(mask.flatten(), as_tuple=False).flatten()
    cu = torch.nn.functional.pad(torch.cumsum(lens, dim=0, dtype=torch.int32), (1, 0))
    return ids.flatten()[indices], indices, cu, int(lens.max())


# ------------------------------------------------------------------------------------------------ 5. contrastive step
def test_mean_pooled_contrastive_step_on_caller_packed_rows():
    """d64_mean_pad, both towers mean-pooled.  Against the padded step of the same model: 5e-3 relative on the embeddings and 2e-3
    absolute on the loss (the bounds of the packed-against-padded test of tests/test_model_gpu.py); the fixture's parameter
    gradients within 6e-2, at least 8 of them (the bounds of the caller-unpadded CLS test there).  The beatmap tower's pooled output
    is, bit for bit, the one of `unpad_inputs = True` on the padded batch: the same rows through the same kernels, summed in the
    same order."""
    name = "d64_mean_pad"
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    inp = _inputs(blob)
    ids_u, indices, cu, max_s = _unpad_like_the_reference(inp["input_ids"], inp["attention_mask"])
    B, S = inp["input_ids"].shape
    extra = {k: v for k, v in inp.items() if k not in ("input_ids", "attention_mask")}
    model = _build(name)
    with torch.no_grad():
        want = model(**inp)
    model.pool_unpadded = True
    out = model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, batch_size=B, seq_len=S, **extra)
    bo = out.beatmap_model_output
    H = CASES[name]["cfg"]["beatmap_config"]["hidden_size"]
    assert bo.last_hidden_state.shape == (ids_u.numel(), H) and bo.pooler_output.shape == (B, H) and bo.pooler_output.dtype == torch.float32
    errs = dict(beatmap_embeds=_rel(out.beatmap_embeds, want.beatmap_embeds), metadata_embeds=_rel(out.metadata_embeds, want.metadata_embeds),
                loss=abs(out.loss.item() - want.loss.item()))
    print(errs)
    assert errs["beatmap_embeds"] <= 5e-3 and errs["metadata_embeds"] <= 5e-3 and errs["loss"] <= 2e-3, errs
    assert _rel(out.logits_per_metadata, want.logits_per_metadata) <= 3e-2
    out.loss.backward()
    params = dict(model.named_parameters())
    checked = 0
    for k, v in blob.items():
        if k.startswith("grad.") and v.norm() >= 1e-8:
            assert _rel(params[k[5:]].grad, v) <= 6e-2, k
            checked += 1
    assert checked >= 8
    other = _build(name)
    other.unpad_inputs = True
    with torch.no_grad():
        oo = other(**inp)
    assert torch.equal(bo.pooler_output.detach(), oo.beatmap_model_output.pooler_output)


# ------------------------------------------------------------------------------------------------ 6. the metadata tower alone
@pytest.mark.parametrize("cls", [False, True], ids=["mean", "cls"])
def test_metadata_tower_pools_caller_packed_rows(cls):
    name = "d64_mean_pad"
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    inp = _inputs(blob)
    cfg = copy.deepcopy(CASES[name]["cfg"])
    cfg["metadata_config"]["cls_embed"] = cls  # (no parameter depends on it: the fixture's weights load either way)
    tower = _build(name, cfg).metadata_model
    assert bool(tower.config.cls_embed) == cls
    ids, mask = inp["metadata_ids"], inp["metadata_attention_mask"]
    ids_u, indices, cu, max_s = _unpad_like_the_reference(ids, mask)
    with torch.no_grad():
        want = tower(input_ids=ids, attention_mask=mask).pooler_output
        with pytest.raises(NotImplementedError, match="Pooling with unpadded input"):
            tower(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s)
        tower.pool_unpadded = True
        out = tower(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s)
    Bn, H = ids.shape[0], tower.config.hidden_size
    assert out.last_hidden_state.shape == (ids_u.numel(), H)
    assert out.pooler_output.shape == (Bn, H) and out.pooler_output.dtype == torch.float32  # 2-D: a packed batch has no variation axis
    err = _rel(out.pooler_output, want)
    print(f"metadata tower cls {cls}: {err:.3e}")
    assert err <= 5e-3
    # the stand-alone class holds the same tower: its switch is the tower's
    from cm3p_amd.modeling_cm3p import CM3PMetadataModel

    alone = CM3PMetadataModel(tower.config).to(DEV)
    alone.metadata_model.load_state_dict(tower.state_dict())
    alone.metadata_model.pool_unpadded = True
    with torch.no_grad():
        again = alone(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s)
    assert torch.equal(again.pooler_output, out.pooler_output)


# ------------------------------------------------------------------------------------------------ 7. MLM head, bf16 stream
def test_mlm_head_on_a_mean_pooled_configuration_with_caller_packed_rows():
    """d64_mlm as the fixture configures it (mean pooling in the beatmap tower; tests/test_model_gpu.py has to switch it to CLS):
    loss and re-padded logits against the padded run of the same model, 2e-3 as there."""
    from cm3p_amd import CM3PConfig, CM3PModel

    blob = load_file(os.path.join(GOLD, "d64_mlm.safetensors"))
    inp = _inputs(blob)
    cfg = CASES["d64_mlm"]["cfg"]
    assert not cfg["beatmap_config"]["cls_embed"]
    torch.manual_seed(0)
    model = CM3PModel(CM3PConfig(**cfg)).to(DEV)
    model.pool_unpadded = True
    ids_u, indices, cu, max_s = _unpad_like_the_reference(inp["input_ids"], inp["attention_mask"])
    B, S = inp["input_ids"].shape
    extra = {k: v for k, v in inp.items() if k not in ("input_ids", "attention_mask", "labels")}
    with torch.no_grad():
        want = model(**inp)
    mask = inp["attention_mask"].bool()
    labels_u = inp["labels"].flatten()[indices]
    out = model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, batch_size=B, seq_len=S, labels=labels_u, **extra)
    assert out.logits.shape == want.logits.shape
    errs = dict(loss=abs(out.loss.item() - want.loss.item()), logits=_rel(out.logits[mask], want.logits[mask]))
    print(errs)
    assert errs["loss"] <= 2e-3 and errs["logits"] <= 2e-3, errs
    assert out.logits[~mask].abs().max().item() == 0.0
    out.loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(torch.isfinite(g).all() for g in grads)
    with pytest.raises(NotImplementedError, match="output_attentions"):
        model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, batch_size=B, seq_len=S, output_attentions=True, **extra)


def test_bf16_stream_training_step_on_caller_packed_rows_with_mean_pooling():
    """set_residual_dtype(bf16, training=True) with pool_unpadded: bf16 rows, fp32 pooled output, finite gradients (the pooling
    gradient enters the stack in bf16), and the loss as close to the reference's fp32 loss as the bf16 stream's padded step is held:
    the bound of tests/test_bf16_train_gpu.py for d64_mlm - 1.25 x the reference's own bf16 loss error, and 3 x the error recorded in
    tests/golden/fixture_errors_bf16_train.json (floored at a tenth of the first)."""
    name = "d64_mlm"
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    inp = _inputs(blob)
    fix = load_file(os.path.join(GOLD, "d64_bf16_train.safetensors"))
    rec = json.load(open(os.path.join(GOLD, "fixture_errors_bf16_train.json")))
    l32, l16 = fix[f"{name}.loss_f32"].item(), fix[f"{name}.loss_bf16"].float().item()
    tol = rec["factor"] * abs(l16 - l32) / abs(l32)
    tol = min(tol, max(3.0 * rec["measured"][name]["loss"], 0.1 * tol))
    model = _build(name).set_residual_dtype(BF, training=True)
    model.pool_unpadded = True
    ids_u, indices, cu, max_s = _unpad_like_the_reference(inp["input_ids"], inp["attention_mask"])
    B, S = inp["input_ids"].shape
    extra = {k: v for k, v in inp.items() if k not in ("input_ids", "attention_mask", "labels")}
    out = model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, batch_size=B, seq_len=S,
                labels=inp["labels"].flatten()[indices], return_loss=True, **extra)
    bo = out.beatmap_model_output
    assert bo.last_hidden_state.dtype == BF and bo.last_hidden_state.shape[0] == ids_u.numel()
    assert bo.pooler_output.dtype == torch.float32 and out.loss.dtype == torch.float32
    err = abs(out.loss.item() - l32) / abs(l32)
    print(f"bf16 stream, packed rows: loss {out.loss.item():.6f} reference fp32 {l32:.6f} rel {err:.3e} bound {tol:.3e}")
    out.loss.backward()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert len(grads) > 20 and all(torch.isfinite(g).all() and g.dtype == torch.float32 for g in grads.values())
    assert err <= tol, (err, tol)
    # forward-only calls on the bf16 stream pool packed rows as well
    fwd = _build(name).eval().set_residual_dtype(BF)
    fwd.pool_unpadded = True
    with torch.no_grad():
        fo = fwd(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, batch_size=B, seq_len=S, **extra)
    assert fo.beatmap_model_output.last_hidden_state.dtype == BF and fo.beatmap_model_output.pooler_output.dtype == torch.float32
    assert torch.isfinite(fo.beatmap_embeds).all()


# ------------------------------------------------------------------------------------------------ 8. default off
def test_switch_off_keeps_the_reference_error_and_launches_nothing(monkeypatch):
    from cm3p_amd import _lib
    from cm3p_amd.modeling_cm3p import CM3PBeatmapModelWithProjection, CM3PForBeatmapClassification

    name = "d64_mean_pad"
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    inp = _inputs(blob)
    ids_u, indices, cu, max_s = _unpad_like_the_reference(inp["input_ids"], inp["attention_mask"])
    mids_u, mind, mcu, mmax = _unpad_like_the_reference(inp["metadata_ids"], inp["metadata_attention_mask"])
    model = _build(name)
    torch.cuda.synchronize()
    launched = []
    real = _lib._launch
    monkeypatch.setattr(_lib, "_launch", lambda n, a: (launched.append(n), real(n, a))[1])
    with pytest.raises(NotImplementedError, match="Pooling with unpadded input"):
        model.beatmap_model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s)
    with pytest.raises(NotImplementedError, match="Pooling with unpadded input"):
        model.metadata_model(input_ids=mids_u, indices=mind, cu_seqlens=mcu, max_seqlen=mmax)
    assert not launched
    with pytest.raises(NotImplementedError, match="Pooling with unpadded input"):
        model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, metadata_ids=inp["metadata_ids"],
              metadata_attention_mask=inp["metadata_attention_mask"])
    monkeypatch.setattr(_lib, "_launch", real)
    model.pool_unpadded = True
    with pytest.raises(NotImplementedError, match="output_attentions"):
        model.beatmap_model(input_ids=ids_u, indices=indices, cu_seqlens=cu, max_seqlen=max_s, output_attentions=True)
    with pytest.raises(NotImplementedError, match="output_attentions"):
        model.metadata_model(input_ids=mids_u, indices=mind, cu_seqlens=mcu, max_seqlen=mmax, output_attentions=True)
    # the classes that hold a beatmap tower take padded batches; the switch on their tower changes nothing there
    bc = model.beatmap_model.config
    for klass in (CM3PBeatmapModelWithProjection, CM3PForBeatmapClassification):
        torch.manual_seed(0)
        m = klass(bc).to(DEV).eval()
        with torch.no_grad():
            a = m(input_ids=inp["input_ids"], attention_mask=inp["attention_mask"])
            m.beatmap_model.pool_unpadded = True
            b = m(input_ids=inp["input_ids"], attention_mask=inp["attention_mask"])
        key = "beatmap_embeds" if klass is CM3PBeatmapModelWithProjection else "logits"
        assert torch.equal(a[key], b[key])
