"""Head sizes 96 and 128 (csrc/attention_hd.hip, behind cm3p_attn_fwd_generic / cm3p_attn_bwd_generic): the kernels against float64
autograd of softmax(scale q k^T + mask) v at every seam a 32-, 64- or 128-row tile can have, their exact conditions (dead rows, padded
keys, window 0, guard rows, repeatability), a padded model-level invariant and a fixture made by the reference itself.

Bounds are the ones tests/test_kernels_gpu.py::test_generic_attention_matches_fp32_reference holds the head-64 MFMA kernels to: out
within 2e-3 + 2e-2 |ref|, lse atol 2e-3 / rtol 1e-4 on live rows, relative L2 error of each of dq / dk / dv below 1e-2.  A CPU emulation
of such a kernel (fp32 scores, P and dS rounded to bf16, bf16 outputs) on these very cases stays inside the forward bound on every
element and has gradient errors of 1.7e-3 .. 2.5e-3: the gradient bound leaves a factor of 4.

CM3P_HD_ERRORS_OUT=<file>: write the errors this run measured there (profiles/attention_hd_err.txt holds the first run's)."""
import copy
import functools
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import cases_hd

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
NH = 3
GUARD = 4          # sentinel rows before and after out / dqkv
GUARD_STAT = 64    # sentinel floats before and after lse / delta
SENTINEL = 777.0   # (exact in bf16)

# name -> (S, window, valid lengths per row | None: B = 2, no mask)
KCASES = {
    "global_pad": (200, -1, [200, 137]),
    "band_pad3": (333, 64, [333, 100, 1]),
    "band_pad": (257, 64, [257, 64]),
    "wide_band": (65, 200, [65, 1]),
    "window0": (129, 0, [129, 65]),
    **{f"global_S{S}": (S, -1, None) for S in (1, 31, 33, 63, 127, 255)},
    "band_nomask": (512, 64, None),
}
DEAD_ROWS = {"band_pad3": 437, "band_pad": 129}  # per head (the issue's count: checks the test's own mask)
GRID = [(D, c) for D in (96, 128) for c in KCASES]

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_HD_ERRORS_OUT")
    if not _SEEN or not path:
        return
    with open(path, "w") as f:
        json.dump(dict(measured=_SEEN, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f, indent=1, sort_keys=True)


def _bf(x):
    return x.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _reference(D, case):
    """float64 autograd of softmax(scale q k^T + mask) v, built as in test_generic_attention_matches_fp32_reference (CPU; once per case)."""
    S, window, lens = KCASES[case]
    g = torch.Generator().manual_seed(1000 * D + S + (window + 1) * 7)
    B = len(lens) if lens else 2
    scale = D ** -0.5
    qkv = _bf(torch.randn(B, S, 3, NH, D, generator=g) * 0.8)
    do = _bf(torch.randn(B * S, NH * D, generator=g) * 0.5)
    mask = (torch.arange(S)[None] < torch.tensor(lens)[:, None]) if lens is not None else None
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))  # (B, nh, S, D)
    sc = (q @ k.transpose(-1, -2)) * scale
    vis = torch.ones(B, 1, S, S, dtype=torch.bool)
    if mask is not None:
        vis = vis & mask[:, None, None, :]
    if window >= 0:
        idx = torch.arange(S)
        vis = vis & ((idx[:, None] - idx[None, :]).abs() <= window)[None, None]
    sc = sc.masked_fill(~vis, float("-inf"))
    dead = ~vis.any(dim=-1)  # (B, 1, S)
    p = torch.softmax(sc, dim=-1).masked_fill(dead[..., None], 0.0)
    o = (p @ v).transpose(1, 2).reshape(B * S, NH * D)
    o.backward(do.double())
    lse = torch.logsumexp(sc, dim=-1).detach()  # -inf on dead rows (the kernels store +inf there)
    return dict(B=B, S=S, window=window, scale=scale, qkv=qkv, do=do, mask=mask, out=o.detach(), lse=lse, grad=x.grad,
                dead=dead.expand(B, NH, S).clone())


def _guarded(rows, cols, dtype, guard):
    buf = torch.full((rows + 2 * guard, cols), SENTINEL, dtype=dtype, device=DEV)
    buf[guard:guard + rows] = float("nan")  # whatever the kernels leave unwritten fails every comparison
    return buf, buf[guard:guard + rows]


def _guards_untouched(buf, rows, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + rows:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _run(D, case):
    """One forward + backward through the C entry points on caller-owned, guard-wrapped buffers; a second one through the wrappers."""
    from cm3p_amd import _lib
    from cm3p_amd import kernels as K

    r = _reference(D, case)
    B, S, window, scale = r["B"], r["S"], r["window"], r["scale"]
    qkv, do = r["qkv"].to(DEV), r["do"].to(DEV)
    km = r["mask"].to(torch.uint8).to(DEV) if r["mask"] is not None else None
    out_b, out = _guarded(B * S, NH * D, torch.bfloat16, GUARD)
    dq_b, dqkv = _guarded(B * S, 3 * NH * D, torch.bfloat16, GUARD)
    lse_b, lse = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    dl_b, delta = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_fwd_generic", ptr(qkv), ptr(out), ptr(lse), ptr(km), B, S, NH, D, window, scale, st())
    _lib.call("cm3p_attn_bwd_generic", ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dqkv), ptr(km), B, S, NH, D, window, scale, st())
    torch.cuda.synchronize()
    guards = dict(out=_guards_untouched(out_b, B * S, GUARD), dqkv=_guards_untouched(dq_b, B * S, GUARD),
                  lse=_guards_untouched(lse_b, B * NH * S, GUARD_STAT), delta=_guards_untouched(dl_b, B * NH * S, GUARD_STAT))
    out2, lse2 = K.attn_fwd_generic(qkv, km, B, S, NH, D, window, scale)
    dqkv2 = K.attn_bwd_generic(qkv, out2, do, lse2, km, B, S, NH, D, window, scale)
    lse_v = lse.view(B, NH, S)
    same = dict(out=torch.equal(out2, out), lse=torch.equal(lse2, lse_v), dqkv=torch.equal(dqkv2.view(B * S, -1), dqkv))
    return dict(out=out.cpu(), lse=lse_v.cpu(), dqkv=dqkv.view(B, S, 3, NH, D).cpu(), guards=guards, same=same)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("D,case", GRID)
def test_hd_attention_matches_float64(D, case):
    r, got = _reference(D, case), _run(D, case)
    B, S = r["B"], r["S"]
    seen = _SEEN.setdefault(f"D{D} {case}", {})
    out, want = got["out"].double(), r["out"]
    err = (out - want).abs()
    seen["out_max_abs"] = err.max().item()
    seen["out_worst_over_bound"] = (err / (2e-3 + 2e-2 * want.abs())).max().item()
    live = ~r["dead"]
    lse_err = (got["lse"].double()[live] - r["lse"][live]).abs()
    seen["lse_max_abs"] = lse_err.max().item() if lse_err.numel() else 0.0
    grads = {}
    for i, nm in enumerate("qkv"):
        g, w = got["dqkv"][:, :, i], r["grad"][:, :, i]
        grads[nm] = (g, w)
        if w.abs().max().item() > 0.0:
            seen[f"d{nm}_rel_l2"] = _rel(g, w)
        else:  # window 0 and S = 1: one visible key per query, dq and dk are exactly zero in the reference - no norm to be relative to
            seen[f"d{nm}_max_abs"] = g.float().abs().max().item()
    print(f"D={D} {case}: " + "  ".join(f"{k}={v:.3e}" for k, v in seen.items()))

    assert bool((err <= 2e-3 + 2e-2 * want.abs()).all()), f"forward: worst error / bound = {seen['out_worst_over_bound']:.3f}"
    assert torch.allclose(got["lse"].double()[live], r["lse"][live], atol=2e-3, rtol=1e-4)
    for nm, (g, w) in grads.items():
        assert torch.isfinite(g.float()).all(), f"d{nm} is not finite"
        if f"d{nm}_max_abs" in seen:
            # exactly zero in the reference (one visible key: dP = delta).  10 x a worst-case fp32 dot-product bound of ~1e-4 for these magnitudes
            assert nm in "qk" and (case == "window0" or S == 1) and seen[f"d{nm}_max_abs"] <= 1e-3
        else:
            assert seen[f"d{nm}_rel_l2"] < 1e-2, f"d{nm} relative L2 error {seen[f'd{nm}_rel_l2']:.3e}"


@pytest.mark.parametrize("D,case", GRID)
def test_hd_attention_exact_conditions(D, case):
    """Dead rows are exact zeros with lse = +inf, padded keys get exactly zero dk / dv, nothing outside the tensors is written, and a
    second call gives the same bits."""
    r, got = _reference(D, case), _run(D, case)
    B, S, dead = r["B"], r["S"], r["dead"]
    if case in DEAD_ROWS:
        assert int(dead[:, 0].sum()) == DEAD_ROWS[case]
    if dead.any():
        lse_dead = got["lse"][dead]
        assert torch.isinf(lse_dead).all() and (lse_dead > 0).all()
        assert got["out"].view(B, S, NH, D).permute(0, 2, 1, 3)[dead].float().abs().max().item() == 0.0
    assert torch.isfinite(got["lse"][~dead]).all()
    if r["mask"] is not None:
        assert got["dqkv"][:, :, 1:].float()[~r["mask"]].abs().max().item() == 0.0
    assert got["guards"] == dict(out=True, dqkv=True, lse=True, delta=True)
    assert got["same"] == dict(out=True, lse=True, dqkv=True)


@pytest.mark.parametrize("D", [96, 128])
def test_hd_window0_copies_v_and_dout(D):
    """window 0: every live query sees its own key only, so out is the v row and dv is the dO row, bit for bit."""
    r, got = _reference(D, "window0"), _run(D, "window0")
    B, S, mask = r["B"], r["S"], r["mask"]
    out = got["out"].view(B, S, NH, D)
    assert torch.equal(out[mask], r["qkv"][:, :, 2][mask])
    assert torch.equal(got["dqkv"][:, :, 2][mask], r["do"].view(B, S, NH, D)[mask])


# ---------------------------------------------------------------------------------------------------------------- model level
def _tower_cfg(D, p_attn=0.0):
    from cm3p_amd import CM3PConfig

    bc = copy.deepcopy(CM3PConfig(**cases_hd.CASE["cfg"]).beatmap_config)  # 2 heads, layer 0 global, layer 1 sliding (|q - k| <= 64)
    bc.hidden_size = 2 * D
    bc.attention_dropout = p_attn
    return bc


def _encoder(cfg):
    from cm3p_amd.encoder import CM3PEncoder

    torch.manual_seed(0)
    enc = CM3PEncoder(cfg)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            p.copy_(torch.randn_like(p) * (0.02 if p.dim() == 2 else 0.1) + (1.0 if p.dim() == 1 else 0.0))
    return enc.to(DEV).train()


def _batch(H, B=3, S=200, short=100, vocab=190):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, vocab, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[-1, short:] = 0
    ids[-1, short:] = 0
    w = torch.randn(B, S, H, generator=g)
    return ids.to(DEV), mask.to(DEV), w.to(DEV)


def _step(enc, ids, mask, w, **kw):
    enc.zero_grad(set_to_none=True)
    y = enc(input_ids=ids, attention_mask=mask, **kw)
    loss = (y * w)[mask.bool()].sum()
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in enc.named_parameters()}, y.detach()


@pytest.mark.parametrize("D", [96, 128])
def test_hd_tower_checkpointing_and_unpad_give_the_same_bits(D):
    cfg = _tower_cfg(D)
    assert [cfg.is_global_layer(i) for i in range(cfg.num_hidden_layers)] == [True, False]
    ids, mask, w = _batch(cfg.hidden_size)
    a, b = _encoder(cfg), _encoder(cfg)
    b.gradient_checkpointing = True
    la, ga, ya = _step(a, ids, mask, w)
    assert torch.isfinite(la) and all(torch.isfinite(g).all() for g in ga.values())
    lb, gb, _ = _step(b, ids, mask, w)
    assert torch.equal(la, lb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    lc, gc, yc = _step(a, ids, mask, w, unpad=True)  # falls back to padded execution at these head sizes
    assert torch.equal(la, lc) and torch.equal(ya, yc)
    for n in ga:
        assert torch.equal(ga[n], gc[n]), n


@pytest.mark.parametrize("D", [96, 128])
def test_hd_tower_refuses_attention_dropout_in_training_only(D):
    cfg = _tower_cfg(D, p_attn=0.1)
    ids, mask, _ = _batch(cfg.hidden_size)
    enc = _encoder(cfg)
    with pytest.raises(NotImplementedError, match="head_dim"):
        enc(input_ids=ids, attention_mask=mask)
    enc.eval()
    with torch.no_grad():
        y = enc(input_ids=ids, attention_mask=mask)
    ref = _encoder(_tower_cfg(D)).eval()
    with torch.no_grad():
        assert torch.equal(y, ref(input_ids=ids, attention_mask=mask))  # eval mode: the dropout-free launches


# ---------------------------------------------------------------------------------------------------------------- reference-made fixture
# the class bounds of tests/test_model_gpu.py (FIX_TOL), restated: bf16 GEMM / attention operands with fp32 accumulation against the
# all-fp32 reference on O(1)-scale weights
FIX_TOL = dict(loss=3e-2, logits=3e-2, embeds=2e-2, pooled=2e-2, grad=6e-2)


def _fixture_model():
    from cm3p_amd import CM3PConfig, CM3PModel

    model = CM3PModel(CM3PConfig(**cases_hd.CASE["cfg"]))
    cases_hd.draw_weights(model)
    return model.to(DEV).train()


def test_hd_model_matches_the_reference_fixture():
    """tests/golden/hd_mean_pad.safetensors (make_golden_hd.py: the reference on the CPU in fp32): beatmap tower at head_dim 128 with a
    global and a sliding layer, metadata tower at head_dim 96, padded rows of S = 203."""
    blob = load_file(os.path.join(GOLD, f"{cases_hd.NAME}.safetensors"))
    inputs = {k[3:]: v.to(DEV) for k, v in blob.items() if k.startswith("in.")}
    for k, v in cases_hd.inputs().items():
        assert torch.equal(v, blob[f"in.{k}"]), k
    model = _fixture_model()
    assert model.config.beatmap_config.hidden_size // model.config.beatmap_config.num_attention_heads == 128
    assert model.config.metadata_config.hidden_size // model.config.metadata_config.num_attention_heads == 96
    out = model(**inputs)
    seen = _SEEN.setdefault("fixture hd_mean_pad", {})

    def fix(key, value, bound):
        seen[key] = float(value)
        assert value <= FIX_TOL[bound], f"{key} = {value:.3e} > {FIX_TOL[bound]:.1e}"

    fix("loss", abs(out.loss.item() - blob["loss"].item()), "loss")
    fix("logits", _rel(out.logits_per_metadata.cpu(), blob["logits_per_metadata"]), "logits")
    fix("metadata_embeds", _rel(out.metadata_embeds.cpu(), blob["metadata_embeds"]), "embeds")
    fix("beatmap_embeds", _rel(out.beatmap_embeds.cpu(), blob["beatmap_embeds"]), "embeds")
    fix("beatmap_pooled", _rel(out.beatmap_model_output.pooler_output.cpu(), blob["beatmap_pooler_output"]), "pooled")
    fix("metadata_pooled", _rel(out.metadata_model_output.pooler_output.cpu(), blob["metadata_pooler_output"]), "pooled")
    out.loss.backward()

    from make_golden_bf16_train import stored_slice

    params = dict(model.named_parameters())
    cpu_inputs = {k[3:]: v for k, v in blob.items() if k.startswith("in.")}
    checked = 0
    for k, v in blob.items():
        if not k.startswith("grad."):
            continue
        name = k[5:].split("[")[0]
        g = params[name].grad
        assert g is not None, k
        suffix, cut = stored_slice(name, params[name], cpu_inputs)
        assert name + suffix == k[5:]
        g = cut(g.float().cpu())
        if v.norm() < 1e-8:
            assert g.norm().item() < 1e-5, k
        else:
            fix(k, _rel(g, v), "grad")
        checked += 1
    assert checked >= 20
    print("fixture hd_mean_pad: " + "  ".join(f"{k}={v:.3e}" for k, v in seen.items()))

    # unpad_inputs = True falls back to padded execution at these head sizes: the same bits
    model.unpad_inputs = True
    with torch.no_grad():
        again = model(**inputs)
    assert torch.equal(again.loss, out.loss.detach()) and torch.equal(again.logits_per_metadata, out.logits_per_metadata.detach())
