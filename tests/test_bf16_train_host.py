"""The bf16 residual stream of training steps on the host (no GPU): the switch (CM3PEncoder.train_residual_dtype,
CM3PPreTrainedModel.set_residual_dtype(dtype, training=True)), the rule that picks the stream, ABI 19, and - as
tests/test_row_kernel_bounds_host.py does for the fp32 kernels - that the per-element bounds tests/test_bf16_train_gpu.py holds the new
LayerNorm backward form to are attainable (a torch fp32 walk of the kernel's path with ONE rounding of dres + LN'(dy) passes) and
sharp (the two-rounding form of a bf16 torch model fails; so does a dw accumulated in bf16)."""
import os
import re

import pytest
import torch

import row_kernel_refs as R
from cases import CASES
from row_kernel_refs import FTZ, U, check, gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cm3p_hip.h")
BF = torch.bfloat16


def _models():
    from cm3p_amd import CM3PConfig, CM3PModel
    from cm3p_amd.modeling_cm3p import (CM3PBeatmapModelWithProjection, CM3PForBeatmapClassification, CM3PForMaskedLM,
                                        CM3PMetadataModelWithProjection)

    cfg = CM3PConfig(**CASES["d64_mean_pad"]["cfg"])
    return [CM3PModel(cfg), CM3PForMaskedLM(cfg.beatmap_config), CM3PForBeatmapClassification(cfg.beatmap_config),
            CM3PBeatmapModelWithProjection(cfg.beatmap_config), CM3PMetadataModelWithProjection(cfg.metadata_config)]


def _encoders(model):
    from cm3p_amd.encoder import CM3PEncoder

    return [m for m in model.modules() if isinstance(m, CM3PEncoder)]


def test_training_switch_reaches_every_encoder_and_the_default_call_leaves_it_alone():
    for model in _models():
        encs = _encoders(model)
        assert encs and all(e.train_residual_dtype is None and e.residual_dtype is None for e in encs)
        assert model.set_residual_dtype(BF) is model  # as before: the forward-only switch alone
        assert all(e.residual_dtype is BF and e.train_residual_dtype is None for e in encs)
        assert model.set_residual_dtype(BF, training=True) is model
        assert all(e.residual_dtype is BF and e.train_residual_dtype is BF for e in encs)
        model.set_residual_dtype(torch.float32, training=True)
        assert all(e.residual_dtype is torch.float32 and e.train_residual_dtype is torch.float32 for e in encs)
        model.set_residual_dtype(None, training=True)
        assert all(e.residual_dtype is None and e.train_residual_dtype is None for e in encs)
        model.set_residual_dtype(BF, training=True)
        model.set_residual_dtype(None)  # training=False does exactly what it did: the training attribute stays
        assert all(e.residual_dtype is None and e.train_residual_dtype is BF for e in encs)


@pytest.mark.parametrize("bad", [torch.float16, torch.float64, torch.int32, "bfloat16", 16])
def test_bad_dtypes_raise_value_error_before_anything_changes(bad):
    model = _models()[0]
    enc = model.beatmap_model.encoder
    with pytest.raises(ValueError):
        enc.train_residual_dtype = bad
    with pytest.raises(ValueError):
        model.set_residual_dtype(bad, training=True)
    assert all(e.residual_dtype is None and e.train_residual_dtype is None for e in _encoders(model))
    model.set_residual_dtype(BF, training=True)
    with pytest.raises(ValueError):
        model.set_residual_dtype(bad, training=True)
    assert all(e.residual_dtype is BF and e.train_residual_dtype is BF for e in _encoders(model))


def test_state_dict_and_config_are_unchanged():
    for model in _models():
        keys, cfg = list(model.state_dict().keys()), model.config.to_dict()
        model.set_residual_dtype(BF, training=True)
        assert list(model.state_dict().keys()) == keys and model.config.to_dict() == cfg
        assert not any("residual" in k for k in keys)


def test_the_rule_that_picks_the_stream():
    """CM3PEncoder._bf16_stream: calls that record a backward follow train_residual_dtype, all others residual_dtype; a dropout plan
    always means fp32."""
    from cm3p_amd.encoder import _DropPlan

    enc = _models()[0].beatmap_model.encoder
    plan = _DropPlan(1, 6554, 0, 0)
    enc.residual_dtype = BF
    assert not enc._bf16_stream(None)  # residual_dtype alone selects nothing on a call that records a backward, as before
    enc.train_residual_dtype = BF
    assert enc._bf16_stream(None)  # grad enabled + trainable parameters
    assert not enc._bf16_stream(plan)  # train-mode dropout
    with torch.no_grad():
        assert enc._bf16_stream(None) and not enc._bf16_stream(plan)
    enc.residual_dtype = None
    assert enc._bf16_stream(None)  # the training switch alone: training calls only
    with torch.no_grad():
        assert not enc._bf16_stream(None)
    enc.requires_grad_(False)
    assert not enc._bf16_stream(None, None)  # frozen tower, no input wants a gradient: a forward-only call
    assert enc._bf16_stream(None, torch.zeros(2, requires_grad=True))  # an input that wants its gradient: a backward is recorded
    enc.train_residual_dtype = torch.float32
    assert not enc._bf16_stream(None, torch.zeros(2, requires_grad=True))


def test_header_binding_and_library_agree_on_abi_19():
    from cm3p_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    text = open(HEADER).read()
    assert int(re.search(r"^#define CM3P_ABI_VERSION (\d+)", text, re.M).group(1)) == _lib.ABI_VERSION >= 19  # (19 brought the arguments below; later versions keep them)
    assert _lib.load().cm3p_abi_version() == _lib.ABI_VERSION
    assert re.search(r"^#define CM3P_ADD_A_BF16 16\b", text, re.M) and _lib.ADD_A_BF16 == 16
    # the dtype arguments this stream added (x_dtype, dres_dtype; dy_dtype twice; dh_dtype), and cm3p_add_f32 with the count it had
    assert len(_lib.SIGNATURES["cm3p_layernorm_bwd"]) == 16 and len(_lib.SIGNATURES["cm3p_embed_ln_bwd"]) == 20
    assert len(_lib.SIGNATURES["cm3p_embed_ln_bwd_sorted"]) == 24 and len(_lib.SIGNATURES["cm3p_pool_bwd"]) == 10
    assert len(_lib.SIGNATURES["cm3p_add_f32"]) == 7


def test_new_entry_forms_refuse_bad_dtype_codes_without_a_gpu():
    from cm3p_amd import _lib

    lib = _lib.load()
    fake = 4096  # an aligned, never dereferenced address: every call below must fail validation first
    ln = lambda xd, rd, dx32, dres=fake: lib.cm3p_layernorm_bwd(fake, 1, fake, xd, fake, fake, fake, dres, rd, dx32, fake, fake, fake, 8, 64, None)
    assert ln(2, 0, None) == -1 and ln(1, 3, None) == -1
    assert lib.cm3p_add_f32(fake, fake, 16, fake, fake, 8, None) == -1  # bf16 first operand: no fp32 result
    assert lib.cm3p_add_f32(fake, fake, 32, fake, None, 8, None) == -1  # unknown flag
    assert lib.cm3p_pool_bwd(fake, None, None, fake, 2, 1, 4, 64, 1, None) == -1
    assert lib.cm3p_embed_ln_bwd(fake, 2, fake, fake, 0, None, None, 0, fake, fake, fake, fake, None, fake, fake, 8, 64, 0, 10, None) == -1


# ------------------------------------------------------------------------------------------------ the bounds, without a GPU
def _ln_bwd_bf16_path(dy, x, w, mean, rstd, dres, two_roundings=False, bf16_dw=False):
    """layernorm_bwd_kernel's all-bf16 dtype form in torch fp32 on bf16 inputs (R.ln_bwd_f32_path is the fp32 walk: fp32 sum, then ONE rounding to bf16).
    two_roundings: bf16(bf16(LN'(dy)) + dres), what a bf16 torch model computes.  bf16_dw: the dw sum kept in bf16."""
    if two_roundings:
        dx_ln, dw = R.ln_bwd_f32_path(dy, x, w, mean, rstd, None)
        dx = (dx_ln.to(BF).float() + dres.float()).to(BF)
    else:
        dx32, dw = R.ln_bwd_f32_path(dy, x, w, mean, rstd, dres)
        dx = dx32.to(BF)
    if bf16_dw:
        xh = (x.float() - mean[:, None]) * rstd[:, None]
        p = dy.float() * xh
        dw = torch.zeros(x.shape[1], dtype=BF)
        for r in range(x.shape[0]):
            dw = dw + p[r].to(BF)
        dw = dw.float()
    return dx, dw


@pytest.mark.parametrize("H", [260, 768, 1792])
def test_bf16_layernorm_backward_bounds_hold_for_one_rounding_and_refuse_two_and_a_bf16_dw(H):
    """The bound of a bf16 dx: the fp32 path's dx_b of R.ln_bwd_ref (float64 at the bf16 inputs as given) plus half a bf16 ulp of its
    binade (R.bf16_bound) - attained by the one-rounding walk.  The two-rounding form misses it wherever the first rounding's half ulp
    of LN'(dy) does not vanish under the second, and a dw summed in bf16 misses the fp32 form's dw bound."""
    g = gen("host-lnb16", H)
    n = 13
    x = (torch.randn(n, H, generator=g) * 2 + 0.5).to(BF)
    w = 1 + 0.2 * torch.randn(H, generator=g)
    _, mean, rstd = R.ln_fwd_f32_path(x.float(), w)
    dy = torch.randn(n, H, generator=g).to(BF)
    c = R.ln_dw_c(n, R.ln_bwd_blocks(n))
    assert c >= 3 + n  # (the walk adds the rows one after another)
    for dres in (None, torch.randn(n, H, generator=g).to(BF)):
        ref = R.ln_bwd_ref(dy.double(), x.double(), w.double(), mean.double(), rstd.double(), None if dres is None else dres.double())
        dx, dw = _ln_bwd_bf16_path(dy, x, w, mean, rstd, dres)
        check(dx, ref["dx"], R.bf16_bound(ref["dx"], ref["dx_b"]), "bf16 dx, one rounding")
        dw_b = c * U * ref["p"].abs().sum(0) * R.SECOND + FTZ
        check(dw, ref["p"].sum(0), dw_b, "dw")
        _, dw_bad = _ln_bwd_bf16_path(dy, x, w, mean, rstd, dres, bf16_dw=True)
        with pytest.raises(AssertionError, match="outside the bound"):
            check(dw_bad, ref["p"].sum(0), dw_b, "dw accumulated in bf16")
        if dres is not None:
            dx2, _ = _ln_bwd_bf16_path(dy, x, w, mean, rstd, dres, two_roundings=True)
            with pytest.raises(AssertionError, match="outside the bound"):
                check(dx2, ref["dx"], R.bf16_bound(ref["dx"], ref["dx_b"]), "bf16 dx, two roundings")


def test_bf16_add_and_pool_backward_bounds_hold_for_one_rounding():
    """bf16(a + b) of two bf16 operands: the fp32 sum of two bf16 values rounds once (u |sum|), then once to bf16.  The pooling
    gradient in bf16: R.pool_bwd_ref's 4u |ref| plus the half ulp."""
    g = gen("host-add16")
    a, b = torch.randn(4096, generator=g).to(BF), (torch.randn(4096, generator=g) * 3).to(BF)
    ref = a.double() + b.double()
    check((a.float() + b.float()).to(BF), ref, R.bf16_bound(ref, U * ref.abs() + FTZ), "bf16(a + b)")
    b32 = torch.randn(4096, generator=g) * 3  # an fp32 second operand (low bits set): it must enter the sum unrounded
    ref32 = a.double() + b32.double()
    check((a.float() + b32).to(BF), ref32, R.bf16_bound(ref32, U * ref32.abs() + FTZ), "bf16(a + b), fp32 b")
    with pytest.raises(AssertionError, match="outside the bound"):  # bf16(a + bf16(b)): the operand rounded first, two roundings
        check(a + b32.to(BF), ref32, R.bf16_bound(ref32, U * ref32.abs() + FTZ), "bf16(a + bf16(b))")
    Bn, S, H = 3, 40, 64
    dp = torch.randn(Bn, H, generator=g)
    mask = torch.ones(Bn, S, dtype=torch.int64)
    mask[1, 17:] = 0
    count = mask.sum(1).double()
    ref, e32 = R.pool_bwd_ref(dp.double(), mask, count, S, False)
    got = (dp[:, None, :] * (mask.float() / count.float()[:, None])[:, :, None]).to(BF)
    check(got, ref, R.bf16_bound(ref, e32 + FTZ), "bf16 pooling gradient")
