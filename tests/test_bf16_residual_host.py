"""The bf16 residual-stream switch on the host (no GPU): where it is set, what it refuses, what it leaves alone, and the C-ABI
pieces it adds (the CM3P_EPI_BF16_RESID epilogue code, the bumped ABI version)."""
import os
import re

import pytest
import torch

from cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cm3p_hip.h")


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


def test_set_residual_dtype_reaches_every_encoder():
    full, mlm, cls, bproj, mproj = _models()
    assert len(_encoders(full)) == 3 and len(_encoders(mlm)) == 2 and len(_encoders(mproj)) == 1  # beatmap, audio, metadata towers
    for model in (full, mlm, cls, bproj, mproj):
        assert all(e.residual_dtype is None for e in _encoders(model))  # the default: fp32 stream
        assert model.set_residual_dtype(torch.bfloat16) is model
        assert all(e.residual_dtype is torch.bfloat16 for e in _encoders(model))
        model.set_residual_dtype(torch.float32)
        assert all(e.residual_dtype is torch.float32 for e in _encoders(model))
        model.set_residual_dtype(None)
        assert all(e.residual_dtype is None for e in _encoders(model))


def test_bf16_parameters_do_not_change_the_default():
    model = _models()[0].to(torch.bfloat16)
    assert all(e.residual_dtype is None for e in _encoders(model))


@pytest.mark.parametrize("bad", [torch.float16, torch.float64, torch.int32, "bfloat16", 16])
def test_bad_dtypes_raise_value_error(bad):
    model = _models()[0]
    enc = model.beatmap_model.encoder
    with pytest.raises(ValueError):
        enc.residual_dtype = bad
    with pytest.raises(ValueError):
        model.set_residual_dtype(bad)
    assert all(e.residual_dtype is None for e in _encoders(model))


def test_state_dict_and_config_are_unchanged():
    for model in _models():
        keys, cfg = list(model.state_dict().keys()), model.config.to_dict()
        model.set_residual_dtype(torch.bfloat16)
        assert list(model.state_dict().keys()) == keys and model.config.to_dict() == cfg
        assert not any("residual" in k for k in keys)


def test_the_stream_runs_bf16_only_on_forward_only_calls_without_dropout():
    """The rule that picks the stream before the embedding runs (CM3PEncoder._bf16_stream)."""
    from cm3p_amd.encoder import _DropPlan

    enc = _models()[0].beatmap_model.encoder
    assert not enc._bf16_stream(None)  # switch off
    enc.residual_dtype = torch.bfloat16
    assert not enc._bf16_stream(None)  # grad enabled, trainable parameters: a backward will follow
    with torch.no_grad():
        assert enc._bf16_stream(None)
        assert not enc._bf16_stream(_DropPlan(1, 6554, 0, 0))  # train-mode dropout plan
    enc.requires_grad_(False)
    assert enc._bf16_stream(None, None)  # frozen tower, grad mode on: nothing is recorded
    assert not enc._bf16_stream(None, torch.zeros(2, requires_grad=True))  # an input that wants its gradient
    enc.residual_dtype = torch.float32
    with torch.no_grad():
        assert not enc._bf16_stream(None)


def test_header_defines_the_bf16_residual_epilogue():
    from cm3p_amd import _lib

    text = open(HEADER).read()
    assert re.search(r"^#define CM3P_EPI_BF16_RESID 7\b", text, re.M)
    assert _lib.EPI_BF16_RESID == 7
    # the code is free: no internal epilogue of csrc/common.h uses 7
    common = open(os.path.join(ROOT, "cm3p_amd", "csrc", "common.h")).read()
    assert not re.search(r"^#define CM3P_EPI_\w+ 7\b", common, re.M)


def test_library_and_binding_agree_on_the_bumped_abi_version():
    from cm3p_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    m = re.search(r"^#define CM3P_ABI_VERSION (\d+)", open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION >= 18
    assert _lib.load().cm3p_abi_version() == _lib.ABI_VERSION
    assert len(_lib.SIGNATURES["cm3p_pool_fwd"]) == 11  # (h, h_dtype, mask, pooled, partial, count, Bn, S, H, cls, stream)
