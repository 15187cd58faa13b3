"""Pooling of caller-packed rows, the part that needs no GPU: cm3p_pool_fwd / cm3p_pool_bwd refuse an inconsistent description of
the layout before any HIP call, and the opt-in switch (`pool_unpadded`) is off on fresh towers and set through CM3PModel."""
import os
import re

import pytest

from cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cm3p_hip.h")
FAKE = 4096  # an aligned, never dereferenced address: every call below must fail validation first


@pytest.fixture(scope="module")
def lib():
    from cm3p_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


PACKED = 2  # CM3P_POOL_PACKED, or-ed into cls: `mask` then carries the int32 cu_seqlens of packed rows


def _fwd(lib, cu=FAKE, H=64, h_dtype=0, cls=0, h=FAKE, partial=FAKE, S=128):
    return lib.cm3p_pool_fwd(h, h_dtype, cu, FAKE, partial, FAKE, 2, S, H, cls | PACKED, None)


def _bwd(lib, cu=FAKE, H=64, dh_dtype=0, cls=0, rows=5, dp=FAKE, dh=FAKE):
    return lib.cm3p_pool_bwd(dp, cu, None, dh, dh_dtype, 2, rows, H, cls | PACKED, None)


@pytest.mark.parametrize("entry", [_fwd, _bwd], ids=["cm3p_pool_fwd", "cm3p_pool_bwd"])
@pytest.mark.parametrize("cls", [0, 1])
def test_inconsistent_layout_descriptions_are_refused_before_any_hip_call(lib, entry, cls):
    """The argument lists are the padded form's (no new parameter, the ABI version stays): the packed layout is a flag in `cls` and
    cu_seqlens travels where the mask does.  So "mask and cu_seqlens together" cannot be said; what can be said wrongly is refused."""
    assert entry(lib, cu=None, cls=cls) == -1  # packed rows without their cu_seqlens
    assert entry(lib, cu=FAKE + 2, cls=cls) == -1  # int32 entries
    assert entry(lib, H=6, cls=cls) == -1  # the existing H % 4 condition
    if entry is _bwd:
        assert entry(lib, rows=0, cls=cls) == -1 and entry(lib, rows=-4, cls=cls) == -1  # packed rows need their total
        assert entry(lib, dh_dtype=2, cls=cls) == -1 and entry(lib, dp=None, cls=cls) == -1 and entry(lib, dh=None, cls=cls) == -1
    else:
        assert entry(lib, S=0, cls=cls) == -1 and entry(lib, h=None, cls=cls) == -1 and entry(lib, h_dtype=2, cls=cls) == -1
        assert entry(lib, h=FAKE + 4, h_dtype=1, cls=cls) == -1  # bf16 rows: 8-byte loads
        if not cls:
            assert entry(lib, partial=None) == -1  # mean pooling needs its workspace


def test_header_and_binding_keep_the_argument_lists_and_name_the_flag():
    from cm3p_amd import _lib

    text = open(HEADER).read()
    assert re.search(r"^#define CM3P_POOL_PACKED 2\b", text, re.M) and _lib.POOL_PACKED == PACKED
    assert len(_lib.SIGNATURES["cm3p_pool_fwd"]) == 11 and len(_lib.SIGNATURES["cm3p_pool_bwd"]) == 10
    assert int(re.search(r"^#define CM3P_ABI_VERSION (\d+)", text, re.M).group(1)) == _lib.ABI_VERSION


def test_kernel_wrappers_refuse_a_packed_description_that_does_not_fit():
    """Raised by the wrapper's own checks, before a pointer is taken (CPU tensors would be refused next)."""
    import torch

    from cm3p_amd import kernels as K

    h = torch.zeros(10, 8)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="mask"):
        K.pool_fwd(h, torch.ones(2, 5, dtype=torch.int64), 2, 6, False, cu=cu)
    with pytest.raises(ValueError, match="Bn \\+ 1"):
        K.pool_fwd(h, None, 3, 6, False, cu=cu)
    with pytest.raises(ValueError, match="total"):
        K.pool_fwd(h, None, 2, 6, False, cu=cu, total=11)
    with pytest.raises(ValueError, match="total"):
        K.pool_bwd(torch.zeros(2, 8), None, None, 2, 6, False, cu=cu)
    with pytest.raises(ValueError, match="total"):
        K.pool_bwd(torch.zeros(2, 8), None, None, 2, 6, False, cu=cu, total=11, out=h)


def test_switch_is_off_on_fresh_towers_and_the_model_property_sets_both():
    from cm3p_amd import CM3PConfig, CM3PModel
    from cm3p_amd.configuration_cm3p import CM3PBeatmapConfig, CM3PMetadataConfig
    from cm3p_amd.modeling_cm3p import CM3PBeatmapModelWithProjection, CM3PBeatmapTransformer, CM3PMetadataModelWithProjection, CM3PMetadataTransformer

    cfg = CASES["d64_mean_pad"]["cfg"]
    bc, mc = CM3PBeatmapConfig(**cfg["beatmap_config"]), CM3PMetadataConfig(**cfg["metadata_config"])
    assert CM3PBeatmapTransformer(bc).pool_unpadded is False and CM3PMetadataTransformer(mc).pool_unpadded is False
    assert CM3PBeatmapModelWithProjection(bc).beatmap_model.pool_unpadded is False
    assert CM3PMetadataModelWithProjection(mc).metadata_model.pool_unpadded is False
    model = CM3PModel(CM3PConfig(**cfg))
    assert model.pool_unpadded is False and model.beatmap_model.pool_unpadded is False and model.metadata_model.pool_unpadded is False
    model.pool_unpadded = True
    assert model.pool_unpadded is True and model.beatmap_model.pool_unpadded is True and model.metadata_model.pool_unpadded is True
    model.metadata_model.pool_unpadded = False  # one tower alone: the model reports the switch as not (fully) on
    assert model.pool_unpadded is False and model.beatmap_model.pool_unpadded is True
    model.pool_unpadded = False
    assert model.beatmap_model.pool_unpadded is False and model.metadata_model.pool_unpadded is False
    assert "pool_unpadded" not in model.state_dict() and "pool_unpadded" not in dict(model.named_modules())
