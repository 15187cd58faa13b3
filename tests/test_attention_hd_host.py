"""Head sizes 96 and 128 without a GPU: what the library says it supports, what the entry points refuse before any HIP call, what
constructs, and that the C ABI did not move (the new kernels sit behind cm3p_attn_fwd_generic / cm3p_attn_bwd_generic)."""
import ctypes
import os
import re

import pytest

import cases_hd
from cases import CASES

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cm3p_hip.h")
ERR_INVALID = -1


def _lib_loaded():
    from cm3p_amd import _lib

    return _lib.load()


def test_supported_head_sizes():
    lib = _lib_loaded()
    for d in (16, 32, 64, 96, 128):
        assert lib.cm3p_attn_generic_supported(d) == 1, d
    for d in (8, 48, 80, 112, 256):
        assert lib.cm3p_attn_generic_supported(d) == 0, d


def test_plain_entries_refuse_a_null_qkv_at_head_dim_128_before_any_hip_call():
    lib = _lib_loaded()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)  # (never dereferenced: the NULL qkv is refused first)
    assert lib.cm3p_attn_fwd_generic(None, p, p, None, 1, 32, 1, 128, -1, 0.1, None) == ERR_INVALID
    assert lib.cm3p_attn_bwd_generic(None, p, p, p, p, p, None, 1, 32, 1, 128, -1, 0.1, None) == ERR_INVALID


@pytest.mark.parametrize("D", [96, 128])
def test_dropout_entries_refuse_the_wide_heads(D):
    """Otherwise valid-looking arguments (aligned non-NULL pointers, thr and layer in range): the kernels of 96 / 128 have no dropout form.
    The refusal comes before any HIP call, so host memory is never touched."""
    lib = _lib_loaded()
    raw = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    assert lib.cm3p_attn_fwd_generic_dropout(p, p, p, None, 1, 32, 1, D, -1, D ** -0.5, 0, 6554, 1234, None) == ERR_INVALID
    assert lib.cm3p_attn_bwd_generic_dropout(p, p, p, p, p, p, None, 1, 32, 1, D, -1, D ** -0.5, 0, 6554, 1234, None) == ERR_INVALID


def test_wide_towers_construct_and_head_dim_8_still_raises():
    from cm3p_amd import CM3PConfig, CM3PModel

    cfg = CM3PConfig(**cases_hd.CASE["cfg"])
    assert (cfg.beatmap_config.hidden_size, cfg.beatmap_config.num_attention_heads) == (256, 2)
    assert (cfg.metadata_config.hidden_size, cfg.metadata_config.num_attention_heads) == (192, 2)
    model = CM3PModel(cfg)
    assert model.beatmap_model.encoder.layers[0].attn.Wqkv.weight.shape == (768, 256)
    assert model.metadata_model.encoder.layers[0].attn.Wqkv.weight.shape == (576, 192)
    bad = {**CASES["c1_tiny_nopad"]["cfg"]}
    bad["beatmap_config"] = {**bad["beatmap_config"], "num_attention_heads": 8}  # head_dim 8: the configuration of test_unsupported_shapes_fail_loudly
    with pytest.raises(NotImplementedError, match="head_dim") as e:
        CM3PModel(CM3PConfig(**bad))
    assert "96" in str(e.value) and "128" in str(e.value)


def test_the_c_abi_did_not_move():
    from cm3p_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"^#define CM3P_ABI_VERSION (\d+)", text, re.M).group(1)) == _lib.ABI_VERSION >= 19  # (20 since cm3p_gemm_route)
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.SIGNATURES)
    assert not any("attn_hd" in n for n in declared)  # the wide-head launchers are plain C++ behind the generic entry points


def test_isa_check_is_registered_for_the_new_file():
    from cm3p_amd import build, isa_check

    assert "attention_hd.hip" in build.SOURCES and "attention_hd.hip" in isa_check.CHECKS
    assert "attention_hd.hip" not in build.AUDIT_SOURCES  # no LDS-DMA in it
