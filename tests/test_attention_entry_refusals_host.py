"""What the twelve launching attention entry points refuse, without a GPU: every refusal returns CM3P_ERR_INVALID before any HIP call.

Each case starts from an argument list that passes every check of its entry point (16-byte-aligned host pointers that are never
dereferenced) and breaks ONE precondition.  The unbroken list is never sent: it would reach a launch.  This is the specification of the
argument checks the entry points share (csrc/attention.hip, csrc/attention_generic.hip)."""
import ctypes

import pytest

ERR_INVALID = -1

_BAND_FWD = "qkv out lse key_mask B S nh window scale q_prescaled"
_BAND_BWD = "qkv out dout lse delta dqkv key_mask B S nh window scale cos_tab sin_tab pos_batch_stride stages q_prescaled"
_VARLEN_FWD = "qkv out lse cu_seqlens B max_seqlen total nh window scale q_prescaled"
_VARLEN_BWD = "qkv out dout lse delta dqkv cu_seqlens B max_seqlen total nh window scale cos_tab sin_tab stages q_prescaled"
_GEN_FWD = "qkv out lse key_mask B S nh head_dim window scale"
_GEN_BWD = "qkv out dout lse delta dqkv key_mask B S nh head_dim window scale"
_DROP = " layer thr seed"
ENTRIES = {
    "cm3p_attn_fwd": _BAND_FWD,
    "cm3p_attn_bwd": _BAND_BWD,
    "cm3p_attn_fwd_varlen": _VARLEN_FWD,
    "cm3p_attn_bwd_varlen": _VARLEN_BWD,
    "cm3p_attn_fwd_dropout": _BAND_FWD + _DROP,
    "cm3p_attn_bwd_dropout": _BAND_BWD + _DROP,
    "cm3p_attn_fwd_dropout_varlen": _VARLEN_FWD + _DROP,
    "cm3p_attn_bwd_dropout_varlen": _VARLEN_BWD + _DROP,
    "cm3p_attn_fwd_generic": _GEN_FWD,
    "cm3p_attn_bwd_generic": _GEN_BWD,
    "cm3p_attn_fwd_generic_dropout": _GEN_FWD + _DROP,
    "cm3p_attn_bwd_generic_dropout": _GEN_BWD + _DROP,
}
ENTRIES = {name: (params + " stream").split() for name, params in ENTRIES.items()}

_raw = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_raw) + 15) & ~15  # aligned, non-NULL, never dereferenced
POINTERS = ("qkv", "out", "dout", "lse", "delta", "dqkv", "key_mask", "cu_seqlens", "cos_tab", "sin_tab")
REQUIRED = ("qkv", "out", "dout", "lse", "delta", "dqkv", "cu_seqlens")  # (key_mask is optional, the rotary tables come as a pair)
ALIGNED = ("qkv", "out", "dout", "dqkv")
# every check passes: 2 sequences of 256, 2 heads, a +-64 window, both stages, p = 0.1 in layer 0
VALID = dict({p: P for p in POINTERS}, B=2, S=256, max_seqlen=256, total=512, nh=2, head_dim=32, window=64, scale=0.125, q_prescaled=1,
             pos_batch_stride=0, stages=3, layer=0, thr=6554, seed=1234, stream=None)
TOO_LONG = 2796203  # rows: S * 3 * nh * 128 = 2^31 + 256 at the 2 heads of VALID (one row fewer is 512 short of 2^31)


def _breaks(name, params):
    """(label, {argument: value}) of every single broken precondition of entry point `name`."""
    band_bwd = "stages" in params
    out = [(f"null_{p}", {p: None}) for p in REQUIRED if p in params]
    out += [(f"misaligned_{p}", {p: P + 8}) for p in ALIGNED if p in params]
    out += [(f"{p}_0", {p: 0}) for p in ("B", "S", "max_seqlen", "nh", "total") if p in params]
    out += [("scale_0", {"scale": 0.0})]
    if band_bwd:
        out += [("cos_without_sin", {"sin_tab": None}), ("sin_without_cos", {"cos_tab": None}), ("stages_0", {"stages": 0}), ("stages_4", {"stages": 4})]
        out += [("rows_past_32_bit_offsets", {"S" if "S" in params else "max_seqlen": TOO_LONG})]
    if "pos_batch_stride" in params:
        out += [("pos_batch_stride_neither_0_nor_S", {"pos_batch_stride": VALID["S"] // 2})]
    if "thr" in params:
        out += [("thr_-1", {"thr": -1}), ("thr_65537", {"thr": 65537}), ("layer_-1", {"layer": -1}), ("layer_2^29", {"layer": 1 << 29})]
    if "head_dim" in params:
        out += [(f"head_dim_{d}", {"head_dim": d}) for d in (8, 48)]
        if "thr" in params:  # the matrix-core kernels of 96 / 128 have no dropout form
            out += [(f"head_dim_{d}_with_dropout", {"head_dim": d}) for d in (96, 128)]
    return out


CASES = [(name, label, broken) for name, params in ENTRIES.items() for label, broken in _breaks(name, params)]


def test_the_argument_lists_are_the_abi_s():
    from cm3p_amd import _lib

    assert len(ENTRIES) == 12
    for name, params in ENTRIES.items():
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, ctype in zip(params, _lib.SIGNATURES[name]):
            assert (ctype is ctypes.c_void_p) == (p in POINTERS or p == "stream"), (name, p)
    assert TOO_LONG * 3 * VALID["nh"] * 128 >= 2 ** 31 > (TOO_LONG - 1) * 3 * VALID["nh"] * 128


def test_the_cases_cover_every_entry():
    per_entry = {name: {label for n, label, _ in CASES if n == name} for name in ENTRIES}
    assert all({"null_qkv", "misaligned_out", "B_0", "nh_0", "scale_0"} <= labels for labels in per_entry.values())
    assert sum("rows_past_32_bit_offsets" in labels for labels in per_entry.values()) == 4
    assert sum("thr_65537" in labels for labels in per_entry.values()) == 6
    assert sum("head_dim_48" in labels for labels in per_entry.values()) == 4
    assert sum("head_dim_128_with_dropout" in labels for labels in per_entry.values()) == 2
    for name, label, broken in CASES:  # one argument of the entry point's own, away from its valid value
        (p, v), = broken.items()
        assert p in ENTRIES[name] and VALID[p] != v, (name, label)


@pytest.mark.parametrize("name,label,broken", CASES, ids=[f"{n}-{l}" for n, l, _ in CASES])
def test_one_broken_precondition_is_refused(name, label, broken):
    from cm3p_amd import _lib

    args = [broken.get(p, VALID[p]) for p in ENTRIES[name]]
    assert args != [VALID[p] for p in ENTRIES[name]]  # (the unbroken list would reach a launch)
    assert getattr(_lib.load(), name)(*args) == ERR_INVALID
