"""What cm3p_attn_bwd_fused refuses and what its two host queries answer, without a GPU (the thirteenth launching attention entry point;
tests/test_attention_entry_refusals_host.py holds the other twelve): every refusal returns CM3P_ERR_INVALID before any HIP call.

Each case starts from an argument list that passes every check (16-byte-aligned host pointers that are never dereferenced) and breaks
ONE precondition.  The unbroken list is never sent: it would reach a launch."""
import ctypes

import pytest

import attention_fused_refs as AF

ERR_INVALID = -1
NAME = "cm3p_attn_bwd_fused"
PARAMS = ("qkv out dout lse dqkv key_mask cu_seqlens B S total nh scale cos_tab sin_tab pos_batch_stride stages q_prescaled workspace "
          "workspace_bytes stream").split()
_raw = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_raw) + 15) & ~15  # aligned, non-NULL, never dereferenced
POINTERS = ("qkv", "out", "dout", "lse", "dqkv", "key_mask", "cu_seqlens", "cos_tab", "sin_tab", "workspace")
REQUIRED = ("qkv", "out", "dout", "lse", "dqkv", "workspace")
ALIGNED = ("qkv", "out", "dout", "dqkv", "workspace")
PREP, MAIN, REDUCE, MAIN_EVEN, MAIN_ODD, ADD1 = 1, 2, 4, 8, 16, 32
# every check passes: 2 padded sequences of 256 (ONE key block: G = 2 by the length rule), 2 heads, a key mask, tables shared by the batch
VALID = dict({p: P for p in POINTERS}, cu_seqlens=None, B=2, S=256, total=0, nh=2, scale=0.125, pos_batch_stride=0, stages=7, q_prescaled=1,
             workspace_bytes=1 << 62, stream=None)
PACKED = dict(VALID, cu_seqlens=P, key_mask=None, total=512)  # the packed form of the same
TOO_LONG = 2796203  # rows: S * 3 * nh * 128 = 2^31 + 256 at 2 heads


def _breaks():
    """(label, base list, {argument: value}) of every single broken precondition."""
    out = [(f"null_{p}", VALID, {p: None}) for p in REQUIRED]
    out += [(f"misaligned_{p}", VALID, {p: P + 8}) for p in ALIGNED]
    out += [("cos_without_sin", VALID, {"sin_tab": None}), ("sin_without_cos", VALID, {"cos_tab": None})]
    out += [("stages_0", VALID, {"stages": 0}), ("stages_256", VALID, {"stages": 256})]
    out += [(f"{p}_0", VALID, {p: 0}) for p in ("B", "S", "nh")] + [("scale_0", VALID, {"scale": 0.0})]
    out += [("packed_total_0", PACKED, {"total": 0}), ("packed_with_a_key_mask", PACKED, {"key_mask": P}),
            ("packed_with_a_batch_stride", PACKED, {"pos_batch_stride": 256})]
    out += [("pos_batch_stride_neither_0_nor_S", VALID, {"pos_batch_stride": 128})]
    out += [("workspace_one_byte_short", VALID, {"workspace_bytes": AF.workspace_bytes(2, 256, 2) - 1})]
    out += [("rows_past_32_bit_offsets", VALID, {"S": TOO_LONG})]
    # G = 2 here: the adding launch of group position 2 (ADD1 << 1 = 64) names a position this group size does not have.  (32 is
    # position 1, which exists; under CM3P_FUSED_SLAB_GROUP=4 the bit 64 would exist too and the call would launch: never sent.)
    out += [("add_bit_of_a_group_position_past_G", VALID, {"stages": ADD1 << 1}), ("add_bit_of_position_3", VALID, {"stages": PREP | (ADD1 << 2)})]
    return out


CASES = _breaks()


def _lib():
    from cm3p_amd import _lib

    return _lib


def test_the_argument_list_is_the_abi_s():
    L = _lib()
    assert len(PARAMS) == len(L.SIGNATURES[NAME]) == 20
    for p, ctype in zip(PARAMS, L.SIGNATURES[NAME]):
        assert (ctype is ctypes.c_void_p) == (p in POINTERS or p == "stream"), p
    assert TOO_LONG * 3 * VALID["nh"] * 128 >= 2 ** 31 > (TOO_LONG - 1) * 3 * VALID["nh"] * 128
    from cm3p_amd import kernels as K

    assert (K.ATTN_BWD_FUSED_PREP, K.ATTN_BWD_FUSED_MAIN, K.ATTN_BWD_FUSED_REDUCE, K.ATTN_BWD_FUSED_MAIN_EVEN, K.ATTN_BWD_FUSED_MAIN_ODD,
            K.ATTN_BWD_FUSED_MAIN_ADD1) == (PREP, MAIN, REDUCE, MAIN_EVEN, MAIN_ODD, ADD1)
    labels = {label for label, _, _ in CASES}
    assert len(labels) == len(CASES) == 6 + 5 + 2 + 2 + 4 + 3 + 1 + 1 + 1 + 2
    for label, base, broken in CASES:  # one argument, away from its valid value
        (p, v), = broken.items()
        assert p in PARAMS and base[p] != v, label
    assert VALID["workspace_bytes"] >= AF.workspace_bytes(TOO_LONG, 256, 2)  # (so that the long S is refused for its offsets alone ...)
    assert VALID["workspace_bytes"] >= AF.workspace_bytes(2, TOO_LONG, 2)


@pytest.mark.parametrize("label,base,broken", CASES, ids=[c[0] for c in CASES])
def test_one_broken_precondition_is_refused(label, base, broken, monkeypatch):
    monkeypatch.delenv("CM3P_FUSED_SLAB_GROUP", raising=False)  # the length rule: G = 2 at one key block
    L = _lib()
    assert L.query("cm3p_attn_bwd_fused_slab_group", base["S"]) == 2
    args = [broken.get(p, base[p]) for p in PARAMS]
    assert args != [base[p] for p in PARAMS]  # (the unbroken list would reach a launch)
    assert getattr(L.load(), NAME)(*args) == ERR_INVALID


def test_the_slab_group_query(monkeypatch):
    q = lambda S: _lib().query("cm3p_attn_bwd_fused_slab_group", S)  # noqa: E731
    monkeypatch.delenv("CM3P_FUSED_SLAB_GROUP", raising=False)
    assert (q(256), q(5888), q(5889), q(AF.LONG_S), q(8192)) == (2, 2, 4, 4, 4)
    for value, want in (("2", (2, 2)), ("4", (4, 4)), ("4x", (2, 4)), ("3", (2, 4)), ("", (2, 4)), ("24", (2, 4)), (" 4", (2, 4))):
        monkeypatch.setenv("CM3P_FUSED_SLAB_GROUP", value)
        assert (q(5888), q(5889)) == want, repr(value)


def test_the_workspace_query_is_the_documented_formula():
    q = lambda *a: _lib().query("cm3p_attn_bwd_fused_workspace_bytes", *a)  # noqa: E731
    shapes = [(c.B, c.S, 2) for c in AF.TABLE_F] + [(1, AF.RELOC_S, 2), (1, AF.LONG_S, 2), (32, 4096, 12), (16, 8192, 12), (2, 256, 2), (1, 1, 1)]
    for B, S, nh in shapes:
        assert q(B, S, nh) == AF.workspace_bytes(B, S, nh) > 0, (B, S, nh)
        assert q(B, S, nh) % 256 == 0
    assert 17e6 < AF.workspace_bytes(1, AF.LONG_S, 2) < 19e6 and AF.workspace_bytes(16, 8192, 12) > 2 ** 31 > AF.workspace_bytes(32, 4096, 12) > 1.6e9
    for bad in ((0, 256, 2), (2, 0, 2), (2, 256, 0), (-1, 256, 2), (2, -256, 2), (2, 256, -2)):
        assert q(*bad) == 0 == AF.workspace_bytes(*bad), bad
