"""What the four launching bf16 GEMM entry points refuse, without a GPU: every refusal returns CM3P_ERR_INVALID before any HIP call.

Each case starts from an argument list that passes every check of its entry point (16-byte-aligned host pointers that are never
dereferenced), optionally moved to another list that passes them too (`base`: the epilogue, layout or split count the broken
precondition belongs to), and breaks ONE precondition.  No unbroken list is ever sent: it would reach a launch.  This is the
specification of the CM3P_REQUIRE clauses of csrc/gemm.hip."""
import ctypes

import pytest

ERR_INVALID = -1
EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_ROPE, EPI_AXPBY, EPI_F32_BIAS, EPI_GEGLU, EPI_BF16_RESID = range(8)  # include/cm3p_hip.h, csrc/common.h

ENTRIES = {
    "cm3p_gemm_bf16": "A B C R M N K lda ldb ldc a_kc b_kc epilogue split_k workspace",
    "cm3p_qkv_gemm_rope": "x Wqkv qkv M N K cos_tab sin_tab S per_batch rope_cols q_scale",
    "cm3p_gemm_geglu": "x w_interleaved a T I K",
    "cm3p_gemm_bf16_batched": "A B C R batch M N K lda ldb ldc stride_a stride_b stride_c stride_r a_kc b_kc alpha beta",
}
ENTRIES = {name: (params + " stream").split() for name, params in ENTRIES.items()}

_raw = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_raw) + 15) & ~15  # aligned, non-NULL, never dereferenced
POINTERS = ("A", "B", "C", "R", "workspace", "x", "Wqkv", "qkv", "cos_tab", "sin_tab", "w_interleaved", "a")

# every check passes: one 64 x 64 x 64 product in the forward layout, fp32 output, every optional pointer present
VALID = {
    "cm3p_gemm_bf16": dict(A=P, B=P, C=P, R=P, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, a_kc=1, b_kc=1, epilogue=EPI_F32, split_k=1,
                           workspace=P, stream=None),
    # two heads: q and k rotated (128 columns), two sequences of 64 rows
    "cm3p_qkv_gemm_rope": dict(x=P, Wqkv=P, qkv=P, M=128, N=192, K=64, cos_tab=P, sin_tab=P, S=64, per_batch=0, rope_cols=128, q_scale=1.0,
                               stream=None),
    # 200 x 1 tiles of 256 x 256: the smallest shape the fused Wi + GeGLU kernel takes
    "cm3p_gemm_geglu": dict(x=P, w_interleaved=P, a=P, T=51200, I=128, K=64, stream=None),
    "cm3p_gemm_bf16_batched": dict(A=P, B=P, C=P, R=P, batch=2, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, stride_a=4096, stride_b=4096,
                                   stride_c=4096, stride_r=4096, a_kc=1, b_kc=1, alpha=1.0, beta=0.5, stream=None),
}


def _layout_breaks():
    """The operand-layout clauses cm3p_gemm_bf16 and cm3p_gemm_bf16_batched share: (label, base, broken)."""
    out = [("K_not_multiple_of_8_k_contiguous", {}, {"K": 60})]
    for flag, ld, extent in (("a_kc", "lda", "M"), ("b_kc", "ldb", "N")):
        out += [(f"{ld}_not_multiple_of_8", {}, {ld: 68}), (f"{ld}_below_K", {}, {ld: 56}),
                (f"{ld}_below_{extent}_k_strided", {flag: 0}, {ld: 56}), (f"{extent}_not_multiple_of_8_k_strided", {flag: 0}, {extent: 60})]
    return out


def _breaks(name):
    """(label, base, broken): `base` moves VALID[name] to another list that passes every check, `broken` breaks one precondition."""
    if name == "cm3p_gemm_bf16":
        out = [(f"null_{p}", {}, {p: None}) for p in "ABC"] + [(f"misaligned_{p}", {}, {p: P + 8}) for p in "ABC"]
        out += [(f"{p}_0", {}, {p: 0}) for p in "MNK"] + _layout_breaks()
        out += [(f"epilogue_{e}", {}, {"epilogue": e}) for e in (-1, EPI_ROPE, EPI_AXPBY, EPI_GEGLU, 8)]  # the internal numbers and past the ends
        out += [("ldc_not_multiple_of_4", {}, {"ldc": 66}), ("N_not_multiple_of_4", {}, {"N": 62}), ("ldc_below_N", {}, {"ldc": 56})]
        for e in (EPI_F32_RESID, EPI_F32_BIAS, EPI_BF16_RESID):
            out += [(f"epilogue_{e}_without_R", {"epilogue": e}, {"R": None}), (f"epilogue_{e}_misaligned_R", {"epilogue": e}, {"R": P + 8})]
        out += [(f"bias_epilogue_k_strided_{f}", {"epilogue": EPI_F32_BIAS}, {f: 0}) for f in ("a_kc", "b_kc")]
        out += [("bf16_resid_N_mod_8_is_4", {"epilogue": EPI_BF16_RESID}, {"N": 60}), ("bf16_resid_ldc_mod_8_is_4", {"epilogue": EPI_BF16_RESID}, {"ldc": 68})]
        out += [("split_k_0", {}, {"split_k": 0}), ("split_k_-1", {}, {"split_k": -1})]
        out += [("split_k_without_workspace", {"split_k": 2}, {"workspace": None}), ("split_k_misaligned_workspace", {"split_k": 2}, {"workspace": P + 8}),
                ("split_k_ldc_not_N", {"split_k": 2}, {"ldc": 72})]
        out += [(f"split_k_epilogue_{e}", {"split_k": 2}, {"epilogue": e}) for e in (EPI_BF16, EPI_F32_RESID, EPI_F32_BIAS, EPI_BF16_RESID)]
        return out
    if name == "cm3p_qkv_gemm_rope":
        ptrs = ("x", "Wqkv", "qkv", "cos_tab", "sin_tab")
        out = [(f"null_{p}", {}, {p: None}) for p in ptrs] + [(f"misaligned_{p}", {}, {p: P + 8}) for p in ptrs]
        out += [(f"{p}_0", {}, {p: 0}) for p in ("M", "N", "K", "S")]
        out += [("K_not_multiple_of_8", {}, {"K": 60}), ("N_not_multiple_of_64", {}, {"N": 200}), ("rope_cols_not_multiple_of_64", {}, {"rope_cols": 96}),
                ("rope_cols_negative", {}, {"rope_cols": -64}), ("rope_cols_past_N", {}, {"rope_cols": 256}),
                ("M_not_multiple_of_S_without_per_batch", {}, {"M": 100}), ("q_scale_0", {}, {"q_scale": 0.0}), ("q_scale_negative", {}, {"q_scale": -1.0})]
        return out
    if name == "cm3p_gemm_geglu":
        ptrs = ("x", "w_interleaved", "a")
        out = [(f"null_{p}", {}, {p: None}) for p in ptrs] + [(f"misaligned_{p}", {}, {p: P + 8}) for p in ptrs]
        out += [(f"{p}_0", {}, {p: 0}) for p in "TIK"]
        out += [("K_not_multiple_of_64", {}, {"K": 96}), ("I_not_multiple_of_32", {}, {"I": 144}), ("T_not_multiple_of_8", {}, {"T": 51204}),
                ("199_tiles", {}, {"T": 50944})]
        return out
    out = [(f"null_{p}", {}, {p: None}) for p in "ABC"] + [(f"misaligned_{p}", {}, {p: P + 8}) for p in "ABCR"]
    out += [(f"{p}_0", {}, {p: 0}) for p in "MNK"] + [("batch_0", {}, {"batch": 0}), ("batch_65536", {}, {"batch": 65536})] + _layout_breaks()
    out += [("ldc_not_multiple_of_8", {}, {"ldc": 68}), ("N_not_multiple_of_8", {}, {"N": 60}), ("ldc_below_N", {}, {"ldc": 56})]
    out += [(f"{p}_not_multiple_of_8", {}, {p: 4100}) for p in ("stride_a", "stride_b", "stride_c", "stride_r")]
    return out


CASES = [(name, label, base, broken) for name in ENTRIES for label, base, broken in _breaks(name)]


def test_the_argument_lists_are_the_abi_s():
    from cm3p_amd import _lib

    assert len(ENTRIES) == 4
    for name, params in ENTRIES.items():
        assert params == list(VALID[name]), name
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, ctype in zip(params, _lib.SIGNATURES[name]):
            assert (ctype is ctypes.c_void_p) == (p in POINTERS or p == "stream"), (name, p)
            assert (ctype is ctypes.c_float) == isinstance(VALID[name][p], float), (name, p)
    assert (EPI_BF16, EPI_F32, EPI_F32_RESID, EPI_F32_BIAS, EPI_BF16_RESID) == (_lib.EPI_BF16, _lib.EPI_F32, _lib.EPI_F32_RESID, _lib.EPI_F32_BIAS,
                                                                              _lib.EPI_BF16_RESID)
    t = VALID["cm3p_gemm_geglu"]
    assert -(-t["T"] // 256) * -(-2 * t["I"] // 256) == 200 and -(-50944 // 256) == 199 and 50944 % 8 == 0


def test_the_cases_cover_every_entry():
    per_entry = {name: {label for n, label, _, _ in CASES if n == name} for name in ENTRIES}
    assert all(any(l.startswith("null_") for l in labels) and any(l.startswith("misaligned_") for l in labels) and "K_0" in labels
               for labels in per_entry.values())
    assert {"lda_below_M_k_strided", "N_not_multiple_of_8_k_strided", "ldb_not_multiple_of_8"} <= per_entry["cm3p_gemm_bf16"] & per_entry["cm3p_gemm_bf16_batched"]
    assert {"epilogue_3", "epilogue_4", "epilogue_6", "epilogue_2_without_R", "epilogue_5_without_R", "epilogue_7_without_R", "bias_epilogue_k_strided_a_kc",
            "bf16_resid_N_mod_8_is_4", "split_k_without_workspace", "split_k_epilogue_0", "split_k_ldc_not_N", "N_not_multiple_of_4"} <= per_entry["cm3p_gemm_bf16"]
    assert {"rope_cols_not_multiple_of_64", "rope_cols_past_N", "q_scale_0", "M_not_multiple_of_S_without_per_batch"} <= per_entry["cm3p_qkv_gemm_rope"]
    assert {"199_tiles", "T_not_multiple_of_8", "I_not_multiple_of_32", "K_not_multiple_of_64"} <= per_entry["cm3p_gemm_geglu"]
    assert {"batch_0", "batch_65536", "stride_r_not_multiple_of_8"} <= per_entry["cm3p_gemm_bf16_batched"]
    for name, label, base, broken in CASES:  # one argument of the entry point's own, away from the value that passes
        (p, v), = broken.items()
        start = dict(VALID[name], **base)
        assert p in ENTRIES[name] and set(base) <= set(ENTRIES[name]) and p not in base and start[p] != v, (name, label)


@pytest.mark.parametrize("name,label,base,broken", CASES, ids=[f"{n}-{l}" for n, l, _, _ in CASES])
def test_one_broken_precondition_is_refused(name, label, base, broken):
    from cm3p_amd import _lib

    start = dict(VALID[name], **base)
    args = [broken.get(p, start[p]) for p in ENTRIES[name]]
    assert args != [start[p] for p in ENTRIES[name]]  # (an unbroken list would reach a launch)
    assert getattr(_lib.load(), name)(*args) == ERR_INVALID
