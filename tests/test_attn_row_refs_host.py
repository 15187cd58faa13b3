"""tests/attn_row_refs.py on the CPU - the emulation of the single-query kernels' roundings passes every check, deliberately wrong
evaluations fail them - and the extension C ABI of include/cm3p_attn_row.h (_lib.ROW_SIGNATURES): header, exports and binding one to
one, every host refusal through ctypes, the ledger of its entry points.  (The kernels: tests/test_attn_row_kernels_gpu.py, `-m gpu`.)"""
import ctypes
import os
import re

import pytest
import torch

import attn_row_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_HEADER = os.path.join(ROOT, "include", "cm3p_attn_row.h")

# Which test checks each entry point of cm3p_attn_row.h against a reference (the rule of tests/test_kernel_ledger.py), or why none does.
LEDGER = {
    "cm3p_attn_row_fwd": ["tests/test_attn_row_kernels_gpu.py::test_row_kernels_against_float64",
                          "tests/test_attn_row_kernels_gpu.py::test_row_forward_agrees_with_row_0_of_the_full_forward"],
    "cm3p_attn_row_bwd": ["tests/test_attn_row_kernels_gpu.py::test_row_kernels_against_float64",
                          "tests/test_attn_row_kernels_gpu.py::test_row_backward_agrees_with_the_full_backward_fed_a_one_row_dout"],
}
EXEMPT = {
    "cm3p_attn_row_abi_version": "host-only constant; test_row_header_exports_and_binding_match_one_to_one compares it with the binding",
}


# ---- the reference against itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.BY_NAME))
def test_emulation_passes_every_check(name):
    case = R.BY_NAME[name]
    ref, got = R.reference(case), R.emulate(case)
    seen, fails = R.check_float64(ref, got, rel_l2=not case.peaked)
    seen2, fails2 = R.check_conditioned(case, got)
    assert not fails + fails2 + R.check_exact(case, ref, got), (name, seen, seen2)


def test_table_covers_what_the_kernels_branch_on():
    t = R.TABLE
    assert {c.S for c in t} >= set(R.SEQ) and {c.nh for c in t} == {1, 3} and {c.pre for c in t} == {False, True}
    for S in (65, 257):
        assert {c.window for c in t if c.S == S and c.mask == "none" and not c.packed} >= {-1, 0, 1, 63, 64, 65, S}
    assert {c.rope for c in t} == {None, "shared", "batch"} and {c.rope for c in t if c.packed} == {None, "batch"}
    assert any(c.mask == "pad" and 1 in c.lens for c in t) and any(c.mask == "key0" for c in t) and any(c.packed and c.lens == (1, 70, 257) for c in t)
    dead = [c for c in t if bool(R.reference(c)["dead"].any())]
    assert {c.mask for c in dead} == {"dead", "key0"}  # a fully masked sequence; window 0 with key 0 masked
    for c in t:
        if c.mask == "key0" and c.window != 0:
            assert not bool(R.reference(c)["dead"].any())


def _fails(case, wrong):
    ref, got = R.reference(case), R.emulate(case, wrong)
    return R.check_float64(ref, got, rel_l2=not case.peaked)[1] + R.check_conditioned(case, got)[1] + R.check_exact(case, ref, got)


def test_wrong_window_edge_fails():
    for S in (65, 257):
        for w in (w for w in (0, 1, 63, 64, 65) if w + 1 < S):  # (a window that already covers every key has no edge to miss)
            case = next(c for c in R.TABLE if c.S == S and c.window == w and c.mask == "none" and not c.packed)
            assert _fails(case, "window_off_by_one"), case.name


def test_delta_from_an_unrounded_out_fails():
    for case in (c for c in R.TABLE if c.peaked):
        fails = _fails(case, "delta_unrounded")
        assert fails and all("given_out" in f for f in fails), (case.name, fails)  # (closer to float64, but not the published delta)


def test_dq_without_the_q_scale_chain_fails():
    cases = [c for c in R.TABLE if c.pre and c.mask == "none" and c.window < 0 and not c.packed and c.S > 1]
    assert cases
    for case in cases:
        assert any(f.startswith("dq") for f in _fails(case, "dq_without_q_scale")), case.name


def test_rotation_applied_forward_fails():
    cases = [c for c in R.TABLE if c.rope and c.mask == "none" and c.S > 1 and c.window != 0]  # (one visible key: dS = 0, nothing to rotate)
    assert {c.rope for c in cases} == {"shared", "batch"}
    for case in cases:
        assert _fails(case, "rotation_not_inverted"), case.name


def test_nonzero_dk_on_a_padded_key_fails():
    for case in (c for c in R.TABLE if c.mask == "pad" or (c.window >= 0 and c.window < c.S - 1)):
        assert any("invisible key" in f for f in _fails(case, "padded_key_dk")), case.name


# ---- the extension ABI --------------------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)  # (the parse of tests/test_cabi.py)
    return sorted(set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text))), text


@pytest.fixture(scope="module")
def lib():
    from cm3p_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_row_header_exports_and_binding_match_one_to_one(lib):
    from cm3p_amd import _lib

    names, text = _declared(ROW_HEADER)
    assert names == sorted(_lib.ROW_SIGNATURES) and len(names) == 3
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    for name, argtypes in _lib.ROW_SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(argtypes), (name, n, len(argtypes))
        assert name not in _lib._RETURNS_INT64
    assert lib.cm3p_attn_row_abi_version() == _lib.ATTN_ROW_ABI_VERSION == int(re.search(r"#define CM3P_ATTN_ROW_ABI_VERSION (\d+)", text).group(1))
    assert not set(_lib.ROW_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))


def test_cm3p_hip_h_abi_20_and_ext_signatures_are_unchanged(lib):
    from cm3p_amd import _lib

    names, text = _declared(os.path.join(ROOT, "include", "cm3p_hip.h"))
    assert names == sorted(_lib.SIGNATURES) and not [n for n in names if "attn_row" in n]
    assert _lib.ABI_VERSION == 20 == lib.cm3p_abi_version() and "#define CM3P_ABI_VERSION 20" in text
    ext, _ = _declared(os.path.join(ROOT, "include", "cm3p_lora.h"))
    assert ext == sorted(_lib.EXT_SIGNATURES) and len(ext) == 5 and _lib.LORA_ABI_VERSION == 1 == lib.cm3p_lora_abi_version()


def test_row_ledger_covers_the_header_and_names_real_tests():
    names, _ = _declared(ROW_HEADER)
    assert sorted(set(LEDGER) | set(EXEMPT)) == names and not set(LEDGER) & set(EXEMPT)
    assert all(LEDGER.values()) and all(r.strip() for r in EXEMPT.values())
    for ids in LEDGER.values():
        for tid in ids:
            path, fn = tid.split("::")
            assert re.search(r"^def " + fn + r"\(", open(os.path.join(ROOT, path)).read(), flags=re.M), tid


def test_row_source_is_registered_and_stays_out_of_the_bounds_audit():
    from cm3p_amd import build, isa_check

    assert "attention_row.hip" in build.SOURCES and "attention_row.hip" in isa_check.CHECKS
    assert "attention_row.hip" not in build.AUDIT_SOURCES  # no LDS-DMA in it
    assert "global_load_lds" not in open(os.path.join(build.CSRC, "attention_row.hip")).read()


def test_row_entries_refuse_bad_arguments_before_any_hip_call(lib):
    """Every refusal answers CM3P_ERR_INVALID (-1) on the host: this process never initialises a GPU, the pointers are never read."""
    P = 0x10000  # a 16-byte aligned, never dereferenced "device" address
    f = dict(qkv=P, out=P + 0x1000, lse=P + 0x2000, key_mask=None, cu=None, B=2, S=8, total=0, nh=1, window=-1, scale=0.125, pre=0)
    b = dict(f, dout=P + 0x3000, dqkv=P + 0x4000, cos=None, sin=None, pbs=0)

    def fwd(**kw):
        a = dict(f, **kw)
        return lib.cm3p_attn_row_fwd(a["qkv"], a["out"], a["lse"], a["key_mask"], a["cu"], a["B"], a["S"], a["total"], a["nh"], a["window"], a["scale"],
                                     a["pre"], None)

    def bwd(**kw):
        a = dict(b, **kw)
        return lib.cm3p_attn_row_bwd(a["qkv"], a["out"], a["dout"], a["lse"], a["dqkv"], a["key_mask"], a["cu"], a["B"], a["S"], a["total"], a["nh"],
                                     a["window"], a["scale"], a["cos"], a["sin"], a["pbs"], a["pre"], None)

    common = [dict(qkv=None), dict(out=None), dict(lse=None), dict(qkv=P + 8), dict(out=P + 2), dict(lse=P + 4), dict(B=0), dict(S=0), dict(nh=0),
              dict(B=-1), dict(scale=0.0), dict(key_mask=P + 0x5000, cu=P + 0x6000, total=16), dict(cu=P + 0x6000, total=0), dict(cu=P + 0x6002, total=16)]
    for kw in common:
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    for kw in (dict(dout=None), dict(dqkv=None), dict(dout=P + 8), dict(dqkv=P + 8), dict(cos=P + 0x7000), dict(sin=P + 0x7000),
               dict(cos=P + 0x7004, sin=P + 0x8000), dict(cos=P + 0x7000, sin=P + 0x8000, pbs=3)):
        assert bwd(**kw) == -1, kw
