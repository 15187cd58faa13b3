"""tests/attn_qrows_refs.py on the CPU - the emulation of the query-list kernels' roundings passes every check, deliberately wrong
evaluations fail them, the table holds every condition tests/test_attn_qrows_kernels_gpu.py states - and the extension C ABI of
include/cm3p_attn_qrows.h (_lib.QROWS_SIGNATURES): header, exports and binding one to one, every host refusal through ctypes, the
ledger of its entry points.  (The kernels: tests/test_attn_qrows_kernels_gpu.py, `-m gpu`.)"""
import ctypes
import os
import re

import pytest
import torch

import attn_qrows_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cm3p_attn_qrows.h")
KG = "tests/test_attn_qrows_kernels_gpu.py::"

# Which test checks each entry point of cm3p_attn_qrows.h against a reference (the rule of tests/test_kernel_ledger.py), or why none does.
LEDGER = {
    "cm3p_attn_qrows_fwd": [KG + "test_qrows_kernels_against_float64", KG + "test_every_row_listed_agrees_with_the_full_kernels",
                            KG + "test_row_0_only_agrees_with_the_single_query_kernels"],
    "cm3p_attn_qrows_bwd": [KG + "test_qrows_kernels_against_float64", KG + "test_every_row_listed_agrees_with_the_full_kernels",
                            KG + "test_row_0_only_agrees_with_the_single_query_kernels",
                            KG + "test_backward_agrees_with_the_full_backward_fed_a_dout_that_is_zero_off_the_list"],
}
EXEMPT = {
    "cm3p_attn_qrows_abi_version": "host-only constant; test_qrows_header_exports_and_binding_match_one_to_one compares it with the binding",
}


# ---- the reference against itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.BY_NAME))
def test_emulation_passes_every_check(name):
    case = R.BY_NAME[name]
    ref, got = R.reference(case), R.emulate(case)
    seen, fails = R.check_float64(ref, got, rel_l2=not case.peaked)
    seen2, fails2 = R.check_conditioned(case, got)
    assert not fails + fails2 + R.check_exact(case, ref, got), (name, seen, seen2)


def test_table_holds_every_condition_the_gpu_test_states():
    t = R.TABLE
    assert {c.S for c in t} == set(R.SEQS) and {c.window for c in t} == set(R.WINDOWS) and {c.pre for c in t} == {False, True}
    assert {len(R.positions(c, b)) for c in t for b in range(R.B)} >= set(R.COUNTS)
    for pre in (False, True):
        assert {c.rope is not None for c in t if c.pre == pre} == {False, True}
    assert {c.rope for c in t} == {None, "shared", "batch"}
    kinds = {k for c in t for k in c.kinds if isinstance(k, str)}
    assert kinds >= {"row0", "last", "all", "third", "padq", "far", "none"}
    for S in R.SEQS:  # row 0 only and every row listed, at every length the cross-checks run on
        assert any(c.S == S and "all" in c.kinds for c in t)
    assert any(c.kinds == ("row0", "row0") and c.window < 0 for c in t) and any(c.kinds == ("row0", "row0") and c.window >= 0 for c in t)
    # a padded query: listed, its own key masked, and still alive
    for c in (c for c in t if "padq" in c.kinds):
        pos, km, ref = c.S // 2, R.key_mask(c), R.reference(c)
        assert pos in R.positions(c, 0) and not bool(km[0, pos]) and not bool(ref["dead"][0, 0, pos])
    # a sliding-layer query more than `window` past the last valid key: listed and without a visible key; every other listed query is alive
    far = [c for c in t if "far" in c.kinds]
    assert far and all(c.window >= 0 for c in far)
    for c in t:
        ref = R.reference(c)
        dl = ref["listed"] & ref["dead"]
        if "far" in c.kinds:
            b = c.kinds.index("far")
            past = [p for p in R.positions(c, b) if p > c.lens[b] - 1 + c.window]
            assert c.lens[b] + c.window in past and len(past) < len(R.positions(c, b))
            assert bool(dl[b, 0, past].all()) and int(dl[:, 0].sum()) == len(past)
        else:
            assert not bool(dl.any()), c.name
    # a sequence with no query beside one with 129; in the packed form a zero-length sequence, first and last
    assert any({len(R.positions(c, b)) for b in range(R.B)} == {0, 129} for c in t)
    packed = [c for c in t if c.packed]
    assert {c.lens.index(0) for c in packed if 0 in c.lens} == {0, 1} and any(0 not in c.lens for c in packed)
    assert any(c.peaked and c.pre for c in t) and any(c.peaked and not c.pre for c in t)
    # every case has a list whose positions differ from their indices (pos_as_index is a different function) unless it lists a prefix
    for c in t:
        rows, qcu, qmax = R.row_list(c)
        assert rows == sorted(set(rows)) and qcu[-1] == len(rows) and qmax == max(b - a for a, b in zip(qcu, qcu[1:]))


def _fails(case, wrong):
    ref, got = R.reference(case), R.emulate(case, wrong)
    return R.check_float64(ref, got, rel_l2=not case.peaked)[1] + R.check_conditioned(case, got)[1] + R.check_exact(case, ref, got)


def test_masking_a_padded_query_fails():
    cases = [c for c in R.TABLE if "padq" in c.kinds]
    assert {c.window < 0 for c in cases} == {False, True}
    for case in cases:
        assert _fails(case, "padded_query_masked"), case.name


def test_taking_the_list_index_as_the_position_fails():
    cases = [c for c in R.TABLE if 0 <= c.window < c.S and any(R.positions(c, b) != tuple(range(len(R.positions(c, b)))) for b in range(R.B))]
    assert {c.window for c in cases} == {0, 16, 64} and any(c.packed for c in cases)
    for case in cases:
        assert _fails(case, "pos_as_index"), case.name


def test_the_row_0_window_rule_fails():
    cases = [c for c in R.TABLE if 0 <= c.window < c.S - 1 and any(p > 0 for b in range(R.B) for p in R.positions(c, b))]
    assert {c.window for c in cases} == {0, 16, 64}
    for case in cases:
        assert _fails(case, "row0_rule"), case.name


def test_dk_dv_summed_over_all_queries_fails():
    cases = [c for c in R.TABLE if not c.peaked and any(0 < len(R.positions(c, b)) < R.seq_len(c, b) for b in range(R.B))]
    assert len(cases) >= 10
    for case in cases:
        fails = _fails(case, "dkdv_all_queries")
        assert any(f.startswith("dk") for f in fails) and any(f.startswith("dv") for f in fails), (case.name, fails)


def test_a_q_third_that_is_not_zeroed_off_the_list_fails():
    cases = [c for c in R.TABLE if not c.peaked and any(0 < len(R.positions(c, b)) < R.seq_len(c, b) for b in range(R.B))]
    for case in cases:
        assert any("q third" in f for f in _fails(case, "q_third_not_zeroed")), case.name


def test_delta_from_an_unrounded_out_fails():
    cases = [c for c in R.TABLE if c.peaked]
    assert cases
    for case in cases:
        fails = _fails(case, "delta_unrounded")
        assert fails and all("given_out" in f for f in fails), (case.name, fails)  # (closer to float64, but not the published delta)


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


def test_qrows_header_exports_and_binding_match_one_to_one(lib):
    from cm3p_amd import _lib

    names, text = _declared(HEADER)
    assert names == sorted(_lib.QROWS_SIGNATURES) and len(names) == 3
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    for name, argtypes in _lib.QROWS_SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(argtypes), (name, n, len(argtypes))
        assert name not in _lib._RETURNS_INT64
    assert lib.cm3p_attn_qrows_abi_version() == _lib.ATTN_QROWS_ABI_VERSION == int(re.search(r"#define CM3P_ATTN_QROWS_ABI_VERSION (\d+)", text).group(1))
    assert not set(_lib.QROWS_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.ROW_SIGNATURES))


def test_the_other_headers_and_their_versions_are_unchanged(lib):
    from cm3p_amd import _lib

    names, text = _declared(os.path.join(ROOT, "include", "cm3p_hip.h"))
    assert names == sorted(_lib.SIGNATURES) and not [n for n in names if "qrows" in n]
    assert _lib.ABI_VERSION == 20 == lib.cm3p_abi_version() and "#define CM3P_ABI_VERSION 20" in text
    row, _ = _declared(os.path.join(ROOT, "include", "cm3p_attn_row.h"))
    assert row == sorted(_lib.ROW_SIGNATURES) and _lib.ATTN_ROW_ABI_VERSION == 1 == lib.cm3p_attn_row_abi_version()


def test_qrows_ledger_covers_the_header_and_names_real_tests():
    names, _ = _declared(HEADER)
    assert sorted(set(LEDGER) | set(EXEMPT)) == names and not set(LEDGER) & set(EXEMPT)
    assert all(LEDGER.values()) and all(r.strip() for r in EXEMPT.values())
    for ids in LEDGER.values():
        for tid in ids:
            path, fn = tid.split("::")
            assert re.search(r"^def " + fn + r"\(", open(os.path.join(ROOT, path)).read(), flags=re.M), tid


def test_qrows_source_is_registered_and_stays_out_of_the_bounds_audit():
    from cm3p_amd import build

    assert "attention_qrows.hip" in build.SOURCES and "attention_qrows.hip" not in build.AUDIT_SOURCES  # no LDS-DMA in it
    assert "global_load_lds" not in open(os.path.join(build.CSRC, "attention_qrows.hip")).read()


def test_qrows_entries_refuse_bad_arguments_before_any_hip_call(lib):
    """Every refusal answers CM3P_ERR_INVALID (-1) on the host: this process never initialises a GPU, the pointers are never read."""
    P = 0x10000  # a 16-byte aligned, never dereferenced "device" address
    f = dict(qkv=P, out=P + 0x1000, lse=P + 0x2000, key_mask=None, cu=None, qrows=P + 0x9000, qcu=P + 0xa000, n=4, qmax=2, B=2, S=8, total=16, nh=1,
             window=-1, scale=0.125, pre=0)
    b = dict(f, dout=P + 0x3000, dqkv=P + 0x4000, cos=None, sin=None, pbs=0)

    def fwd(**kw):
        a = dict(f, **kw)
        return lib.cm3p_attn_qrows_fwd(a["qkv"], a["out"], a["lse"], a["key_mask"], a["cu"], a["qrows"], a["qcu"], a["n"], a["qmax"], a["B"], a["S"],
                                       a["total"], a["nh"], a["window"], a["scale"], a["pre"], None)

    def bwd(**kw):
        a = dict(b, **kw)
        return lib.cm3p_attn_qrows_bwd(a["qkv"], a["out"], a["dout"], a["lse"], a["dqkv"], a["key_mask"], a["cu"], a["qrows"], a["qcu"], a["n"], a["qmax"],
                                       a["B"], a["S"], a["total"], a["nh"], a["window"], a["scale"], a["cos"], a["sin"], a["pbs"], a["pre"], None)

    common = [dict(qkv=None), dict(out=None), dict(lse=None), dict(qrows=None), dict(qcu=None), dict(qkv=P + 8), dict(out=P + 2), dict(lse=P + 4),
              dict(qrows=P + 0x9002), dict(qcu=P + 0xa001), dict(B=0), dict(S=0), dict(nh=0), dict(B=-1), dict(n=-1), dict(qmax=0), dict(qmax=-3),
              dict(scale=0.0), dict(scale=-1.0), dict(total=0), dict(total=17), dict(key_mask=P + 0x5000, cu=P + 0x6000), dict(cu=P + 0x6002)]
    for kw in common:
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    for kw in (dict(dout=None), dict(dqkv=None), dict(dout=P + 8), dict(dqkv=P + 8), dict(cos=P + 0x7000), dict(sin=P + 0x7000),
               dict(cos=P + 0x7004, sin=P + 0x8000), dict(cos=P + 0x7000, sin=P + 0x8000, pbs=3)):
        assert bwd(**kw) == -1, kw
    assert fwd(n=0, qmax=0, out=None, lse=None, qrows=None) == 0  # an empty list is valid: the forward launches nothing
