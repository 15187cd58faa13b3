"""tests/mlm_topk_refs.py on the CPU: the acceptance rule is attainable (a torch fp32 restatement of the kernel's path - tile maxima,
per-tile candidates, ascending merge - passes the calls tests/test_mlm_topk_kernels_gpu.py makes) and sharp (each wrong evaluation fails
them); the share of rows with an ambiguous rank stays under its cap over the seam set; include/ext/predict/cm3p_mlm_topk.h, the
library's exports and _lib.MLM_TOPK_SIGNATURES name the same functions; every refusal happens before a HIP call; the workspace formula
is the restated one."""
import ctypes
import os
import re

import pytest
import torch

import mlm_topk_refs as TR
from mlm_topk_refs import check, gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "predict", "cm3p_mlm_topk.h")
SHAPES = ((129, 5, 8), (130, 129, 72), (300, 200, 64), (65, 3167, 136), (40, 300, 72))  # (T, V, H)


def _fails(what, fn):
    with pytest.raises(AssertionError):
        fn()
    print(f"{what}: refused")


# ================================================================================================ the rule: attainable and sharp
@pytest.mark.parametrize("T,V,H", SHAPES)
@pytest.mark.parametrize("bias", (True, False))
def test_restatement_fits_and_wrong_evaluations_do_not(T, V, H, bias):
    k = 8
    y, W, b = TR.topk_case(T, V, H, gen("host topk", T, V, H, bias), bias=bias)
    ref = TR.topk_ref(y, W, b, V, k)
    idx, val, lse = TR.topk_f32_path(y, W, b, V, k)
    TR.check_topk(idx, val, ref, "top-k")
    check(lse, ref["lse"], ref["lse_b"], "lse")
    if V < k:
        assert bool((idx[:, V:] == -1).all()) and bool((idx[:, :V].sort(1).values == torch.arange(V)).all())
    if TR.vp_of(V) > V:
        w = TR.topk_f32_path(y, W, b, V, k, wrong="pad_as_logits")
        _fails("a pad column treated as a logit", lambda: TR.check_topk(w[0], w[1], ref, "top-k"))
        w = TR.topk_f32_path(y, W, b, V, k, wrong="lse_over_vp")
        TR.check_topk(w[0], w[1], ref, "top-k")  # (only lse is wrong)
        _fails("lse over Vp instead of V", lambda: check(w[2], ref["lse"], ref["lse_b"], "lse"))
    if V > k:
        w = TR.topk_f32_path(y, W, b, V, k, wrong="rank_shift")
        _fails("rank k + 1 returned at rank k", lambda: TR.check_topk(w[0], w[1], ref, "top-k"))
    if k <= V <= 200:  # (at most two tiles, the first with most of the columns: some row has its k winners in it)
        assert any(len({c // TR.TILE for c in row}) == 1 for row in ref["cols"][:, :k].tolist())
        w = TR.topk_f32_path(y, W, b, V, k, wrong="merge_drops_kth")
        _fails("the merge dropping a tile's k-th candidate", lambda: TR.check_topk(w[0], w[1], ref, "top-k"))
    for kk in (1, 5):  # the first kk ranks of the k = 8 answer are the k = kk answer
        r2 = TR.topk_ref(y, W, b, V, kk)
        i2, v2, _ = TR.topk_f32_path(y, W, b, V, kk)
        TR.check_topk(i2, v2, r2, f"top-{kk}")
        n = min(kk, V)
        assert bool((i2[:, :n] == idx[:, :n]).all())


@pytest.mark.parametrize("V,H", ((5, 8), (129, 8), (200, 16), (1100, 8)))
def test_exact_rows_and_ties(V, H):
    k = 8
    y, W, kinds = TR.exact_case(V, H, gen("host topk exact", V, H))
    ref = TR.topk_ref(y, W, None, V, k, exact=True)
    idx, val, lse = TR.topk_f32_path(y, W, None, V, k)
    TR.check_exact(idx, val, ref, "exact")
    TR.check_topk(idx, val, ref, "exact")
    check(lse, ref["lse"], ref["lse_b"], "lse")
    n = min(k, V)
    assert idx[kinds.index("all equal"), :n].tolist() == list(range(n))
    if V > k:
        assert idx[kinds.index("winners at 0 and V - 1"), :2].tolist() == [V - 1, 0]
    for c in (63, 127):
        if f"equal maxima at {c} and {c + 1}" in kinds:
            assert idx[kinds.index(f"equal maxima at {c} and {c + 1}"), :3].tolist() == [c, c + 1, 0]
    if "winners 128 columns apart" in kinds:
        assert sorted(idx[kinds.index("winners 128 columns apart")].tolist()) == [5 + 128 * t for t in range(8)]
    w = TR.topk_f32_path(y, W, None, V, k, wrong="ties_high")
    _fails("ties to the higher column", lambda: TR.check_exact(w[0], w[1], ref, "exact"))
    if V > 1:  # an exact tie is an ambiguous rank of the float64 rule; what refuses the wrong order there is check_exact
        assert TR.ambiguous_rows(ref) >= 1


def test_ambiguous_rows_stay_under_the_cap_over_the_seam_set():
    """The exact index comparison is skipped only at ambiguous ranks; over SEAM_T x CAP_V x SEAM_H at k = 8 fewer than AMBIGUOUS_CAP of
    the rows have one.  From the reference alone."""
    rows = amb = 0
    for T in TR.SEAM_T:
        for V in TR.CAP_V:
            for H in TR.SEAM_H:
                y, W, b = TR.topk_case(T, V, H, gen("topk", T, V, H, True), bias=True)
                ref = TR.topk_ref(y, W, b, V, 8)
                rows += T
                amb += TR.ambiguous_rows(ref)
    print(f"{amb} of {rows} rows hold an ambiguous rank ({100.0 * amb / rows:.2f} %)")
    assert rows == 19180 and amb <= TR.AMBIGUOUS_CAP * rows


# ================================================================================================ header, exports, binding
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from cm3p_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_binding_name_the_same_functions(lib):
    from cm3p_amd import _lib

    text, names = _declared()
    assert names == sorted(_lib.MLM_TOPK_SIGNATURES) and len(names) == 3
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    for name, argtypes in _lib.MLM_TOPK_SIGNATURES.items():
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        params = m.group(2).strip()
        assert (0 if params in ("", "void") else params.count(",") + 1) == len(argtypes), name
        assert (m.group(1) == "int64_t") == (getattr(lib, name).restype is ctypes.c_int64), name
    assert lib.cm3p_mlm_topk_abi_version() == _lib.MLM_TOPK_ABI_VERSION == 1
    assert int(re.search(r"#define CM3P_MLM_TOPK_ABI_VERSION (\d+)", text).group(1)) == 1
    # the core header's and the loss extension's tables hold none of these names (tests/test_cabi.py pins their ABI numbers)
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.MLM_LOSS_SIGNATURES))


def test_workspace_formula(lib):
    for T, Vp in ((0, 64), (1, 64), (127, 128), (129, 192), (300, 3200), (131072, 3200), (65536, 50368), (33000, 65600)):
        for k in (1, 5, 8):
            assert lib.cm3p_mlm_topk_workspace_bytes(T, Vp, k) == TR.workspace_bytes(T, Vp, k)
    assert TR.workspace_bytes(2048, 4096, 8) * 64 == 2048 * 4096 * 4 * 9  # 9 / 64 of the fp32 logits: 14 %
    for T, Vp, k in ((-1, 64, 5), (4, 0, 5), (4, 96, 5), (4, -64, 5), (4, 64, 0), (4, 64, 9), (4, 64, -1)):
        assert lib.cm3p_mlm_topk_workspace_bytes(T, Vp, k) == -1


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    """NULL tensors, k outside 1..8, V > Vp, shapes outside the header's, misaligned buffers and an undersized workspace answer
    CM3P_ERR_INVALID (-1); every address is an aligned one that is never dereferenced."""
    fake = 4096
    T, H, V, Vp, k = 300, 72, 200, 256, 5
    a = dict(y=fake, W=fake, bias=fake, T=T, H=H, V=V, Vp=Vp, k=k, idx=fake, val=fake, lse=fake, ws=fake, nws=TR.workspace_bytes(T, Vp, k), stream=None)

    def f(**kw):
        c = dict(a, **kw)
        return lib.cm3p_mlm_topk(c["y"], c["W"], c["bias"], c["T"], c["H"], c["V"], c["Vp"], c["k"], c["idx"], c["val"], c["lse"], c["ws"], c["nws"],
                                 c["stream"])

    ptrs = ("y", "W", "idx", "val", "lse", "ws")
    for p in ptrs:
        assert f(**{p: None}) == -1, (p, "NULL")
    for p in ptrs + ("bias",):
        assert f(**{p: fake + 8}) == -1, (p, "misaligned")
    assert f(k=0) == -1 and f(k=9) == -1 and f(k=-3) == -1
    assert f(V=Vp + 1) == -1 and f(V=0) == -1
    assert f(Vp=Vp + 32) == -1 and f(Vp=0, V=0) == -1
    assert f(H=H + 4) == -1 and f(H=0) == -1
    assert f(T=-1) == -1
    assert f(nws=a["nws"] - 1) == -1
    assert f(k=8) == -1  # (the workspace of k = 5 is too small for k = 8)
    # T = 0 is a valid call that launches nothing (and touches none of the addresses); so is a NULL bias
    assert f(T=0, nws=0) == 0 and f(T=0, nws=0, bias=None) == 0
