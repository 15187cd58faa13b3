"""tests/mlm_loss_refs.py on the CPU: every bound is attainable (a torch fp32 restatement of the kernels' path passes the same `check`
calls tests/test_mlm_loss_kernels_gpu.py makes) and sharp (each wrong evaluation fails them); include/ext/cm3p_mlm_loss.h, the
library's exports and _lib.MLM_LOSS_SIGNATURES name the same functions; every refusal of the two entry points happens before a HIP
call; the workspace formulas are the restated ones."""
import ctypes
import math
import os
import re

import pytest
import torch

import mlm_loss_refs as MR
from mlm_loss_refs import IGNORE, check, gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "cm3p_mlm_loss.h")
SHAPES = ((129, 5, 8), (130, 129, 72), (300, 200, 64), (65, 3167, 136))  # (T, V, H)


def _fails(what, fn):
    with pytest.raises(AssertionError):
        fn()
    print(f"{what}: refused")


# ================================================================================================ bounds: attainable and sharp
@pytest.mark.parametrize("T,V,H", SHAPES)
@pytest.mark.parametrize("bias", (True, False))
def test_lse_restatement_fits_and_wrong_sums_do_not(T, V, H, bias):
    y, W, b, lab = MR.mlm_case(T, V, H, gen("host mlm", T, V, H, bias), bias=bias)
    ref = MR.lse_ref(y, W, b, V, lab)
    loss, lse = MR.lse_f32_path(y, W, b, V, lab)
    check(lse, ref["lse"], ref["lse_b"], "lse")
    check(loss, ref["loss"], ref["loss_b"], "loss")
    dead = ~ref["live"]
    assert dead.any() and ref["live"].any() and not (loss[dead] != 0).any() and not (lse[dead] != 0).any()
    assert bool(torch.isnan(y.float()[dead]).all())  # (the rows that take no part hold NaN)
    # the bound is the fp32 logits' error and a few units of the fp32 spacing, not a tolerance: logits of size 10 from H products
    assert float(ref["loss_b"].max()) < 2 * H * 2.0 ** -24 * 400 + 1e-4
    w = MR.lse_f32_path(y, W, b, V, lab, wrong="target_neighbour")[0]
    _fails("the target's logit from the neighbouring column", lambda: check(w, ref["loss"], ref["loss_b"], "loss"))
    if MR.vp_of(V) > V:
        w = MR.lse_f32_path(y, W, b, V, lab, wrong="pad_as_logits")[1]
        _fails("pad columns read as logits", lambda: check(w, ref["lse"], ref["lse_b"], "lse"))


@pytest.mark.parametrize("V,H", ((129, 8), (200, 16), (3167, 72)))
@pytest.mark.parametrize("bias", (True, False))
def test_exact_rows_fit_without_a_gemm_term_and_have_the_losses_they_are_named_for(V, H, bias):
    y, W, b, lab, kinds = MR.exact_case(V, H, gen("host exact", V, H, bias), bias=bias)
    ref = MR.lse_ref(y, W, b, V, lab, exact=True)
    loss, lse = MR.lse_f32_path(y, W, b, V, lab)
    check(lse, ref["lse"], ref["lse_b"], "lse")
    check(loss, ref["loss"], ref["loss_b"], "loss")
    assert float(ref["loss_b"].max()) < 1e-4  # lse up to 100, loss up to 200: a few 1e-5
    if not bias:
        for r, k in enumerate(kinds):
            if k == "all equal":
                assert abs(float(ref["loss"][r]) - math.log(V)) < 1e-12
            elif k.endswith("target on the +100"):
                assert 0 <= float(ref["loss"][r]) < 1e-80 and float(ref["loss_b"][r]) > 5e-6
            elif k.endswith("target on a -100"):
                assert abs(float(ref["loss"][r]) - 200.0) < 1e-12
    assert int(lab[kinds.index("target at column 0")]) == 0 and int(lab[kinds.index("target at column cols - 1")]) == V - 1
    assert int(lab[-1]) // MR.TILE == (V - 1) // MR.TILE and V % MR.TILE != 0  # the last tile is a partial one
    sel = torch.tensor([k.startswith("one +100") or k.startswith("all about") for k in kinds])
    w = MR.lse_f32_path(y, W, b, V, lab, wrong="no_max")[1]
    _fails("lse without the max shift", lambda: check(w[sel], ref["lse"][sel], ref["lse_b"][sel], "lse"))
    w = MR.lse_f32_path(y, W, b, V, lab, wrong="pad_as_logits")[1]
    _fails("pad columns read as logits", lambda: check(w, ref["lse"], ref["lse_b"], "lse"))


@pytest.mark.parametrize("T,V,H", SHAPES)
@pytest.mark.parametrize("bias", (True, False))
def test_dlogits_restatement_fits_and_wrong_gradients_do_not(T, V, H, bias):
    y, W, b, lab = MR.mlm_case(T, V, H, gen("host mlm dl", T, V, H, bias), bias=bias)
    _, lse = MR.lse_f32_path(y, W, b, V, lab)
    n = int((lab != IGNORE).sum())
    for sa in (0.37, -2.0, 0.0):
        sa, sb = float(torch.tensor(sa, dtype=torch.float32)), float(torch.tensor(1.0 / n, dtype=torch.float32))
        ref = MR.dlogits_ref(y, W, b, V, lab, lse.double(), sa, sb)
        dl, colsum = MR.dlogits_f32_path(y, W, b, V, lab, lse, sa, sb)
        check(dl, ref["g"], ref["dl_b"], f"dl s=({sa:.3g}, 1/n)")
        check(colsum, ref["colsum"], ref["colsum_b"], f"colsum s=({sa:.3g}, 1/n)")
        assert not (dl[~ref["live"]].float() != 0).any() and not (dl[:, V:].float() != 0).any()
        if sa == 0:
            assert not (dl.float() != 0).any()
            continue
        w = MR.dlogits_f32_path(y, W, b, V, lab, lse, sa, sb, wrong="colsum_of_rounded")[1]
        _fails("colsum of the bf16 values", lambda: check(w, ref["colsum"], ref["colsum_b"], "colsum"))
        if MR.vp_of(V) > V:
            w = MR.dlogits_f32_path(y, W, b, V, lab, lse, sa, sb, wrong="pad_as_logits")[0]
            _fails("a gradient on the pad columns", lambda: check(w, ref["g"], ref["dl_b"], "dl"))


def test_accumulate_bound_covers_two_halves():
    T, V, H = 300, 200, 64
    y, W, b, lab = MR.mlm_case(T, V, H, gen("host mlm acc"), bias=True)
    _, lse = MR.lse_f32_path(y, W, b, V, lab)
    sa, sb = 0.37, float(torch.tensor(1.0 / int((lab != IGNORE).sum()), dtype=torch.float32))
    sa = float(torch.tensor(sa, dtype=torch.float32))
    h = 128
    first = MR.dlogits_f32_path(y[:h], W, b, V, lab[:h], lse[:h], sa, sb)[1]
    both = MR.dlogits_f32_path(y[h:], W, b, V, lab[h:], lse[h:], sa, sb, colsum0=first)[1]
    ref = MR.dlogits_ref(y, W, b, V, lab, lse.double(), sa, sb, colsum0=torch.zeros(MR.vp_of(V), dtype=torch.float64))
    check(both, ref["colsum"], ref["colsum_b"], "colsum of two halves")


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
    assert names == sorted(_lib.MLM_LOSS_SIGNATURES) and len(names) == 5
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    for name, argtypes in _lib.MLM_LOSS_SIGNATURES.items():
        m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        params = m.group(2).strip()
        assert (0 if params in ("", "void") else params.count(",") + 1) == len(argtypes), name
        assert (m.group(1) == "int64_t") == (getattr(lib, name).restype is ctypes.c_int64), name
    assert lib.cm3p_mlm_loss_abi_version() == _lib.MLM_LOSS_ABI_VERSION == 1
    assert int(re.search(r"#define CM3P_MLM_LOSS_ABI_VERSION (\d+)", text).group(1)) == 1
    # the core header and its table are not touched by the extension
    assert not set(names) & set(_lib.SIGNATURES) and _lib.ABI_VERSION == 20


def test_workspace_formulas(lib):
    for T, Vp in ((0, 64), (1, 64), (127, 128), (129, 192), (300, 3200), (131072, 3200), (65536, 50368), (33000, 65600)):
        assert lib.cm3p_mlm_lse_workspace_bytes(T, Vp) == MR.lse_workspace_bytes(T, Vp) <= T * Vp // 8
        assert lib.cm3p_mlm_dlogits_workspace_bytes(T, Vp) == MR.dlogits_workspace_bytes(T, Vp)
    for T, Vp in ((-1, 64), (4, 0), (4, 96), (4, -64)):
        assert lib.cm3p_mlm_lse_workspace_bytes(T, Vp) == -1 and lib.cm3p_mlm_dlogits_workspace_bytes(T, Vp) == -1
    assert MR.chunk_rows(3200) == 41856 and MR.chunk_rows(50368) == 2560 and MR.chunk_rows(2 ** 21) == 128


def test_entry_points_refuse_bad_arguments_before_any_hip_call(lib):
    """NULL tensors, V > Vp, shapes outside the header's, misaligned buffers and an undersized workspace answer CM3P_ERR_INVALID (-1);
    every address is an aligned one that is never dereferenced."""
    fake = 4096
    T, H, V, Vp = 300, 72, 200, 256
    a = dict(y=fake, W=fake, bias=fake, target=fake, ignore=-100, lse=fake, sa=fake, sb=fake, T=T, H=H, V=V, Vp=Vp, loss=fake, dl=fake, colsum=fake,
             acc=0, ws=fake, ws_lse=MR.lse_workspace_bytes(T, Vp), ws_dl=MR.dlogits_workspace_bytes(T, Vp), stream=None)

    def lse(**kw):
        k = dict(a, **kw)
        return lib.cm3p_mlm_lse(k["y"], k["W"], k["bias"], k["target"], k["ignore"], k["T"], k["H"], k["V"], k["Vp"], k["loss"], k["lse"], k["ws"],
                                k["ws_lse"], k["stream"])

    def dlg(**kw):
        k = dict(a, **kw)
        return lib.cm3p_mlm_dlogits(k["y"], k["W"], k["bias"], k["target"], k["ignore"], k["lse"], k["sa"], k["sb"], k["T"], k["H"], k["V"], k["Vp"],
                                    k["dl"], k["colsum"], k["acc"], k["ws"], k["ws_dl"], k["stream"])

    for f, ptrs in ((lse, ("y", "W", "target", "loss", "lse", "ws")), (dlg, ("y", "W", "target", "lse", "sa", "sb", "dl", "colsum", "ws"))):
        for p in ptrs:
            assert f(**{p: None}) == -1, (f.__name__, p, "NULL")
        for p in ptrs + ("bias",):
            if p not in ("sa", "sb"):  # (the two scalars are single floats)
                assert f(**{p: fake + 8}) == -1, (f.__name__, p, "misaligned")
        assert f(V=Vp + 1) == -1 and f(V=0) == -1
        assert f(Vp=Vp + 32) == -1 and f(Vp=0, V=0) == -1
        assert f(H=H + 4) == -1 and f(H=0) == -1
        assert f(T=-1) == -1
    assert lse(ws_lse=a["ws_lse"] - 1) == -1
    assert dlg(ws_dl=a["ws_dl"] - 1) == -1
    # T = 0 is a valid call that launches nothing (and touches none of the addresses)
    assert lse(T=0, ws_lse=0) == 0 and dlg(T=0, ws_dl=0) == 0
