"""cm3p_mlm_topk (include/ext/predict/cm3p_mlm_topk.h) through the C ABI against the float64 reference and the acceptance rule of
tests/mlm_topk_refs.py: every row, column and k seam of the 128 x 128 x 64 tile with and without a bias at k = 8, the model's vocabulary
at k = 1, 5 and 8, pad rows of W and pad entries of the bias that would read as inf, rows with exact logits (ties, winners at the
edges, in one tile and one per tile, a vocabulary smaller than k), guarded buffers and repeatable bits.
tests/test_mlm_topk_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

Each check prints its largest error / bound (`pytest -rP`)."""
import pytest
import torch

import mlm_topk_refs as TR
from mlm_topk_refs import bits_equal, check, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64          # sentinel elements before and after a caller-owned output
SENTINEL = 777


def _guarded(n, dtype):
    """A flat output of n elements filled with NaN (int32: a value no result takes) between two runs of GUARD sentinels."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = float("nan") if dtype.is_floating_point else -(2 ** 31)
    out = buf[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    return buf, out


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _topk(y, W, b, V, k):
    """One call into guarded buffers -> (idx [T, k], val [T, k], lse [T]); everything inside was written, nothing outside."""
    from cm3p_amd import _lib as L

    T, H = y.shape
    Vp = W.shape[0]
    yd, Wd = y.to(DEV), W.to(DEV)
    bd = b.to(DEV) if b is not None else None
    ib, idx = _guarded(T * k, torch.int32)
    vb, val = _guarded(T * k, torch.float32)
    lb, lse = _guarded(T, torch.float32)
    nws = L.query("cm3p_mlm_topk_workspace_bytes", T, Vp, k)
    assert nws == TR.workspace_bytes(T, Vp, k)
    wb, ws = _guarded(nws // 4, torch.float32)
    L.call("cm3p_mlm_topk", L.ptr(yd), L.ptr(Wd), L.ptr(bd), T, H, V, Vp, k, L.ptr(idx), L.ptr(val), L.ptr(lse), L.ptr(ws), nws, L.stream())
    torch.cuda.synchronize()
    for name, buf, t in (("top_idx", ib, idx), ("top_val", vb, val), ("lse_rows", lb, lse), ("workspace", wb, ws)):
        assert _intact(buf, t.numel()), f"{name}: a store outside the buffer"
    assert not torch.isnan(val).any() and not torch.isnan(lse).any() and not bool((idx == -(2 ** 31)).any()), "an element was left unwritten"
    return idx.view(T, k), val.view(T, k), lse


def _check_case(y, W, b, V, k, tag, exact=False):
    ref = TR.topk_ref(y, W, b, V, k, exact=exact)
    idx, val, lse = _topk(y, W, b, V, k)
    TR.check_topk(idx, val, ref, f"top-{k} {tag}")
    check(lse, ref["lse"], ref["lse_b"], f"lse {tag}")
    idx2, val2, lse2 = _topk(y, W, b, V, k)
    bits_equal(idx2, idx.cpu(), "top_idx again")
    bits_equal(val2, val.cpu(), "top_val again")
    bits_equal(lse2, lse.cpu(), "lse_rows again")
    return ref, idx, val, lse


# ================================================================================================ seams
@pytest.mark.parametrize("V", TR.SEAM_V)
@pytest.mark.parametrize("T", TR.SEAM_T)
def test_every_row_column_and_k_seam_with_and_without_bias(T, V):
    for H in TR.SEAM_H:
        for bias in (True, False):
            y, W, b = TR.topk_case(T, V, H, gen("topk", T, V, H, bias), bias=bias)
            assert TR.vp_of(V) == V or (bool((W[V:].float() > 2.9e38).all()) and (b is None or bool((b[V:] > 2.9e38).all())))
            _check_case(y, W, b, V, 8, f"{T}x{V}x{H} bias={bias}")


@pytest.mark.parametrize("k", (1, 5, 8))
def test_the_model_vocabulary(k):
    T, V, H = 300, 3167, 72
    y, W, b = TR.topk_case(T, V, H, gen("topk", T, V, H, True), bias=True)
    ref, idx, val, _ = _check_case(y, W, b, V, k, f"{T}x{V}x{H} k={k}")
    if k == 1:  # argmax of the float64 logits wherever the first gap is wider than the bounds
        sure = ~ref["amb"][:, 0]
        assert bool((idx.cpu()[sure, 0] == ref["x"].argmax(1)[sure]).all()) and int(sure.sum()) > T * 0.95


# ================================================================================================ exact rows
@pytest.mark.parametrize("V,H", ((5, 8), (129, 8), (200, 16), (1100, 8)))
@pytest.mark.parametrize("k", (1, 5, 8))
def test_rows_with_exact_logits(V, H, k):
    y, W, kinds = TR.exact_case(V, H, gen("topk exact", V, H))
    ref = TR.topk_ref(y, W, None, V, k, exact=True)
    idx, val, lse = _topk(y, W, None, V, k)
    TR.check_exact(idx, val, ref, f"exact {V}x{H} k={k}")
    check(lse, ref["lse"], ref["lse_b"], f"lse exact {V}x{H}")
    assert bool(torch.isfinite(lse).all())
    idx = idx.cpu()
    n = min(k, V)
    assert idx[kinds.index("all equal"), :n].tolist() == list(range(n))
    if V < k:
        assert bool((idx[:, V:] == -1).all()) and bool((val.cpu()[:, V:] == float("-inf")).all())
    assert idx[kinds.index("winners at 0 and V - 1"), :2].tolist() == [V - 1, 0][:k]
    for c in (63, 127):
        if f"equal maxima at {c} and {c + 1}" in kinds:
            assert idx[kinds.index(f"equal maxima at {c} and {c + 1}"), :3].tolist() == [c, c + 1, 0][:k]
    if "winners in 8 adjacent columns" in kinds:
        assert set(idx[kinds.index("winners in 8 adjacent columns")].tolist()) <= set(range(16, 24))
    if "winners 128 columns apart" in kinds:
        assert set(idx[kinds.index("winners 128 columns apart")].tolist()) <= {5 + 128 * t for t in range(8)}
