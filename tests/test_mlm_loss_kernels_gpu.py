"""cm3p_mlm_lse and cm3p_mlm_dlogits (include/ext/cm3p_mlm_loss.h) through the C ABI against the float64 references and derived
bounds of tests/mlm_loss_refs.py: every row, column and k seam of the 128 x 128 x 64 tile with and without a bias, rows with exact
logits, pad rows of W and pad entries of the bias that would read as inf, ignored rows whose y holds NaN (one whole row tile of them),
guarded buffers, repeatable bits, the accumulate flag, and one shape whose [T, Vp] offsets pass 2^31 elements.
tests/test_mlm_loss_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

Each check prints its largest error / bound (`pytest -rP`)."""
import pytest
import torch

import mlm_loss_refs as MR
from mlm_loss_refs import IGNORE, bits_equal, check, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64          # sentinel elements before and after a caller-owned output
SENTINEL = 777.0    # (exact in bf16)


def _guarded(n, dtype):
    """A NaN-filled flat output of n elements between two runs of GUARD sentinels (n elements keep the start 16-byte aligned)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    out = buf[GUARD:GUARD + n]
    assert out.data_ptr() % 16 == 0
    return buf, out


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _dev_scalar(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


class _Run:
    """One set of operands on the device; lse() and dlogits() call the C entry points into guarded, NaN-filled buffers and check that
    everything inside was written and nothing outside."""

    def __init__(self, y, W, b, lab, V):
        from cm3p_amd import _lib

        self.L = _lib
        self.T, self.H = y.shape
        self.V, self.Vp = V, W.shape[0]
        self.y, self.W, self.lab = y.to(DEV), W.to(DEV), lab.to(DEV)
        self.b = b.to(DEV) if b is not None else None

    def _done(self, bufs):
        torch.cuda.synchronize()
        for name, buf, t in bufs:
            assert _intact(buf, t.numel()), f"{name}: a store outside the buffer"
            assert not torch.isnan(t.float()).any(), f"{name}: an element was left unwritten (or is NaN)"

    def lse(self):
        L, T = self.L, self.T
        lo_b, loss = _guarded(T, torch.float32)
        ls_b, lse = _guarded(T, torch.float32)
        nws = L.query("cm3p_mlm_lse_workspace_bytes", T, self.Vp)
        assert nws == MR.lse_workspace_bytes(T, self.Vp)
        ws_b, ws = _guarded(nws // 4, torch.float32)
        L.call("cm3p_mlm_lse", L.ptr(self.y), L.ptr(self.W), L.ptr(self.b), L.ptr(self.lab, torch.int64), IGNORE, T, self.H, self.V, self.Vp,
               L.ptr(loss), L.ptr(lse), L.ptr(ws), nws, L.stream())
        self._done((("loss_rows", lo_b, loss), ("lse_rows", ls_b, lse)))
        assert _intact(ws_b, ws.numel()), "workspace: a store outside the buffer"
        return loss, lse

    def dlogits(self, lse, sa, sb, rows=None, colsum=None, accumulate=False):
        L = self.L
        r0, r1 = rows if rows is not None else (0, self.T)
        n = r1 - r0
        dl_b, dl = _guarded(n * self.Vp, torch.bfloat16)
        if colsum is None:
            cs_b, colsum = _guarded(self.Vp, torch.float32)
        else:
            cs_b = None
        nws = L.query("cm3p_mlm_dlogits_workspace_bytes", n, self.Vp)
        assert nws == MR.dlogits_workspace_bytes(n, self.Vp)
        ws_b, ws = _guarded(nws // 4, torch.float32)
        L.call("cm3p_mlm_dlogits", L.ptr(self.y[r0:r1]), L.ptr(self.W), L.ptr(self.b), L.ptr(self.lab[r0:r1], torch.int64), IGNORE, L.ptr(lse[r0:r1]),
               L.ptr(sa), L.ptr(sb), n, self.H, self.V, self.Vp, L.ptr(dl), L.ptr(colsum), int(accumulate), L.ptr(ws), nws, L.stream())
        self._done((("dlogits", dl_b, dl), ("workspace", ws_b, ws)) + ((("colsum", cs_b, colsum),) if cs_b is not None else ()))
        return dl.view(n, self.Vp), colsum


def _check_case(y, W, b, lab, V, tag, exact=False):
    run = _Run(y, W, b, lab, V)
    ref = MR.lse_ref(y, W, b, V, lab, exact=exact)
    loss, lse = run.lse()
    check(lse, ref["lse"], ref["lse_b"], f"lse {tag}")
    check(loss, ref["loss"], ref["loss_b"], f"loss {tag}")
    dead = (~ref["live"]).to(DEV)
    assert not (loss.view(torch.int32)[dead] != 0).any() and not (lse.view(torch.int32)[dead] != 0).any(), "loss_rows / lse_rows of a dead row are not +0"
    loss2, lse2 = run.lse()
    bits_equal(loss2, loss.cpu(), "loss_rows again")
    bits_equal(lse2, lse.cpu(), "lse_rows again")
    n = max(int((lab != IGNORE).sum()), 1)
    sa, sb = _dev_scalar(0.37), _dev_scalar(1.0 / n)
    dref = MR.dlogits_ref(y, W, b, V, lab, lse.cpu().double(), float(sa), float(sb), exact=exact)
    dl, colsum = run.dlogits(lse, sa, sb)
    check(dl, dref["g"], dref["dl_b"], f"dl {tag}")
    check(colsum, dref["colsum"], dref["colsum_b"], f"colsum {tag}")
    bits = dl.view(torch.int16)
    assert not (bits[:, V:] != 0).any() and not (bits[dead] != 0).any(), "dead rows / pad columns of dlogits are not +0"
    assert not (colsum[V:].view(torch.int32) != 0).any()
    dl2, colsum2 = run.dlogits(lse, sa, sb)
    bits_equal(dl2, dl.cpu(), "dlogits again")
    bits_equal(colsum2, colsum.cpu(), "colsum again")
    return run, lse, sa, sb, dref, dl, colsum


# ================================================================================================ seams
@pytest.mark.parametrize("V", MR.SEAM_V)
@pytest.mark.parametrize("T", MR.SEAM_T)
def test_every_row_column_and_k_seam_with_and_without_bias(T, V):
    for H in MR.SEAM_H:
        for bias in (True, False):
            y, W, b, lab = MR.mlm_case(T, V, H, gen("mlm", T, V, H, bias), bias=bias)
            assert MR.vp_of(V) == V or bool((W[V:].float() > 2.9e38).all())  # (PAD_VALUE as bf16 rounds it)
            _check_case(y, W, b, lab, V, f"{T}x{V}x{H} bias={bias}")


@pytest.mark.parametrize("V,H", ((129, 8), (200, 16), (3167, 72)))
@pytest.mark.parametrize("bias", (False, True))
def test_rows_with_exact_logits(V, H, bias):
    y, W, b, lab, kinds = MR.exact_case(V, H, gen("mlm exact", V, H, bias), bias=bias)
    _, lse, *_ = _check_case(y, W, b, lab, V, f"exact {V}x{H} bias={bias}", exact=True)
    if not bias:  # an all-equal row of a bf16-representable value: lse = v + log V to the last fp32 bits' bound, and never inf
        assert bool(torch.isfinite(lse).all())


def test_a_whole_row_tile_ignored_leaves_zeros_and_the_rest_unaffected():
    T, V, H = 300, 200, 72
    g = gen("mlm ignored tile")
    y, W, b, lab = MR.mlm_case(T, V, H, g, ignored_tile=1)
    assert bool((lab[128:256] == IGNORE).all()) and bool(torch.isnan(y[128:256].float()).all())
    assert {int(lab[2]), int(lab[3]), int(lab[4])} == {V, -5, IGNORE}  # a label == V, a negative label other than -100, ignore_index
    run, lse, sa, sb, dref, dl, colsum = _check_case(y, W, b, lab, V, "ignored tile")
    assert not (dl[128:256].view(torch.int16) != 0).any()
    # the same live rows without the ignored tile between them: their results do not depend on it, in bits
    keep = torch.cat((torch.arange(0, 128), torch.arange(256, T)))
    run2 = _Run(y[keep], W, b, lab[keep], V)
    loss2, lse2 = run2.lse()
    bits_equal(lse2, lse.cpu()[keep], "lse_rows without the ignored tile")
    dl2, _ = run2.dlogits(lse2, sa, sb)
    bits_equal(dl2, dl.cpu()[keep], "dlogits without the ignored tile")


def test_accumulate_sums_two_halves_of_the_rows():
    T, V, H = 300, 200, 64
    y, W, b, lab = MR.mlm_case(T, V, H, gen("mlm acc"), bias=True)
    run = _Run(y, W, b, lab, V)
    _, lse = run.lse()
    sa, sb = _dev_scalar(-2.0), _dev_scalar(1.0 / int((lab != IGNORE).sum()))
    cs_b, colsum = _guarded(run.Vp, torch.float32)
    dl_a, _ = run.dlogits(lse, sa, sb, rows=(0, 128), colsum=colsum, accumulate=False)
    first = colsum.clone()
    dl_b, _ = run.dlogits(lse, sa, sb, rows=(128, T), colsum=colsum, accumulate=True)
    torch.cuda.synchronize()
    assert _intact(cs_b, run.Vp)
    ref = MR.dlogits_ref(y, W, b, V, lab, lse.cpu().double(), float(sa), float(sb), colsum0=torch.zeros(run.Vp, dtype=torch.float64))
    check(colsum, ref["colsum"], ref["colsum_b"], "colsum of two halves")
    check(torch.cat((dl_a, dl_b)), ref["g"], ref["dl_b"], "dl of two halves")
    assert bool((colsum != first).any())
    # the row chunks write the rows the whole call writes
    dl, _ = run.dlogits(lse, sa, sb)
    bits_equal(torch.cat((dl_a, dl_b)), dl.cpu(), "dlogits in two chunks")


def test_offsets_past_2_to_31_elements():
    """T = 33000, V = Vp = 65600, H = 8: the last row starts 2.16e9 elements into dlogits.  Rows 0, 1, T - 2 and T - 1 are live."""
    from cm3p_amd import _lib as L

    T, V, H = 33000, 65600, 8
    assert (T - 1) * V > 2 ** 31 and MR.vp_of(V) == V
    g = gen("mlm 2^31")
    live = torch.tensor([0, 1, T - 2, T - 1])
    yl = torch.randn(4, H, generator=g).to(torch.bfloat16)
    W = (torch.randn(V, H, generator=g) * 3 / H ** 0.5).to(torch.bfloat16)
    b = torch.randn(V, generator=g)
    labl = torch.tensor([0, V - 1, int(torch.randint(0, V, (1,), generator=g)), V - 1])
    y = torch.full((T, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    y[live.to(DEV)] = yl.to(DEV)
    lab = torch.full((T,), IGNORE, dtype=torch.int64, device=DEV)
    lab[live.to(DEV)] = labl.to(DEV)
    lab[7], lab[T - 9] = V, -5
    Wd, bd = W.to(DEV), b.to(DEV)
    loss = torch.full((T,), float("nan"), device=DEV)
    lse = torch.full((T,), float("nan"), device=DEV)
    nws = L.query("cm3p_mlm_lse_workspace_bytes", T, V)
    ws = torch.empty((nws,), dtype=torch.uint8, device=DEV)
    L.call("cm3p_mlm_lse", L.ptr(y), L.ptr(Wd), L.ptr(bd), L.ptr(lab), IGNORE, T, H, V, V, L.ptr(loss), L.ptr(lse), L.ptr(ws), nws, L.stream())
    ref = MR.lse_ref(yl, W, b, V, labl)
    check(lse[live.to(DEV)], ref["lse"], ref["lse_b"], "lse of the four live rows")
    check(loss[live.to(DEV)], ref["loss"], ref["loss_b"], "loss of the four live rows")
    assert not (lse[2:T - 2].view(torch.int32) != 0).any() and not (loss[2:T - 2].view(torch.int32) != 0).any()
    del ws
    sa, sb = _dev_scalar(0.37), _dev_scalar(0.25)
    dl_buf, dl = _guarded(T * V, torch.bfloat16)
    colsum = torch.full((V,), float("nan"), device=DEV)
    nws = L.query("cm3p_mlm_dlogits_workspace_bytes", T, V)
    ws = torch.empty((nws,), dtype=torch.uint8, device=DEV)
    L.call("cm3p_mlm_dlogits", L.ptr(y), L.ptr(Wd), L.ptr(bd), L.ptr(lab), IGNORE, L.ptr(lse), L.ptr(sa), L.ptr(sb), T, H, V, V, L.ptr(dl),
           L.ptr(colsum), 0, L.ptr(ws), nws, L.stream())
    torch.cuda.synchronize()
    assert _intact(dl_buf, T * V), "dlogits: a store outside the buffer"
    dl = dl.view(T, V)
    dref = MR.dlogits_ref(yl, W, b, V, labl, lse[live.to(DEV)].cpu().double(), float(sa), float(sb))
    check(dl[live.to(DEV)], dref["g"], dref["dl_b"], "dl of the four live rows")
    assert bool((dl[T - 1] != 0).any())
    # colsum is the four rows' sum; its bound counts the depth of all ceil(T / 128) row tiles (the others add exact zeros)
    cs_b = dref["colsum_b"] + (MR.colsum_depth(T) - MR.colsum_depth(4)) * MR.U * dref["g"].abs().sum(0) * MR.SECOND
    check(colsum, dref["colsum"], cs_b, "colsum of the four live rows")
    assert not bool(dl[2:T - 2].view(torch.int16).any()), "the zero fill of the ignored rows"
    for r in (2, 7, 127, 128, 16500, T - 9, T - 3):  # a sample of ignored rows, read back
        assert not (dl[r].cpu().view(torch.int16) != 0).any(), r
