"""The bounds of tests/test_row_kernels_gpu.py, checked without a GPU: a torch fp32 evaluation on the CPU that walks the kernel's
addition path (tests/row_kernel_refs.py: elementwise IEEE operations in the kernel's order) goes through the same reference and
bound functions and must pass - the bound is attainable - and a deliberately wrong evaluation must fail - the bound is sharp
enough to see the mistake."""
import pytest
import torch

import row_kernel_refs as R
from row_kernel_refs import FTZ, U, check, gen


def _fails(got, ref, bound, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        check(got, ref, bound, what)


def _ln_rows(H, g):
    return torch.cat([torch.randn(7, H, generator=g) * 2 + 0.5, R.ln_special_rows(H, g)])


@pytest.mark.parametrize("H", [4, 260, 768, 1028, 2048])
def test_layernorm_forward_bounds_hold_for_the_fp32_path_and_refuse_wrong_statistics(H):
    g = gen("host-lnf", H)
    x = _ln_rows(H, g)
    w = 1 + 0.2 * torch.randn(H, generator=g)
    for xx in (x, x.to(torch.bfloat16).float()):
        ref = R.ln_fwd_ref(xx.double(), w.double())
        y, mean, rstd = R.ln_fwd_f32_path(xx, w)
        check(mean, ref["mean"], ref["mean_b"], "mean")
        check(rstd, ref["rstd"], ref["rstd_b"], "rstd")
        check(y, ref["y"], ref["y_b"], "y")
        check(y.to(torch.bfloat16), ref["y"], R.bf16_bound(ref["y"], ref["y_b"]), "y bf16")
        # the mean over H - 1 columns
        y, mean, rstd = R.ln_fwd_f32_path(xx, w, wrong="mean_h_minus_1")
        _fails(mean[:7], ref["mean"][:7], ref["mean_b"][:7], "mean over H - 1 columns")
        _fails(y[:7], ref["y"][:7], ref["y_b"][:7], "y with the mean over H - 1 columns")
    # E[x^2] - mean^2 on the rows whose mean is 10^4 times their spread (fp32 x; in bf16 row 0 collapses to a constant)
    ref = R.ln_fwd_ref(x.double(), w.double())
    y, mean, rstd = R.ln_fwd_f32_path(x, w, wrong="one_pass")
    if H >= 260:  # (four values of spread 0.1 around 1000 are too few for a variance to speak of)
        _fails(rstd[7:8], ref["rstd"][7:8], ref["rstd_b"][7:8], "rstd of a one-pass variance, large-mean row")
        _fails(y[7:8], ref["y"][7:8], ref["y_b"][7:8], "y of a one-pass variance, large-mean row")
        _fails(rstd[8:9], ref["rstd"][8:9], ref["rstd_b"][8:9], "rstd of a one-pass variance, large-mean row on the bf16 grid")
    check(rstd[:7], ref["rstd"][:7], ref["rstd_b"][:7] * 64, "(on the usual rows a one-pass variance is only a little worse)")


@pytest.mark.parametrize("H", [260, 768, 1792])
def test_layernorm_backward_bounds_hold_for_the_fp32_path_and_refuse_a_lost_row(H):
    g = gen("host-lnb", H)
    x = _ln_rows(H, g)
    n = x.shape[0]
    w = 1 + 0.2 * torch.randn(H, generator=g)
    _, mean, rstd = R.ln_fwd_f32_path(x, w)
    fwd64 = R.ln_fwd_ref(x.double(), w.double())
    for dy in (torch.randn(n, H, generator=g), torch.randn(n, H, generator=g).to(torch.bfloat16).float()):
        for dres in (None, torch.randn(n, H, generator=g)):
            ref = R.ln_bwd_ref(dy.double(), x.double(), w.double(), mean.double(), rstd.double(), None if dres is None else dres.double())
            dx, dw = R.ln_bwd_f32_path(dy, x, w, mean, rstd, dres)
            check(dx, ref["dx"], ref["dx_b"], "dx")
            # (the walk adds the 13 rows one after another: 3 + 13 roundings, inside the kernel's count for 13 rows)
            c = R.ln_dw_c(n, R.ln_bwd_blocks(n))
            assert c >= 3 + n
            check(dw, ref["p"].sum(0), c * U * ref["p"].abs().sum(0) * R.SECOND + FTZ, "dw")
            _, dw_bad = R.ln_bwd_f32_path(dy, x, w, mean, rstd, dres, wrong="dw_drops_a_row")
            _fails(dw_bad, ref["p"].sum(0), c * U * ref["p"].abs().sum(0) * R.SECOND + FTZ, "dw without one row")
            if dres is not None:
                r64 = R.ln_bwd_ref(dy.double(), x.double(), w.double(), fwd64["mean"], fwd64["rstd"], dres.double())
                dx_s, p_s = R.ln_bwd_stats_slack(fwd64, r64, dy.double())
                check(dx, r64["dx"], r64["dx_b"] + dx_s, "dx, float64 statistics")
                check(dw, r64["p"].sum(0), c * U * r64["p"].abs().sum(0) * R.SECOND + p_s.sum(0) + FTZ, "dw, float64 statistics")
    # at 4097 rows (beyond the backward's grid) the bound still sees one lost row: the exact sum less one row, rounded to fp32
    rows = 4097
    x = torch.randn(rows, H, generator=g) * 2 + 0.5
    dy = torch.randn(rows, H, generator=g)
    f = R.ln_fwd_ref(x.double(), w.double())
    p = R.ln_bwd_ref(dy.double(), x.double(), w.double(), f["mean"], f["rstd"])["p"]
    c = R.ln_dw_c(rows, R.ln_bwd_blocks(rows))
    bound = c * U * p.abs().sum(0) * R.SECOND + FTZ
    check(p.sum(0).float(), p.sum(0), bound, f"dw at {rows} rows (c = {c})")
    _fails((p.sum(0) - p[rows // 2]).float(), p.sum(0), bound, f"dw at {rows} rows without one of them")


@pytest.mark.parametrize("H,S", [(128, 300), (1028, 129), (4, 4096)])
def test_pooling_bounds_hold_for_the_fp32_path_and_refuse_a_masked_row(H, S):
    g = gen("host-pool", H, S)
    Bn = 3
    for h in (torch.randn(Bn, S, H, generator=g) + 0.25, (torch.randn(Bn, S, H, generator=g) + 0.25).to(torch.bfloat16).float()):
        mask = (torch.rand(Bn, S, generator=g) < 0.5).long()
        mask[0, 0], mask[0, 1] = 1, 0
        mask[2] = 0  # a row with no kept position
        for m in (None, mask):
            ref, cnt, bnd = R.pool_ref(h.double(), m, False)
            check(R.pool_fwd_f32_path(h, m), ref, bnd, f"pool mask {m is not None}")
        _fails(R.pool_fwd_f32_path(h, mask, wrong="counts_a_masked_row"), ref, bnd, "pool that counts a masked row")
        ref, _, bnd = R.pool_ref(h.double(), mask, True)
        check(h[:, 0], ref, bnd, "cls")
        _fails(h[:, 1], ref, bnd, "cls from the wrong row")


@pytest.mark.parametrize("T,I", [(64, 64), (5, 1152)])
def test_geglu_bounds_hold_for_the_fp32_path_and_refuse_tanh_gelu_and_swapped_halves(T, I):
    g = gen("host-geglu", T, I)
    h = R.geglu_h(T, I, g)
    dg = torch.randn(T, I, generator=g).to(torch.bfloat16)
    ref, bnd = R.geglu_fwd_ref(h.double())
    check(R.geglu_fwd_f32_path(h), ref, bnd, "geglu fwd")
    _fails(R.geglu_fwd_f32_path(h, wrong="tanh"), ref, bnd, "tanh GELU")
    _fails(R.geglu_fwd_f32_path(h, wrong="swapped"), ref, bnd, "halves swapped")
    ref, bnd = R.geglu_bwd_ref(dg.double(), h.double())
    got = R.geglu_bwd_f32_path(dg, h)
    check(got, ref, bnd, "geglu bwd")
    _fails(torch.cat([got[:, I:], got[:, :I]], 1), ref, bnd, "gradient halves swapped")


def test_half_ulp_of_bf16():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.999, 2.0, 3e-3, -0.75, 0.0], dtype=torch.float64)
    hu = R.half_ulp_bf16(v)
    assert hu[0].item() == 2.0 ** -8 and hu[2].item() == 2.0 ** -8 and hu[3].item() == 2.0 ** -7 and hu[5].item() == 2.0 ** -9
    # every float64 rounds to bf16 within half an ulp of itself, and some reach it (1 + 2^-8 is a tie)
    x = torch.randn(100000, generator=gen("hu"), dtype=torch.float64) * 10
    err = (x.float().to(torch.bfloat16).double() - x).abs()
    assert (err <= R.half_ulp_bf16(x) * (1 + 2.0 ** -15)).all()  # (the intermediate fp32 rounding adds half an fp32 ulp, 2^-16 of a bf16 one)
    assert (v[1].float().to(torch.bfloat16).double() - v[1]).abs().item() == hu[1].item()
    assert (err > 2.0 ** -9 * x.abs()).any()  # the relative form 2^-9 |x| is not a bound
