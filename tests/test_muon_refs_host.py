"""The references, bounds and case tables of tests/test_muon_kernels_gpu.py, checked without a GPU: the fp32 path restatements of
tests/muon_refs.py pass every check the GPU test makes on every case, the restated block count and the Newton-Schulz routes agree
with the library's own answers (cm3p_muon_partials, cm3p_gemm_route), every wrong evaluation a kernel could fall into fails the check
named for it, and the pinned oracle's step (oracle/muon_oracle.py, exact=True) agrees with the meanings stated here within the
fixture tolerances of tests/test_muon_gpu.py."""
import functools
import os
import sys

import pytest
import torch

import muon_refs as MR
from muon_refs import MOMENTUM, bits_equal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

NEG_LR = -0.02
ALIGNED = [1, 0]
NESTEROV = [True, False]


def _fails_bits(fn):
    with pytest.raises(AssertionError, match="elements differ"):
        fn()


def _fails(fn):
    with pytest.raises(AssertionError, match="outside the bound"):
        fn()


def _n_host(rows, cols):
    """The large case runs one matrix here (the three differ only in their data)."""
    return 1 if rows * cols > 100000 else MR.N_MAT


@functools.lru_cache(maxsize=None)
def _stage(rows, cols, kind, nesterov, aligned16):
    """The three stage kernels' path restatements chained as cm3p_amd.muon chains them -> everything the checks take."""
    n = _n_host(rows, cols)
    g, buf, p = (t[:n] for t in MR.stage_data(rows, cols, kind))
    vec = MR.is_vec(cols, aligned16)
    buf2, u, x = MR.momentum_f32_path(g, buf, MOMENTUM, nesterov)
    parts = torch.stack([MR.partials_f32_path(x[i], rows, cols, vec) for i in range(n)])
    img = torch.zeros(n, MR.up8(rows), MR.up8(cols), dtype=torch.bfloat16)
    img[:, :rows, :cols] = x
    xn = MR.normalize_f32_path(img, parts)
    return dict(n=n, g=g, buf=buf, p=p, vec=vec, buf2=buf2, u=u, x=x, parts=parts, img=img, xn=xn)


# ================================================================================================ the tables and the library
def test_block_count_and_partition_are_the_librarys():
    from cm3p_amd import _lib

    for rows, cols in MR.STAGE_SHAPES:
        assert MR.n_partials(rows, cols) == _lib.query("cm3p_muon_partials", rows, cols), (rows, cols)
    for numel, want in ((16384, 1), (16385, 2), (64 * 16384, 64), (64 * 16384 + 1, 64), (1, 1)):
        assert MR.n_partials(1, numel) == _lib.query("cm3p_muon_partials", 1, numel) == want, numel
    # the seams the shapes are there for
    blocks = {s: MR.n_partials(*s) for s in MR.STAGE_SHAPES}
    assert blocks[(128, 128)] == 1 and blocks[(113, 145)] == 2 and blocks[(129, 128)] == 2 and blocks[(1032, 1020)] == 64
    assert 113 * 145 == 16385 and -(-1032 * 1020 // 16384) == 65
    assert MR.up8(21) == 24 and 30 % 4 == 2 and not MR.is_vec(145, 1) and MR.is_vec(128, 1) and not MR.is_vec(128, 0)
    for vec in (True, False):
        per, ranges = MR.partition(1032, 1020, vec)
        assert ranges[0][0] == 0 and ranges[-1][1] == 1032 * 1020 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert 0 < ranges[-1][1] - ranges[-1][0] < ranges[0][1] - ranges[0][0] == per * (4 if vec else 1)  # the last block is short
    # apply (4 elements per thread) and normalise (8) want more than their 128 blocks only at the large shape
    for rows, cols in MR.STAGE_SHAPES:
        big = (rows, cols) == (1032, 1020)
        assert (-(-rows * cols // 1024) > 128) == big and (-(-MR.up8(rows) * MR.up8(cols) // 2048) > 128) == big
    # AdamW: the full launch has 64 blocks and loops; the 65537-element tensor's last pass is a single element; first3 is one block
    assert MR.adamw_stride(max(MR.ADAMW_NUMELS)) == 16384 and 65536 % 16384 == 0 and MR.adamw_stride(1024) == 256
    assert all(abs(w) < 0.5 for w in MR.ADAMW_WEIGHTS[0]) and all(abs(w) >= 0.5 for w in MR.ADAMW_WEIGHTS[1])


def _route(n, M, N, K, lda, ldb, a_kc, b_kc):
    from cm3p_amd import _lib

    code = _lib.query("cm3p_gemm_route", M, N, K, lda, ldb, a_kc, b_kc, MR.EPI_AXPBY, 1, 0, n)
    assert code >= 0, (n, M, N, K)
    return code & 3


def test_newton_schulz_cases_land_on_the_kernels_the_table_states(monkeypatch):
    monkeypatch.delenv("CM3P_GEMM_IMPL", raising=False)
    for n, rows, cols in MR.NS_CASES:
        want = MR.KRING if (n, rows, cols) in MR.NS_RING else MR.K128
        for call in MR.ns_gemm_calls(rows, cols):
            assert _route(n, *call) == want, (n, rows, cols, call)
    assert len(MR.NS_SMALL) == 5 and len(MR.NS_RING) == 2
    for n, _, _ in MR.NS_RING:
        order = MR.ns_ring_order(n)
        assert len(order) == n and order.tolist() != sorted(order.tolist())


def test_restated_constants_are_the_products():
    from cm3p_amd import muon

    assert (MR.NS_A, MR.NS_B, MR.NS_C, MR.NS_EPS) == (muon.NS_A, muon.NS_B, muon.NS_C, muon.NS_EPS)
    assert MR.up8(13) == muon._up8(13) and MR.up8(16) == muon._up8(16)


# ================================================================================================ momentum and partials
@pytest.mark.parametrize("nesterov", NESTEROV)
@pytest.mark.parametrize("rows,cols,kind", MR.STAGE_CASES)
def test_momentum_path_passes_and_wrong_evaluations_fail(rows, cols, kind, nesterov):
    s = _stage(rows, cols, kind, nesterov, 1)
    g, buf = s["g"], s["buf"]
    what = f"{rows}x{cols} {kind} nesterov {nesterov}"
    assert MR.momentum_check(s["buf2"], s["x"], g, buf, MOMENTUM, nesterov, what) <= 1
    if kind == "zero_mat":
        assert not s["x"][MR.ZERO_MAT].any() and not s["buf2"][MR.ZERO_MAT].any()
    if rows * cols < 64:
        return  # (too few elements for every wrong evaluation to show; the next shape up has them)
    for wrong, fails in (("one_rounding", _fails_bits), ("u_is_buf", _fails), ("flag_ignored", _fails), ("trunc", _fails)):
        b2, _, x = MR.momentum_f32_path(g, buf, MOMENTUM, nesterov, wrong=wrong)
        fails(lambda: MR.momentum_check(b2, x, g, buf, MOMENTUM, nesterov, f"{what} {wrong}"))


@pytest.mark.parametrize("aligned16", ALIGNED)
@pytest.mark.parametrize("rows,cols,kind", MR.STAGE_CASES)
def test_partials_path_passes_and_wrong_evaluations_fail(rows, cols, kind, aligned16):
    s = _stage(rows, cols, kind, True, aligned16)
    vec = s["vec"]
    what = f"{rows}x{cols} {kind} vec {vec}"
    for i in range(s["n"]):
        r_blk, r_tot = MR.partials_check(s["parts"][i], s["x"][i], rows, cols, vec, f"{what} [{i}]")
        assert r_blk <= 1 and r_tot <= 1
    i = 0
    for wrong in ("tail_dropped", "block_twice"):
        got = MR.partials_f32_path(s["x"][i], rows, cols, vec, wrong=wrong)
        _fails(lambda: MR.partials_check(got, s["x"][i], rows, cols, vec, f"{what} {wrong}"))
    if kind == "tiny" or rows * cols > 100000:
        got = MR.partials_f32_path(s["x"][i], rows, cols, vec, wrong="sum_of_u2", u=s["u"][i])
        _fails(lambda: MR.partials_check(got, s["x"][i], rows, cols, vec, f"{what} sum of u^2"))


def test_float4_and_scalar_partitions_cover_the_same_elements_and_agree_within_the_bound():
    for rows, cols in ((129, 128), (1032, 1020)):
        a, b = _stage(rows, cols, "normal", True, 1), _stage(rows, cols, "normal", True, 0)
        assert a["vec"] and not b["vec"]
        bits_equal(a["x"], b["x"], "X")
        tot = float(a["x"][0].double().square().sum())
        depth = sum(MR.partials_depth(MR.partition(rows, cols, vec)[0], vec) for vec in (True, False))
        assert abs(float(a["parts"][0].double().sum() - b["parts"][0].double().sum())) <= depth * MR.U * MR.SECOND * tot


# ================================================================================================ normalise
@pytest.mark.parametrize("nesterov", NESTEROV)
@pytest.mark.parametrize("rows,cols,kind", MR.STAGE_CASES)
def test_normalise_path_passes_and_wrong_evaluations_fail(rows, cols, kind, nesterov):
    s = _stage(rows, cols, kind, nesterov, 1)
    what = f"{rows}x{cols} {kind}"
    MR.normalize_check(s["xn"], s["img"], s["parts"], what)
    assert MR.padding_is_zero(s["xn"], rows, cols) and bool(torch.isfinite(s["xn"].float()).all())
    if kind == "zero_mat":
        assert not s["xn"][MR.ZERO_MAT].any()
    else:
        # the normalised image has Frobenius norm 1 up to bf16's roundings - except where eps counts
        nrm = s["xn"].double().flatten(1).norm(dim=1)
        assert bool(((nrm - 1).abs() < 2.0 ** -6).all()) == (kind != "tiny"), nrm
    if rows * cols >= 64:
        _fails_bits(lambda: MR.normalize_check(MR.normalize_f32_path(s["img"], s["parts"], wrong="norm_fp32"), s["img"], s["parts"], what))
    no_eps = MR.normalize_f32_path(s["img"][:1], s["parts"][:1], wrong="no_eps")
    if kind == "tiny":
        _fails_bits(lambda: MR.normalize_check(no_eps, s["img"][:1], s["parts"][:1], f"{what} no eps"))
    else:
        MR.normalize_check(no_eps, s["img"][:1], s["parts"][:1], f"{what} no eps")  # invisible: bf16(norm + 1e-7) = norm
    # A quotient taken in float64 and rounded once is NOT a wrong evaluation here, on any data: X and denom are bf16 numbers, m1 2^e1 and
    # m2 2^e2 with integers m1, m2 < 2^8.  A bf16 tie is t 2^e with an odd integer t < 2^9, and m1 / m2 - t 2^k = (m1 - t m2 2^k) / m2
    # has an integer numerator (after scaling by a power of two): the quotient is either the tie itself or at least 2^-17 of its value
    # away from it.  An fp32 rounding (2^-24) cannot carry it across, so one rounding and two give the same bits - and so does any
    # fp32 division that is good to a few ulp.  Shown on every case instead of being refused.
    MR.normalize_check(MR.normalize_f32_path(s["img"], s["parts"], wrong="quotient_f64"), s["img"], s["parts"], f"{what} quotient from float64")


def test_rne64_bf16_is_one_rounding():
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.7, 1e-8], dtype=torch.float64)
    want = torch.tensor([1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -3.703125, 1e-8], dtype=torch.float64)
    want[4] = float(torch.tensor(1e-8).to(torch.bfloat16))
    assert torch.equal(MR.rne64_bf16(x).double(), want)
    assert float(x[:1].float().to(torch.bfloat16)) == 1.0  # (torch's two-step conversion loses the 2^-30)


# ================================================================================================ apply
@pytest.mark.parametrize("rows,cols,kind", MR.STAGE_CASES)
def test_apply_path_passes_and_wrong_evaluations_fail(rows, cols, kind):
    s = _stage(rows, cols, kind, True, 1)
    p, xn = s["p"], s["xn"]
    what = f"{rows}x{cols} {kind}"
    assert MR.apply_check(MR.apply_f32_path(p, xn, rows, cols, NEG_LR), p, xn, rows, cols, NEG_LR, what) <= 1
    if kind == "zero_mat":
        bits_equal(MR.apply_f32_path(p, xn, rows, cols, NEG_LR)[MR.ZERO_MAT], p[MR.ZERO_MAT], "the all-zero matrix's parameter")

    def wrong(name):
        return lambda: MR.apply_check(MR.apply_f32_path(p, xn, rows, cols, NEG_LR, wrong=name), p, xn, rows, cols, NEG_LR, f"{what} {name}")

    if rows > cols:  # (a scale of 1 needs no rounding)
        _fails(wrong("no_bf16"))
    if cols % 8:
        _fails(wrong("ldx_cols"))
    if MR.shape_scale(rows, cols) != MR.shape_scale(MR.up8(rows), MR.up8(cols)):
        _fails(wrong("padded_scale"))
    if rows * cols >= 10000:
        got = MR.apply_f32_path(p, xn, rows, cols, NEG_LR, wrong="two_roundings")
        x = xn[:, :rows, :cols].double()
        o = (x * float(MR.f32(MR.shape_scale(rows, cols)))).float().to(torch.bfloat16).double()
        ref = float(MR.f32(NEG_LR)) * o + p.double()
        share = float(((got.double() - ref).abs() > MR.half_ulp_f32(ref) + 2.0 ** -52 * ref.abs()).double().mean())
        print(f"{what}: two roundings exceed half an ulp on {share:.5f} of the elements")  # (~ |lr o| / |p|: the product's own rounding)
        assert share * got.numel() >= 3
        _fails(wrong("two_roundings"))
    assert {(r, c) for r, c in MR.STAGE_SHAPES if c % 8} == {(8, 4), (13, 21), (24, 30), (113, 145), (1032, 1020)}


# ================================================================================================ AdamW rule
@pytest.mark.parametrize("decay", MR.ADAMW_DECAYS)
@pytest.mark.parametrize("w", MR.ADAMW_WEIGHTS)
def test_adamw_path_passes_and_wrong_evaluations_fail(w, decay):
    numels = MR.ADAMW_LAUNCHES["all"]
    args = (w[0], w[1], MR.ADAMW_EPS, decay, MR.ADAMW_STEP_ALPHA)
    for (p, g, m1, m2), numel in zip(MR.adamw_data(numels, w), numels):
        what = f"adamw {numel} w {w} decay {decay}"
        assert bool((g == 0).any()) and bool(((g == 0) & (m2 == 0)).any())
        for contract in (False, True):
            pn, a, b = MR.adamw_f32_path(p, g, m1, m2, *args, contract=contract)
            rp, r1, r2, refs = MR.adamw_check(pn, a, b, p, g, m1, m2, *args, f"{what} contract {contract}")
            assert max(rp, r1, r2) <= 1
        for ref, bound in refs.values():  # no bound is wider than the fixture test's tolerance
            assert bool((bound <= 1e-7 + 2e-6 * ref.abs()).all())
        if numel < 255:
            continue
        for wrong in (("decay_after",) if decay != 1.0 else ()) + ("eps_inside", "pass_skipped"):
            pn, a, b = MR.adamw_f32_path(p, g, m1, m2, *args, wrong=wrong, max_numel=max(numels))
            if wrong == "pass_skipped" and numel <= 65536:
                bits_equal(pn, MR.adamw_f32_path(p, g, m1, m2, *args)[0], what)
                continue
            _fails(lambda: MR.adamw_check(pn, a, b, p, g, m1, m2, *args, f"{what} {wrong}"))


# ================================================================================================ one Newton-Schulz iteration
@pytest.mark.parametrize("n,rows,cols", MR.NS_CASES)
def test_newton_schulz_path_passes_and_wrong_evaluations_fail(n, rows, cols):
    ring = (n, rows, cols) in MR.NS_RING
    x = MR.ns_data(n, rows, cols)
    if ring:
        order = MR.ns_ring_order(n)
        first = [int((order == d).nonzero()[0]) for d in range(MR.NS_RING_DISTINCT)]
        for i in range(n):
            assert torch.equal(x[i], x[first[int(order[i])]])
        assert not torch.equal(x[first[0]], x[first[1]]) and not torch.equal(x[first[1]], x[first[2]])
        x = x[:1]  # (one matrix here)
    what = f"ns {n}x{rows}x{cols}"
    assert MR.padding_is_zero(x, rows, cols)
    A, B, Xn = MR.ns_f32_path(x)
    assert max(MR.ns_check(A, B, Xn, x, what)) <= 1
    assert MR.padding_is_zero(Xn, rows, cols)
    bits_equal(A, A.transpose(1, 2).contiguous(), "A is symmetric")

    A2, B2, X2 = MR.ns_f32_path(x, wrong="ca_rounded")
    _fails(lambda: MR.ns_check(A2, B2, X2, x, f"{what} c A rounded"))
    A2, B2, X2 = MR.ns_f32_path(x, wrong="x_from_a")
    _fails(lambda: MR.ns_check(A2, B2, X2, x, f"{what} X' from A"))
    A2, B2, X2 = MR.ns_f32_path(x, wrong="resid_other_buffer", resid_other=torch.zeros_like(x))
    _fails(lambda: MR.ns_check(A2, B2, X2, x, f"{what} residual from the other image"))
    if MR.up8(rows) < MR.up8(cols):
        A2, B2, X2 = MR.ns_f32_path(x, wrong="tall_on_wide")
        _fails(lambda: MR.ns_check(A2, B2, X2, x, f"{what} tall form on a wide weight"))
    # six iterations: finite, padding still zero, singular values drawn towards 1
    for _ in range(5):
        _, _, Xn = MR.ns_f32_path(Xn)
    assert MR.padding_is_zero(Xn, rows, cols) and bool(torch.isfinite(Xn.float()).all())
    if not ring:
        sv = torch.linalg.svdvals(Xn[0, :rows, :cols].float())
        assert 0.3 < float(sv.min()) and float(sv.max()) < 1.7, sv


# ================================================================================================ the pinned oracle
def test_the_oracles_step_agrees_with_the_meanings_stated_here():
    """oracle/muon_oracle.py (exact=True: the reference's bf16 tensor arithmetic, pinned by tests/golden/muon_steps.safetensors) on the
    fixture's shapes and gradients against this file's restatements chained into a step: momentum buffers and the AdamW rule within
    the fixture test's rtol 2e-6 / atol 1e-7, the Muon-branch step within its 6 % (Frobenius)."""
    from muon_cases import SHAPES, VARIANTS, gradients, initial_params

    from oracle import muon_oracle as MO

    named = list(initial_params().items())
    listed = {k for k, _ in MO.split_like_train_py(named)[1]}
    for variant, hp in VARIANTS.items():
        lr, ratio = hp["lrs"][0], hp["adamw_lr"] / hp["lr"]
        b1, b2 = hp["adamw_betas"]
        for k, p0 in named:
            g = gradients(0)[k]
            p_ref, st = p0.clone(), {}
            if MO.routes_to_muon(p0, k in listed):
                rows, cols = g.shape[0], g.numel() // g.shape[0]
                g2 = g.reshape(1, rows, cols)
                buf = torch.randn(1, rows, cols, generator=MR.gen("oracle-buf", k)) * 0.3
                st["momentum_buffer"] = buf[0].clone()
                MO.muon_matrix_update(p_ref, g, st, lr, hp["momentum"], hp["nesterov"], hp["ns_steps"], exact=True)
                buf2, _, x = MR.momentum_f32_path(g2, buf, hp["momentum"], hp["nesterov"])
                torch.testing.assert_close(buf2[0], st["momentum_buffer"], rtol=2e-6, atol=1e-7)
                torch.testing.assert_close((g2.double() * 1 + hp["momentum"] * buf.double())[0].float(), st["momentum_buffer"], rtol=2e-6, atol=1e-7)
                img = torch.zeros(1, MR.up8(rows), MR.up8(cols), dtype=torch.bfloat16)
                img[:, :rows, :cols] = x
                parts = MR.partials_f32_path(x[0], rows, cols, MR.is_vec(cols, 1))[None]
                xi = MR.normalize_f32_path(img, parts)
                for _ in range(hp["ns_steps"]):
                    xi = MR.ns_f32_path(xi)[2]
                p_here = MR.apply_f32_path(p0.reshape(1, rows, cols), xi, rows, cols, -lr)[0].reshape(p0.shape)
                step_ref, step_here = p_ref - p0, p_here - p0
                d = float((step_here - step_ref).norm() / step_ref.norm())
                print(f"{variant} {k}: step {d:.4f} from the oracle's")
                assert d <= 6e-2, (variant, k, d)
            else:
                st = dict(step=2, moment1=torch.randn(g.shape, generator=MR.gen("oracle-m1", k)) * 0.05,
                          moment2=torch.randn(g.shape, generator=MR.gen("oracle-m2", k)).square() * 0.01)
                m1, m2 = st["moment1"].clone(), st["moment2"].clone()
                MO.adamw_like_update(p_ref, g, st, lr, ratio, (b1, b2), hp["adamw_eps"], hp["adamw_wd"])
                scale = (1 - b1 ** 3) / (1 - b2 ** 3) ** 0.5
                args = (1 - b1, 1 - b2, hp["adamw_eps"], 1 - lr * ratio * hp["adamw_wd"], -lr / scale)
                f = lambda t: t.reshape(-1)  # noqa: E731
                pn, a, b = MR.adamw_f32_path(f(p0), f(g), f(m1), f(m2), *args)
                for got, want in ((pn, p_ref), (a, st["moment1"]), (b, st["moment2"])):
                    torch.testing.assert_close(got, f(want), rtol=2e-6, atol=1e-7)
                # ... and the float64 meaning: the oracle's results pass within the tolerance
                _, _, _, refs = MR.adamw_check(pn, a, b, f(p0), f(g), f(m1), f(m2), *args, f"{variant} {k}")
                for name, want in (("p", p_ref), ("m1", st["moment1"]), ("m2", st["moment2"])):
                    torch.testing.assert_close(f(want).double(), refs[name][0], rtol=2e-6, atol=1e-7)
    assert len(SHAPES) == len(named)
