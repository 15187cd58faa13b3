"""tests/loss_head_refs.py on the CPU: every bound is attainable (a torch fp32 walk of the kernel's addition path passes the same
`check` calls tests/test_loss_head_gpu.py makes) and sharp (each wrong evaluation listed there fails them), the node bound at its
largest allowed margin still refuses a denominator that is off by one, and the case tables reach the seams they claim."""
import math

import pytest
import torch

import loss_head_refs as LR
from loss_head_refs import IGNORE, bits_equal, check, gen

ROWS = 130  # two 64-row workgroups and two rows of a third


def _fails(what, fn):
    with pytest.raises(AssertionError):
        fn()
    print(f"{what}: refused")


def _ce(cols, pitch, rows=ROWS, **kw):
    x, lab, kinds = LR.ce_case(cols, pitch, rows, gen("host ce", cols, pitch, rows), **kw)
    return x, lab, kinds


# ================================================================================================ masked cross entropy
@pytest.mark.parametrize("cols,pitch", LR.CE_COLS)
def test_ce_stats_walk_fits_and_wrong_sums_do_not(cols, pitch):
    x, lab, kinds = _ce(cols, pitch)
    ref = LR.ce_stats_ref(x.double(), cols, lab)
    loss, lse = LR.ce_stats_f32_path(x, cols, lab)
    check(lse, ref["lse"], ref["lse_b"], "lse")
    check(loss, ref["loss"], ref["loss_b"], "loss")
    skipped = ~ref["live"]
    assert skipped.any() and not (loss[skipped] != 0).any() and not (lse[skipped] != 0).any()
    # the bound is of the size of the fp32 spacing, not of the loss: a row with loss 200 or lse 100 is held to a few 1e-5
    assert float(ref["loss_b"].max()) < 1e-4
    if cols > 1:
        special = torch.tensor([k != "random" for k in kinds]) & ref["live"]
        _, lse_w = LR.ce_stats_f32_path(x, cols, lab, wrong="no_max")
        _fails("lse without the max subtraction", lambda: check(lse_w[special], ref["lse"][special], ref["lse_b"][special], "lse"))
    if pitch > cols:
        _, lse_w = LR.ce_stats_f32_path(x, cols, lab, wrong="sum_over_pitch")
        _fails("lse summed over the pitch", lambda: check(lse_w, ref["lse"], ref["lse_b"], "lse"))


def test_ce_special_rows_have_the_losses_they_are_named_for():
    cols, pitch = 257, 260
    x, lab, kinds = _ce(cols, pitch)
    ref = LR.ce_stats_ref(x.double(), cols, lab)
    for r, k in enumerate(kinds[:len(LR.CE_KINDS)]):
        if k == "all equal":
            assert abs(float(ref["loss"][r]) - math.log(cols)) < 1e-12
        elif k.endswith("target on the +100"):
            assert 0 <= float(ref["loss"][r]) < 1e-80 and float(ref["loss_b"][r]) > 5e-6  # loss about 0: the absolute floor u |lse|
        elif k.endswith("target on a -100"):
            assert abs(float(ref["loss"][r]) - 200.0) < 1e-12
        elif k.startswith("label"):
            assert not ref["live"][r] and float(ref["loss"][r]) == 0
    assert {kinds.index(k) for k in LR.CE_KINDS} == set(range(len(LR.CE_KINDS)))
    assert bool((x[:, cols:] == LR.PAD_VALUE).all())


@pytest.mark.parametrize("cols,pitch", LR.CE_COLS)
def test_ce_dlogits_walk_fits_and_wrong_gradients_do_not(cols, pitch):
    x, lab, _ = _ce(cols, pitch)
    _, lse = LR.ce_stats_f32_path(x, cols, lab)
    n = int((lab != IGNORE).sum())
    for sa, sb in LR.CE_SCALES:
        sb = float(LR._f32(1.0 / n)) if sb is None else sb
        sa = float(LR._f32(sa))
        ref = LR.ce_dlogits_ref(x.double(), cols, lab, lse.double(), sa, sb)
        dl, colsum, partial = LR.ce_dlogits_f32_path(x, cols, lab, lse, sa, sb)
        check(dl, ref["g"], ref["dl_b"], f"dl s=({sa:.3g}, 1/n)")
        check(colsum, ref["colsum"], ref["colsum_b"], f"colsum s=({sa:.3g}, 1/n)")
        assert not (dl[~ref["live"]].float() != 0).any() and not (dl[:, cols:].float() != 0).any()
        if sa == 0:
            assert not (dl.float() != 0).any()
            continue
        if cols > 1:
            w = LR.ce_dlogits_f32_path(x, cols, lab, lse, sa, sb, wrong="onehot_t_plus_1")[0]
            _fails("one-hot at t + 1", lambda: check(w, ref["g"], ref["dl_b"], "dl"))
            w = LR.ce_dlogits_f32_path(x, cols, lab, lse, sa, sb, wrong="ignored_row_gradient")[0]
            _fails("a gradient on an ignored row", lambda: check(w, ref["g"], ref["dl_b"], "dl"))
            w = LR.ce_dlogits_f32_path(x, cols, lab, lse, sa, sb, wrong="colsum_of_rounded")[1]
            _fails("colsum of the bf16 values", lambda: check(w, ref["colsum"], ref["colsum_b"], "colsum"))
            w = LR.ce_dlogits_f32_path(x, cols, lab, lse, sa, sb, wrong="no_scale_b")
            _fails("s without scale_b (dl)", lambda: check(w[0], ref["g"], ref["dl_b"], "dl"))
            _fails("s without scale_b (colsum)", lambda: check(w[1], ref["colsum"], ref["colsum_b"], "colsum"))
        else:  # one column: softmax = onehot = 1, every gradient is an exact zero
            assert not (dl.float() != 0).any()


def test_ce_dlogits_first_block_all_ignored_leaves_zeros():
    cols, pitch = 257, 260
    x, lab, _ = _ce(cols, pitch, first_block_ignored=True)
    assert bool((lab[:64] == IGNORE).all()) and bool(LR.ce_live(lab[64:], cols).any())
    _, lse = LR.ce_stats_f32_path(x, cols, lab)
    sb = 1.0 / int((lab != IGNORE).sum())
    dl, colsum, partial = LR.ce_dlogits_f32_path(x, cols, lab, lse, 0.37, sb)
    assert not (partial[0] != 0).any() and not (dl[:64].float() != 0).any() and (partial[1] != 0).any()
    ref = LR.ce_dlogits_ref(x.double(), cols, lab, lse.double(), float(LR._f32(0.37)), float(LR._f32(sb)))
    check(colsum, ref["colsum"], ref["colsum_b"], "colsum")


# ================================================================================================ the one-workgroup reductions
def _labels(n, kind, g):
    lab = torch.randint(0, 50, (n,), generator=g)
    if kind == "all ignored":
        return torch.full((n,), IGNORE, dtype=torch.int64)
    if kind == "mixed":
        return torch.where(torch.rand(n, generator=g) < 0.6, torch.full_like(lab, IGNORE), lab)
    if kind == "out of range":
        lab = torch.where(torch.rand(n, generator=g) < 0.5, torch.full_like(lab, IGNORE), lab)
        lab[::3] = torch.tensor([10 ** 6, -5, -1])[torch.arange(lab[::3].numel()) % 3]
    return lab


@pytest.mark.parametrize("n", LR.REDUCE_N)
def test_inv_valid_count_reference(n):
    for kind in ("none ignored", "all ignored", "mixed", "out of range"):
        lab = _labels(n, kind, gen("host inv", n, kind))
        count = sum(1 for v in lab.tolist() if v != IGNORE)  # everything != IGNORE counts, in or out of any vocabulary
        want = LR.inv_valid_count_ref(lab)
        assert want.dtype == torch.float32 and float(want) == float(torch.tensor(1.0) / torch.tensor(float(max(count, 1))))
        if kind == "all ignored":
            assert float(want) == 1.0
        if count not in (0,):
            _fails("count + 1", lambda: bits_equal(LR.inv_valid_count_ref(lab, wrong="count_plus_1"), want, "inv"))


def _sum_data(n, kind, g):
    if kind == "random":
        return torch.randn(n, generator=g)
    return (1e4 * (1 - 2 * (torch.arange(n) % 2)).float()) + torch.randn(n, generator=g)  # alternating +-1e4 plus noise


@pytest.mark.parametrize("n", LR.REDUCE_N)
def test_sum_walk_fits_and_a_dropped_tail_does_not(n):
    for kind in ("random", "cancelling"):
        x = _sum_data(n, kind, gen("host sum", n, kind))
        scale = float(LR._f32(0.37))
        ref, b = LR.sum_ref(x.double(), scale)
        check(LR.sum_f32_path(x, scale), ref, b, f"sum {kind}")
        out0 = torch.tensor([-3.25])
        ref, b = LR.sum_ref(x.double(), scale, out0.double())
        check(LR.sum_f32_path(x, scale, out0), ref, b, f"sum {kind} accumulate")
        if n % 4096:
            ref, b = LR.sum_ref(x.double(), scale)
            _fails("sum without its tail", lambda: check(LR.sum_f32_path(x, scale, wrong="drops_tail"), ref, b, "sum"))


def test_scale_by_reference_is_the_fp32_product():
    x, s = torch.randn(1000, generator=gen("host scale")), torch.tensor([0.3])
    bits_equal(LR.scale_by_ref(x, s), (x.double() * s.double()).float(), "scale_by")  # fp32 x fp32 rounded once either way


# ================================================================================================ l2norm
@pytest.mark.parametrize("D", LR.L2_D)
def test_l2norm_walk_fits_and_wrong_formulas_do_not(D):
    rows = 9
    x, dy, kinds = LR.l2_case(rows, D, gen("host l2", D))
    ref = LR.l2norm_fwd_ref(x.double())
    y, norm = LR.l2norm_fwd_f32_path(x)
    check(y, ref["y"], ref["y_b"], "y")
    check(norm, ref["norm"], ref["norm_b"], "norm")
    for r, k in enumerate(kinds):
        if k in ("one-hot", "one nonzero at the last column"):
            nz = x[r] != 0
            assert int(nz.sum()) == 1 and abs(float(y[r][nz])) == 1.0
    yw, nw = LR.l2norm_fwd_f32_path(x, wrong="eps")
    _fails("l2norm with eps (norm)", lambda: check(nw, ref["norm"], ref["norm_b"], "norm"))
    _fails("l2norm with eps (y)", lambda: check(yw, ref["y"], ref["y_b"], "y"))
    dref, db = LR.l2norm_bwd_ref(dy.double(), y.double(), norm.double())
    dx = LR.l2norm_bwd_f32_path(dy, y, norm)
    check(dx, dref, db, "dx")
    for r, k in enumerate(kinds):
        if k in ("one-hot", "one nonzero at the last column"):
            assert float(dx[r][x[r] != 0]) == 0.0  # dy - y (y dy) with y = +-1: exact
    _fails("l2norm_bwd without the projection", lambda: check(LR.l2norm_bwd_f32_path(dy, y, norm, wrong="no_projection"), dref, db, "dx"))
    if D > 1:  # (D = 1: y = +-1 and dx = 0 whatever multiplies it)
        _fails("l2norm_bwd times norm", lambda: check(LR.l2norm_bwd_f32_path(dy, y, norm, wrong="times_norm"), dref, db, "dx"))


# ================================================================================================ first_zero_index
def test_first_zero_reference_and_cases():
    for B in LR.FZ_B:
        for V in LR.FZ_V:
            c = LR.fz_case(B, V, gen("host fz", B, V))
            want = LR.first_zero_ref(c)
            walk = [next((v for v in range(V) if row[v] == 0), 0) for row in c.tolist()]
            assert want.tolist() == walk
            if B >= 4:
                assert want[0] == 0 and want[1] == V - 1 and want[2] == 0 and want[3] == 0
                assert not (c[2] == 0).any() and (int((c[3] == 0).sum()) >= 2 or V == 1)
                assert bool((c < 0).any()) and bool((c > 2 ** 31).any())


# ================================================================================================ the head
HOST_HEAD = ((130, 64, 37), (65, 128, 1000))


@pytest.fixture(scope="module", params=HOST_HEAD)
def head(request):
    T, H, V = request.param
    g = gen("host head", T, H, V)
    p = LR.head_params(T, H, V, g)
    lab = LR.head_labels(T, V, g)
    return p, lab, LR.head_eval(p, lab, False), LR.head_eval(p, lab, True)


def test_head_rounding_distance_leaves_room_below_a_denominator_off_by_one(head):
    p, lab, R, E = head
    n = int((lab != IGNORE).sum())
    assert 2 <= n <= LR.HEAD_MAX_LABELLED and LR.M_NODE <= LR.M_NODE_MAX
    for k in ("logits", "loss") + LR.GRADS:
        d = LR.rel_l2(E[k], R[k])
        print(f"{k}: |E - R| / |R| = {d:.3g}")
        assert 0 < d and LR.M_NODE_MAX * d < 1.0 / (n + 1), (k, d, n)
        LR.node_check(E[k], R[k], E[k], k, m=1.0)  # the rounded formula itself sits at ratio 1


def test_head_wrong_formulas_fail_the_node_bound_at_its_largest_margin(head):
    p, lab, R, E = head
    m = LR.M_NODE_MAX

    def refused(wrong, names):
        W = LR.head_eval(p, lab, True, wrong=wrong)  # the wrong formula with the node's own roundings: as close as it can get
        for k in names:
            _fails(f"{wrong}: {k}", lambda: LR.node_check(W[k], R[k], E[k], k, m=m))

    refused("denominator_plus_1", ("loss",) + LR.GRADS)
    refused("no_dbdec", ("dbdec",))
    refused("ln_bwd_without_mean_dy", ("dh", "dWd", "dbd"))
    refused("gelu_grad_without_x_pdf", ("dh", "dWd", "dbd"))


def test_head_reference_variants():
    T, H, V = 130, 64, 37
    g = gen("host head variants")
    p = LR.head_params(T, H, V, g)
    lab = LR.head_labels(T, V, g, "out_of_range")
    n = int((lab != IGNORE).sum())
    live = LR.ce_live(lab, V)
    assert int(live.sum()) == n - 1
    R = LR.head_eval(p, lab, False)
    # the mean's denominator counts the out-of-range label, the sum does not
    clean = torch.where(live, lab, torch.full_like(lab, IGNORE))
    want = torch.nn.functional.cross_entropy(R["logits"], clean, ignore_index=IGNORE, reduction="sum") / n
    assert abs(float(R["loss"]) - float(want)) < 1e-14 * abs(float(want))
    assert not (R["dh"][~live] != 0).any()
    # num_items: the sum divided by it
    R2 = LR.head_eval(p, lab, False, num_items=57)
    assert abs(float(R2["loss"]) * 57 - float(R["loss"]) * n) < 1e-12
    # nothing labelled: loss 0 and zero gradients
    R0 = LR.head_eval(p, LR.head_labels(T, V, g, "none"), False)
    assert float(R0["loss"]) == 0 and all(not (R0[k] != 0).any() for k in LR.GRADS)
    # the gradient of the logits is rounded twice when the logits are used outside the loss as well
    w = torch.randn(T, V, generator=g) * 1e-2
    Ew = LR.head_eval(p, lab, True, w_ext=w)
    Rw = LR.head_eval(p, lab, False, w_ext=w)
    for k in LR.GRADS:
        assert 0 < LR.rel_l2(Ew[k], Rw[k]) < 2e-2, k
    # no biases
    pn = LR.head_params(T, H, V, g, bias=False)
    Rn = LR.head_eval(pn, lab, False)
    assert Rn["dbd"] is None and Rn["dbdec"] is None


# ================================================================================================ the seams the case tables claim
def test_case_tables_reach_the_seams():
    # rows per 64-row dlogits workgroup: a short single block, one row short of full, full, one past, two full and a remainder
    assert [(-(-r // LR.DL_ROWS), r % LR.DL_ROWS) for r in LR.CE_ROWS] == [(1, 1), (1, 63), (1, 0), (2, 1), (3, 2)]
    # columns: one; around the 256 threads of the stats kernel; 4096-column windows of the dlogits kernel
    cols = [c for c, _ in LR.CE_COLS]
    assert {1, 255, 256, 257} <= set(cols)
    assert all(p % 4 == 0 and 0 <= p - c < 64 for c, p in LR.CE_COLS)
    windows = {p: (-(-p // LR.DL_WINDOW), (p - 1) % LR.DL_WINDOW // 4 + 1) for _, p in LR.CE_COLS}
    assert windows[4096] == (1, 1024) and windows[4100] == (2, 1) and windows[8200] == (3, 2) and windows[3200] == (1, 800)
    assert {LR.ce_sum_depth(c) - 8 for c in cols} >= {1, 2, 13, 17, 33}
    # the 1024-thread reductions: n around 1024 (threads with no element / one / two), around 4096 (the unrolled body runs for no
    # thread / all / and leaves a tail), 3073 and 7169 (exactly one thread stays in the unrolled loop), and many blocks plus a tail
    for k in (1024, 4096):
        assert {k - 1, k, k + 1} <= set(LR.REDUCE_N)
    for n in (3073, 7169):
        assert n in LR.REDUCE_N and sum(1 for t in range(1024) if t + n // 4096 * 4096 + 3072 < n) == 1
    assert max(LR.REDUCE_N) > 32 * 4096 and max(LR.REDUCE_N) % 4096 % 1024 != 0
    assert max(LR.SCALE_BY_N) > 1024 * 256 and {255, 257} <= set(LR.SCALE_BY_N)
    # l2norm: four rows per workgroup, 64 lanes per row; first_zero_index: 64 rows per workgroup
    assert {3, 4, 5} <= set(LR.L2_ROWS) and {63, 64, 65} <= set(LR.L2_D) and any(d % 64 and d > 64 * 8 for d in LR.L2_D)
    assert {63, 64, 65} <= set(LR.FZ_B) and max(LR.FZ_B) > 3 * 64
    # the head: vocabulary padding 37 -> 64, 1000 -> 1024, 3167 -> 3200, none at 128; row blocks of 64
    assert [LR.vp_of(V) for _, _, V in LR.HEAD_SHAPES] == [64, 1024, 3200, 128]
    assert [T % 64 for T, _, _ in LR.HEAD_SHAPES] == [2, 1, 2, 0]
