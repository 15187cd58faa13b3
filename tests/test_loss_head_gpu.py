"""The masked-LM loss kernels, the remaining kernels of csrc/head.hip and the masked-LM head's autograd nodes against the float64
references and derived bounds of tests/loss_head_refs.py: special logit rows (all equal, +-100, about -90, about +88, targets at the
first and last column, labels outside the vocabulary, pad columns that would read as inf), every column and row seam of the two loss
kernels, the 1024-thread reductions around their seams, l2norm and first_zero_index at their workgroup seams, and the head nodes in
every variant against the node bound |got - R| <= m |E - R|.  tests/test_loss_head_refs_host.py shows on the CPU that a correct kernel
fits these checks and that wrong ones do not.

Each check prints its largest error / bound (`pytest -rP`).  CM3P_LOSS_HEAD_ERRORS_OUT=<file>: write the worst ratios this run
measured there (profiles/loss_head_err.txt holds one run's)."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

import loss_head_refs as LR
from loss_head_refs import IGNORE, bits_equal, check, gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64          # sentinel elements before and after a caller-owned output
SENTINEL = 777.0    # (exact in bf16)

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_LOSS_HEAD_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for seen in _SEEN.values():
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, margin=LR.M_NODE, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f,
                  indent=1, sort_keys=True)


def _note(test, quantity, ratio):
    seen = _SEEN.setdefault(test, {})
    seen[quantity] = max(seen.get(quantity, 0.0), float(ratio))


@pytest.fixture(scope="module")
def K():
    from cm3p_amd import kernels

    return kernels


def _guarded(n, dtype):
    """A NaN-filled (int64: -1-filled) flat output of n elements between two runs of GUARD sentinels."""
    buf = torch.full((n + 2 * GUARD,), int(SENTINEL) if dtype == torch.int64 else SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = -1 if dtype == torch.int64 else float("nan")
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _dev_scalar(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


# ================================================================================================ ce_masked_stats / ce_masked_dlogits
@functools.lru_cache(maxsize=None)
def _ce(cols, pitch, rows, first_block_ignored=False):
    x, lab, kinds = LR.ce_case(cols, pitch, rows, gen("ce", cols, pitch, rows), first_block_ignored=first_block_ignored)
    return x, lab, kinds, LR.ce_stats_ref(x.double(), cols, lab)


def _check_ce(K, cols, pitch, rows, test, first_block_ignored=False):
    x, lab, kinds, ref = _ce(cols, pitch, rows, first_block_ignored)
    xd, ld = x.to(DEV), lab.to(DEV)
    loss_rows, lse_rows = K.ce_masked_stats(xd, cols, ld, IGNORE)
    tag = f"{cols}/{pitch} x {rows}"
    _note(test, "stats lse", check(lse_rows, ref["lse"], ref["lse_b"], f"lse {tag}"))
    _note(test, "stats loss", check(loss_rows, ref["loss"], ref["loss_b"], f"loss {tag}"))
    skipped = (~ref["live"]).to(DEV)
    zero = torch.zeros((), dtype=torch.int32, device=DEV)
    assert not (loss_rows.view(torch.int32)[skipped] != zero).any() and not (lse_rows.view(torch.int32)[skipped] != zero).any(), \
        "loss_rows / lse_rows of a skipped row are not +0"
    loss2, lse2 = K.ce_masked_stats(xd, cols, ld, IGNORE)
    bits_equal(loss2, loss_rows.cpu(), "loss_rows again")
    bits_equal(lse2, lse_rows.cpu(), "lse_rows again")
    n = int((lab != IGNORE).sum())
    lse_in = lse_rows.cpu().double()
    for sa, sb in LR.CE_SCALES:
        sa_t, sb_t = _dev_scalar(sa), _dev_scalar(1.0 / max(n, 1) if sb is None else sb)
        dref = LR.ce_dlogits_ref(x.double(), cols, lab, lse_in, float(sa_t), float(sb_t))
        dl, colsum = K.ce_masked_dlogits_bf16(xd, cols, ld, IGNORE, lse_rows, sa_t, sb_t)
        assert dl.dtype == torch.bfloat16 and dl.shape == (rows, pitch) and colsum.shape == (pitch,)
        _note(test, "dlogits dl", check(dl, dref["g"], dref["dl_b"], f"dl {tag} s=({sa}, 1/n)"))
        _note(test, "dlogits colsum", check(colsum, dref["colsum"], dref["colsum_b"], f"colsum {tag} s=({sa}, 1/n)"))
        bits = dl.view(torch.int16)
        assert not (bits[:, cols:] != 0).any() and not (bits[skipped] != 0).any(), "skipped rows / pad columns of dl are not +0"
        assert not (colsum[cols:] != 0).any()
        dl2, colsum2 = K.ce_masked_dlogits_bf16(xd, cols, ld, IGNORE, lse_rows, sa_t, sb_t)
        bits_equal(dl2, dl.cpu(), "dl again")
        bits_equal(colsum2, colsum.cpu(), "colsum again")


@pytest.mark.parametrize("cols,pitch", LR.CE_COLS)
def test_masked_ce_stats_and_dlogits_at_every_seam(K, cols, pitch):
    for rows in LR.CE_ROWS:
        _check_ce(K, cols, pitch, rows, f"ce[{cols}-{pitch}]")


def test_masked_ce_with_a_whole_row_block_ignored_into_guarded_buffers(K):
    """Rows 0 .. 63 all ignored, rows 64 .. 129 not, two column windows (the second one 4-column group wide), through the C entry
    points into caller-owned NaN-filled buffers between sentinels: the ignored block's partial row and dl rows are written, as zeros;
    nothing is left unwritten and nothing is written outside."""
    from cm3p_amd import _lib

    cols, pitch, rows = 4097, 4100, 130
    _check_ce(K, cols, pitch, rows, "ce[first block ignored]", first_block_ignored=True)
    x, lab, _, ref = _ce(cols, pitch, rows, True)
    assert bool((lab[:64] == IGNORE).all()) and bool(ref["live"][64:].any())
    xd, ld = x.to(DEV), lab.to(DEV)
    nblk = _lib.query("cm3p_ce_masked_dlogits_blocks", rows)
    assert nblk == 3
    lo_b, loss_rows = _guarded(rows, torch.float32)
    ls_b, lse_rows = _guarded(rows, torch.float32)
    dl_b, dl = _guarded(rows * pitch, torch.bfloat16)
    pa_b, part = _guarded(nblk * pitch, torch.float32)
    cs_b, colsum = _guarded(pitch, torch.float32)
    assert dl.data_ptr() % 8 == 0 and part.data_ptr() % 16 == 0
    sa, sb = _dev_scalar(0.37), _dev_scalar(1.0 / int((lab != IGNORE).sum()))
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_ce_masked_stats", ptr(xd), rows, cols, pitch, ptr(ld), IGNORE, ptr(loss_rows), ptr(lse_rows), st())
    _lib.call("cm3p_ce_masked_dlogits_bf16", ptr(xd), rows, cols, pitch, ptr(ld), IGNORE, ptr(lse_rows), ptr(sa), ptr(sb), ptr(dl), ptr(part),
              ptr(colsum), st())
    torch.cuda.synchronize()
    for name, buf, t in (("loss_rows", lo_b, loss_rows), ("lse_rows", ls_b, lse_rows), ("dl", dl_b, dl), ("partial", pa_b, part), ("colsum", cs_b, colsum)):
        assert _intact(buf, t.numel()), f"{name}: a store outside the buffer"
        assert not torch.isnan(t.float()).any(), f"{name}: an element was left unwritten"
    part, dl = part.view(nblk, pitch), dl.view(rows, pitch)
    assert not (part[0].view(torch.int32) != 0).any(), "the partial row of the all-ignored block is not zero"
    assert not (dl[:64].view(torch.int16) != 0).any(), "dl rows of the all-ignored block are not zero"
    assert bool((part[1] != 0).any()) and bool((part[2] != 0).any())
    dl_w, colsum_w = K.ce_masked_dlogits_bf16(xd, cols, ld, IGNORE, lse_rows.clone(), sa, sb)
    bits_equal(dl, dl_w.cpu(), "dl: C entry point against the wrapper")
    bits_equal(colsum, colsum_w.cpu(), "colsum: C entry point against the wrapper")


# ================================================================================================ inv_valid_count, sum_f32, scale_by
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
def test_inv_valid_count_is_the_fp32_quotient_in_bits(K, n):
    """'out of range' pins the rule include/cm3p_hip.h states: everything != ignore_index counts, a label the loss kernels skip too."""
    for kind in ("none ignored", "all ignored", "mixed", "out of range"):
        lab = _labels(n, kind, gen("inv", n, kind))
        got = K.inv_valid_count(lab.to(DEV), IGNORE)
        bits_equal(got, LR.inv_valid_count_ref(lab), f"inv_valid_count {kind}")
        if kind == "all ignored":
            assert float(got) == 1.0
        bits_equal(K.inv_valid_count(lab.to(DEV), IGNORE), got.cpu(), "again")


def _sum_data(n, kind, g):
    if kind == "random":
        return torch.randn(n, generator=g)
    return (1e4 * (1 - 2 * (torch.arange(n) % 2)).float()) + torch.randn(n, generator=g)  # alternating +-1e4 plus noise


@pytest.mark.parametrize("n", LR.REDUCE_N)
def test_sum_f32_against_float64(K, n):
    for kind in ("random", "cancelling"):
        x = _sum_data(n, kind, gen("sum", n, kind))
        xd = x.to(DEV)
        for scale in (1.0, 0.37):
            s32 = float(LR._f32(scale))
            ref, b = LR.sum_ref(x.double(), s32)
            got = K.sum_f32(xd, scale)
            _note(f"sum[{n}]", "sum_f32", check(got, ref, b, f"sum {kind} n={n} scale={scale}"))
            bits_equal(K.sum_f32(xd, scale), got.cpu(), "again")
            out = torch.tensor([-3.25], device=DEV)
            ref, b = LR.sum_ref(x.double(), s32, torch.tensor(-3.25, dtype=torch.float64))
            got = K.sum_f32(xd, scale, out=out, accumulate=True)
            assert got.data_ptr() == out.data_ptr()
            _note(f"sum[{n}]", "sum_f32 accumulate", check(got, ref, b, f"sum {kind} n={n} scale={scale} accumulate"))


@pytest.mark.parametrize("n", LR.SCALE_BY_N)
def test_scale_by_is_the_fp32_product_in_bits(K, n):
    from cm3p_amd import _lib

    g = gen("scale_by", n)
    x = torch.randn(n, generator=g) * 3
    xd = x.to(DEV)
    for s in (0.37, -2.0, 0.0, 1.0 / 3):
        st = torch.tensor([s], dtype=torch.float32)
        sd = st.to(DEV)
        buf, y = _guarded(n, torch.float32)
        _lib.call("cm3p_scale_by", _lib.ptr(xd), _lib.ptr(sd), _lib.ptr(y), n, _lib.stream())
        torch.cuda.synchronize()
        assert _intact(buf, n)
        bits_equal(y, LR.scale_by_ref(x, st), f"scale_by n={n} s={s}")
        bits_equal(K.scale_by(xd, sd), y.cpu(), "wrapper")


# ================================================================================================ l2norm
@pytest.mark.parametrize("D", LR.L2_D)
def test_l2norm_forward_and_backward_against_float64(K, D):
    from cm3p_amd import _lib

    ptr, st = _lib.ptr, _lib.stream
    for rows in LR.L2_ROWS:
        x, dy, kinds = LR.l2_case(rows, D, gen("l2", rows, D))
        ref = LR.l2norm_fwd_ref(x.double())
        xd, dyd = x.to(DEV), dy.to(DEV)
        y_b, y = _guarded(rows * D, torch.float32)
        n_b, norm = _guarded(rows, torch.float32)
        dx_b, dx = _guarded(rows * D, torch.float32)
        _lib.call("cm3p_l2norm_fwd", ptr(xd), ptr(y), ptr(norm), rows, D, st())
        _lib.call("cm3p_l2norm_bwd", ptr(dyd), ptr(y), ptr(norm), ptr(dx), rows, D, st())
        torch.cuda.synchronize()
        assert _intact(y_b, rows * D) and _intact(n_b, rows) and _intact(dx_b, rows * D), "a store outside y / norm / dx"
        y, dx = y.view(rows, D), dx.view(rows, D)
        tag = f"{rows} x {D}"
        _note(f"l2[{D}]", "l2norm y", check(y, ref["y"], ref["y_b"], f"y {tag}"))
        _note(f"l2[{D}]", "l2norm norm", check(norm, ref["norm"], ref["norm_b"], f"norm {tag}"))
        dref, db = LR.l2norm_bwd_ref(dy.double(), y.cpu().double(), norm.cpu().double())
        _note(f"l2[{D}]", "l2norm dx", check(dx, dref, db, f"dx {tag}"))
        for r, k in enumerate(kinds):
            if k in ("one-hot", "one nonzero at the last column"):
                hot = (x[r] != 0).to(DEV)
                assert abs(float(y[r][hot])) == 1.0 and float(norm[r]) == abs(float(x[r][hot.cpu()])), f"row {r} ({k}): y is not +-1"
                assert float(dx[r][hot]) == 0.0, f"row {r} ({k}): dx on the hot column is not an exact 0"
        yw, nw = K.l2norm_fwd(xd)
        bits_equal(yw, y.cpu(), "y: wrapper")
        bits_equal(nw, norm.cpu(), "norm: wrapper")
        bits_equal(K.l2norm_bwd(dyd, yw, nw), dx.cpu(), "dx: wrapper")


# ================================================================================================ first_zero_index
@pytest.mark.parametrize("V", LR.FZ_V)
def test_first_zero_index_is_the_argmax_of_the_zero_mask(K, V):
    from cm3p_amd import _lib

    for B in LR.FZ_B:
        c = LR.fz_case(B, V, gen("fz", B, V))
        cd = c.to(DEV)
        buf, idx = _guarded(B, torch.int64)
        _lib.call("cm3p_first_zero_index", _lib.ptr(cd), B, V, _lib.ptr(idx), _lib.stream())
        torch.cuda.synchronize()
        assert _intact(buf, B)
        assert torch.equal(idx.cpu(), LR.first_zero_ref(c)), f"B={B} V={V}"
        assert torch.equal(K.first_zero_index(cd).cpu(), LR.first_zero_ref(c))


# ================================================================================================ the head nodes
def _nodes():
    from cm3p_amd import modeling_cm3p as M

    return M


def _leaves(p, h_dtype, p_dtype, h_grad=True):
    """The node's inputs on the device, and the values they hold as float64 reference inputs."""
    dev, vals = {}, {}
    for k, v in p.items():
        if v is None:
            dev[k] = vals[k] = None
            continue
        t = v.to(h_dtype if k == "h" else p_dtype)
        vals[k] = t.double()
        dev[k] = t.to(DEV).requires_grad_(h_grad if k == "h" else True)
    return dev, vals


def _apply_loss(M, d, lab, num_items=None):
    return M._MLMHeadLossFn.apply(d["h"], d["Wd"], d["bd"], d["nw"], d["Wdec"], d["bdec"], LR.HEAD_EPS, lab, num_items)


def _grads_of(d):
    out = {}
    for name, key in zip(LR.GRADS, ("h", "Wd", "bd", "nw", "Wdec", "bdec")):
        t = d[key]
        out[name] = None if t is None else t.grad
    return out


def _run_head(T, H, V, *, h_dtype=torch.float32, p_dtype=torch.float32, bias=True, num_items=None, lab_form="int64", h_grad=True,
              labels="quarter", ext=False, test="head"):
    """One _MLMHeadLossFn forward + backward in the given variant, checked against the node bound; -> what the caller checks further."""
    M = _nodes()
    g = gen("head", T, H, V, bias)
    p = LR.head_params(T, H, V, g, bias=bias)
    lab = LR.head_labels(T, V, g, labels)
    w_ext = torch.randn(T, V, generator=g) * 1e-2 if ext else None
    d, vals = _leaves(p, h_dtype, p_dtype, h_grad)
    Vp = LR.vp_of(V)
    B = 5 if T % 5 == 0 else 1
    lab_dev = lab.view(B, T // B).to(DEV)
    if lab_form == "int32":
        lab_dev = lab_dev.to(torch.int32)
    n_ref = None
    ni = None
    if num_items == "int":
        ni = n_ref = 57
    elif num_items == "tensor":
        n_ref = 57
        ni = torch.tensor(57, device=DEV)
    dloss = 0.7
    logits, loss = _apply_loss(M, d, lab_dev, ni)
    assert logits.shape == (T, Vp) and logits.dtype == torch.float32 and loss.shape == () and loss.dtype == torch.float32
    obj = dloss * loss
    if ext:
        obj = obj + (logits[:, :V] * w_ext.to(DEV)).sum()
    obj.backward()
    got = _grads_of(d)
    out_bf16 = tuple(n for n, k in zip(LR.GRADS, ("h", "Wd", "bd", "nw", "Wdec", "bdec")) if (h_dtype if k == "h" else p_dtype) == torch.bfloat16)
    R = LR.head_eval(vals, lab, False, num_items=n_ref, w_ext=w_ext, dloss=dloss)
    E = LR.head_eval(vals, lab, True, num_items=n_ref, w_ext=w_ext, dloss=dloss, out_bf16=out_bf16)
    assert not (logits[:, V:] != 0).any(), "pad columns of the logits are not zero"
    tag = f"{T}x{H}x{V}"
    _note(test, "node logits", LR.node_check(logits[:, :V], R["logits"], E["logits"], f"logits {tag}"))
    _note(test, "node loss", LR.node_check(loss, R["loss"], E["loss"], f"loss {tag}"))
    for name in LR.GRADS:
        if name == "dh" and not h_grad:
            assert got[name] is None
            continue
        if R[name] is None:
            assert got[name] is None, name
            continue
        want_dtype = h_dtype if name == "dh" else p_dtype
        assert got[name] is not None and got[name].dtype == want_dtype and got[name].shape == R[name].shape, (name, got[name].dtype)
        _note(test, f"node {name}", LR.node_check(got[name], R[name], E[name], f"{name} {tag}"))
    if h_grad and not ext:
        skipped = (~LR.ce_live(lab, V)).to(DEV)
        assert not (got["dh"][skipped] != 0).any(), "dh of a row without a label is not zero"
    return dict(d=d, lab_dev=lab_dev, ni=ni, logits=logits, loss=loss, got=got, dloss=dloss, M=M, p=p, lab=lab)


@pytest.mark.parametrize("T,H,V", LR.HEAD_SHAPES)
def test_head_loss_node_plain_variant(T, H, V):
    r = _run_head(T, H, V, test=f"head[{T}-{H}-{V}]")
    # repeatable bits
    M, d = r["M"], r["d"]
    for t in d.values():
        if t is not None:
            t.grad = None
    logits, loss = _apply_loss(M, d, r["lab_dev"], r["ni"])
    (r["dloss"] * loss).backward()
    bits_equal(logits, r["logits"].detach().cpu(), "logits again")
    bits_equal(loss, r["loss"].detach().cpu(), "loss again")
    for name, gd in _grads_of(d).items():
        bits_equal(gd, r["got"][name].cpu(), f"{name} again")


@pytest.mark.parametrize("variant", ["h bf16", "no biases", "parameters bf16", "all bf16 no biases", "num_items int", "num_items tensor",
                                     "labels int32", "h without grad", "out of range label", "all labelled", "logits used outside"])
def test_head_loss_node_variants(variant):
    kw = {"h bf16": dict(h_dtype=torch.bfloat16), "no biases": dict(bias=False), "parameters bf16": dict(p_dtype=torch.bfloat16),
          "all bf16 no biases": dict(h_dtype=torch.bfloat16, p_dtype=torch.bfloat16, bias=False),
          "num_items int": dict(num_items="int"), "num_items tensor": dict(num_items="tensor"), "labels int32": dict(lab_form="int32"),
          "h without grad": dict(h_grad=False), "out of range label": dict(labels="out_of_range"), "all labelled": dict(labels="all"),
          "logits used outside": dict(ext=True)}[variant]
    T, H, V = (33, 64, 37) if variant == "all labelled" else (65, 128, 1000) if variant in ("parameters bf16", "logits used outside") else (130, 64, 37)
    _run_head(T, H, V, test=f"head[{variant}]", **kw)


@pytest.mark.parametrize("h_dtype,p_dtype,bias", [(torch.float32, torch.float32, True), (torch.bfloat16, torch.bfloat16, False)])
def test_head_loss_node_with_nothing_labelled(h_dtype, p_dtype, bias):
    M = _nodes()
    T, H, V = 130, 64, 37
    g = gen("head none", bias)
    d, _ = _leaves(LR.head_params(T, H, V, g, bias=bias), h_dtype, p_dtype)
    lab = LR.head_labels(T, V, g, "none").to(DEV)
    logits, loss = _apply_loss(M, d, lab)
    loss.backward()
    assert loss.detach().reshape(1).view(torch.int32).item() == 0, "the loss of a batch without a label is not +0"
    for name, gd in _grads_of(d).items():
        if gd is not None:
            assert bool(torch.isfinite(gd).all()) and not (gd != 0).any(), f"{name} of a batch without a label is not zero"
    assert bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("T,H,V", [(130, 64, 37), (64, 64, 128)])
def test_head_node_equals_the_loss_nodes_logits_path_in_bits(T, H, V):
    """_MLMHeadFn (logits only) against float64, and _MLMHeadLossFn differentiated through its logits only against it in bits."""
    M = _nodes()
    g = gen("head fn", T, H, V)
    p = LR.head_params(T, H, V, g)
    lab = LR.head_labels(T, V, g)
    w = torch.randn(T, V, generator=g) * 1e-2
    Vp = LR.vp_of(V)
    wp = torch.zeros(T, Vp)
    wp[:, :V] = w
    d1, vals = _leaves(p, torch.float32, torch.float32)
    l1 = M._MLMHeadFn.apply(d1["h"], d1["Wd"], d1["bd"], d1["nw"], d1["Wdec"], d1["bdec"], LR.HEAD_EPS)
    (l1 * wp.to(DEV)).sum().backward()
    d2, _ = _leaves(p, torch.float32, torch.float32)
    l2, loss = _apply_loss(M, d2, lab.to(DEV))
    (l2 * wp.to(DEV)).sum().backward()
    bits_equal(l2, l1.detach().cpu(), "logits of the two nodes")
    g1, g2 = _grads_of(d1), _grads_of(d2)
    R = LR.head_eval(vals, lab, False, w_ext=w, use_loss=False)
    E = LR.head_eval(vals, lab, True, w_ext=w, use_loss=False)
    assert not (l1[:, V:] != 0).any()
    test = f"headfn[{T}-{H}-{V}]"
    _note(test, "node logits", LR.node_check(l1[:, :V], R["logits"], E["logits"], "logits"))
    for name in LR.GRADS:
        bits_equal(g2[name], g1[name].cpu(), f"{name}: the loss node through its logits only")
        if name == "dbdec":
            # the column sums of the fp32 gradient handed in, unrounded: E = R here, so the node bound has nothing to scale by.  A sum
            # of T fp32 terms has at most T - 1 roundings on a path in whatever order: (T - 1) u sum_r |w|.
            _note(test, "dbdec (logits only)", check(g1[name], R[name], (T - 1) * LR.U * w.double().abs().sum(0) * LR.SECOND, name))
            continue
        _note(test, f"node {name} (logits only)", LR.node_check(g1[name], R[name], E[name], name))


def test_add_scaled_node_in_bits():
    M = _nodes()
    for a, b, c, gv in ((1.2345678, 0.7654321, 0.5, 1.0), (-3.1, 7.7e-3, 0.5, 0.37), (0.0, 2.5, -1.75, -2.0)):
        at = torch.tensor(a, device=DEV, requires_grad=True)
        bt = torch.tensor(b, device=DEV, requires_grad=True)
        out = M._AddScaledFn.apply(at, bt, c)
        out.backward(torch.tensor(gv, device=DEV))
        a32, b32, c32, g32 = (LR._f32(v) for v in (a, b, c, gv))
        # a + c b: the product rounded and then the sum, or the two fused - whichever the compiler chose, within one of the two forms
        plain = a32 + c32 * b32
        fused = (a32.double() + c32.double() * b32.double()).float()
        assert out.dtype == torch.float32 and out.shape == ()
        bits = [t.detach().cpu().reshape(1).view(torch.int32).item() for t in (out, plain, fused)]
        assert bits[0] in bits[1:], (a, b, c)
        bits_equal(at.grad, g32, "d/da")
        bits_equal(bt.grad, c32 * g32, "d/db")


@pytest.mark.parametrize("B", [1, 6, 257])
@pytest.mark.parametrize("labels", [2, 5, 37])
def test_masked_cross_entropy_node_against_float64(B, labels):
    """_MaskedCrossEntropyFn (the single-label classifier's loss; the pitch is the number of labels, no multiple of 4) against float64
    F.cross_entropy(ignore_index=-100) with an upstream gradient != 1.  The kernel shares ce_masked_stats' sum, so that bound holds
    per row; the mean adds the sum kernel's path and two roundings; a gradient element is the dlogits kernel's fp32 value, and one
    more product with the upstream gradient."""
    M = _nodes()
    g = gen("mce", B, labels)
    x = torch.randn(B, labels, generator=g) * 3
    lab = torch.randint(0, labels, (B,), generator=g)
    if B > 1:
        lab[torch.rand(B, generator=g) < 0.3] = IGNORE
        lab[0] = labels - 1
    up = -0.37
    xr = x.double().requires_grad_(True)
    n = int((lab != IGNORE).sum())
    want = F.cross_entropy(xr, lab, ignore_index=IGNORE)
    (want * float(LR._f32(up))).backward()
    xd = x.to(DEV).requires_grad_(True)
    loss = M._MaskedCrossEntropyFn.apply(xd, lab.to(DEV))
    loss.backward(torch.tensor(up, device=DEV))
    ref = LR.ce_stats_ref(x.double(), labels, lab)
    b_loss = (ref["loss_b"].sum() + LR.sum_depth(B) * LR.U * ref["loss"].abs().sum()) / n * LR.SECOND + 3 * LR.U * abs(float(want))
    _note("mce", "masked CE loss", check(loss.reshape(1), want.detach().reshape(1), b_loss.reshape(1), f"loss B={B} labels={labels}"))
    # gradient: s (p - onehot) with s = up / n: the dlogits kernel's e32 at the float64 lse plus the kernel's own lse error times |s| p
    dref = LR.ce_dlogits_ref(x.double(), labels, lab, ref["lse"], float(LR._f32(up)), 1.0 / n)
    p = torch.exp(x.double() - ref["lse"][:, None]) * ref["live"][:, None]
    b_g = dref["e32"] + abs(up / n) * p * ref["lse_b"][:, None] * LR.SECOND + 4 * LR.U * dref["g"].abs()
    _note("mce", "masked CE gradient", check(xd.grad, xr.grad, b_g, f"dlogits B={B} labels={labels}"))
    assert not (xd.grad[(lab == IGNORE).to(DEV)] != 0).any()


def test_masked_cross_entropy_node_with_nothing_labelled():
    M = _nodes()
    x = torch.randn(6, 5, generator=gen("mce none")).to(DEV).requires_grad_(True)
    loss = M._MaskedCrossEntropyFn.apply(x, torch.full((6,), IGNORE, dtype=torch.int64, device=DEV))
    loss.backward(torch.tensor(2.0, device=DEV))
    assert loss.detach().reshape(1).view(torch.int32).item() == 0 and not (x.grad != 0).any()
