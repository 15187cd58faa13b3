"""The query-list attention kernels (csrc/attention_qrows.hip) through the C ABI of include/cm3p_attn_qrows.h against the float64
reference and the bounds of tests/attn_qrows_refs.py: every seam of the 128-slot workgroups and the 32-row wave and key tiles, every
list kind, padding, a padded query, queries without a visible key, sequences without a query, packed sequences (one of length 0), the
windows, both q modes, the inverse rotation in its three table forms; and against the library itself - cm3p_attn_fwd / cm3p_attn_bwd
with every row listed and with a dout that is zero off the list, cm3p_attn_row_fwd / _bwd with row 0 only."""
import dataclasses
import functools

import pytest
import torch

import attn_qrows_refs as R
from attn_qrows_refs import B, NH, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0
GUARD = 8


def _guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + rows] = float("nan")  # whatever the kernels leave unwritten fails every comparison
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf, rows):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + rows:] == SENTINEL).all())


def _device_inputs(case):
    x = R.inputs(case)
    S = case.S
    qkv, do = x["qkv_dev"], R.compact(case, x["do"])
    cos = sin = None
    if case.rope is not None:
        n = S if (case.rope == "shared" and not case.packed) else B * S
        cos, sin = x["cos"][:n], x["sin"][:n]
    km = cu = None
    if case.packed:
        qkv = R.pack(case, qkv)
        if cos is not None:
            cos, sin = R.pack(case, cos.view(B, S, 32)), R.pack(case, sin.view(B, S, 32))
        cu = torch.tensor(R.cu_seqlens(case), dtype=torch.int32, device=DEV)
    else:
        m = R.key_mask(case)
        km = m.to(torch.uint8).to(DEV) if m is not None else None
    rows, qcu, qmax = R.row_list(case)
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    return dict(qkv=dev(qkv).view(-1, 3 * NH * 64), do=dev(do).view(-1, NH * 64), cos=dev(cos), sin=dev(sin), km=km, cu=cu,
                qrows=torch.tensor(rows, dtype=torch.int32, device=DEV), qcu=torch.tensor(qcu, dtype=torch.int32, device=DEV), n=len(rows), qmax=qmax,
                pbs=S if (case.rope == "batch" and not case.packed) else 0)


def _direct(case):
    """cm3p_attn_qrows_fwd + cm3p_attn_qrows_bwd on caller-owned, guard-wrapped, NaN-filled buffers."""
    from cm3p_amd import _lib

    d = _device_inputs(case)
    rows, n = d["qkv"].shape[0], d["n"]
    out_b, out = _guarded(n, NH * 64, torch.bfloat16)
    lse_b, lse = _guarded(NH * n, 1, torch.float32)
    dq_b, dqkv = _guarded(rows, 3 * NH * 64, torch.bfloat16)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_qrows_fwd", ptr(d["qkv"]), ptr(out), ptr(lse), ptr(d["km"]), ptr(d["cu"]), ptr(d["qrows"]), ptr(d["qcu"]), n, d["qmax"], B, case.S,
              rows, NH, case.window, SCALE, int(case.pre), st())
    _lib.call("cm3p_attn_qrows_bwd", ptr(d["qkv"]), ptr(out), ptr(d["do"]), ptr(lse), ptr(dqkv), ptr(d["km"]), ptr(d["cu"]), ptr(d["qrows"]), ptr(d["qcu"]),
              n, d["qmax"], B, case.S, rows, NH, case.window, SCALE, ptr(d["cos"]), ptr(d["sin"]), d["pbs"], int(case.pre), st())
    torch.cuda.synchronize()
    guards = dict(out=_guards_untouched(out_b, n), lse=_guards_untouched(lse_b, NH * n), dqkv=_guards_untouched(dq_b, rows))
    return out, lse, dqkv, guards


def _split(case, out, lse, dqkv):
    """The device layouts -> tests/attn_qrows_refs.py's full padded shapes on the CPU."""
    S = case.S
    g = dqkv.view(-1, 3, NH, 64).cpu()
    g = R.unpack_rows(case, g) if case.packed else g.view(B, S, 3, NH, 64)
    n = out.shape[0]
    return dict(out=R.heads_of(R.spread(case, out.view(n, NH, 64).cpu())), lse=R.spread(case, lse.view(NH, n).t().contiguous().cpu()).permute(0, 2, 1),
                dq=R.heads_of(g[:, :, 0]), dk=R.heads_of(g[:, :, 1]), dv=R.heads_of(g[:, :, 2]))


@functools.lru_cache(maxsize=None)
def _run(case):
    from cm3p_amd import kernels as K

    out, lse, dqkv, guards = _direct(case)
    out2, lse2, dqkv2, _ = _direct(case)
    same = dict(again=torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(dqkv2, dqkv))
    d = _device_inputs(case)
    rope = (d["cos"], d["sin"]) if d["cos"] is not None else None
    out_w, lse_w = K.attn_qrows_fwd(d["qkv"], d["qrows"], d["qcu"], d["qmax"], d["km"], d["cu"], B, case.S, NH, case.window, SCALE, prescaled=case.pre)
    dqkv_w = K.attn_qrows_bwd(d["qkv"], out_w, d["do"], lse_w, d["qrows"], d["qcu"], d["qmax"], d["km"], d["cu"], B, case.S, NH, case.window, SCALE,
                              rope=rope, per_batch=case.rope == "batch", prescaled=case.pre)
    same["wrappers"] = torch.equal(out_w, out) and torch.equal(lse_w.reshape(-1, 1), lse) and torch.equal(dqkv_w, dqkv)
    nan_left = any(bool(torch.isnan(t.float()).any()) for t in (out, lse, dqkv))
    return dict(got=_split(case, out, lse, dqkv), guards=guards, same=same, nan_left=nan_left)


@functools.lru_cache(maxsize=None)
def _reference(case):
    return R.reference(case)


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_qrows_kernels_against_float64(case):
    run, ref = _run(case), _reference(case)
    assert not run["nan_left"], "an element of out / lse / dqkv was never written"
    assert all(run["guards"].values()), run["guards"]
    seen, fails = R.check_float64(ref, run["got"], rel_l2=not case.peaked)
    seen2, fails2 = R.check_conditioned(case, run["got"])
    print(case.name, {k: round(v, 4) for k, v in {**seen, **seen2}.items()})
    assert not fails + fails2, (seen, seen2)


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_qrows_kernels_exact_conditions(case):
    run, ref = _run(case), _reference(case)
    assert not R.check_exact(case, ref, run["got"])
    assert run["same"]["again"], "two calls on equal inputs gave different bits"
    assert run["same"]["wrappers"], "cm3p_amd.kernels.attn_qrows_fwd / attn_qrows_bwd differ from the direct calls"


def test_an_empty_list_launches_nothing_forward_and_zeroes_dqkv_backward():
    from cm3p_amd import _lib

    case = R.TABLE[0]
    d = _device_inputs(case)
    rows = d["qkv"].shape[0]
    dq_b, dqkv = _guarded(rows, 3 * NH * 64, torch.bfloat16)
    qcu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_qrows_fwd", ptr(d["qkv"]), None, None, None, None, None, ptr(qcu), 0, 0, B, case.S, rows, NH, -1, SCALE, 0, st())
    _lib.call("cm3p_attn_qrows_bwd", ptr(d["qkv"]), None, None, None, ptr(dqkv), None, None, None, ptr(qcu), 0, 0, B, case.S, rows, NH, -1, SCALE, None, None, 0,
              0, st())
    torch.cuda.synchronize()
    assert _guards_untouched(dq_b, rows) and bool((dqkv == 0).all())


def _full(case, dout_full):
    """cm3p_attn_fwd and cm3p_attn_bwd (fed `dout_full` [B, S, NH * 64], without tables) on the inputs of a padded case."""
    from cm3p_amd import _lib

    S = case.S
    d = _device_inputs(case)
    out = torch.empty(B * S, NH * 64, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, NH, S, dtype=torch.float32, device=DEV)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_fwd", ptr(d["qkv"]), ptr(out), ptr(lse), ptr(d["km"]), B, S, NH, case.window, SCALE, int(case.pre), st())
    dqkv = torch.full((B * S, 3 * NH * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    delta = torch.empty_like(lse)
    _lib.call("cm3p_attn_bwd", ptr(d["qkv"]), ptr(out), ptr(dout_full.contiguous().to(DEV)), ptr(lse), ptr(delta), ptr(dqkv), ptr(d["km"]), B, S, NH, case.window,
              SCALE, None, None, 0, 3, int(case.pre), st())
    torch.cuda.synchronize()
    g = dqkv.view(B, S, 3, NH, 64).cpu()
    return dict(out=R.heads_of(out.view(B, S, NH, 64).cpu()), lse=lse.cpu(), dq=R.heads_of(g[:, :, 0]), dk=R.heads_of(g[:, :, 1]), dv=R.heads_of(g[:, :, 2]))


def _agree(case, a, b, names):
    """Both results hold the float64 bounds of the case, so they differ by at most twice the bound (lse: twice its tolerance)."""
    ref = _reference(case)
    for got in (a, b):
        seen, fails = R.check_float64(ref, got, names, rel_l2=False)
        assert not fails, (seen, fails)
    seen, fails = R.check_float64(dict(ref, **{nm: a[nm].double() for nm in names}), b, names, rel_l2=False, factor=2.0)
    assert not fails, (seen, fails)
    dl = ref["listed"] & ref["dead"]
    assert torch.equal(a["lse"][dl], b["lse"][dl]), "lse of a listed query without a visible key"


NO_ROPE = [dataclasses.replace(c, rope=None) for c in R.TABLE if not c.packed]  # (the same data: the full backward runs without tables here)
EVERY_ROW = [c for c in NO_ROPE if "all" in c.kinds]
ROW_0 = [c for c in R.TABLE if c.kinds == ("row0", "row0")]


@pytest.mark.parametrize("case", EVERY_ROW, ids=lambda c: c.name)
def test_every_row_listed_agrees_with_the_full_kernels(case):
    case = dataclasses.replace(case, kinds=("all", "all"))
    _agree(case, _run(case)["got"], _full(case, R.inputs(case)["do"].view(B, case.S, NH * 64)), ("out", "lse", "dq", "dk", "dv"))


@pytest.mark.parametrize("case", NO_ROPE, ids=lambda c: c.name)
def test_backward_agrees_with_the_full_backward_fed_a_dout_that_is_zero_off_the_list(case):
    _agree(case, _run(case)["got"], _full(case, R.inputs(case)["do"].view(B, case.S, NH * 64)), ("dq", "dk", "dv"))


@pytest.mark.parametrize("case", ROW_0, ids=lambda c: c.name)
def test_row_0_only_agrees_with_the_single_query_kernels(case):
    from cm3p_amd import kernels as K

    d = _device_inputs(case)
    rope = (d["cos"], d["sin"]) if d["cos"] is not None else None
    out, lse = K.attn_row_fwd(d["qkv"], d["km"], d["cu"], B, case.S, NH, case.window, SCALE, prescaled=case.pre)
    dqkv = K.attn_row_bwd(d["qkv"], out, d["do"], lse, d["km"], d["cu"], B, case.S, NH, case.window, SCALE, rope=rope, per_batch=case.rope == "batch",
                          prescaled=case.pre)
    torch.cuda.synchronize()
    row = _split(case, out, lse.t().contiguous(), dqkv)  # (the single-query kernels store lse as [B, nh])
    _agree(case, _run(case)["got"], row, ("out", "lse", "dq", "dk", "dv"))


def test_entries_refuse_bad_arguments_on_the_device_too():
    """Every refusal answers CM3P_ERR_INVALID with real device buffers as well (tests/test_attn_qrows_refs_host.py walks the whole list
    without a GPU); nothing is launched, the buffers keep their NaN fill."""
    from cm3p_amd import _lib

    case = R.TABLE[0]
    d = _device_inputs(case)
    rows, n = d["qkv"].shape[0], d["n"]
    out = torch.full((n, NH * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((NH, n), float("nan"), dtype=torch.float32, device=DEV)
    lib, p = _lib.load(), lambda t: t.data_ptr()
    good = [p(d["qkv"]), p(out), p(lse), None, None, p(d["qrows"]), p(d["qcu"]), n, d["qmax"], B, case.S, rows, NH, -1, SCALE, 0, None]
    for i, v in ((0, None), (1, p(out) + 2), (5, None), (6, None), (7, -1), (8, 0), (9, 0), (10, 0), (11, rows + 1), (12, 0), (14, 0.0), (3, p(d["qcu"]))):
        args = list(good)
        args[i] = v
        if i == 3:
            args[4] = p(d["qcu"])  # a key mask together with cu_seqlens
        assert lib.cm3p_attn_qrows_fwd(*args) == -1, i
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(lse).all())
