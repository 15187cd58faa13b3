"""The single-query attention kernels (csrc/attention_row.hip) through the C ABI of include/cm3p_attn_row.h against the float64
reference and the derived bounds of tests/attn_row_refs.py: every seam of the key loop, every window edge, padding, a masked key 0,
queries without a visible key, packed sequences, both q modes, the inverse rotation in its three table forms; and against the library
itself - row 0 of cm3p_attn_fwd / cm3p_attn_bwd on the same inputs."""
import dataclasses
import functools

import pytest
import torch

import attn_row_refs as R
from attn_row_refs import SCALE

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
    B, S, nh = case.B, case.S, case.nh
    qkv = x["qkv_dev"]
    cos = sin = None
    if case.rope is not None:
        n = S if (case.rope == "shared" and not case.packed) else B * S
        cos, sin = x["cos"][:n], x["sin"][:n]
    km = cu = None
    total = 0
    if case.packed:
        qkv = R.pack(case, qkv)
        if cos is not None:
            cos, sin = R.pack(case, cos.view(B, S, 32)), R.pack(case, sin.view(B, S, 32))
        cu = torch.tensor([0] + list(torch.tensor(case.lens).cumsum(0)), dtype=torch.int32, device=DEV)
        total = qkv.shape[0]
    else:
        m = R.key_mask(case)
        km = m.to(torch.uint8).to(DEV) if m is not None else None
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    return dict(qkv=dev(qkv).view(-1, 3 * nh * 64), do=dev(x["do"]).view(B, nh * 64), cos=dev(cos), sin=dev(sin), km=km, cu=cu, total=total,
                pbs=S if (case.rope == "batch" and not case.packed) else 0)


def _direct(case):
    """cm3p_attn_row_fwd + cm3p_attn_row_bwd on caller-owned, guard-wrapped, NaN-filled buffers."""
    from cm3p_amd import _lib

    B, S, nh = case.B, case.S, case.nh
    d = _device_inputs(case)
    rows = d["qkv"].shape[0]
    out_b, out = _guarded(B, nh * 64, torch.bfloat16)
    lse_b, lse = _guarded(B * nh, 1, torch.float32)
    dq_b, dqkv = _guarded(rows, 3 * nh * 64, torch.bfloat16)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_row_fwd", ptr(d["qkv"]), ptr(out), ptr(lse), ptr(d["km"]), ptr(d["cu"]), B, S, d["total"], nh, case.window, SCALE, int(case.pre), st())
    _lib.call("cm3p_attn_row_bwd", ptr(d["qkv"]), ptr(out), ptr(d["do"]), ptr(lse), ptr(dqkv), ptr(d["km"]), ptr(d["cu"]), B, S, d["total"], nh, case.window,
              SCALE, ptr(d["cos"]), ptr(d["sin"]), d["pbs"], int(case.pre), st())
    torch.cuda.synchronize()
    guards = dict(out=_guards_untouched(out_b, B), lse=_guards_untouched(lse_b, B * nh), dqkv=_guards_untouched(dq_b, rows))
    return out, lse, dqkv, guards


def _split(case, out, lse, dqkv):
    """The device layouts -> tests/attn_row_refs.py's shapes on the CPU (+ the whole q third, [B, S, nh, 64])."""
    B, S, nh = case.B, case.S, case.nh
    g = dqkv.view(-1, 3, nh, 64).cpu()
    g = R.unpack_rows(case, g) if case.packed else g.view(B, S, 3, nh, 64)
    return dict(out=out.view(B, nh, 64).cpu(), lse=lse.view(B, nh).cpu(), dq=g[:, 0, 0], dk=g[:, :, 1].permute(0, 2, 1, 3), dv=g[:, :, 2].permute(0, 2, 1, 3),
                q_third=g[:, :, 0])


@functools.lru_cache(maxsize=None)
def _run(case):
    from cm3p_amd import kernels as K

    out, lse, dqkv, guards = _direct(case)
    out2, lse2, dqkv2, _ = _direct(case)
    same = dict(again=torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(dqkv2, dqkv))
    d = _device_inputs(case)
    rope = (d["cos"], d["sin"]) if d["cos"] is not None else None
    out_w, lse_w = K.attn_row_fwd(d["qkv"], d["km"], d["cu"], case.B, case.S, case.nh, case.window, SCALE, prescaled=case.pre)
    dqkv_w = K.attn_row_bwd(d["qkv"], out_w, d["do"], lse_w, d["km"], d["cu"], case.B, case.S, case.nh, case.window, SCALE, rope=rope,
                            per_batch=case.rope == "batch", prescaled=case.pre)
    same["wrappers"] = torch.equal(out_w, out) and torch.equal(lse_w.reshape(-1, 1), lse) and torch.equal(dqkv_w, dqkv)
    nan_left = any(bool(torch.isnan(t.float()).any()) for t in (out, lse, dqkv))
    return dict(got=_split(case, out, lse, dqkv), guards=guards, same=same, nan_left=nan_left)


@functools.lru_cache(maxsize=None)
def _reference(case):
    return R.reference(case)


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_row_kernels_against_float64(case):
    run, ref = _run(case), _reference(case)
    assert not run["nan_left"], "an element of out / lse / dqkv was never written"
    assert all(run["guards"].values()), run["guards"]
    seen, fails = R.check_float64(ref, run["got"], rel_l2=not case.peaked)
    seen2, fails2 = R.check_conditioned(case, run["got"])
    print(case.name, {k: round(v, 4) for k, v in {**seen, **seen2}.items()})
    assert not fails + fails2, (seen, seen2)


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_row_kernels_exact_conditions(case):
    run, ref = _run(case), _reference(case)
    assert not R.check_exact(case, ref, run["got"])
    qt = run["got"]["q_third"].float()
    assert qt[:, 1:].abs().max().item() == 0.0 if case.S > 1 else True, "the q third is not exactly zero off the query rows"
    if case.packed:  # (unpack_rows zero-fills behind each sequence: look at the packed rows themselves)
        assert not bool(torch.isnan(qt).any())
    assert run["same"]["again"], "two calls on equal inputs gave different bits"
    assert run["same"]["wrappers"], "cm3p_amd.kernels.attn_row_fwd / attn_row_bwd differ from the direct calls"


def _full(case, one_row_dout):
    """cm3p_attn_fwd (and cm3p_attn_bwd fed a dout that is zero off row 0, without tables) on the inputs of a padded case."""
    from cm3p_amd import _lib

    B, S, nh = case.B, case.S, case.nh
    d = _device_inputs(case)
    out = torch.empty(B * S, nh * 64, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, nh, S, dtype=torch.float32, device=DEV)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_fwd", ptr(d["qkv"]), ptr(out), ptr(lse), ptr(d["km"]), B, S, nh, case.window, SCALE, int(case.pre), st())
    got = dict(out=out.view(B, S, nh, 64)[:, 0].cpu(), lse=lse[:, :, 0].cpu())
    if one_row_dout:
        do = torch.zeros(B, S, nh * 64, dtype=torch.bfloat16, device=DEV)
        do[:, 0] = d["do"]
        dqkv = torch.full((B * S, 3 * nh * 64), float("nan"), dtype=torch.bfloat16, device=DEV)
        delta = torch.empty_like(lse)
        _lib.call("cm3p_attn_bwd", ptr(d["qkv"]), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dqkv), ptr(d["km"]), B, S, nh, case.window, SCALE, None, None, 0,
                  3, int(case.pre), st())
        g = dqkv.view(B, S, 3, nh, 64).cpu()
        got.update(dq=g[:, 0, 0], dk=g[:, :, 1].permute(0, 2, 1, 3), dv=g[:, :, 2].permute(0, 2, 1, 3))
    torch.cuda.synchronize()
    return got


PADDED = [c for c in R.TABLE if not c.packed]


def _within_both(ref, a, b, names):
    for nm in names:
        bound = ref["bound"][nm] + ref["bound_band"][nm]
        x, y = a[nm].double(), b[nm].double()
        if nm == "lse":
            live = ~ref["dead"]
            assert torch.equal(x[~live], y[~live]), "lse of a query without a visible key"
            x, y, bound = x[live], y[live], bound[live]
        err = (x - y).abs()
        assert bool((err <= bound).all()), f"{nm}: worst difference / (sum of both bounds) = {(err / bound).max().item():.3f}"


@pytest.mark.parametrize("case", PADDED, ids=lambda c: c.name)
def test_row_forward_agrees_with_row_0_of_the_full_forward(case):
    _within_both(_reference(case), _run(case)["got"], _full(case, False), ("out", "lse"))


@pytest.mark.parametrize("case", PADDED, ids=lambda c: c.name)
def test_row_backward_agrees_with_the_full_backward_fed_a_one_row_dout(case):
    case = dataclasses.replace(case, rope=None)  # (the same data: both backwards run without tables here)
    _within_both(_reference(case), _run(case)["got"], _full(case, True), ("dq", "dk", "dv"))
