"""Head size 64 (csrc/attention.hip, attention_fwd.hip, attention_bwd_fused.hip behind cm3p_attn_fwd / cm3p_attn_bwd / cm3p_attn_bwd_fused
and their varlen, dropout and probs relatives): the kernels against float64 autograd of softmax(scale q k^T + mask) v at every window
and tile seam of tests/attention_refs.py's case table - componentwise bounds derived there from the kernels' roundings, a count probe
that turns lse into an exact per-row count of the mask rule, the exact conditions (dead rows, masked keys, guard rows, repeatability,
stages, wrappers), packed against padded, the probabilities and dropout at windows other than 64.
tests/test_attention_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

CM3P_D64_ERRORS_OUT=<file>: write the worst error / bound ratios this run measured there (profiles/attention_d64_err.txt holds one run's)."""
import functools
import json
import os

import pytest
import torch

import attention_refs as AR
from attention_refs import NH, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4          # sentinel rows before and after out / dqkv
GUARD_STAT = 64    # sentinel floats before and after lse / delta
SENTINEL = 777.0   # (exact in bf16)
SEED, LAYER = 0x5EED0123456789, 3

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_D64_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for seen in _SEEN.values():
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _reference(case):
    return AR.reference(case)


def _guarded(rows, cols, dtype, guard):
    buf = torch.full((rows + 2 * guard, cols), SENTINEL, dtype=dtype, device=DEV)
    buf[guard:guard + rows] = float("nan")  # whatever the kernels leave unwritten fails every comparison
    return buf, buf[guard:guard + rows]


def _guards_untouched(buf, rows, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + rows:] == SENTINEL).all())


def _km(case):
    km = AR.key_mask(case)
    return km.to(torch.uint8).to(DEV) if km is not None else None


def _split(case, out, lse, dqkv):
    """The packed device layouts -> tests/attention_refs.py's [B, NH, S, 64] on the CPU."""
    B, S = case.B, case.S
    got = dict(out=AR.heads(out.view(B, S, NH, 64)).cpu(), lse=lse.view(B, NH, S).cpu())
    if dqkv is not None:
        g = dqkv.view(B, S, 3, NH, 64).cpu()
        got.update(dq=AR.heads(g[:, :, 0]), dk=AR.heads(g[:, :, 1]), dv=AR.heads(g[:, :, 2]))
    return got


def _direct(case, window=None, do=None, stages=(3,)):
    """cm3p_attn_fwd + cm3p_attn_bwd on caller-owned, guard-wrapped, NaN-filled buffers -> (out, lse, dqkv, delta, guards)."""
    from cm3p_amd import _lib

    B, S = case.B, case.S
    window = case.window if window is None else window
    x = AR.inputs(case)
    qkv = x["qkv_dev"].to(DEV)
    do = (x["do"] if do is None else do).reshape(B * S, NH * 64).to(DEV)
    km = _km(case)
    out_b, out = _guarded(B * S, NH * 64, torch.bfloat16, GUARD)
    dq_b, dqkv = _guarded(B * S, 3 * NH * 64, torch.bfloat16, GUARD)
    lse_b, lse = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    dl_b, delta = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_fwd", ptr(qkv), ptr(out), ptr(lse), ptr(km), B, S, NH, window, SCALE, int(case.pre), st())
    for stage in stages:
        _lib.call("cm3p_attn_bwd", ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dqkv), ptr(km), B, S, NH, window, SCALE, None, None, 0, stage,
                  int(case.pre), st())
    torch.cuda.synchronize()
    guards = dict(out=_guards_untouched(out_b, B * S, GUARD), dqkv=_guards_untouched(dq_b, B * S, GUARD),
                  lse=_guards_untouched(lse_b, B * NH * S, GUARD_STAT), delta=_guards_untouched(dl_b, B * NH * S, GUARD_STAT))
    return out, lse, dqkv, delta, guards


@functools.lru_cache(maxsize=None)
def _run(case):
    """One forward + backward through the C entry points; a second one; the stages as two calls; the Python wrappers; for table G also
    the fused backward (K.attn_bwd at window -1)."""
    from cm3p_amd import kernels as K

    B, S = case.B, case.S
    out, lse, dqkv, delta, guards = _direct(case)
    out2, lse2, dqkv2, delta2, _ = _direct(case)
    _, _, dqkv3, _, _ = _direct(case, stages=(1, 2))
    same = dict(again=torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(dqkv2, dqkv) and torch.equal(delta2, delta),
                stages=torch.equal(dqkv3, dqkv))
    x = AR.inputs(case)
    qkv, do, km = x["qkv_dev"].to(DEV), x["do"].reshape(B * S, NH * 64).to(DEV), _km(case)
    out_w, lse_w = K.attn_fwd(qkv, km, B, S, NH, case.window, SCALE, prescaled=case.pre)
    same["fwd_wrapper"] = torch.equal(out_w, out) and torch.equal(lse_w.reshape(-1, 1), lse)
    dqkv_w = K.attn_bwd(qkv, out_w, do, lse_w, km, B, S, NH, case.window, SCALE, prescaled=case.pre)
    got = _split(case, out, lse, dqkv)
    fused = None
    if case.window < 0:
        fused = _split(case, out, lse, dqkv_w)
        same["fused_again"] = torch.equal(K.attn_bwd(qkv, out_w, do, lse_w, km, B, S, NH, -1, SCALE, prescaled=case.pre), dqkv_w)
    else:
        same["bwd_wrapper"] = torch.equal(dqkv_w.view(B * S, -1), dqkv)
    nan_left = any(bool(torch.isnan(t.float()).any()) for t in (out, lse, dqkv, delta))
    return dict(got=got, fused=fused, delta=delta.view(B, NH, S).cpu(), guards=guards, same=same, nan_left=nan_left)


def _note(case, seen, prefix=""):
    _SEEN.setdefault(case.name, {}).update({prefix + k: v for k, v in seen.items()})
    print(f"{case.name} {prefix}: " + "  ".join(f"{k}={v:.3g}" for k, v in seen.items()))


def test_the_binding_and_the_references_agree_on_the_q_scale_and_the_instances():
    from cm3p_amd import kernels as K

    assert K.SOFTMAX_Q_SCALE == AR.SOFTMAX_Q_SCALE
    for case in AR.TABLE:  # the instances the host test counts are the ones the library routes to
        pipelined = bool(K.query("cm3p_attn_fwd_impl", case.S, NH, case.window, int(case.pre)))
        assert pipelined == ("attn_fwd_g_kernel" in AR.instances(case)), case.name
    # four forward, four dq and two dkv instances, each at a window other than 64
    assert AR.ALL_INSTANCES <= set().union(*(AR.instances(c) for c in AR.TABLE if c.window != 64))


@pytest.mark.parametrize("case", AR.TABLE, ids=lambda c: c.name)
def test_matches_float64(case):
    """out, lse, dq, dk, dv against float64 within the derived componentwise bounds (and the secondary lse / relative-L2 bounds); dq and
    dk also against the float64 backward that takes delta from the stored out, without the delta term.  Table G: the pipelined (pre-scaled
    q) or three-wave (plain q) forward, cm3p_attn_bwd at window -1 and cm3p_attn_bwd_fused."""
    ref, run = _reference(case), _run(case)
    seen, fails = AR.check_float64(ref, run["got"])
    cond = AR.conditioned(case, run["got"]["out"])
    s2, f2 = AR.check_conditioned(cond, run["got"])
    _note(case, dict(seen, **s2))
    fails += f2
    if run["fused"] is not None:
        s3, f3 = AR.check_float64(ref, run["fused"], fused=True, quantities=("dq", "dk", "dv"))
        s4, f4 = AR.check_conditioned(cond, run["fused"], fused=True)
        _note(case, dict(s3, **s4), "fused ")
        fails += [f"fused {f}" for f in f3 + f4]
    # the published delta is rowsum(dO o stored out) in fp32: a 64-term dot product
    do, out = AR.heads(AR.inputs(case)["do"].double()), run["got"]["out"].double()
    derr = (run["delta"].double() - (do * out).sum(-1)).abs()
    assert bool((derr <= 70.0 * AR.U * (do * out).abs().sum(-1) + AR.FTZ).all()), "delta is not rowsum(dO o out) of the stored out"
    assert not fails, fails


@pytest.mark.parametrize("case", AR.TABLE, ids=lambda c: c.name)
def test_exact_conditions(case):
    """Dead rows are exact zeros with lse = +inf, masked and padded keys get exactly zero dk / dv, nothing outside the tensors is written
    and nothing inside is left unwritten, a second call gives the same bits, so do the Python wrappers, and the stages DQ then DKV as two
    calls equal the single call with both."""
    ref, run = _reference(case), _run(case)
    assert not AR.check_exact(case, ref, run["got"])
    if run["fused"] is not None:
        assert not AR.check_exact(case, ref, run["fused"])
    assert run["guards"] == dict(out=True, dqkv=True, lse=True, delta=True)
    assert not run["nan_left"]
    assert all(run["same"].values()), run["same"]


def test_window0_copies_v_and_dout():
    """window 0: every live query sees its own key only, so out is the v row and dv is the dO row, bit for bit."""
    for pre in (False, True):
        case = AR.BY_NAME[f"A-S300-w0-pad-{'pre' if pre else 'plain'}"]
        got, x, km = _run(case)["got"], AR.inputs(case), AR.key_mask(case)
        v, do = x["qkv_dev"][:, :, 2], x["do"]
        live = km[:, :, None].expand(-1, -1, NH)  # [B, S, NH]
        assert torch.equal(got["out"].permute(0, 2, 1, 3)[live], v[live])
        assert torch.equal(got["dv"].permute(0, 2, 1, 3)[live], do[live])


@pytest.mark.parametrize("case", AR.TABLE_P, ids=lambda c: c.name)
def test_count_probe(case):
    """q = k = 0: lse = ln n_vis(q) counts the visible keys of every row exactly, out = (sum of +-1) / n to one rounding, dq = dk = 0."""
    ref, run = _reference(case), _run(case)
    seen, fails = AR.check_probe(case, ref, run["got"])
    _note(case, seen, "probe ")
    assert not fails + AR.check_exact(case, ref, run["got"]), fails
    assert run["guards"] == dict(out=True, dqkv=True, lse=True, delta=True) and not run["nan_left"] and all(run["same"].values())


def test_band_equals_global_when_the_window_covers_everything():
    """Windows S - 1 and S are the global mask: the band kernels give the same bits at both, and meet cm3p_attn_bwd at window -1 (the same
    kernels without band arithmetic) and the global forward within the derived bounds."""
    for pre in (False, True):
        sfx = "pre" if pre else "plain"
        a, b = AR.BY_NAME[f"A-S300-w299-pad-{sfx}"], AR.BY_NAME[f"A-S300-w300-pad-{sfx}"]
        ga, gb = _run(a)["got"], _run(b)["got"]
        for nm in ga:
            assert torch.equal(ga[nm], gb[nm]), nm
        ref = _reference(b)
        out, lse, dqkv, _, guards = _direct(b, window=-1)
        gg = _split(b, out, lse, dqkv)
        seen, fails = AR.check_float64(ref, gg)
        _note(b, seen, "at window -1 ")
        assert not fails + AR.check_exact(b, ref, gg), fails
        assert all(guards.values())
        for nm in ("out", "dq", "dk", "dv"):
            assert bool(((gg[nm].double() - gb[nm].double()).abs() <= 2.0 * ref["bound"][nm]).all()), nm


def test_the_largest_window_is_the_window_s_in_bits():
    """window = 2^31 - 1: the launchers clamp a window to S before the band kernels do arithmetic with it (qrow + window, Q1 + window
    and q0 + QW - 1 + window would leave int), so the call is the window = S call bit for bit, forward and backward."""
    for pre in (False, True):
        case = AR.BY_NAME[f"A-S300-w300-pad-{'pre' if pre else 'plain'}"]
        out, lse, dqkv, delta, guards = _direct(case, window=2 ** 31 - 1)
        out_s, lse_s, dqkv_s, delta_s, _ = _direct(case, window=case.S)
        assert torch.equal(out, out_s) and torch.equal(lse, lse_s) and torch.equal(dqkv, dqkv_s) and torch.equal(delta, delta_s)
        assert all(guards.values())
        assert not AR.check_float64(_reference(case), _split(case, out, lse, dqkv))[1]


@pytest.mark.parametrize("window", [1, 33, 96, 200])
def test_varlen_equals_padded(window):
    """cm3p_attn_fwd_varlen / cm3p_attn_bwd_varlen on the packed sequences give the bits of the padded call on every valid row (masked keys
    contribute exact zeros; padded queries carry no gradient), as tests/test_kernels_gpu.py holds at window 64."""
    from cm3p_amd import kernels as K

    for pre in (False, True):
        case = AR.BY_NAME[f"A-S300-w{window}-pad-{'pre' if pre else 'plain'}"]
        B, S, lens = case.B, case.S, list(case.lens)
        x, km = AR.inputs(case), AR.key_mask(case)
        do = x["do"] * km[:, :, None, None].to(torch.bfloat16)
        out, lse, dqkv, _, _ = _direct(case, do=do)
        idx = torch.nonzero(km.flatten()).flatten().to(DEV)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        qkv_p = x["qkv_dev"].to(DEV).reshape(B * S, 3, NH, 64)[idx].contiguous()
        do_p = do.to(DEV).reshape(B * S, NH * 64)[idx].contiguous()
        out_p, lse_p = K.attn_fwd_varlen(qkv_p, cu, B, max(lens), NH, window, SCALE, pre)
        dqkv_p = K.attn_bwd_varlen(qkv_p, out_p, do_p, lse_p, cu, B, max(lens), NH, window, SCALE, None, pre)
        torch.cuda.synchronize()
        assert torch.equal(out_p, out[idx])
        assert torch.equal(lse_p, lse.view(B, NH, S).permute(1, 0, 2).reshape(NH, B * S)[:, idx])
        assert torch.equal(dqkv_p.reshape(len(idx), -1), dqkv[idx])


@pytest.mark.parametrize("window", [1, 33, 96])
def test_probs(window):
    """cm3p_attn_probs with the forward's lse against the float64 softmax within attention_refs.probs_bound (3 e32 p: the fp32 dot
    product and the stored lse in the exponent); invisible keys are exact zeros, dead rows 1 / S, rows sum to 1."""
    from cm3p_amd import kernels as K

    for case in (AR.BY_NAME[f"A-S300-w{window}-pad-plain"], AR.BY_NAME[f"C-S300-w{window}-holes-pre"]):
        B, S = case.B, case.S
        ref, x = _reference(case), AR.inputs(case)
        out, lse, _, _, _ = _direct(case, stages=())
        probs = K.attn_probs(x["qkv_dev"].to(DEV), lse.view(B, NH, S).contiguous(), _km(case), B, S, NH, window, SCALE, prescaled=case.pre).cpu()
        vis, dead, _, p64 = AR.softmax64(case, x)
        err = (probs.double() - p64).abs()
        live = ~ref["dead"]
        bound = AR.probs_bound(ref, p64)
        ratio = (err / bound)[live].max().item()
        _note(case, dict(probs=ratio))
        assert bool((err <= bound)[live].all()), ratio
        assert probs[live][~vis.expand(-1, NH, -1, -1)[live]].abs().max().item() == 0.0
        if ref["dead"].any():
            assert bool((probs[ref["dead"]] == torch.tensor(1.0) / torch.tensor(float(S))).all())
        sums = probs.double().sum(-1)
        assert bool(((sums - 1.0).abs() <= 3.0 * ref["e32"][..., 0] * AR.SECOND + S * AR.U)[live].all())
        assert bool(((sums - 1.0).abs() <= 2.0 * S * AR.U)[~live].all())


@pytest.mark.parametrize("window", [1, 33, 96])
def test_dropout_at_other_windows(window):
    """Attention-probability dropout (p = 0.1) on the band kernels at windows other than 64: out and the three gradients against float64
    with the kernels' own keep mask (K.dropout_keep, pinned to the contract by tests/test_dropout_gpu.py) within the bounds with P o Z in
    place of P, lse bit-identical to the dropout-free call, and thr = 0 the plain band kernels bit for bit, forward and backward."""
    from cm3p_amd import kernels as K

    thr = K.dropout_threshold(0.1)
    for pre in (False, True):
        case = AR.BY_NAME[f"A-S300-w{window}-pad-{'pre' if pre else 'plain'}"]
        B, S = case.B, case.S
        x, km, plain = AR.inputs(case), _km(case), _run(case)
        qkv, do = x["qkv_dev"].to(DEV), x["do"].reshape(B * S, NH * 64).to(DEV)
        keep = K.dropout_keep(B * NH, S, S, LAYER, K.SITE_ATTN_PROBS, thr, SEED, DEV).cpu().view(B, NH, S, S).bool()
        p_drop = thr / 65536.0
        ref = AR.reference(case, keep, p_drop)
        out, lse = K.attn_fwd(qkv, km, B, S, NH, window, SCALE, prescaled=pre, drop=(thr, SEED, LAYER))
        dqkv = K.attn_bwd(qkv, out, do, lse, km, B, S, NH, window, SCALE, prescaled=pre, drop=(thr, SEED, LAYER))
        got = _split(case, out, lse, dqkv)
        assert torch.equal(got["lse"], plain["got"]["lse"])  # the statistics see the undropped probabilities
        seen, fails = AR.check_float64(ref, got)
        s2, f2 = AR.check_conditioned(AR.conditioned(case, got["out"], keep, p_drop), got)
        _note(case, dict(seen, **s2), "dropout ")
        assert not fails + f2 + AR.check_exact(case, ref, got), fails + f2
        out0, lse0 = K.attn_fwd(qkv, km, B, S, NH, window, SCALE, prescaled=pre, drop=(0, SEED, LAYER))
        dqkv0 = K.attn_bwd(qkv, out0, do, lse0, km, B, S, NH, window, SCALE, prescaled=pre, drop=(0, SEED, LAYER))
        g0 = _split(case, out0, lse0, dqkv0)
        for nm in g0:
            assert torch.equal(g0[nm], plain["got"][nm]), f"thr = 0: {nm}"
