"""Head sizes 16 and 32, and 64 as the MFMA kernels' cross-check (csrc/attention_generic.hip behind cm3p_attn_fwd_generic /
cm3p_attn_bwd_generic and their _dropout forms): the kernels against the float64 reference of tests/attn_generic_refs.py at every window
and tile seam of its case table - componentwise bounds derived there from the kernels' roundings (1 u: P stays fp32), a derived fp32
bound on lse, a count probe that turns lse into an exact per-row count of the mask rule, the exact conditions (dead rows, padded keys,
window 0, guards, repeatability, wrappers), dropout against the host Philox restatement, and windows that cover the whole axis up to
2^31 - 1.  tests/test_attn_generic_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

Each check prints its worst |got - R| / bound (`pytest -rP`).  CM3P_ATTN_GENERIC_ERRORS_OUT=<file>: write the ratios this run measured
there."""
import functools
import json
import os

import pytest
import torch

import attention_refs as AR
import attn_generic_refs as GR
from attn_generic_refs import NH
from test_dropout_host import keep_mask_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4          # sentinel rows before and after out / dqkv
GUARD_STAT = 64    # sentinel floats before and after lse / delta
SENTINEL = 777.0   # (exact in bf16)
SEED, LAYER = 0x5EED0123456789, 3
INT_MAX = 2 ** 31 - 1

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_ATTN_GENERIC_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for name, seen in _SEEN.items():
        head = ("dropout " if name.startswith("dropout") else "") + name.split("-")[0].split(" ")[-1]  # "d16", "dropout d32", ...
        for k, v in seen.items():
            worst[f"{head} {k}"] = max(worst.get(f"{head} {k}", 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f, indent=1, sort_keys=True)


def _note(g, seen, prefix=""):
    _SEEN.setdefault(prefix + g.name, {}).update(seen)
    print(f"{prefix}{g.name}: " + "  ".join(f"{k}={v:.3g}" for k, v in seen.items()))


@functools.lru_cache(maxsize=None)
def _reference(g):
    return GR.reference(g)


def _guarded(rows, cols, dtype, guard):
    buf = torch.full((rows + 2 * guard, cols), SENTINEL, dtype=dtype, device=DEV)
    buf[guard:guard + rows] = float("nan")  # whatever the kernels leave unwritten fails every comparison
    return buf, buf[guard:guard + rows]


def _guards_untouched(buf, rows, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + rows:] == SENTINEL).all())


def _km(g):
    km = AR.key_mask(g.case)
    return km.to(torch.uint8).to(DEV) if km is not None else None


def _split(g, out, lse, dqkv):
    """The packed device layouts -> tests/attn_generic_refs.py's [B, NH, S, D] on the CPU."""
    B, S, D = g.B, g.S, g.D
    d = dqkv.view(B, S, 3, NH, D).cpu()
    return dict(out=AR.heads(out.view(B, S, NH, D)).cpu(), lse=lse.view(B, NH, S).cpu(), dq=AR.heads(d[:, :, 0]), dk=AR.heads(d[:, :, 1]),
                dv=AR.heads(d[:, :, 2]))


def _direct(g, window=None, drop=None):
    """cm3p_attn_fwd_generic + cm3p_attn_bwd_generic [_dropout: drop = (thr, seed, layer)] on caller-owned, guard-wrapped, NaN-filled
    buffers -> dict(raw: the four device tensors, got: the CPU split, delta, guards, nan_left)."""
    from cm3p_amd import _lib

    B, S, D = g.B, g.S, g.D
    window = g.case.window if window is None else window
    x = GR.inputs(g)
    qkv, do, km = x["qkv"].to(DEV), x["do"].reshape(B * S, NH * D).to(DEV), _km(g)
    out_b, out = _guarded(B * S, NH * D, torch.bfloat16, GUARD)
    dq_b, dqkv = _guarded(B * S, 3 * NH * D, torch.bfloat16, GUARD)
    lse_b, lse = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    dl_b, delta = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    ptr, st = _lib.ptr, _lib.stream
    sfx, extra = ("", ()) if drop is None else ("_dropout", (drop[2], drop[0], drop[1]))
    _lib.call("cm3p_attn_fwd_generic" + sfx, ptr(qkv), ptr(out), ptr(lse), ptr(km), B, S, NH, D, window, g.scale, *extra, st())
    _lib.call("cm3p_attn_bwd_generic" + sfx, ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dqkv), ptr(km), B, S, NH, D, window, g.scale, *extra,
              st())
    torch.cuda.synchronize()
    guards = dict(out=_guards_untouched(out_b, B * S, GUARD), dqkv=_guards_untouched(dq_b, B * S, GUARD),
                  lse=_guards_untouched(lse_b, B * NH * S, GUARD_STAT), delta=_guards_untouched(dl_b, B * NH * S, GUARD_STAT))
    raw = (out, lse, dqkv, delta)
    return dict(raw=raw, got=_split(g, out, lse, dqkv), delta=delta.view(B, NH, S).cpu(), guards=guards,
                nan_left=any(bool(torch.isnan(t.float()).any()) for t in raw))


def _same_bits(a, b):
    return all(torch.equal(s, t) for s, t in zip(a["raw"], b["raw"]))


ALL_GUARDS = dict(out=True, dqkv=True, lse=True, delta=True)


@functools.lru_cache(maxsize=None)
def _run(g):
    """One forward + backward through the C entry points; a second one; the Python wrappers."""
    from cm3p_amd import kernels as K

    B, S, D = g.B, g.S, g.D
    run = _direct(g)
    same = dict(again=_same_bits(run, _direct(g)))
    x = GR.inputs(g)
    qkv, do, km = x["qkv"].to(DEV), x["do"].reshape(B * S, NH * D).to(DEV), _km(g)
    out_w, lse_w = K.attn_fwd_generic(qkv, km, B, S, NH, D, g.case.window, g.scale)
    dqkv_w = K.attn_bwd_generic(qkv, out_w, do, lse_w, km, B, S, NH, D, g.case.window, g.scale)
    out, lse, dqkv, _ = run["raw"]
    same["wrappers"] = torch.equal(out_w, out) and torch.equal(lse_w.reshape(-1, 1), lse) and torch.equal(dqkv_w.view(B * S, -1), dqkv)
    return dict(run, same=same)


def _delta_is_the_rowsum_of_the_stored_out(g, run):
    """the published delta is rowsum(dO o stored out) in fp32: a D-term fma chain"""
    do, out = AR.heads(GR.inputs(g)["do"].double()), run["got"]["out"].double()
    derr = (run["delta"].double() - (do * out).sum(-1)).abs()
    return bool((derr <= (g.D + 2.0) * GR.U * (do * out).abs().sum(-1) + GR.FTZ).all())


@pytest.mark.parametrize("g", GR.TABLE, ids=lambda g: g.name)
def test_matches_float64(g):
    """out, lse, dq, dk, dv against float64 within the derived componentwise bounds; the exact conditions: dead rows are zeros with lse =
    +inf, padded and masked keys get exactly zero dk / dv, nothing outside the tensors is written and nothing inside is left unwritten, a
    second call gives the same bits and so do the Python wrappers."""
    ref, run = _reference(g), _run(g)
    seen, fails = GR.all_checks(g, ref, run["got"])
    _note(g, seen)
    assert not fails, fails
    assert _delta_is_the_rowsum_of_the_stored_out(g, run)
    assert run["guards"] == ALL_GUARDS and not run["nan_left"]
    assert all(run["same"].values()), run["same"]


@pytest.mark.parametrize("D", GR.HEAD_DIMS)
def test_window0_copies_v_and_dout(D):
    """window 0: every live query sees its own key only, so out is the v row and dv is the dO row, bit for bit."""
    g = GR.BY_NAME[f"d{D}-A-S300-w0-pad-plain"]
    got, x, km = _run(g)["got"], GR.inputs(g), AR.key_mask(g.case)
    live = km[:, :, None].expand(-1, -1, NH)  # [B, S, NH]
    assert torch.equal(got["out"].permute(0, 2, 1, 3)[live], x["qkv"][:, :, 2][live])
    assert torch.equal(got["dv"].permute(0, 2, 1, 3)[live], x["do"][live])


@pytest.mark.parametrize("g", GR.TABLE_P, ids=lambda g: g.name)
def test_count_probe(g):
    """q = k = 0: lse = ln n_vis(q) counts the visible keys of every row exactly, out = (sum of +-1 over them) / n to one rounding,
    dq = dk = 0 - at every window of table A."""
    ref, run = _reference(g), _run(g)
    seen, fails = GR.all_checks(g, ref, run["got"])
    _note(g, seen)
    assert not fails, fails
    assert run["guards"] == ALL_GUARDS and not run["nan_left"] and all(run["same"].values())


@functools.lru_cache(maxsize=None)
def _host_keep(n2, S, thr):
    from cm3p_amd import kernels as K

    return torch.from_numpy(keep_mask_ref(n2, S, S, LAYER, K.SITE_ATTN_PROBS, thr, SEED)).bool()  # [B NH, query, key]


@pytest.mark.parametrize("p", GR.DROPOUT_PS)
@pytest.mark.parametrize("g", GR.TABLE_DROP, ids=lambda g: g.name)
def test_dropout(g, p):
    """Attention-probability dropout with the HOST restatement of the keep mask (tests/test_dropout_host.py's Philox; n2 = B NH, n1 =
    query, n0 = key): out and the gradients against float64 with P o Z within the bounds, lse bit-equal to the dropout-free call, thr = 0
    the plain kernels bit for bit, thr = 65536 zero out and gradients with lse unchanged."""
    from cm3p_amd import kernels as K

    thr = K.dropout_threshold(p)
    keep = _host_keep(g.B * NH, g.S, thr).view(g.B, NH, g.S, g.S)
    ref = GR.reference(g, keep, thr / 65536.0)
    plain = _run(g)
    run = _direct(g, drop=(thr, SEED, LAYER))
    seen, fails = GR.all_checks(g, ref, run["got"])
    _note(g, seen, f"dropout {p} ")
    assert not fails, fails
    assert torch.equal(run["got"]["lse"], plain["got"]["lse"])  # the statistics see the undropped probabilities
    assert _delta_is_the_rowsum_of_the_stored_out(g, run)
    assert run["guards"] == ALL_GUARDS and not run["nan_left"]
    assert _same_bits(run, _direct(g, drop=(thr, SEED, LAYER)))
    zero = _direct(g, drop=(0, SEED, LAYER))
    assert _same_bits(zero, plain) and zero["guards"] == ALL_GUARDS
    full = _direct(g, drop=(65536, SEED, LAYER))
    assert full["guards"] == ALL_GUARDS and not full["nan_left"]
    assert torch.equal(full["got"]["lse"], plain["got"]["lse"])
    for nm in ("out", "dq", "dk", "dv"):
        assert full["got"][nm].float().abs().max().item() == 0.0, nm


@pytest.mark.parametrize("name", ["A-S300-w300-pad-plain", "G-S257-w-1-pad-plain", "B-S449-w449-nomask-plain"])
@pytest.mark.parametrize("D", GR.HEAD_DIMS + (64,))
def test_a_window_that_covers_the_axis_is_the_global_mask_in_bits(D, name):
    """Windows S - 1, S, 2^30 and 2^31 - 1 visit every tile and skip no key: the bits of window -1 (the launcher clamps the window to S
    before the kernels do arithmetic with it, so row + window stays inside int)."""
    g = GR.GCase(D, AR.BY_NAME[name])
    glob = _direct(g, window=-1)
    assert glob["guards"] == ALL_GUARDS and not glob["nan_left"]
    assert not GR.check_exact(g, GR.reference(GR.GCase(D, AR.Case(g.case.table, g.S, -1, g.case.lens, False))), glob["got"])
    for window in (g.S - 1, g.S, 2 ** 30, INT_MAX):
        run = _direct(g, window=window)
        assert _same_bits(run, glob), window
        assert run["guards"] == ALL_GUARDS, window


@pytest.mark.parametrize("p", GR.DROPOUT_PS)
def test_dropout_at_a_window_that_covers_the_axis(p):
    from cm3p_amd import kernels as K

    g = GR.BY_NAME["d16-A-S300-w300-pad-plain"]
    drop = (K.dropout_threshold(p), SEED, LAYER)
    glob = _direct(g, window=-1, drop=drop)
    for window in (g.S, 2 ** 30, INT_MAX):
        assert _same_bits(_direct(g, window=window, drop=drop), glob), window


@pytest.mark.parametrize("g", GR.TABLE_64, ids=lambda g: g.name)
def test_head_64_both_kernel_families_meet_their_own_float64_bounds(g):
    """At D = 64 the MFMA kernels (K.attn_fwd / K.attn_bwd: bounds of tests/attention_refs.py, 2 u) and the generic ones (bounds of
    tests/attn_generic_refs.py, 1 u) run on the same tensors and each satisfies its own float64 bounds."""
    from cm3p_amd import kernels as K

    case, B, S = g.case, g.B, g.S
    x = AR.inputs(case)
    assert x["qkv_dev"] is GR.inputs(g)["qkv"] and g.scale == AR.SCALE
    seen, fails = GR.all_checks(g, _reference(g), _run(g)["got"])
    assert not fails, fails
    qkv, do, km = x["qkv_dev"].to(DEV), x["do"].reshape(B * S, NH * 64).to(DEV), _km(g)
    out, lse = K.attn_fwd(qkv, km, B, S, NH, case.window, AR.SCALE, prescaled=False)
    dqkv = K.attn_bwd(qkv, out, do, lse, km, B, S, NH, case.window, AR.SCALE, prescaled=False)
    mfma = _split(g, out, lse, dqkv)
    ref = AR.reference(case)
    s2, f2 = AR.check_float64(ref, mfma, fused=case.window < 0)  # (K.attn_bwd at window -1 is the fused backward)
    _note(g, {f"mfma_{k}": v for k, v in s2.items()})
    assert not f2 + AR.check_exact(case, ref, mfma), f2
    assert (ref["out"] - _reference(g)["out"]).abs().max().item() < 1e-12  # one reference, two derivations of the bounds
