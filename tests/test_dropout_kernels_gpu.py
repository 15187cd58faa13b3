"""The dropout kernels against tests/dropout_refs.py and the dropout tables of tests/attention_refs.py: the materialiser and
cm3p_dropout_f32 in bits, the GeGLU dropout kernels against float64 within bounds derived from their roundings, head-64 attention
with dropout (cm3p_attn_fwd_dropout / cm3p_attn_bwd_dropout and their packed relatives) against float64 autograd at every case of
TABLE_DROP and both probabilities.  Every keep mask is the host's Philox restatement (tests/test_dropout_host.py::keep_mask_ref), never
the library's materialiser; every result buffer is caller-owned, wrapped in sentinel guard rows and NaN-filled.
tests/test_dropout_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

CM3P_DROPOUT_ERRORS_OUT=<file>: write the worst error / bound ratios this run measured there (profiles/dropout_err.txt holds one run's)."""
import json
import os

import numpy as np
import pytest
import torch

import attention_refs as AR
import dropout_refs as DR
from attention_refs import NH, SCALE
from test_dropout_host import keep_mask_ref, threshold_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4          # sentinel rows before and after every row buffer
GUARD_STAT = 64    # sentinel floats before and after lse / delta
SENTINEL = 777.0   # (exact in bf16)
SEED, LAYER = DR.SEED, DR.LAYER

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_DROPOUT_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for seen in _SEEN.values():
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f, indent=1, sort_keys=True)


def _note(name, seen, prefix=""):
    _SEEN.setdefault(name, {}).update({prefix + k: v for k, v in seen.items()})
    print(f"{name} {prefix}: " + "  ".join(f"{k}={v:.3g}" for k, v in seen.items()))


def _guarded(rows, cols, dtype, guard=GUARD, fill=None):
    """-> (whole buffer, the [rows, cols] view between its guards).  fill: the tensor the view starts as (default NaN: whatever a kernel
    leaves unwritten fails every comparison)."""
    buf = torch.full((rows + 2 * guard, cols), SENTINEL, dtype=dtype, device=DEV)
    if fill is None:
        buf[guard:guard + rows] = float("nan")
    else:
        buf[guard:guard + rows] = fill.to(DEV)
    return buf, buf[guard:guard + rows]


def _guards_untouched(buf, rows, guard=GUARD):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + rows:] == SENTINEL).all())


def _layout_args(layout):
    """(S, cu_seqlens pointer, n_seqs) of the element entry points, and the tensor that keeps the pointer alive."""
    from cm3p_amd import _lib

    if not layout.packed:
        return (layout.S, None, 0), None
    cu = torch.tensor(layout.cu, dtype=torch.int32, device=DEV)
    return (layout.S, _lib.ptr(cu, torch.int32), layout.n_seqs), cu


# ================================================================================================ the materialiser
KEEP_CASES = [((8, 513, 1021), LAYER, 3, 6554, SEED),            # 525,312 work items: past 2048 x 256, a ragged last group
              ((1, 1, 1), LAYER, 1, 6554, SEED), ((3, 7, 8), LAYER, 2, 6554, SEED),
              ((3, 7, 8), (1 << 29) - 1, 3, 6554, SEED),          # the last layer the entry points take
              ((2, 5, 37), LAYER, 1, 6554, 2 ** 64 - 1), ((2, 5, 37), LAYER, 1, 6554, 2 ** 63), ((2, 5, 37), LAYER, 1, 6554, 0xABCDEF0100000000),
              *[((2, 5, 37), LAYER, 0, thr, SEED) for thr in (0, 1, 6554, 32768, 65535, 65536)]]
assert 8 * 513 * ((1021 + 7) // 8) > 2048 * 256


@pytest.mark.parametrize("shape,layer,site,thr,seed", KEEP_CASES)
def test_materialiser_in_bits(shape, layer, site, thr, seed):
    from cm3p_amd import _lib

    n = int(np.prod(shape))
    buf = torch.full((n + 128,), 0xAA, dtype=torch.uint8, device=DEV)  # 64 guard bytes either side; 0xAA is neither 0 nor 1
    keep = buf[64:64 + n]
    _lib.call("cm3p_dropout_keep", _lib.ptr(keep), *shape, layer, site, thr, seed, _lib.stream())
    torch.cuda.synchronize()
    want = keep_mask_ref(*shape, layer, site, thr, seed)
    assert np.array_equal(keep.cpu().numpy().reshape(shape), want)
    assert bool((buf[:64] == 0xAA).all()) and bool((buf[64 + n:] == 0xAA).all())
    if thr in (0, 65536):
        assert want.all() == (thr == 0) and want.any() == (thr == 0)
    if n > 1000 and 0 < thr < 65536:
        assert 0 < int(want.sum()) < n


# ================================================================================================ cm3p_dropout_f32
FORMS = ("f32", "bf16", "both", "in_place")


def _dropout_f32(layout, H, site, thr, form, with_resid, layer=LAYER, seed=SEED, data=None):
    """One cm3p_dropout_f32 call on guarded buffers -> (y_f32 or None, y_bf16 or None, the contract's pair).  data: (x, resid) other
    than the layout's own draw."""
    from cm3p_amd import _lib

    rows = layout.rows
    x, resid = data or DR.f32_data(rows, H)
    want = DR.dropout_f32_path(x, resid if with_resid else None, layout, layer, site, thr, seed)
    xb, xd = _guarded(rows, H, torch.float32, fill=x)
    rd = resid.to(DEV) if with_resid else None
    y32b = y16b = y32 = y16 = None
    if form in ("f32", "both"):
        y32b, y32 = _guarded(rows, H, torch.float32)
    if form == "in_place":
        y32b, y32 = xb, xd
    if form in ("bf16", "both"):
        y16b, y16 = _guarded(rows, H, torch.bfloat16)
    lay, cu = _layout_args(layout)
    _lib.call("cm3p_dropout_f32", _lib.ptr(xd, torch.float32), _lib.ptr(rd, torch.float32), _lib.ptr(y32), _lib.ptr(y16), rows, H, *lay, layer, site,
              thr, seed, _lib.stream())
    torch.cuda.synchronize()
    for b in (xb, y32b, y16b):
        assert b is None or _guards_untouched(b, rows)
    if form != "in_place":
        assert torch.equal(xd.cpu(), x)  # the input is read only
    return (None if y32 is None else y32.cpu()), (None if y16 is None else y16.cpu()), want


def _assert_contract(y32, y16, want, what):
    if y32 is not None:
        assert torch.equal(y32, want[0]), f"{what}: the fp32 result is not fl(fl(x scale) + resid) in bits"
    if y16 is not None:
        assert torch.equal(y16, want[1]), f"{what}: the bf16 result is not the RNE of the fp32 one"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_resid", [False, True])
def test_dropout_f32_every_output_form_at_one_group_per_row(form, with_resid):
    """H = 8; fp32 only, bf16 only, both in one call, in place (y_f32 == x); with and without the residual."""
    thr = threshold_ref(0.1)
    y32, y16, want = _dropout_f32(DR.PADDED_SMALL, 8, DR.SITE_ATTN_OUT, thr, form, with_resid)
    _assert_contract(y32, y16, want, f"{form}, resid={with_resid}")


@pytest.mark.parametrize("p", DR.DROPOUT_PS)
def test_dropout_f32_past_the_grid(p):
    """4104 x 1024 as 8 sequences of 513: 525,312 work items, so the grid-stride loop takes a second trip; both outputs in one call."""
    y32, y16, want = _dropout_f32(DR.PADDED_BIG, 1024, DR.SITE_ATTN_OUT, threshold_ref(p), "both", True)
    _assert_contract(y32, y16, want, "past the grid")


@pytest.mark.parametrize("site", [0, 1, 2, 3])
def test_dropout_f32_every_site_and_the_edge_thresholds(site):
    lay = DR.PADDED_SMALL
    y32, y16, want = _dropout_f32(lay, 136, site, threshold_ref(0.5), "both", site == DR.SITE_ATTN_OUT, layer=DR.LAYER_HIGH, seed=DR.SEED_TOP_BIT)
    _assert_contract(y32, y16, want, f"site {site}")
    x, resid = DR.f32_data(lay.rows, 136)
    # thr = 65536 drops everything: the residual exactly (+0 without one); thr = 0 keeps everything at scale 1: x (+ resid) in bits
    y32, y16, want = _dropout_f32(lay, 136, site, 65536, "both", True)
    _assert_contract(y32, y16, want, "thr 65536")
    assert torch.equal(y32, resid)
    y32, _, _ = _dropout_f32(lay, 136, site, 65536, "f32", False)
    assert not y32.any() and not torch.signbit(y32).any()
    y32, _, _ = _dropout_f32(lay, 136, site, 0, "in_place", True)
    assert torch.equal(y32, x + resid)


@pytest.mark.parametrize("layout", DR.PACKED, ids=lambda lay: lay.name)
def test_dropout_f32_packed_layouts(layout):
    """H = 136 on every packed layout: the contract directly, and the rows of the padded call on the same tokens."""
    thr = threshold_ref(0.1)
    y32, y16, want = _dropout_f32(layout, 136, DR.SITE_EMBED, thr, "both", True)
    _assert_contract(y32, y16, want, layout.name)
    twin, idx = DR.padded_twin(layout)
    x, resid = DR.f32_data(layout.rows, 136)
    xt, rt = torch.zeros(twin.rows, 136), torch.zeros(twin.rows, 136)
    xt[idx], rt[idx] = x, resid
    yt, yt16, want_t = _dropout_f32(twin, 136, DR.SITE_EMBED, thr, "both", True, data=(xt, rt))
    _assert_contract(yt, yt16, want_t, twin.name)
    assert torch.equal(yt[idx], y32) and torch.equal(yt16[idx], y16)


# ================================================================================================ GeGLU with dropout
def _geglu(case, thr=None, layout=None, h=None, dg=None):
    """cm3p_geglu_fwd_dropout and cm3p_geglu_bwd_dropout on guarded buffers -> (g [T, I], dh [T, 2I]) on the CPU."""
    from cm3p_amd import _lib

    layout = layout or case.layout
    thr = case.thr if thr is None else thr
    T, I = layout.rows, case.I
    if h is None:
        h, dg = DR.geglu_data(T, I)
    hd, dgd = h.to(DEV), dg.to(DEV)
    gb, g = _guarded(T, I, torch.bfloat16)
    dhb, dh = _guarded(T, 2 * I, torch.bfloat16)
    lay, cu = _layout_args(layout)
    _lib.call("cm3p_geglu_fwd_dropout", _lib.ptr(hd, torch.bfloat16), _lib.ptr(g), T, I, *lay, LAYER, thr, SEED, _lib.stream())
    _lib.call("cm3p_geglu_bwd_dropout", _lib.ptr(dgd, torch.bfloat16), _lib.ptr(hd, torch.bfloat16), _lib.ptr(dh), T, I, *lay, LAYER, thr, SEED,
              _lib.stream())
    torch.cuda.synchronize()
    assert _guards_untouched(gb, T) and _guards_untouched(dhb, T)
    assert torch.equal(hd.cpu(), h) and torch.equal(dgd.cpu(), dg)
    return g.cpu(), dh.cpu()


@pytest.mark.parametrize("case", DR.GEGLU_CASES, ids=lambda c: c.name)
def test_geglu_dropout_against_float64(case):
    """g = bf16(gelu_erf(a) b Z) and dh from the unrounded dg Z against float64 within the derived bounds, exact zeros where dropped;
    packed layouts (forward AND backward) also give the bits of the padded call on the same tokens."""
    g, dh = _geglu(case)
    seen, fails = DR.check_geglu(case, g, dh)
    _note(case.name, seen)
    assert not fails, fails
    if case.layout.packed:
        twin, idx = DR.padded_twin(case.layout)
        h, dg = DR.geglu_data(case.layout.rows, case.I)
        ht, dgt = torch.zeros(twin.rows, 2 * case.I, dtype=torch.bfloat16), torch.zeros(twin.rows, case.I, dtype=torch.bfloat16)
        ht[idx], dgt[idx] = h, dg
        gt, dht = _geglu(case, layout=twin, h=ht, dg=dgt)
        assert torch.equal(gt[idx], g) and torch.equal(dht[idx], dh)


@pytest.mark.parametrize("I", [8, 136])
def test_geglu_dropout_at_the_edge_thresholds(I):
    """thr = 0 is the plain kernels bit for bit, forward and backward; thr = 65536 gives exact zeros."""
    from cm3p_amd import kernels as K

    case = DR.GEGLU_BY_NAME[f"padded-2x200-I{I}-p0.1"]
    h, dg = DR.geglu_data(case.layout.rows, I)
    g, dh = _geglu(case, thr=0)
    assert torch.equal(g, K.geglu_fwd(h.to(DEV)).cpu()) and torch.equal(dh, K.geglu_bwd(dg.to(DEV), h.to(DEV)).cpu())
    g, dh = _geglu(case, thr=65536)
    assert not g.float().any() and not dh.float().any()


# ================================================================================================ head-64 attention with dropout
def _km(case):
    km = AR.key_mask(case)
    return km.to(torch.uint8).to(DEV) if km is not None else None


def _split(case, out, lse, dqkv):
    B, S = case.B, case.S
    g = dqkv.view(B, S, 3, NH, 64).cpu()
    return dict(out=AR.heads(out.view(B, S, NH, 64)).cpu(), lse=lse.view(B, NH, S).cpu(), dq=AR.heads(g[:, :, 0]), dk=AR.heads(g[:, :, 1]),
                dv=AR.heads(g[:, :, 2]))


def _direct(case, thr, seed, layer, stages=(3,)):
    """cm3p_attn_fwd_dropout + cm3p_attn_bwd_dropout on caller-owned, guard-wrapped, NaN-filled buffers -> (out, lse, dqkv, delta, guards)."""
    from cm3p_amd import _lib

    B, S = case.B, case.S
    x = AR.inputs(case)
    qkv, do, km = x["qkv_dev"].to(DEV), x["do"].reshape(B * S, NH * 64).to(DEV), _km(case)
    out_b, out = _guarded(B * S, NH * 64, torch.bfloat16)
    dq_b, dqkv = _guarded(B * S, 3 * NH * 64, torch.bfloat16)
    lse_b, lse = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    dl_b, delta = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_fwd_dropout", ptr(qkv), ptr(out), ptr(lse), ptr(km), B, S, NH, case.window, SCALE, int(case.pre), layer, thr, seed, st())
    for stage in stages:
        _lib.call("cm3p_attn_bwd_dropout", ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dqkv), ptr(km), B, S, NH, case.window, SCALE, None, None,
                  0, stage, int(case.pre), layer, thr, seed, st())
    torch.cuda.synchronize()
    guards = dict(out=_guards_untouched(out_b, B * S), dqkv=_guards_untouched(dq_b, B * S),
                  lse=_guards_untouched(lse_b, B * NH * S, GUARD_STAT), delta=_guards_untouched(dl_b, B * NH * S, GUARD_STAT))
    return out, lse, dqkv, delta, guards


def _run(case, thr, seed=SEED, layer=LAYER):
    """One dropout forward + backward through the C entry points; a second one; the stages as two calls; the Python wrappers
    (K.attn_fwd / K.attn_bwd with drop=); the thr = 0 call and, where it runs the band kernel too, the dropout-free entry point."""
    from cm3p_amd import kernels as K

    B, S = case.B, case.S
    out, lse, dqkv, delta, guards = _direct(case, thr, seed, layer)
    out2, lse2, dqkv2, delta2, _ = _direct(case, thr, seed, layer)
    _, _, dqkv3, _, _ = _direct(case, thr, seed, layer, stages=(1, 2))
    same = dict(again=torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(dqkv2, dqkv) and torch.equal(delta2, delta),
                stages=torch.equal(dqkv3, dqkv))
    x = AR.inputs(case)
    qkv, do, km = x["qkv_dev"].to(DEV), x["do"].reshape(B * S, NH * 64).to(DEV), _km(case)
    drop = (thr, seed, layer)
    out_w, lse_w = K.attn_fwd(qkv, km, B, S, NH, case.window, SCALE, prescaled=case.pre, drop=drop)
    dqkv_w = K.attn_bwd(qkv, out_w, do, lse_w, km, B, S, NH, case.window, SCALE, prescaled=case.pre, drop=drop)
    same["wrappers"] = torch.equal(out_w, out) and torch.equal(lse_w.reshape(-1, 1), lse) and torch.equal(dqkv_w.view(B * S, -1), dqkv)
    _, lse0 = K.attn_fwd(qkv, km, B, S, NH, case.window, SCALE, prescaled=case.pre, drop=(0, seed, layer))
    same["lse_of_thr_0"] = torch.equal(lse0.reshape(-1, 1), lse)  # the statistics see the undropped probabilities
    if not K.query("cm3p_attn_fwd_impl", S, NH, case.window, int(case.pre)):  # (the pipelined forward has another summation order)
        _, lse_nd = K.attn_fwd(qkv, km, B, S, NH, case.window, SCALE, prescaled=case.pre)
        same["lse_of_the_dropout_free_call"] = torch.equal(lse_nd.reshape(-1, 1), lse)
    nan_left = any(bool(torch.isnan(t.float()).any()) for t in (out, lse, dqkv, delta))
    return dict(got=_split(case, out, lse, dqkv), guards=guards, same=same, nan_left=nan_left)


def _check_attention(case, thr, seed, layer, label):
    keep = DR.attention_keep(case, thr, seed, layer)
    p_drop = thr / 65536.0
    ref, run = AR.reference(case, keep, p_drop), _run(case, thr, seed, layer)
    got = run["got"]
    seen, fails = AR.check_float64(ref, got)
    s2, f2 = AR.check_conditioned(AR.conditioned(case, got["out"], keep, p_drop), got)
    _note(case.name, dict(seen, **s2), label)
    fails += f2 + AR.check_exact(case, ref, got)
    gone = AR.all_dropped_rows(case, keep)  # live rows whose visible keys are all dropped
    if bool(gone.any()):
        assert got["out"].float()[gone].abs().max().item() == 0.0 and bool(torch.isfinite(got["lse"][gone]).all())
    assert not fails, fails
    assert run["guards"] == dict(out=True, dqkv=True, lse=True, delta=True)
    assert not run["nan_left"]
    assert all(run["same"].values()), run["same"]
    return gone


@pytest.mark.parametrize("p", AR.DROPOUT_PS)
@pytest.mark.parametrize("case", AR.TABLE_DROP, ids=lambda c: c.name)
def test_attention_dropout_matches_float64(case, p):
    """out, dq, dk, dv against float64 with the host's keep mask within the derived bounds (P o Z in place of P), dq and dk also given
    the stored out, the exact conditions, guards untouched and no NaN left, lse bit-identical to the thr = 0 call of the same entry point
    and - where that call runs the band kernel too - to the dropout-free entry point (a global layer with pre-scaled q takes the
    pipelined forward without dropout, which sums in another order: there only the thr = 0 identity can hold), a second call the same bits, the stages DQ then DKV as two calls equal to the one call with both, the Python wrappers the same bits."""
    gone = _check_attention(case, threshold_ref(p), SEED, LAYER, f"p{p} ")
    if p == 0.5 and case.table == "A" and case.window in (0, 1):
        assert bool(gone.any())


@pytest.mark.parametrize("name", ["A-S300-w64-pad-pre", "B-S257-w127-nomask-plain", "C-S300-w33-holes-pre", "G-S449-w-1-nomask-pre"])
def test_attention_dropout_with_a_top_bit_seed_and_another_layer(name):
    _check_attention(AR.BY_NAME[name], threshold_ref(0.1), DR.SEED_TOP_BIT, DR.LAYER_HIGH, "top-bit seed, layer 11 ")


PACKED_ATTENTION = [c for c in AR.TABLE_DROP if (c.table == "A" and c.window in (1, 64, 300)) or (c.table == "G" and c.lens is not None)]
assert len(PACKED_ATTENTION) == 10


@pytest.mark.parametrize("p", AR.DROPOUT_PS)
@pytest.mark.parametrize("case", PACKED_ATTENTION, ids=lambda c: c.name)
def test_packed_attention_dropout_matches_float64(case, p):
    """cm3p_attn_fwd_dropout_varlen / cm3p_attn_bwd_dropout_varlen on the packed rows against the same float64 reference, gathered to
    the valid rows (its dO is zero on the padded query rows, which the packed call does not have), on guarded buffers of exactly
    `total` rows."""
    from cm3p_amd import _lib
    from cm3p_amd import kernels as K

    thr = threshold_ref(p)
    B, S, lens = case.B, case.S, list(case.lens)
    km = AR.key_mask(case)
    x = AR.inputs(case)
    x = dict(x, do=x["do"] * km[:, :, None, None].to(torch.bfloat16))
    keep, p_drop = DR.attention_keep(case, thr), thr / 65536.0
    ref = AR.reference(case, keep, p_drop, x=x)
    idx = torch.nonzero(km.flatten()).flatten()
    total = int(idx.numel())
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    qkv_p = x["qkv_dev"].reshape(B * S, 3, NH, 64)[idx].contiguous().to(DEV)
    do_p = x["do"].reshape(B * S, NH * 64)[idx].contiguous().to(DEV)
    out_b, out_p = _guarded(total, NH * 64, torch.bfloat16)
    dq_b, dqkv_p = _guarded(total, 3 * NH * 64, torch.bfloat16)
    lse_b, lse_flat = _guarded(NH * total, 1, torch.float32, GUARD_STAT)
    dl_b, delta = _guarded(NH * total, 1, torch.float32, GUARD_STAT)
    ptr, st = _lib.ptr, _lib.stream
    _lib.call("cm3p_attn_fwd_dropout_varlen", ptr(qkv_p), ptr(out_p), ptr(lse_flat), ptr(cu, torch.int32), B, max(lens), total, NH, case.window, SCALE,
              int(case.pre), LAYER, thr, SEED, st())
    _lib.call("cm3p_attn_bwd_dropout_varlen", ptr(qkv_p), ptr(out_p), ptr(do_p), ptr(lse_flat), ptr(delta), ptr(dqkv_p), ptr(cu, torch.int32), B, max(lens),
              total, NH, case.window, SCALE, None, None, 3, int(case.pre), LAYER, thr, SEED, st())
    torch.cuda.synchronize()
    assert _guards_untouched(out_b, total) and _guards_untouched(dq_b, total)
    assert _guards_untouched(lse_b, NH * total, GUARD_STAT) and _guards_untouched(dl_b, NH * total, GUARD_STAT)
    assert not bool(torch.isnan(delta).any())
    lse_p = lse_flat.view(NH, total)
    # the Python wrappers (which allocate their own outputs and issue the two stages as two calls) give the same bits
    drop = (thr, SEED, LAYER)
    out_w, lse_w = K.attn_fwd_varlen(qkv_p, cu, B, max(lens), NH, case.window, SCALE, case.pre, drop=drop)
    dqkv_w = K.attn_bwd_varlen(qkv_p, out_w, do_p, lse_w, cu, B, max(lens), NH, case.window, SCALE, None, case.pre, drop=drop)
    assert torch.equal(out_w, out_p) and torch.equal(lse_w, lse_p) and torch.equal(dqkv_w.reshape(total, -1), dqkv_p)
    g = dqkv_p.reshape(total, 3, NH, 64).cpu()
    got = dict(out=out_p.view(total, NH, 64).cpu(), dq=g[:, 0], dk=g[:, 1], dv=g[:, 2])  # [total, NH, 64]
    valid = km[:, None, :].expand(-1, NH, -1)  # [B, NH, S]; boolean indexing walks (b, h, s): rows of sequence b, head h

    def rows(t):  # [B, NH, S, ...] -> [total, NH, ...] in packed order
        return t.permute(0, 2, 1, *range(3, t.dim()))[km]

    seen, fails = {}, []
    for nm in ("out", "dq", "dk", "dv"):
        seen[nm], nbad = AR.ratio(got[nm], rows(ref[nm]), rows(ref["bound"][nm]))
        if nbad:
            fails.append(f"{nm}: {nbad} elements outside the bound, worst error / bound = {seen[nm]:.3f}")
    cond = AR.conditioned(case, _unpack(case, got["out"], km), keep, p_drop, x=x)
    for nm in ("dq", "dk"):
        seen[f"{nm}_given_out"], nbad = AR.ratio(got[nm], rows(cond[nm]), rows(cond["bound"][nm]))
        if nbad:
            fails.append(f"{nm} given the stored out: {nbad} elements outside the bound, worst {seen[f'{nm}_given_out']:.3f}")
    lse_want = rows(ref["lse"])  # [total, NH]
    lse_err = (lse_p.cpu().double().t() - lse_want).abs()
    seen["lse_max_abs"] = lse_err.max().item()
    assert bool((lse_err <= AR.LSE_ATOL + AR.LSE_RTOL * lse_want.abs()).all())
    assert valid.sum().item() == total * NH
    _note(case.name, seen, f"packed p{p} ")
    assert not fails, fails
    assert not any(bool(torch.isnan(t.float()).any()) for t in (out_p, lse_p, dqkv_p))
    gone = rows(AR.all_dropped_rows(case, keep))
    if bool(gone.any()):
        assert got["out"].float()[gone].abs().max().item() == 0.0


def _unpack(case, out_rows, km):
    """[total, NH, 64] of the packed rows -> [B, NH, S, 64] with zeros on the padded rows (what their stored out would multiply: dO = 0)."""
    full = torch.zeros(case.B, case.S, NH, 64, dtype=out_rows.dtype)
    full[km] = out_rows
    return AR.heads(full)
