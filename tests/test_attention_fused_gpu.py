"""cm3p_attn_bwd_fused (csrc/attention_bwd_fused.hip) past one dQ slab, against float64: table F of tests/attention_fused_refs.py at
G = 2 and G = 4 key blocks per slab - more than one slab, adding launches at group positions 2 and 3, partial last groups, every residue
of the ring's unroll, a global mask with holes -, the inverse RoPE of both epilogues, the packed form, a count probe, one valid key
block moved along the sequence (exact), and the length rule that picks G = 4.  The C entry is called directly on guard-wrapped,
NaN-filled dqkv and on a workspace of exactly cm3p_attn_bwd_fused_workspace_bytes bytes between sentinel guards that is filled with NaN
bytes before every call: the header promises that nothing is carried between calls, so a slab element that reaches dq without having been
written shows as NaN.  out and lse come from cm3p_attn_fwd on the same case and are checked against float64 too.
tests/test_attention_fused_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

CM3P_FUSED_ERRORS_OUT=<file>: write the worst error / bound ratios this run measured there (profiles/attention_fused_err.txt holds one run's)."""
import contextlib
import functools
import json
import os

import pytest
import torch

import attention_fused_refs as AF
import attention_refs as AR
from attention_fused_refs import TABLE_F
from attention_refs import NH, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4           # sentinel rows before and after out / dqkv
GUARD_STAT = 64     # sentinel floats before and after lse
GUARD_WS = 256      # sentinel bytes before and after the workspace (keeps its 16-byte alignment)
SENTINEL = 777.0    # (exact in bf16)
SENTINEL_BYTE = 0x5A
PREP, MAIN, REDUCE, MAIN_EVEN, MAIN_ODD, ADD1 = 1, 2, 4, 8, 16, 32
ENV = "CM3P_FUSED_SLAB_GROUP"

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_FUSED_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for key, seen in _SEEN.items():
        G = key.split()[1]
        for k, v in seen.items():
            worst[f"{G} {k}"] = max(worst.get(f"{G} {k}", 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f, indent=1, sort_keys=True)


def _note(case, G, seen, what=""):
    _SEEN.setdefault(f"{case.name} G{G}", {}).update({(what + " " if what else "") + k: v for k, v in seen.items()})
    print(f"{case.name} G{G} {what}: " + "  ".join(f"{k}={v:.3g}" for k, v in seen.items()))


@contextlib.contextmanager
def _group(G):
    """CM3P_FUSED_SLAB_GROUP = G for the calls inside (None: unset - the library's length rule); the library reads it per call."""
    old = os.environ.get(ENV)
    if G is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = str(G)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


@functools.lru_cache(maxsize=None)
def _reference(case, packed=False):
    return AR.reference(case, x=AF.padded_rows_zeroed(case) if packed else None)


def _guarded(rows, cols, dtype, guard):
    buf = torch.full((rows + 2 * guard, cols), SENTINEL, dtype=dtype, device=DEV)
    buf[guard:guard + rows] = float("nan")  # whatever the kernels leave unwritten fails every comparison
    return buf, buf[guard:guard + rows]


def _guards_untouched(buf, rows, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + rows:] == SENTINEL).all())


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _forward(qkv, km, B, S, pre):
    """cm3p_attn_fwd (global) on guard-wrapped, NaN-filled buffers -> out [B S, NH 64], lse [B NH S, 1], guards."""
    from cm3p_amd import _lib

    out_b, out = _guarded(B * S, NH * 64, torch.bfloat16, GUARD)
    lse_b, lse = _guarded(B * NH * S, 1, torch.float32, GUARD_STAT)
    _lib.call("cm3p_attn_fwd", _lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(km), B, S, NH, -1, SCALE, int(pre), _lib.stream())
    torch.cuda.synchronize()
    return out, lse, _guards_untouched(out_b, B * S, GUARD) and _guards_untouched(lse_b, B * NH * S, GUARD_STAT)


def _fused(qkv, out, do, lse, km, B, S, pre, stages=(7,), rope=None, stride=0, cu=None, total=0):
    """cm3p_attn_bwd_fused through _lib.call, one call per entry of `stages`: dqkv guard-wrapped and NaN-filled, the workspace exactly
    cm3p_attn_bwd_fused_workspace_bytes bytes between sentinel guards and filled with NaN bytes (0xFF: a NaN as bf16 and as fp32) -> dqkv
    [rows, 3 NH 64], True if no guard was touched."""
    from cm3p_amd import _lib

    rows = total if cu is not None else B * S
    need = _lib.query("cm3p_attn_bwd_fused_workspace_bytes", B, S, NH)
    assert need == AF.workspace_bytes(B, S, NH)
    ws_b = torch.full((need + 2 * GUARD_WS,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    ws = ws_b[GUARD_WS:GUARD_WS + need]
    ws.fill_(0xFF)
    dq_b, dqkv = _guarded(rows, 3 * NH * 64, torch.bfloat16, GUARD)
    cos, sin = rope if rope is not None else (None, None)
    ptr = _lib.ptr
    for stage in stages:
        _lib.call("cm3p_attn_bwd_fused", ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), ptr(km), ptr(cu), B, S, total if cu is not None else 0, NH,
                  SCALE, ptr(cos), ptr(sin), stride, stage, int(pre), ptr(ws), need, _lib.stream())
    torch.cuda.synchronize()
    ok = (_guards_untouched(dq_b, rows, GUARD) and bool((ws_b[:GUARD_WS] == SENTINEL_BYTE).all()) and bool((ws_b[GUARD_WS + need:] == SENTINEL_BYTE).all()))
    return dqkv, ok


def _split(case, out, lse, dqkv):
    """The device layouts -> tests/attention_refs.py's [B, NH, S, 64] on the CPU."""
    B, S = case.B, case.S
    got = dict(out=AR.heads(out.view(B, S, NH, 64)).cpu(), lse=lse.view(B, NH, S).cpu())
    if dqkv is not None:
        g = dqkv.view(B, S, 3, NH, 64).cpu()
        got.update(dq=AR.heads(g[:, :, 0]), dk=AR.heads(g[:, :, 1]), dv=AR.heads(g[:, :, 2]))
    return got


def _device_inputs(case, packed_do=False):
    x = AF.padded_rows_zeroed(case) if packed_do else AR.inputs(case)
    km = AR.key_mask(case)
    return _dev(x["qkv_dev"]), _dev(x["do"].reshape(case.B * case.S, NH * 64)), (_dev(km.to(torch.uint8)) if km is not None else None)


@functools.lru_cache(maxsize=None)
def _fwd(case):
    qkv, _, km = _device_inputs(case)
    return _forward(qkv, km, case.B, case.S, case.pre)


def _rope_dev(case, form):
    cos, sin, _ = AF.rope_tables(case, form)
    return _dev(cos), _dev(sin)


@functools.lru_cache(maxsize=None)
def _run(case, G):
    """One forward (shared by both G) + the fused backward under CM3P_FUSED_SLAB_GROUP = G; the same again; the stages as PREP, MAIN_EVEN,
    MAIN_ODD, REDUCE and as one launch per call (what K._attn_bwd_fused issues); the Python wrapper."""
    from cm3p_amd import _lib
    from cm3p_amd import kernels as K

    B, S = case.B, case.S
    qkv, do, km = _device_inputs(case)
    out, lse, fwd_guards = _fwd(case)
    with _group(G):
        assert _lib.query("cm3p_attn_bwd_fused_slab_group", S) == G
        dqkv, ok = _fused(qkv, out, do, lse, km, B, S, case.pre)
        dqkv2, ok2 = _fused(qkv, out, do, lse, km, B, S, case.pre)
        dqkv3, ok3 = _fused(qkv, out, do, lse, km, B, S, case.pre, stages=(PREP, MAIN_EVEN, MAIN_ODD, REDUCE))
        adds = [ADD1 << (p - 1) for p in range(1, min(G, AF.key_blocks(S)))]
        dqkv4, ok4 = _fused(qkv, out, do, lse, km, B, S, case.pre, stages=(PREP, MAIN_EVEN, *adds, REDUCE))
        dqkv_w = K.attn_bwd(qkv, out, do, lse.view(B, NH, S), km, B, S, NH, -1, SCALE, prescaled=case.pre)
        torch.cuda.synchronize()
    same = dict(again=torch.equal(dqkv2, dqkv), four_stages=torch.equal(dqkv3, dqkv), one_launch_per_call=torch.equal(dqkv4, dqkv),
                wrapper=torch.equal(dqkv_w.view(B * S, -1), dqkv))
    return dict(got=_split(case, out, lse, dqkv), dqkv=dqkv.cpu(), guards=fwd_guards and ok and ok2 and ok3 and ok4, same=same)


CASES_G = [(c, G) for c in TABLE_F for G in AF.groups_of(c)]
_ids = [f"{c.name}-G{G}" for c, G in CASES_G]


def test_the_binding_and_the_references_agree():
    from cm3p_amd import kernels as K

    assert K.SOFTMAX_Q_SCALE == AR.SOFTMAX_Q_SCALE
    assert (K.ATTN_BWD_FUSED_PREP, K.ATTN_BWD_FUSED_MAIN, K.ATTN_BWD_FUSED_REDUCE, K.ATTN_BWD_FUSED_MAIN_EVEN, K.ATTN_BWD_FUSED_MAIN_ODD,
            K.ATTN_BWD_FUSED_MAIN_ADD1) == (PREP, MAIN, REDUCE, MAIN_EVEN, MAIN_ODD, ADD1)
    for case in TABLE_F:  # pre-scaled q: the pipelined forward; plain q: the three-wave one
        assert bool(K.query("cm3p_attn_fwd_impl", case.S, NH, -1, int(case.pre))) == case.pre, case.name


@pytest.mark.parametrize("case,G", CASES_G, ids=_ids)
def test_matches_float64(case, G):
    """out and lse of cm3p_attn_fwd, dq, dk, dv of cm3p_attn_bwd_fused against float64 within the componentwise bounds (dq: the G-dependent
    one), dq and dk also against the float64 backward that takes delta from the stored out; dead rows and masked keys exact zeros, no NaN
    (no slab element reached dq unwritten), no guard of out, lse, dqkv or the workspace touched."""
    ref, run = _reference(case), _run(case, G)
    seen, fails = AR.check_float64(ref, run["got"], fused=True, G=G)
    s2, f2 = AR.check_conditioned(AR.conditioned(case, run["got"]["out"]), run["got"], fused=True, G=G)
    _note(case, G, dict(seen, **s2))
    fails = fails + f2 + AR.check_exact(case, ref, run["got"])
    assert not fails, fails
    assert run["guards"]


@pytest.mark.parametrize("case,G", CASES_G, ids=_ids)
def test_same_bits(case, G):
    """A second call, the four stages as four calls, one launch per call and the Python wrapper give the bits of the single call; dk and dv
    do not depend on the slabs: the same bits at G = 2 and G = 4."""
    run = _run(case, G)
    assert all(run["same"].values()), run["same"]
    if G == 4:
        other = _run(case, 2)
        for nm in ("dk", "dv"):
            assert torch.equal(run["got"][nm], other["got"][nm]), nm


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
def test_one_valid_key_block_moved_along_the_sequence(pre):
    """S = 1280 (five exact key blocks), only the keys of block j valid, j = 0 .. 4, and the K, V and mask rows of that block the same 256
    rows in every run; q, dO, out and lse (one forward, run 0) are the same.  The other blocks' K-image rows are zeros, their partials
    exact zeros that are stored or added, and the reduce adds exact zeros: dq is the same in all five runs (torch.equal), at G = 2 and at
    G = 4; the block's dk / dv rows are the same rows at another place, every other dk / dv row is exactly zero."""
    S = AF.RELOC_S
    _, do_h, _, _, _, _ = AF.relocation_data()
    do = _dev(do_h.reshape(S, NH * 64))
    qkv0, km0 = AF.relocation_qkv(0, pre)
    out, lse, guards = _forward(_dev(qkv0), _dev(km0.to(torch.uint8)), 1, S, pre)
    assert guards and not bool(torch.isnan(out.float()).any()) and bool(torch.isfinite(lse).all())
    for G in (2, 4):
        first = None
        for j in range(AF.RELOC_BLOCKS):
            qkv, km = AF.relocation_qkv(j, pre)
            with _group(G):
                dqkv, ok = _fused(_dev(qkv), out, do, lse, _dev(km.to(torch.uint8)), 1, S, pre)
            assert ok
            g = dqkv.view(S, 3, NH, 64).cpu()
            assert not bool(torch.isnan(g.float()).any())
            blk = slice(256 * j, 256 * j + 256)
            dq, dkv_blk = g[:, 0], g[blk, 1:]
            rest = torch.ones(S, dtype=torch.bool)
            rest[blk] = False
            assert g[rest, 1:].float().abs().max().item() == 0.0, (G, j)
            assert dq.float().abs().max().item() > 0.0 and dkv_blk.float().abs().max().item() > 0.0
            if first is None:
                first = (dq, dkv_blk)
            else:
                assert torch.equal(dq, first[0]), (G, j, "dq")
                assert torch.equal(dkv_blk, first[1]), (G, j, "dk / dv of the block")


ROPE_CASES = [(c, G, form) for c in TABLE_F if c.S in AF.ROPE_S for G in AF.groups_of(c) for form in ("shared", "batch")]


@pytest.mark.parametrize("case,G,form", ROPE_CASES, ids=[f"{c.name}-G{G}-{f}" for c, G, f in ROPE_CASES])
def test_rope_epilogues_match_float64(case, G, form):
    """cos / sin tables: dq (the reduce) and dk (the main kernel's epilogue) against the inverse rotation of the float64 reference within
    the rotated bounds, with pos_batch_stride 0 (one table) and S (batch b at positions 7 b ..); dv is the call's without tables, bit for
    bit; the Python wrapper gives the same bits."""
    from cm3p_amd import kernels as K

    B, S = case.B, case.S
    ref, plain = _reference(case), _run(case, G)
    qkv, do, km = _device_inputs(case)
    out, lse, _ = _fwd(case)
    cos, sin = _rope_dev(case, form)
    stride = S if form == "batch" else 0
    with _group(G):
        dqkv, ok = _fused(qkv, out, do, lse, km, B, S, case.pre, rope=(cos, sin), stride=stride)
        dqkv_w = K.attn_bwd(qkv, out, do, lse.view(B, NH, S), km, B, S, NH, -1, SCALE, rope=(cos, sin), per_batch=form == "batch", prescaled=case.pre)
        torch.cuda.synchronize()
    assert ok and torch.equal(dqkv_w.view(B * S, -1), dqkv)
    got = _split(case, out, lse, dqkv)
    assert torch.equal(got["dv"], plain["got"]["dv"])
    assert not torch.equal(got["dq"], plain["got"]["dq"]) and not torch.equal(got["dk"], plain["got"]["dk"])
    tabs = AF.rope_tables(case, form)
    seen, fails = AF.check_rotated(AF.rotated(ref, *tabs, G), got)
    s2, f2 = AF.check_rotated(AF.rotated(AR.conditioned(case, got["out"]), *tabs, G), got)
    _note(case, G, dict(seen, **{k + "_given_out": v for k, v in s2.items()}), form)
    assert not fails + f2 + AR.check_exact(case, ref, got), fails + f2


PACKED_CASES = [(c, G) for c, G in CASES_G if c.lens]


@pytest.mark.parametrize("case,G", PACKED_CASES, ids=[f"{c.name}-G{G}" for c, G in PACKED_CASES])
def test_packed_equals_padded_and_matches_float64(case, G):
    """cu_seqlens on the packed rows (forward: cm3p_attn_fwd_varlen), without tables and with per-token tables whose sequences start at
    positions 7 b: the bits of the padded call (dO zero on padded rows; tables per batch at 7 b) on every valid row, and the packed
    result itself within the float64 bounds."""
    from cm3p_amd import kernels as K

    B, S, lens = case.B, case.S, list(case.lens)
    km_h = AR.key_mask(case)
    qkv, do, km = _device_inputs(case, packed_do=True)
    out, lse, _ = _fwd(case)
    idx = torch.nonzero(km_h.flatten()).flatten().to(DEV)
    total = int(idx.numel())
    cu = torch.tensor(AF.cu_seqlens(case), dtype=torch.int32, device=DEV)
    qkv_p = qkv.reshape(B * S, 3, NH, 64)[idx].contiguous()
    do_p = do[idx].contiguous()
    out_p, lse_p = K.attn_fwd_varlen(qkv_p, cu, B, max(lens), NH, -1, SCALE, case.pre)
    torch.cuda.synchronize()
    assert torch.equal(out_p, out[idx])
    assert torch.equal(lse_p, lse.view(B, NH, S).permute(1, 0, 2).reshape(NH, B * S)[:, idx])
    ref = _reference(case, packed=True)
    for form in (None, "packed"):
        with _group(G):
            pad, ok = _fused(qkv, out, do, lse, km, B, S, case.pre, rope=_rope_dev(case, "batch") if form else None, stride=S if form else 0)
            pk, ok_p = _fused(qkv_p, out_p, do_p, lse_p, None, B, max(lens), case.pre, rope=_rope_dev(case, "packed") if form else None, cu=cu, total=total)
            pk_w = K.attn_bwd_varlen(qkv_p, out_p, do_p, lse_p, cu, B, max(lens), NH, -1, SCALE, _rope_dev(case, "packed") if form else None, case.pre)
            torch.cuda.synchronize()
        assert ok and ok_p
        assert torch.equal(pk, pad[idx]), form
        assert torch.equal(pk_w.reshape(total, -1), pk), form
        full = torch.zeros(B * S, 3 * NH * 64, dtype=torch.bfloat16, device=DEV)
        full[idx] = pk
        got = _split(case, out, lse, full)
        cond = AR.conditioned(case, got["out"], x=AF.padded_rows_zeroed(case))
        if form:
            tabs = AF.rope_tables(case, "batch")  # (the same table row for every valid (b, row) as the per-token table's)
            seen, fails = AF.check_rotated(AF.rotated(ref, *tabs, G), got)
            s2, f2 = AF.check_rotated(AF.rotated(cond, *tabs, G), got)
            s2 = {k + "_given_out": v for k, v in s2.items()}
            s3, f3 = AR.check_float64(ref, got, quantities=("dv",))
            seen.update(s3)
            fails += f3
        else:
            seen, fails = AR.check_float64(ref, got, fused=True, G=G, quantities=("dq", "dk", "dv"))
            s2, f2 = AR.check_conditioned(cond, got, fused=True, G=G)
        _note(case, G, dict(seen, **s2), "packed rope" if form else "packed")
        assert not fails + f2 + AR.check_exact(case, ref, got), (form, fails + f2)


PROBE_CASES = [AR.Case("F", 513, -1, (513, 256, 65), pre, True) for pre in (False, True)] + [AR.Case("F", 1300, -1, None, pre, True, True) for pre in (False, True)]


@pytest.mark.parametrize("case", PROBE_CASES, ids=lambda c: c.name)
def test_count_probe(case):
    """q = k = 0: lse = ln n_vis(q), the exact count of every row's visible keys (half of ln((n + 1) / n) at n = 1300 is 3.8e-4, the
    tolerance 1e-4), out = (sum of +-1) / n to one fp32 product and the bf16 store, dq = dk = 0 exactly - at G = 2 and G = 4."""
    ref = AR.reference(case)
    for G in (2, 4):
        run = _run(case, G)
        seen, fails = AR.check_probe(case, ref, run["got"])
        seen["out"], nbad = AR.ratio(run["got"]["out"], ref["out"], AR.probe_out_bound(ref))
        _note(case, G, seen, "probe")
        assert not fails + AR.check_exact(case, ref, run["got"]) and not nbad, (fails, nbad)
        assert run["guards"] and all(run["same"].values())
    assert int(ref["nvis"].max()) == case.S if not case.holes else int(ref["nvis"].max()) == 1299


def test_the_length_rule_picks_four_key_blocks_per_slab():
    """S = 5900 (24 key blocks), no override: the library's own choice is G = 4.  dq of three query tiles - tile 0, one in the middle, the
    ragged last one - against the row-subset float64 reference within the G = 4 bound; the whole dqkv is the call's under
    CM3P_FUSED_SLAB_GROUP=4 bit for bit, dk / dv the call's under =2."""
    from cm3p_amd import _lib

    case = AR.Case("F", AF.LONG_S, -1, None, True, False, False, 1)
    B, S = 1, case.S
    qkv, do, km = _device_inputs(case)
    out, lse, guards = _forward(qkv, km, B, S, True)
    with _group(None):
        assert _lib.query("cm3p_attn_bwd_fused_slab_group", S) == 4 and _lib.query("cm3p_attn_bwd_fused_slab_group", 5888) == 2
        dqkv, ok = _fused(qkv, out, do, lse, km, B, S, True)
    with _group(4):
        dqkv4, ok4 = _fused(qkv, out, do, lse, km, B, S, True)
    with _group(2):
        dqkv2, ok2 = _fused(qkv, out, do, lse, km, B, S, True)
    assert guards and ok and ok4 and ok2
    assert torch.equal(dqkv, dqkv4)
    third = NH * 64
    assert torch.equal(dqkv[:, third:], dqkv2[:, third:]) and not torch.equal(dqkv[:, :third], dqkv2[:, :third])
    assert not bool(torch.isnan(dqkv.float()).any())
    rows = AF.long_rows()
    full = _split(case, out, lse, dqkv)
    got = {nm: full[nm][:, :, rows] for nm in ("out", "lse", "dq")}
    ref = AR.reference(case, rows=rows)
    seen, fails = AR.check_float64(ref, got, fused=True, G=4, quantities=("out", "lse", "dq"))
    s2, f2 = AR.check_conditioned(AR.conditioned(case, got["out"], rows=rows), got, fused=True, G=4)
    _note(case, 4, dict(seen, **s2), "three tiles")
    assert not fails + f2, fails + f2
