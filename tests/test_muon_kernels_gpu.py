"""The optimizer step's kernels (csrc/muon.hip behind cm3p_muon_momentum / _normalize / _apply and cm3p_adamw_multi) and one
Newton-Schulz iteration (cm3p_amd.muon.newton_schulz_batched: three cm3p_gemm_bf16_batched calls) stage by stage against
tests/muon_refs.py: the C entry points on caller-owned, guard-wrapped buffers with hand-built address tables, every stage checked
from the kernel's own previous output - bit for bit where the stage is a chain of single IEEE operations (the momentum buffer, the
normalisation), within bounds counted from the roundings elsewhere.  Then the same seams through the Muon class.
tests/test_muon_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

The normalisation is compared bit for bit and needs no allowance: sqrtf and the fp32 division are correctly rounded under the
build's flags, and even a division a few ulp off would give the same bf16 quotient (a quotient of two bf16 numbers is a bf16 tie
exactly or at least 2^-17 away from one: tests/test_muon_refs_host.py).

CM3P_MUON_ERRORS_OUT=<file>: write the worst error / bound ratios this run measured there (profiles/muon_kernels_err.txt holds one
run's)."""
import functools
import json
import os

import pytest
import torch

import muon_refs as MR
from muon_refs import MOMENTUM, bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64         # sentinel elements before and after every buffer (256 bytes of fp32, 128 of bf16: alignment is kept)
SENTINEL = 776.0   # (97 x 2^3: exact in bf16)
NEG_LR = -0.02
NAN = float("nan")

_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_MUON_ERRORS_OUT")
    if not _SEEN or not path:
        return
    worst = {}
    for seen in _SEEN.values():
        for k, v in seen.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with open(path, "w") as f:
        json.dump(dict(worst=worst, measured=_SEEN, toolchain=dict(hip=str(torch.version.hip), torch=torch.__version__)), f, indent=1, sort_keys=True)


def _note(name, **seen):
    _SEEN.setdefault(name, {}).update(seen)
    assert all(v <= 1 for v in seen.values()), (name, seen)


def _guarded(numel, dtype, offset=0, fill=NAN):
    """[GUARD sentinels | offset sentinels | numel x fill | GUARD sentinels] -> (whole, body).  offset 1 on an fp32 buffer puts the body
    4 bytes past a 16-byte boundary.  Whatever a kernel leaves unwritten of a NaN body fails every comparison."""
    buf = torch.full((numel + 2 * GUARD + offset,), SENTINEL, dtype=dtype, device=DEV)
    body = buf[GUARD + offset:GUARD + offset + numel]
    if torch.is_tensor(fill):
        body.copy_(fill.reshape(-1))
    else:
        body.fill_(fill)
    assert body.data_ptr() % 16 == (4 * offset if dtype == torch.float32 else 0)
    return buf, body


def _guards_untouched(buf, numel, offset=0):
    lo = GUARD + offset
    assert buf.numel() == numel + lo + GUARD
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + numel:] == SENTINEL).all())


def _table(bodies):
    return torch.tensor([b.data_ptr() for b in bodies], dtype=torch.int64, device=DEV)


def _image(n, rows, cols, interior, padding):
    """A guarded bf16 [n, rp, cp] workspace image: `padding` outside rows x cols, `interior` (a value or bf16 [n, rows, cols]) inside."""
    rp, cp = MR.up8(rows), MR.up8(cols)
    whole, body = _guarded(n * rp * cp, torch.bfloat16, fill=padding)
    img = body.view(n, rp, cp)
    img[:, :rows, :cols] = interior
    return whole, body, img


def _padding_holds(img, rows, cols, value):
    keep = img.float().cpu().clone()
    keep[:, :rows, :cols] = value
    return bool((keep == value).all())


@functools.lru_cache(maxsize=None)
def _stages(rows, cols, kind, nesterov, aligned16, keep=(0, 1, 2)):
    """cm3p_muon_momentum, cm3p_muon_normalize and cm3p_muon_apply one after another on the matrices `keep` of the case's data.
    Momentum writes a workspace whose padding holds the sentinel; the normalisation runs on a zero-padded copy of its output (as
    the product's workspace is); apply reads the normalised values out of a sentinel-padded image."""
    from cm3p_amd import _lib

    ptr, st = _lib.ptr, _lib.stream
    keep = list(keep)
    n = len(keep)
    g, buf, p = (t[keep] for t in MR.stage_data(rows, cols, kind))
    rp, cp = MR.up8(rows), MR.up8(cols)
    numel, xs = rows * cols, rp * cp
    off = 0 if aligned16 else 1
    gs = [_guarded(numel, torch.float32, off, g[i]) for i in range(n)]
    bufs = [_guarded(numel, torch.float32, off, buf[i]) for i in range(n)]
    ps = [_guarded(numel, torch.float32, 0, p[i]) for i in range(n)]
    nparts = _lib.query("cm3p_muon_partials", rows, cols)
    parts_w, parts = _guarded(n * nparts, torch.float32)
    xm_w, xm, xm_img = _image(n, rows, cols, NAN, SENTINEL)
    gt, bt, pt = _table([b for _, b in gs]), _table([b for _, b in bufs]), _table([b for _, b in ps])
    out = dict(n=n, g=g, buf=buf, p=p, vec=MR.is_vec(cols, aligned16), guards={})

    _lib.call("cm3p_muon_momentum", ptr(gt), ptr(bt), ptr(xm), ptr(parts), n, rows, cols, cp, xs, MOMENTUM, int(nesterov), int(aligned16), st())
    torch.cuda.synchronize()
    out["buf2"] = torch.stack([b.cpu() for _, b in bufs]).view(n, rows, cols)
    out["g_after"] = torch.stack([b.cpu() for _, b in gs]).view(n, rows, cols)
    out["x"] = xm_img[:, :rows, :cols].cpu().contiguous()
    out["parts"] = parts.view(n, nparts).cpu().clone()
    out["momentum_padding"] = _padding_holds(xm_img, rows, cols, SENTINEL)
    out["guards"].update(g=all(_guards_untouched(w, numel, off) for w, _ in gs), buf=all(_guards_untouched(w, numel, off) for w, _ in bufs),
                         partials=_guards_untouched(parts_w, n * nparts), x_momentum=_guards_untouched(xm_w, n * xs))

    xz_w, xz, xz_img = _image(n, rows, cols, xm_img[:, :rows, :cols], 0.0)
    out["img"] = xz_img.cpu().clone()
    _lib.call("cm3p_muon_normalize", ptr(xz), ptr(parts), n, rows, cols, xs, MR.NS_EPS, st())
    torch.cuda.synchronize()
    out["xn"] = xz_img.cpu().clone()
    out["guards"].update(x_normalize=_guards_untouched(xz_w, n * xs), partials_after=_guards_untouched(parts_w, n * nparts))
    out["parts_unchanged"] = torch.equal(parts.view(n, nparts).cpu(), out["parts"])

    xa_w, xa, xa_img = _image(n, rows, cols, xz_img[:, :rows, :cols], SENTINEL)
    before = xa_w.clone()
    _lib.call("cm3p_muon_apply", ptr(pt), ptr(xa), n, rows, cols, cp, xs, MR.shape_scale(rows, cols), NEG_LR, st())
    torch.cuda.synchronize()
    out["p2"] = torch.stack([b.cpu() for _, b in ps]).view(n, rows, cols)
    out["apply_left_x_alone"] = torch.equal(before.view(torch.int16), xa_w.view(torch.int16))
    out["guards"].update(p=all(_guards_untouched(w, numel) for w, _ in ps))
    return out


# ================================================================================================ the stage kernels
@pytest.mark.parametrize("aligned16", [1, 0])
@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("rows,cols,kind", MR.STAGE_CASES)
def test_stage_kernels_against_their_references(rows, cols, kind, nesterov, aligned16):
    """Momentum (buf' bit for bit, X within its bound, each partial and their sum within theirs), the normalisation (bit for bit
    over the padded image) and apply (half an fp32 ulp of the float64 neg_lr o + p), with 16-byte aligned pointers and the float4
    kernel where cols allows it, and with g and buf 4 bytes past a boundary."""
    r = _stages(rows, cols, kind, nesterov, aligned16)
    what = f"{rows}x{cols} {kind} nesterov {nesterov} aligned16 {aligned16}"
    assert all(r["guards"].values()), (what, r["guards"])
    bits_equal(r["g_after"], r["g"], f"{what}: the gradient is read only")
    assert r["momentum_padding"], f"{what}: momentum wrote outside rows x cols"
    seen = dict(x=MR.momentum_check(r["buf2"], r["x"], r["g"], r["buf"], MOMENTUM, nesterov, what))
    blk = [MR.partials_check(r["parts"][i], r["x"][i], rows, cols, r["vec"], f"{what} [{i}]") for i in range(r["n"])]
    seen.update(partials=max(b[0] for b in blk), partials_sum=max(b[1] for b in blk))
    MR.normalize_check(r["xn"], r["img"], r["parts"], what)
    assert r["parts_unchanged"] and MR.padding_is_zero(r["xn"], rows, cols), what
    assert r["apply_left_x_alone"], f"{what}: apply wrote X"
    seen.update(p=MR.apply_check(r["p2"], r["p"], r["xn"], rows, cols, NEG_LR, what))
    _note(f"stage {rows}x{cols} {kind} nesterov={int(nesterov)} aligned16={aligned16}", **seen)


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("rows,cols,kind", [c for c in MR.STAGE_CASES if c[1] % 4 == 0])
def test_float4_and_scalar_momentum_kernels_give_the_same_bits(rows, cols, kind, nesterov):
    a, b = _stages(rows, cols, kind, nesterov, 1), _stages(rows, cols, kind, nesterov, 0)
    assert a["vec"] and not b["vec"]
    bits_equal(a["buf2"], b["buf2"], "buf'")
    bits_equal(a["x"], b["x"], "X")


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("rows,cols", MR.DATA_SHAPES)
def test_an_all_zero_matrix_stays_zero_and_leaves_its_group_alone(rows, cols, nesterov):
    """A weight no batch has used (zero gradient, zero buffer) inside a group of three: X = 0 / (0 + eps) = 0, nothing in the group
    is NaN or Inf, its parameter keeps its bits, and its neighbours come out as in a group without it."""
    z = MR.ZERO_MAT
    for aligned16 in (1, 0):
        r = _stages(rows, cols, "zero_mat", nesterov, aligned16)
        assert not r["x"][z].any() and not r["xn"][z].any() and not r["buf2"][z].any()
        assert float(r["parts"][z].abs().sum()) == 0.0
        assert bool(torch.isfinite(r["xn"].float()).all()) and bool(torch.isfinite(r["p2"]).all())
        bits_equal(r["p2"][z], r["p"][z], "the all-zero matrix's parameter")
        assert bool(r["xn"][0].any()) and bool(r["xn"][2].any())
        alone = _stages(rows, cols, "zero_mat", nesterov, aligned16, keep=(0, 2))
        assert all(alone["guards"].values())
        for name in ("buf2", "x", "parts", "xn", "p2"):
            bits_equal(r[name][[0, 2]], alone[name], f"{name} of the neighbours")


# ================================================================================================ the AdamW rule
@functools.lru_cache(maxsize=None)
def _adamw(launch, w, decay):
    from cm3p_amd import _lib

    ptr = _lib.ptr
    numels = MR.ADAMW_LAUNCHES[launch]
    data = MR.adamw_data(numels, w)
    runs = []
    for _ in range(2):
        bufs = [[_guarded(numel, torch.float32, 0, t) for t in item] for item, numel in zip(data, numels)]
        tabs = [_table([b[j][1] for b in bufs]) for j in range(4)]
        nt = torch.tensor(numels, dtype=torch.int64, device=DEV)
        _lib.call("cm3p_adamw_multi", ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]), ptr(nt), len(numels), max(numels), w[0], w[1],
                  MR.ADAMW_EPS, decay, MR.ADAMW_STEP_ALPHA, _lib.stream())
        torch.cuda.synchronize()
        runs.append(dict(out=[[b[j][1].cpu() for j in range(4)] for b in bufs],
                         guards=all(_guards_untouched(b[j][0], numel) for b, numel in zip(bufs, numels) for j in range(4))))
    return data, runs


@pytest.mark.parametrize("decay", MR.ADAMW_DECAYS)
@pytest.mark.parametrize("w", MR.ADAMW_WEIGHTS)
@pytest.mark.parametrize("launch", list(MR.ADAMW_LAUNCHES))
def test_adamw_multi_against_float64(launch, w, decay):
    """One launch over tensors from 1 to 200003 elements (64 blocks, up to 13 grid-stride passes) and one over the first three (a
    grid of one block): p', m1', m2' within the bounds counted in muon_refs.adamw_check, nothing written behind any tensor, the
    gradient untouched, and the same bits from the same state twice."""
    data, runs = _adamw(launch, w, decay)
    seen = dict(p=0.0, m1=0.0, m2=0.0)
    assert runs[0]["guards"] and runs[1]["guards"]
    for (p, g, m1, m2), first, second, numel in zip(data, runs[0]["out"], runs[1]["out"], MR.ADAMW_LAUNCHES[launch]):
        what = f"adamw {launch} {numel} w {w} decay {decay}"
        bits_equal(first[1], g, f"{what}: the gradient is read only")
        rp, r1, r2, _ = MR.adamw_check(first[0], first[2], first[3], p, g, m1, m2, w[0], w[1], MR.ADAMW_EPS, decay, MR.ADAMW_STEP_ALPHA, what)
        seen = dict(p=max(seen["p"], rp), m1=max(seen["m1"], r1), m2=max(seen["m2"], r2))
        for a, b, name in zip(first, second, ("p'", "g", "m1'", "m2'")):
            bits_equal(b, a, f"{what}: {name} of a second launch")
    _note(f"adamw {launch} w={w} decay={decay}", **seen)


# ================================================================================================ one Newton-Schulz iteration
def _ns_run(n, rows, cols, steps):
    from cm3p_amd.muon import _Group, newton_schulz_batched

    ws = _Group(n, rows, cols, DEV)
    x = MR.ns_data(n, rows, cols)
    ws.X.copy_(x)
    for t in (ws.X2, ws.A, ws.B):
        t.fill_(NAN)
    out = newton_schulz_batched(ws, steps)
    torch.cuda.synchronize()
    assert out is (ws.X2 if steps % 2 else ws.X)
    return x, ws, out


@pytest.mark.parametrize("n,rows,cols", MR.NS_CASES)
def test_one_newton_schulz_iteration_against_float64(n, rows, cols):
    """newton_schulz_batched(ws, 1) on a _Group: A from X, B from the kernel's A, X' from the kernel's B and X, each within the
    bf16 rounding of the float64 value plus the fp32 accumulation term; the padding of X' is bit-zero and X is left as it was.  The
    two ring cases check 3 distinct matrices against float64 and every one of the 32 against the matrix it copies."""
    x, ws, out = _ns_run(n, rows, cols, 1)
    what = f"ns {n}x{rows}x{cols}"
    bits_equal(ws.X.cpu(), x, f"{what}: the input image")
    A, B, Xn = ws.A.cpu(), ws.B.cpu(), out.cpu()
    assert MR.padding_is_zero(Xn, rows, cols), f"{what}: padding of X'"
    pick = list(range(n))
    if (n, rows, cols) in MR.NS_RING:
        order = MR.ns_ring_order(n)
        pick = [int((order == d).nonzero()[0]) for d in range(MR.NS_RING_DISTINCT)]
        for i in range(n):
            for t, name in ((A, "A"), (B, "B"), (Xn, "X'")):
                bits_equal(t[i], t[pick[int(order[i])]], f"{what}: {name}[{i}] against the matrix it copies")
    ra, rb, rx = MR.ns_check(A[pick], B[pick], Xn[pick], x[pick], what)
    _note(what, ns_a=ra, ns_b=rb, ns_x=rx)


@pytest.mark.parametrize("n,rows,cols", MR.NS_ODD + MR.NS_RING[:1])
def test_six_iterations_keep_the_padding_zero_and_everything_finite(n, rows, cols):
    _, ws, out = _ns_run(n, rows, cols, 6)
    for t in (ws.X, ws.X2):
        assert MR.padding_is_zero(t.cpu(), rows, cols)
    for t in (ws.X, ws.X2, ws.A, ws.B):
        assert bool(torch.isfinite(t.float()).all())
    if (n, rows, cols) in MR.NS_ODD:  # (the host test holds the fp32 path to the same band)
        sv = torch.linalg.svdvals(out[0, :rows, :cols].float().cpu())
        assert 0.3 < float(sv.min()) and float(sv.max()) < 1.7, sv


# ================================================================================================ through the Muon class
def _offset_view(t):
    """The same values in a view that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _class_steps(shapes, n, misalign, steps=2):
    from cm3p_amd.muon import Muon

    gn = MR.gen("muon-class", tuple(shapes), n)
    init = {(s, i): torch.randn(s, generator=gn) * 0.5 for s in shapes for i in range(n)}
    grads = [{k: torch.randn(k[0], generator=gn) * 0.1 for k in init} for _ in range(steps)]
    params = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in init.items()}
    opt = Muon(muon_params=list(params.values()), lr=0.02, momentum=MOMENTUM, nesterov=True, ns_steps=6)
    for s in range(steps):
        for k, p in params.items():
            g = grads[s][k].to(DEV)
            p.grad = _offset_view(g) if misalign and k[1] == 0 else g
        opt.step()
    torch.cuda.synchronize()
    return params, grads, opt


def test_two_steps_of_the_class_at_the_block_seams_aligned_and_not():
    """Two 1032 x 1020 and two 129 x 128 weights, two steps, one gradient of each group handed over 4 bytes off a 16-byte boundary
    (the whole group then takes the scalar kernel): the momentum buffers are the two-rounding fp32 recurrence bit for bit, the
    workspaces' padding is still zero, and the parameters equal those of a run with aligned gradients bit for bit."""
    shapes = [(1032, 1020), (129, 128)]
    runs = {mis: _class_steps(shapes, 2, mis) for mis in (False, True)}
    m = MR.f32(MOMENTUM)
    for mis, (params, grads, opt) in runs.items():
        for k, p in params.items():
            want = (grads[0][k] * m) + grads[1][k]  # buf1 = fl(0 m) + g1 = g1
            bits_equal(opt.state[p]["momentum_buffer"].cpu(), want, f"momentum_buffer {k} misaligned {mis}")
        assert len(opt._workspaces) == len(shapes)
        for (_, (rows, cols)), ws in opt._workspaces.items():
            assert ws.n == 2 and MR.padding_is_zero(ws.X.cpu(), rows, cols) and MR.padding_is_zero(ws.X2.cpu(), rows, cols), (rows, cols, mis)
            assert bool(torch.isfinite(ws.X.float()).all())
    for k in runs[False][0]:
        bits_equal(runs[True][0][k].detach().cpu(), runs[False][0][k].detach().cpu(), f"parameter {k}: misaligned against aligned")
        assert not torch.equal(runs[False][0][k].detach().cpu(), torch.zeros(k[0]))


def test_a_weight_with_an_all_zero_gradient_keeps_its_bits():
    """Three 13 x 21 weights without nesterov (u = g): after a first step that filled the buffers, the second weight's gradient is
    all zero - X = 0 / (0 + eps) = 0, its parameter keeps its bits, its buffer becomes fl(momentum buf), the others step."""
    from cm3p_amd.muon import Muon

    gn = MR.gen("muon-class-zero")
    params = [torch.nn.Parameter((torch.randn(13, 21, generator=gn) * 0.5).to(DEV)) for _ in range(3)]
    opt = Muon(muon_params=params, lr=0.02, momentum=MOMENTUM, nesterov=False, ns_steps=6)
    for p in params:
        p.grad = (torch.randn(13, 21, generator=gn) * 0.1).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    before = [p.detach().cpu().clone() for p in params]
    bufs = [opt.state[p]["momentum_buffer"].cpu().clone() for p in params]
    for i, p in enumerate(params):
        p.grad = torch.zeros(13, 21, device=DEV) if i == 1 else (torch.randn(13, 21, generator=gn) * 0.1).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    bits_equal(params[1].detach().cpu(), before[1], "the parameter with a zero gradient")
    bits_equal(opt.state[params[1]]["momentum_buffer"].cpu(), bufs[1] * MR.f32(MOMENTUM), "its momentum buffer")
    assert bool(bufs[1].any())
    for i in (0, 2):
        assert not torch.equal(params[i].detach().cpu(), before[i]) and bool(torch.isfinite(params[i]).all())
