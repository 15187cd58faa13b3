"""Cross-rank negatives for (B, V, L) metadata-variation training batches (cm3p_amd/dist.py) on the real kernels.

Parity definition: with DDP's gradient averaging, the mean of the per-rank losses equals the reference's 3-D cm3p_loss on the
concatenated (N*b, V, N*b) batch, and the averaged gradients equal its gradients.

1. simulated ranks in one process (`variation_head` has no collective in it) against float64, held to 3 x the error of the existing
   single-process head on the same values;  2. a world-1 RCCL group: gather on == gather off, exactly two all-gathers;
3. eval mode stays rank-local;  4. two ranks under DDP on the reference-made fixture d64_variations.
"""
import os
import socket
import warnings
import zlib

import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

from cases import CASES

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
NAME = "d64_variations"
LOSS_TOL_FIXTURE = 3e-2  # tests/test_model_gpu.py FIX_TOL["loss"]
LAYOUT_ATOL = 1e-3


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build(name=NAME):
    from cm3p_amd import CM3PConfig, CM3PModel

    model = CM3PModel(CM3PConfig(**CASES[name]["cfg"]))
    sd = load_file(os.path.join(GOLD, "weights_d64.safetensors"))
    blob = load_file(os.path.join(GOLD, f"{name}.safetensors"))
    sd.update({k[2:]: v for k, v in blob.items() if k.startswith("w.")})
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train()


def _inputs(blob):
    return {k[3:]: v.to("cuda") for k, v in blob.items() if k.startswith("in.")}  # the CURRENT device


# ------------------------------------------------------------------------------------ 1. simulated ranks, one process
def _leaf(t):
    return t.to(DEV).clone().requires_grad_(True)  # a leaf of its own on the device


def _classes(n, V, g):
    """One class-0 slot per row at (i + 1) % V (varies, not always slot 0), classes 1 / 2 elsewhere, one -1 (padding) class in row 0."""
    classes = torch.randint(1, 3, (n, V), generator=g)
    slot = (torch.arange(n) + 1) % V
    classes[torch.arange(n), slot] = 0
    classes[0, (slot[0] + 1) % V] = -1
    return classes


@pytest.mark.parametrize("N,b,V,P", [(4, 2, 3, 32), (2, 3, 5, 64), (2, 2, 256, 512)])  # the last: the recipe's V, 1024 columns in a row
def test_simulated_ranks_match_float64_reference_loss_and_gradients(N, b, V, P, monkeypatch):
    """Every rank r of N driven through `variation_head` with its own slices; the "gathered" buffers are separate leaves whose gradients
    accumulate over the loop (what the reduce-scatter sums).  Reference: float64 O.cm3p_loss on the concatenated batch, autograd.
    Bound per quantity (loss, d me, d be, d logit_scale; largest absolute error): 3 x the error of the EXISTING single-process path
    (_LogitsFn + cm3p_loss_hip on the concatenated batch in one piece) against the same float64 values, + 1e-6.  3: the gathered form
    keeps the two directions' dlogits in two buffers and runs two GEMMs where the local form sums them into one; a few more roundings,
    nothing larger."""
    from cm3p_amd import kernels as K
    from cm3p_amd import modeling_cm3p as M
    from cm3p_amd.dist import variation_head
    from oracle import cm3p_oracle as O

    g = torch.Generator().manual_seed(zlib.crc32(repr((N, b, V, P)).encode()))
    n = N * b
    me0 = O.l2_normalize(torch.randn(n, V, P, generator=g))  # fp32 values, the same on every side
    be0 = O.l2_normalize(torch.randn(n, P, generator=g))
    s0 = torch.tensor(2.6592600)  # log(1 / 0.07), the reference's logit_scale_init_value
    classes = _classes(n, V, g)

    # float64 reference on the concatenated batch
    me64, be64, s64 = (t.double().requires_grad_(True) for t in (me0, be0, s0))
    sim64 = (me64.reshape(n * V, P) @ be64.t() * s64.exp()).view(n, V, n)
    ref_loss = O.cm3p_loss(sim64, classes)
    ref_loss.backward()
    ref = dict(loss=ref_loss.detach(), me=me64.grad, be=be64.grad, logit_scale=s64.grad)

    def errors(loss, gme, gbe, gs):
        got = dict(loss=torch.as_tensor(loss, dtype=torch.float64), me=gme, be=gbe, logit_scale=gs)
        return {k: (got[k].detach().double().cpu() - ref[k]).abs().max().item() for k in ref}

    # the existing single-process path, in one piece
    me_l, be_l, s_l = (_leaf(t) for t in (me0, be0, s0))
    lpm = M._LogitsFn.apply(me_l.reshape(n * V, P), be_l, s_l)
    loss_l = M.cm3p_loss_hip(lpm.view(n, V, n), classes.to(DEV))
    loss_l.backward()
    e_local = errors(loss_l.item(), me_l.grad, be_l.grad, s_l.grad)

    # the gathered form, rank by rank; every CE launch recorded
    calls = []
    orig = M._CrossEntropySumFn

    class _Rec:
        @staticmethod
        def apply(specs, *logits):
            calls.append((specs, [l.detach() for l in logits]))
            return orig.apply(specs, *logits)

    monkeypatch.setattr(M, "_CrossEntropySumFn", _Rec)
    me_g, be_g, s_g = (_leaf(t) for t in (me0, be0, s0))
    m_all = _leaf(me0)  # (N*b, V, P) in rank, row, variation order
    b_all = _leaf(be0)
    idx = K.first_zero_index(classes.to(DEV))
    assert torch.equal(idx.cpu(), O.true_variation_index(classes))
    losses = []
    for r in range(N):
        sl = slice(r * b, (r + 1) * b)
        lpm_r, lpb_r, loss_r = variation_head(me_g[sl], be_g[sl], m_all, b_all, idx[sl], r, s_g)
        assert lpm_r.shape == (b, V, n) and lpb_r.shape == (b, n * V)
        # layout: this rank's logits are its rows of the global tensor, both ways.  A wrong row is off by O(1); LAYOUT_ATOL is above the
        # worst case of an fp32 dot product of unit vectors times e^s, P u e^s = 512 x 6e-8 x 14.3 = 4.4e-4
        assert torch.allclose(lpm_r.detach().double().cpu(), sim64[sl].detach(), atol=LAYOUT_ATOL)
        assert torch.allclose(lpb_r.detach().double().cpu().view(b, n, V), sim64.detach().permute(2, 0, 1)[sl], atol=LAYOUT_ATOL)
        losses.append(loss_r)
    (torch.stack(losses).sum() / N).backward()  # DDP's average of the rank gradients
    mean_loss = sum(l.double().item() for l in losses) / N
    e_gath = errors(mean_loss, me_g.grad + m_all.grad, be_g.grad + b_all.grad, s_g.grad)

    # (`pytest -rP` shows the line; profiles/gathered_variations_err.txt holds the lines of one MI355X run)
    print(f"N={N} b={b} V={V} P={P}: " + "  ".join(
        f"{k}: gathered {e_gath[k]:.3e} local {e_local[k]:.3e} bound {3 * e_local[k] + 1e-6:.3e}" for k in ref))
    for k in ref:
        assert e_gath[k] <= 3 * e_local[k] + 1e-6, (k, e_gath[k], e_local[k])

    # every captured CE spec row against float64 on the kernel's own logits (the bound of
    # test_cross_entropy_with_the_specs_of_the_contrastive_loss)
    assert len(calls) == N
    for r, (specs, logits) in enumerate(calls):
        assert len(specs) == 2 and [s[0] for s in specs] == [0, 1]
        for (ti, rows, cols, rs, cs, roff, target, coef) in specs:
            L = logits[ti].contiguous()
            loss_rows = K.cross_entropy(L, rows, cols, rs, cs, target, roff, coef / rows, None)
            base = roff.cpu() if roff is not None else torch.arange(rows) * rs
            pos = base[:, None] + torch.arange(cols)[None, :] * cs
            assert int(pos.min()) >= 0 and int(pos.max()) < L.numel()
            x = L.reshape(-1).double().cpu()[pos]
            t = target.cpu()
            lse = torch.logsumexp(x, 1)
            xt = x[torch.arange(rows), t]
            want = F.cross_entropy(x, t, reduction="none")
            bound = 1e-6 + 1e-6 * (lse.abs() + xt.abs())
            err = (loss_rows.double().cpu() - want).abs()
            assert (err <= bound).all(), (r, ti, err.max().item(), bound.min().item())
            # and the rows are this rank's rows of the global loss: the target column holds the positive pair's logit
            i = torch.arange(rows) + r * b
            assert torch.allclose(xt, sim64.detach()[i, O.true_variation_index(classes)[i], i], atol=LAYOUT_ATOL)


# ------------------------------------------------------------------------------------ 2., 3. a world-1 RCCL group
@pytest.fixture(scope="module")
def world_one_group():
    import torch.distributed as dist

    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


class _CountAllGathers:
    """Counts torch.distributed.all_gather_into_tensor calls (the one collective cm3p_amd.dist gathers with)."""

    def __init__(self, monkeypatch):
        import torch.distributed as dist

        self.calls = 0
        orig = dist.all_gather_into_tensor

        def counted(*a, **kw):
            self.calls += 1
            return orig(*a, **kw)

        monkeypatch.setattr(dist, "all_gather_into_tensor", counted)


def test_gathered_variations_world_size_one_equals_local_loss(world_one_group, monkeypatch):
    """Train mode, gather on versus off over RCCL with one rank: the same loss, logits and gradients (bounds of the 2-D twin in
    tests/test_model_gpu.py), no warning, and exactly two all-gathers in the forward (without that count the test would pass on a
    rank-local fallback)."""
    blob = load_file(os.path.join(GOLD, f"{NAME}.safetensors"))
    model = _build()
    out0 = model(**_inputs(blob))
    out0.loss.backward()
    g0 = model.beatmap_model.encoder.layers[0].attn.Wqkv.weight.grad.clone()
    s0 = model.logit_scale.grad.clone()
    model.zero_grad(set_to_none=True)
    model.gather_negatives = True
    counter = _CountAllGathers(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out1 = model(**_inputs(blob))
    assert counter.calls == 2
    out1.loss.backward()
    assert abs(out0.loss.item() - out1.loss.item()) <= 1e-6
    assert out1.logits_per_metadata.shape == (4, 3, 4) and out1.logits_per_beatmap.shape == (4, 4, 3)
    assert torch.allclose(out0.logits_per_metadata, out1.logits_per_metadata, atol=1e-6)
    assert torch.allclose(out0.logits_per_beatmap, out1.logits_per_beatmap, atol=1e-6)
    assert _rel(model.beatmap_model.encoder.layers[0].attn.Wqkv.weight.grad, g0) <= 5e-3  # bf16 re-rounding of grads
    assert abs(model.logit_scale.grad.item() - s0.item()) <= 1e-4


def test_gathered_variations_eval_stays_rank_local(world_one_group, monkeypatch):
    """Eval mode: no collective, the (B, B, V) logits_per_beatmap that evaluation code indexes [i, i], bit for bit the gather-off
    result, and the warning that says so, once per process."""
    from cm3p_amd import dist as D

    blob = load_file(os.path.join(GOLD, f"{NAME}.safetensors"))
    model = _build().eval()
    with torch.no_grad():
        out0 = model(**_inputs(blob))
    model.gather_negatives = True
    counter = _CountAllGathers(monkeypatch)
    monkeypatch.setattr(D, "_warned_3d", False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            out1 = model(**_inputs(blob))
            out2 = model(**_inputs(blob))
    assert counter.calls == 0
    mine = [w for w in caught if issubclass(w.category, RuntimeWarning) and "gather_negatives" in str(w.message)]
    assert len(mine) == 1 and "eval" in str(mine[0].message) and "training mode only" in str(mine[0].message)
    for o in (out1, out2):
        assert o.logits_per_beatmap.shape == (4, 4, 3) and o.logits_per_metadata.shape == (4, 3, 4)
        assert torch.equal(o.logits_per_beatmap, out0.logits_per_beatmap)
        assert torch.equal(o.logits_per_metadata, out0.logits_per_metadata)
        assert torch.equal(o.loss, out0.loss)


# ------------------------------------------------------------------------------------ 4. two ranks under DDP
def _two_rank_worker(rank, world, port, out, backend):
    import datetime

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = rank if backend == "nccl" else 0  # gloo: two ranks share the one GPU of the test box; nccl (RCCL): one GPU per rank
    torch.cuda.set_device(dev)
    kw = dict(device_id=torch.device("cuda", dev)) if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300), **kw)
    try:
        blob = load_file(os.path.join(GOLD, f"{NAME}.safetensors"))
        model = _build()
        model.gather_negatives = True
        for p in model.beatmap_model.audio_encoder.parameters():
            p.requires_grad_(False)  # no input_features in this case: DDP needs every trainable parameter to get a gradient
        ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev])
        full = _inputs(blob)
        b = full["input_ids"].shape[0] // world
        part = {k: v[rank * b:(rank + 1) * b].contiguous() for k, v in full.items()}
        o = ddp(**part)
        o.loss.backward()
        torch.cuda.synchronize()
        out[rank] = (o.loss.item(), model.beatmap_model.encoder.layers[1].attn.Wqkv.weight.grad.cpu(),
                     model.logit_scale.grad.cpu(), model.metadata_projection.weight.grad.cpu(),
                     tuple(o.logits_per_metadata.shape), tuple(o.logits_per_beatmap.shape))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_rank_gathered_variations_step_equals_single_process_global_batch(backend):
    """d64_variations split 2 + 2 under DDP with gathered variations == one process on the whole batch (the bounds of the 2-D twin), and
    the mean of the rank losses within the fixture bound of the loss the reference itself computed.  gloo: both ranks share cuda:0;
    nccl: RCCL with one GPU per rank, skipped unless the box has two GPUs."""
    import torch.multiprocessing as mp

    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_two_rank_worker, args=(2, port, out, backend), nprocs=2, join=True)

    blob = load_file(os.path.join(GOLD, f"{NAME}.safetensors"))
    model = _build()
    o = model(**_inputs(blob))
    o.loss.backward()
    mean_loss = sum(out[r][0] for r in range(2)) / 2
    assert abs(mean_loss - o.loss.item()) <= 2e-3
    assert abs(mean_loss - blob["loss"].item()) <= LOSS_TOL_FIXTURE
    for r in range(2):
        assert out[r][4] == (2, 3, 4)  # this rank's 2 x 3 metadata rows against all 4 beatmaps
        assert out[r][5] == (2, 4, 3)  # this rank's 2 beatmaps against all 4 x 3 metadata rows
        assert _rel(out[r][1], model.beatmap_model.encoder.layers[1].attn.Wqkv.weight.grad) <= 2e-2
        assert abs(out[r][2].item() - model.logit_scale.grad.item()) <= 2e-3 * max(1.0, abs(model.logit_scale.grad.item()))
        assert _rel(out[r][3], model.metadata_projection.weight.grad) <= 2e-2
