"""gloo tests of the cross-rank negatives exchange for (B, V, L) metadata variations, on CPU (the pattern of test_dist_gloo.py).

The product's collective plumbing (cm3p_amd.dist.start_gather) and its integer bookkeeping (cm3p_amd.dist.variation_targets)
are device agnostic; the arithmetic around them in this test is torch's.  Invariant: with DDP-style gradient AVERAGING, the
parameter gradients on every rank equal the gradients of the reference's 3-D loss on the concatenated (N*b, V, N*b) batch, and
the mean of the per-rank losses equals that loss (tolerance 1e-6, fp32).
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

P = 16


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _towers(params, xm, xb):
    """Stand-in towers: one linear map per modality, then L2 normalisation as the reference does.  xm (n, V, 12) -> (n, V, P)."""
    from oracle import cm3p_oracle as O

    return O.l2_normalize(xm @ params["wm"].t()), O.l2_normalize(xb @ params["wb"].t())


def _make(world, b, V, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = world * b
    params = {"wm": torch.randn(P, 12, generator=g), "wb": torch.randn(P, 20, generator=g), "s": torch.tensor(1.3)}
    xm = torch.randn(n, V, 12, generator=g)
    xb = torch.randn(n, 20, generator=g)
    # variation classes: one class-0 slot per row at (i + 1) % V (varies, and is not always slot 0), classes 1 / 2 elsewhere;
    # row 0 carries a -1 (padding) class, an ordinary column as in the reference; with V >= 3 one row has a second 0 behind its
    # first (the first one counts)
    classes = torch.randint(1, 3, (n, V), generator=g)
    slot = (torch.arange(n) + 1) % V
    classes[torch.arange(n), slot] = 0
    classes[0, (slot[0] + 1) % V] = -1
    if V >= 3 and n >= 2 and slot[-1] < V - 1:
        classes[n - 1, V - 1] = 0
    return params, xm, xb, classes


def _worker(rank, world, port, b, V, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cm3p_amd.dist import start_gather, variation_targets
        from oracle import cm3p_oracle as O

        params, xm, xb, classes = _make(world, b, V)
        params = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        sl = slice(rank * b, (rank + 1) * b)
        n = world * b
        # the product's order of events (gathered_contrastive_variations): the beatmap gather starts as soon as its embeddings
        # exist, the metadata gather as soon as its own do; the metadata-direction logits are taken between the two joins
        be = _towers(params, xm[sl], xb[sl])[1]
        pending_b = start_gather(be)
        me = _towers(params, xm[sl], xb[sl])[0]
        pending_m = start_gather(me)
        idx = O.true_variation_index(classes[sl])
        roff, tgt_m, tgt_b = variation_targets(rank, b, V, n, idx)
        scale = params["s"].exp()
        b_all = pending_b.wait()
        lpm = me.reshape(b * V, P) @ b_all.t() * scale  # (b*V, N*b), flat = the (b, V, N*b) logits the row offsets index
        m_all = pending_m.wait()
        assert m_all.shape == (n, V, P) and b_all.shape == (n, P)
        lpb = be @ m_all.reshape(n * V, P).t() * scale  # (b, N*b*V)
        rows_m = lpm.reshape(-1)[roff[:, None] + torch.arange(n)[None, :]]
        loss = 0.5 * (F.cross_entropy(rows_m, tgt_m) + F.cross_entropy(lpb, tgt_b))
        loss.backward()
        grads = {}
        for k, p in params.items():
            gavg = p.grad.clone()
            dist.all_reduce(gavg)  # what DDP does: sum, then divide by world size
            grads[k] = gavg / world
        lmean = loss.detach().clone()
        dist.all_reduce(lmean)
        out[rank] = (lmean / world, grads, m_all.detach(), b_all.detach())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,b,V", [(2, 3, 4), (2, 1, 2), (4, 2, 3), (8, 1, 3)])
def test_gathered_variation_loss_and_grads_equal_single_process_reference(world, b, V):
    from oracle import cm3p_oracle as O

    # (test_dist_gloo.py's rule and reason: a rank's first backward() opens the visible GPU even for CPU tensors; eight rank
    # processes beside the test process are more than one shared GPU should carry for a CPU test)
    if world > 4 and torch.cuda.is_available():
        pytest.skip("world 8 would hold the visible GPU open in 8 rank processes; covered by the run without a GPU")
    port = _free_port()
    mgr = mp.get_context("spawn").Manager()  # (a forked manager would inherit this process's open GPU handle)
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, b, V, out), nprocs=world, join=True)

    params, xm, xb, classes = _make(world, b, V)
    n = world * b
    idx = O.true_variation_index(classes)
    assert (classes == -1).sum() == 1 and (idx != 0).any() and (n < 2 or len(set(idx.tolist())) > 1)  # what the cases are about
    params = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    me, be = _towers(params, xm, xb)
    sim = (me.reshape(n * V, P) @ be.t() * params["s"].exp()).view(n, V, n)
    ref_loss = O.cm3p_loss(sim, classes)  # ref:cm3p/modeling_cm3p.py:33-51 (3-D branch) on the global batch
    ref_loss.backward()
    assert sorted(out.keys()) == list(range(world))
    for rank in range(world):
        lmean, grads, m_all, b_all = out[rank]
        assert torch.allclose(m_all, me.detach(), atol=1e-7) and torch.allclose(b_all, be.detach(), atol=1e-7)  # rank order
        assert abs(lmean.item() - ref_loss.item()) <= 1e-6
        for k, p in params.items():
            assert torch.allclose(grads[k], p.grad, atol=1e-6, rtol=1e-5), (rank, k, (grads[k] - p.grad).abs().max())


def test_variation_targets_at_world_one_are_the_local_loss_specs(monkeypatch):
    """Rank 0 of a world of 1: the offsets and targets are the ones cm3p_loss_hip builds for a (B, V, B) logits tensor (captured by
    swapping its autograd node for a recorder and its index kernel for the oracle's argmax: no GPU in this test)."""
    from cm3p_amd import modeling_cm3p as M
    from cm3p_amd.dist import variation_targets
    from oracle import cm3p_oracle as O

    got = {}

    class _Rec:
        @staticmethod
        def apply(specs, *logits):
            got["specs"] = specs
            return torch.zeros(())

    monkeypatch.setattr(M, "_CrossEntropySumFn", _Rec)
    monkeypatch.setattr(M.K, "first_zero_index", lambda c: O.true_variation_index(c).to(torch.int64))
    n, V = 5, 4
    _, _, _, classes = _make(1, n, V)
    classes[2] = 1  # a row without a 0: index 0, as the reference's argmax gives
    M.cm3p_loss_hip(torch.zeros(n, V, n), classes)
    (_, rows0, cols0, rs0, cs0, roff_ref, tgt_m_ref, _), (_, rows1, cols1, rs1, cs1, none1, tgt_b_ref, _) = got["specs"]
    idx = O.true_variation_index(classes)
    assert idx[2] == 0 and (idx != 0).any()
    roff, tgt_m, tgt_b = variation_targets(0, n, V, n, idx)
    for a, b_ in ((roff, roff_ref), (tgt_m, tgt_m_ref), (tgt_b, tgt_b_ref)):
        assert a.dtype == torch.int64 and a.device == idx.device and torch.equal(a, b_)
    assert (rows0, cols0, rs0, cs0) == (n, n, 0, 1) and (rows1, cols1) == (n, n * V) and none1 is None
    # and any rank of any world: the same rows of the local logits, targets shifted to this rank's block of the gathered columns
    roff3, tgt_m3, tgt_b3 = variation_targets(3, n, V, 4 * n, idx)
    assert torch.equal(roff3, (torch.arange(n) * V + idx) * 4 * n)
    assert torch.equal(tgt_m3, 3 * n + torch.arange(n)) and torch.equal(tgt_b3, (3 * n + torch.arange(n)) * V + idx)
