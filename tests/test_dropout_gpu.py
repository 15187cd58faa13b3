"""Embedding, attention and MLP dropout on the GPU: the mask materialiser against the Python restatement of the RNG contract
(tests/test_dropout_host.py), the element and attention kernels against fp32 restatements that use that mask, the encoder against
transformers' own ModernBertModel with its nn.Dropout modules and its attention function replaced by mask-applying ones, and the behaviour a training loop relies on (eval is dropout-free, seeds reproduce,
checkpointing recomputes the same masks, packed == padded, HF Trainer steps)."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from cases import CASES
from test_dropout_host import keep_mask_ref, scale_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x5DEECE66D1234567


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _next_draw_seed(torch_seed):
    """The seed the encoder will draw after torch.manual_seed(torch_seed) (encoder._dropout_plan: one int64 from the CPU generator)."""
    torch.manual_seed(torch_seed)
    s = int(torch.randint(-(2 ** 63), 2 ** 63 - 1, (), dtype=torch.int64)) & (2 ** 64 - 1)
    torch.manual_seed(torch_seed)
    return s


# ---------------------------------------------------------------------------------------------------------------- materialiser
@pytest.mark.parametrize("shape,layer,site,p", [((2, 5, 37), 2, 3, 0.1), ((3, 70, 130), 5, 1, 0.5), ((1, 8, 64), 0, 0, 0.9)])
def test_materialiser_equals_the_restatement(shape, layer, site, p):
    from cm3p_amd import kernels as K

    thr = K.dropout_threshold(p)
    got = K.dropout_keep(*shape, layer, site, thr, SEED, DEV).cpu().numpy()
    assert np.array_equal(got, keep_mask_ref(*shape, layer, site, thr, SEED))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_no_reused_counters(p):
    from cm3p_amd import kernels as K

    thr = K.dropout_threshold(p)
    a = K.dropout_keep(64, 512, 512, 3, 1, thr, SEED, DEV)  # 1.7e7 decisions
    n = a.numel()
    q = 1.0 - thr / 65536.0
    rate = a.float().mean().item()
    assert abs(rate - q) <= 5 * (q * (1 - q) / n) ** 0.5, (rate, q)
    agree = q * q + (1 - q) ** 2
    others = {"site": K.dropout_keep(64, 512, 512, 3, 3, thr, SEED, DEV), "layer": K.dropout_keep(64, 512, 512, 4, 1, thr, SEED, DEV),
              "seed": K.dropout_keep(64, 512, 512, 3, 1, thr, SEED + 1, DEV)}
    for what, b in others.items():
        r = (a == b).float().mean().item()
        assert abs(r - agree) <= 5 * (agree * (1 - agree) / n) ** 0.5, (what, r, agree)
    r = (a[1:] == a[:-1]).float().mean().item()  # neighbouring heads (counter word 2)
    m = a[1:].numel()
    assert abs(r - agree) <= 5 * (agree * (1 - agree) / m) ** 0.5, ("head", r, agree)


# ---------------------------------------------------------------------------------------------------------------- element kernels
def _packed_layout(lens, S):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int32), 0)
    idx = torch.cat([torch.arange(b * S, b * S + n) for b, n in enumerate(lens)])
    return cu.to(DEV), idx.to(DEV)


def test_dropout_f32_matches_the_mask_and_packed_equals_padded():
    from cm3p_amd import kernels as K

    B, S, H, p = 3, 200, 136, 0.1
    thr = K.dropout_threshold(p)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B * S, H, device=DEV, generator=g)
    keep = torch.from_numpy(keep_mask_ref(B, S, H, 0, K.SITE_EMBED, thr, SEED)).to(DEV).reshape(B * S, H).bool()
    scale = torch.tensor(scale_ref(thr), dtype=torch.float32, device=DEV)
    want = torch.where(keep, x * scale, torch.zeros_like(x))
    y = K.dropout_f32(x, thr, SEED, 0, K.SITE_EMBED, S)
    assert torch.equal(y, want)
    # the backward is the same operation: dy o Z
    assert torch.equal(K.dropout_f32(want, thr, SEED, 0, K.SITE_EMBED, S), torch.where(keep, want * scale, torch.zeros_like(x)))
    # packed rows of the same tokens decide alike
    cu, idx = _packed_layout([200, 17, 150], S)
    yp = K.dropout_f32(x[idx].contiguous(), thr, SEED, 0, K.SITE_EMBED, S, cu)
    assert torch.equal(yp, y[idx])
    # thr = 0 is the identity, thr = 65536 drops everything
    assert torch.equal(K.dropout_f32(x, 0, SEED, 0, 0, S), x)
    assert not K.dropout_f32(x, 65536, SEED, 0, 0, S).any()


def test_geglu_dropout_forward_and_backward():
    from cm3p_amd import kernels as K

    B, S, I, layer = 2, 200, 192, 3
    T = B * S
    g = torch.Generator(device=DEV).manual_seed(1)
    h = torch.randn(T, 2 * I, device=DEV, generator=g).to(torch.bfloat16)
    dg = torch.randn(T, I, device=DEV, generator=g).to(torch.bfloat16)
    # p = 0: the dropout instances are the plain kernels, bit for bit
    assert torch.equal(K.geglu_fwd_dropout(h, 0, SEED, layer, S), K.geglu_fwd(h))
    assert torch.equal(K.geglu_bwd_dropout(dg, h, 0, SEED, layer, S), K.geglu_bwd(dg, h))
    thr = K.dropout_threshold(0.1)
    keep = torch.from_numpy(keep_mask_ref(B, S, I, layer, K.SITE_MLP, thr, SEED)).to(DEV).reshape(T, I).bool()
    sc = scale_ref(thr)
    gd = K.geglu_fwd_dropout(h, thr, SEED, layer, S)
    g0 = K.geglu_fwd(h).float()
    assert not gd[~keep].float().any()
    torch.testing.assert_close(gd.float()[keep], g0[keep] * sc, rtol=8e-3, atol=1e-6)  # one extra bf16 rounding on the right
    dh = K.geglu_bwd_dropout(dg, h, thr, SEED, layer, S)
    kk = torch.cat((keep, keep), 1)
    assert not dh[~kk].float().any()
    # (this reference rounds dg * scale to bf16, which the kernel does not: it hands the fp32 product to the GeGLU derivative.  The
    # tolerance below absorbs that extra rounding; tests/test_dropout_kernels_gpu.py::test_geglu_dropout_against_float64 holds the kernel
    # to the unrounded float64 value within its derived bound.)
    ref = K.geglu_bwd((dg.float() * sc).to(torch.bfloat16), h).float()
    torch.testing.assert_close(dh.float()[kk], ref[kk], rtol=2e-2, atol=1e-5)
    # packed rows
    cu, idx = _packed_layout([200, 130], S)
    assert torch.equal(K.geglu_fwd_dropout(h[idx].contiguous(), thr, SEED, layer, S, cu), gd[idx])


# ---------------------------------------------------------------------------------------------------------------- attention kernels
def _assert_close(got, want, atol, rtol, what):
    got, want = got.float().cpu(), want.float().cpu()
    bad = (got - want).abs() > atol + rtol * want.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} elements off, max |diff| {(got - want).abs().max().item():.3e}"


def _band_bwd_nodrop(qkv, out, do, lse, km, B, S, nh, window, prescaled):
    """cm3p_attn_bwd itself (the band kernels at every window; kernels.attn_bwd sends global layers to the fused kernel)."""
    from cm3p_amd._lib import call, ptr, stream

    dqkv, delta = torch.empty_like(qkv), torch.empty_like(lse)
    call("cm3p_attn_bwd", ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dqkv), ptr(km), B, S, nh, window, 0.125, None, None, 0, 3,
         int(prescaled), stream())
    return dqkv


@pytest.mark.parametrize("S,window,lens,prescaled", [(200, -1, [200, 150, 100], True), (200, 64, [200, 60, 1], True),
                                                     (1000, -1, None, False), (1000, 64, [1000, 700], False), (256, -1, [256, 1], False)])
def test_attention_dropout_matches_fp32_restatement(S, window, lens, prescaled):
    """out = (softmax o Z) V and its three gradients against fp32 autograd with the materialised mask; lse is the dropout-free one, bit
    for bit; rows with no visible key and padded keys give exact zeros; thr = 0 is the band kernels bit for bit."""
    from cm3p_amd import kernels as K
    from oracle import cm3p_oracle as O

    B, nh, layer = (2 if lens is None else len(lens)), 2, 2
    g = torch.Generator().manual_seed(S + window)
    qkv = torch.randn(B, S, 3, nh, 64, generator=g).to(torch.bfloat16)
    c = K.SOFTMAX_Q_SCALE
    qkv_dev = qkv.clone()
    x = qkv.float()
    if prescaled:  # the kernels get q * scale * log2(e) rounded once; the restatement that q divided back (as test_kernels_gpu does)
        qkv_dev[:, :, 0] = (qkv[:, :, 0].float() * c).to(torch.bfloat16)
        x[:, :, 0] = qkv_dev[:, :, 0].float() / c
    x.requires_grad_(True)
    mask = None if lens is None else (torch.arange(S)[None] < torch.tensor(lens)[:, None]).long()
    allowed = O.attention_allowed(mask, B, S, window if window >= 0 else None)
    if allowed is None:
        allowed = torch.ones(B, 1, S, S, dtype=torch.bool)
    thr = K.dropout_threshold(0.1)
    z = K.dropout_keep(B * nh, S, S, layer, K.SITE_ATTN_PROBS, thr, SEED, DEV).cpu().view(B, nh, S, S).float() * scale_ref(thr)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    live = allowed.any(-1, keepdim=True)
    s = torch.where(live, s.masked_fill(~allowed, float("-inf")), torch.zeros_like(s))
    pr = torch.where(live, torch.softmax(s, -1), torch.zeros_like(s))
    o = ((pr * z) @ v).transpose(1, 2).reshape(B * S, nh * 64)
    do = torch.randn(B * S, nh * 64, generator=g).to(torch.bfloat16)
    o.backward(do.float())

    km = mask.to(torch.uint8).to(DEV) if mask is not None else None
    qd, dod = qkv_dev.to(DEV), do.to(DEV)
    out, lse = K.attn_fwd(qd, km, B, S, nh, window, 0.125, prescaled=prescaled, drop=(thr, SEED, layer))
    _assert_close(out, o.detach(), 2e-3, 2e-2, "out")
    out0, lse0 = K.attn_fwd(qd, km, B, S, nh, window, 0.125, prescaled=prescaled, drop=(0, SEED, layer))
    assert torch.equal(lse, lse0)  # the statistics see the undropped probabilities
    if not K.query("cm3p_attn_fwd_impl", S, nh, window, int(prescaled)):  # the dropout-free call runs the band kernel too
        o_nd, l_nd = K.attn_fwd(qd, km, B, S, nh, window, 0.125, prescaled=prescaled)
        assert torch.equal(out0, o_nd) and torch.equal(lse0, l_nd)
    dead = ~live.expand(B, nh, S, 1)[..., 0].transpose(1, 2).reshape(B * S, nh)
    if dead.any():
        assert not out.view(B * S, nh, 64).cpu()[dead].any()
    dqkv = K.attn_bwd(qd, out, dod, lse, km, B, S, nh, window, 0.125, prescaled=prescaled, drop=(thr, SEED, layer))
    want = x.grad
    _assert_close(dqkv, want, 2e-2 * want.abs().max().item(), 3e-2, "dqkv")
    for i, nm in enumerate("qkv"):
        e = (dqkv[:, :, i].float().cpu() - want[:, :, i]).norm() / want[:, :, i].norm().clamp_min(1e-9)
        assert e < 2e-2, f"d{nm} relative L2 error {e:.3e}"
    d = dqkv.view(B * S, 3, nh, 64).cpu()
    if dead.any():
        assert not d[:, 0][dead].any()  # dead rows: dq = 0
    if mask is not None:
        pad = mask.reshape(B * S) == 0
        assert not d[pad][:, 1:].any()  # padded keys: dk = dv = 0
    dq0 = K.attn_bwd(qd, out0, dod, lse0, km, B, S, nh, window, 0.125, prescaled=prescaled, drop=(0, SEED, layer))
    assert torch.equal(dq0, _band_bwd_nodrop(qd, out0, dod, lse0, km, B, S, nh, window, prescaled))


@pytest.mark.parametrize("D,S,window,lens", [(16, 200, -1, [200, 120]), (16, 333, 64, [333, 60]), (32, 130, 64, None), (32, 257, -1, [257, 1])])
def test_generic_attention_dropout_matches_fp32_restatement(D, S, window, lens):
    """head_dim 16 / 32 (csrc/attention_generic.hip): out and the three gradients against fp32 autograd with the materialised mask, lse the
    dropout-free one, exact zeros for dead rows and padded keys, thr = 0 equal to the dropout-free kernels bit for bit."""
    from cm3p_amd import kernels as K
    from oracle import cm3p_oracle as O

    B, nh, layer, scale = (2 if lens is None else len(lens)), 3, 1, D ** -0.5
    g = torch.Generator().manual_seed(D + S)
    qkv = torch.randn(B, S, 3, nh, D, generator=g).to(torch.bfloat16)
    x = qkv.float().requires_grad_(True)
    mask = None if lens is None else (torch.arange(S)[None] < torch.tensor(lens)[:, None]).long()
    allowed = O.attention_allowed(mask, B, S, window if window >= 0 else None)
    if allowed is None:
        allowed = torch.ones(B, 1, S, S, dtype=torch.bool)
    thr = K.dropout_threshold(0.1)
    z = K.dropout_keep(B * nh, S, S, layer, K.SITE_ATTN_PROBS, thr, SEED, DEV).cpu().view(B, nh, S, S).float() * scale_ref(thr)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * scale
    live = allowed.any(-1, keepdim=True)
    s = torch.where(live, s.masked_fill(~allowed, float("-inf")), torch.zeros_like(s))
    pr = torch.where(live, torch.softmax(s, -1), torch.zeros_like(s))
    o = ((pr * z) @ v).transpose(1, 2).reshape(B * S, nh * D)
    do = torch.randn(B * S, nh * D, generator=g).to(torch.bfloat16)
    o.backward(do.float())

    km = mask.to(torch.uint8).to(DEV) if mask is not None else None
    qd, dod = qkv.reshape(B * S, 3 * nh * D).to(DEV), do.to(DEV)
    out, lse = K.attn_fwd_generic(qd, km, B, S, nh, D, window, scale, drop=(thr, SEED, layer))
    _assert_close(out, o.detach(), 2e-3, 2e-2, "out")
    o_nd, l_nd = K.attn_fwd_generic(qd, km, B, S, nh, D, window, scale)
    assert torch.equal(lse, l_nd)
    out0, lse0 = K.attn_fwd_generic(qd, km, B, S, nh, D, window, scale, drop=(0, SEED, layer))
    assert torch.equal(out0, o_nd) and torch.equal(lse0, l_nd)
    dead = ~live.expand(B, nh, S, 1)[..., 0].transpose(1, 2).reshape(B * S, nh)
    if dead.any():
        assert not out.view(B * S, nh, D).cpu()[dead].any()
    dqkv = K.attn_bwd_generic(qd, out, dod, lse, km, B, S, nh, D, window, scale, drop=(thr, SEED, layer))
    want = x.grad.reshape(B * S, 3, nh, D)
    got = dqkv.view(B * S, 3, nh, D)
    _assert_close(got, want, 2e-2 * want.abs().max().item(), 3e-2, "dqkv")
    for i, nm in enumerate("qkv"):
        e = (got[:, i].float().cpu() - want[:, i]).norm() / want[:, i].norm().clamp_min(1e-9)
        assert e < 2e-2, f"d{nm} relative L2 error {e:.3e}"
    d = got.cpu()
    if dead.any():
        assert not d[:, 0][dead].any()
    if mask is not None:
        assert not d[mask.reshape(B * S) == 0][:, 1:].any()
    assert torch.equal(K.attn_bwd_generic(qd, out0, dod, lse0, km, B, S, nh, D, window, scale, drop=(0, SEED, layer)),
                       K.attn_bwd_generic(qd, o_nd, dod, l_nd, km, B, S, nh, D, window, scale))


# (-1, True), the configuration the encoder's global layers run: the band forward's lazy-max shift is a wave-wide decision that the
# padded batch's extra query rows take part in, so packed and padded differ in the last bits of a few rows - with and without dropout,
# in the same (row, head) pairs, which is what that case pins; the dropout masks themselves agree, as the other three show bit for bit.
@pytest.mark.parametrize("window,prescaled", [(-1, False), (64, True), (64, False), (-1, True)])
def test_attention_dropout_varlen_equals_padded(window, prescaled):
    from cm3p_amd import kernels as K

    torch.manual_seed(0)
    B, S, nh, layer = 4, 333, 2, 1
    lens = [333, 200, 97, 64]
    qkv = (torch.randn(B, S, 3, nh, 64, device=DEV) * 0.7).bfloat16()
    mask = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    do = torch.randn(B * S, nh * 64, device=DEV).bfloat16() * mask.reshape(B * S, 1).bfloat16()
    idx = torch.nonzero(mask.flatten()).flatten()
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    qkv_p = qkv.reshape(B * S, 3, nh, 64)[idx].contiguous()

    def run(thr):
        drop = (thr, SEED, layer)
        out, lse = K.attn_fwd(qkv, mask, B, S, nh, window, 0.125, prescaled, drop=drop)
        dqkv = K.attn_bwd(qkv, out, do, lse, mask, B, S, nh, window, 0.125, None, False, prescaled, drop=drop)
        out_p, lse_p = K.attn_fwd_varlen(qkv_p, cu, B, max(lens), nh, window, 0.125, prescaled, drop=drop)
        dqkv_p = K.attn_bwd_varlen(qkv_p, out_p, do[idx].contiguous(), lse_p, cu, B, max(lens), nh, window, 0.125, None, prescaled, drop=drop)
        return (out[idx], out_p), (lse.permute(1, 0, 2).reshape(nh, B * S)[:, idx], lse_p), (dqkv.reshape(B * S, 3, nh, 64)[idx], dqkv_p)

    o, l, d = run(K.dropout_threshold(0.1))
    if not (window < 0 and prescaled):
        assert torch.equal(o[1], o[0]) and torch.equal(l[1], l[0]) and torch.equal(d[1], d[0])
        return
    o0, l0, _ = run(0)
    rows = (o[1] != o[0]).view(-1, nh, 64).any(-1)  # (row, head) pairs that differ under dropout ...
    assert torch.equal(rows, (o0[1] != o0[0]).view(-1, nh, 64).any(-1))  # ... are the ones that differ without it
    assert torch.equal(l[1] != l[0], l0[1] != l0[0])
    assert rows.float().mean().item() < 0.01
    _assert_close(o[1], o[0], 1e-2, 1e-2, "packed out")
    assert _rel(d[1], d[0]) < 1e-2


def test_attention_output_dropout_site():
    """x_mid = x + Z o t (out_drop before the residual add) and its backward's bf16 operand Z o dy."""
    from cm3p_amd import kernels as K

    B, S, H, layer = 2, 200, 128, 3
    thr = K.dropout_threshold(0.1)
    g = torch.Generator(device=DEV).manual_seed(4)
    t, x = torch.randn(B * S, H, device=DEV, generator=g), torch.randn(B * S, H, device=DEV, generator=g)
    keep = torch.from_numpy(keep_mask_ref(B, S, H, layer, K.SITE_ATTN_OUT, thr, SEED)).to(DEV).reshape(B * S, H).bool()
    zt = torch.where(keep, t * torch.tensor(scale_ref(thr), device=DEV), torch.zeros_like(t))
    assert torch.equal(K.dropout_f32(t, thr, SEED, layer, K.SITE_ATTN_OUT, S, resid=x), x + zt)
    assert torch.equal(K.dropout_f32(t, thr, SEED, layer, K.SITE_ATTN_OUT, S, bf16_only=True), zt.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------- model level
def _tower_cfg(p_emb=0.1, p_mlp=0.1, p_attn=None, case="d64_cls_nopad"):
    from cm3p_amd import CM3PConfig

    # d64: H 128, 2 heads, 4 layers (global 0, 3; band 1, 2).  c1: the reference's tiny tower, H 64, 4 heads of 16 (generic kernels)
    bc = copy.deepcopy(CM3PConfig(**CASES[case]["cfg"]).beatmap_config)
    bc.embedding_dropout, bc.mlp_dropout = p_emb, p_mlp
    bc.attention_dropout = p_mlp if p_attn is None else p_attn
    return bc


def _encoder(cfg, torch_seed=0):
    from cm3p_amd.encoder import CM3PEncoder

    torch.manual_seed(torch_seed)
    enc = CM3PEncoder(cfg)
    for n, p in enc.named_parameters():
        with torch.no_grad():
            p.copy_(torch.randn_like(p) * (0.02 if p.dim() == 2 else 0.1) + (1.0 if p.dim() == 1 else 0.0))
    return enc.to(DEV).train()


def _batch(B=3, S=200, short=150, vocab=190, H=128):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, vocab, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[-1, short:] = 0
    ids[-1, short:] = 0
    w = torch.randn(B, S, H, generator=g)
    return ids.to(DEV), mask.to(DEV), w.to(DEV)


class _MaskDrop(nn.Module):
    def __init__(self, keep, scale):
        super().__init__()
        self.keep, self.scale = keep, scale

    def forward(self, x):
        return x * (self.keep.to(x.dtype) * self.scale)


@pytest.mark.parametrize("case", ["d64_cls_nopad", "c1_tiny_nopad"])
def test_encoder_matches_transformers_modernbert_with_the_same_masks(monkeypatch, case):
    from transformers import ModernBertConfig, ModernBertModel

    from cm3p_amd import kernels as K

    cfg = _tower_cfg(case=case)
    enc = _encoder(cfg)
    ids, mask, w = _batch(H=cfg.hidden_size)
    B, S = ids.shape
    valid = mask.bool()
    seed = _next_draw_seed(77)
    y = enc(input_ids=ids, attention_mask=mask)
    loss = (y * w)[valid].sum()
    loss.backward()

    hc = ModernBertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                          num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                          global_attn_every_n_layers=cfg.global_attn_every_n_layers, local_attention=cfg.local_attention,
                          global_rope_theta=cfg.global_rope_theta, local_rope_theta=cfg.local_rope_theta, norm_eps=cfg.norm_eps,
                          max_position_embeddings=cfg.max_position_embeddings, pad_token_id=cfg.pad_token_id, bos_token_id=1,
                          eos_token_id=2, cls_token_id=1, sep_token_id=2, embedding_dropout=0.1, mlp_dropout=0.1,
                          attention_dropout=0.1, attn_implementation="eager")
    ref = ModernBertModel(hc).float()
    ref.load_state_dict({k: v.detach().cpu() for k, v in enc.state_dict().items()}, strict=True)
    ref.train()
    thr = K.dropout_threshold(0.1)
    sc = scale_ref(thr)
    ref.embeddings.drop = _MaskDrop(torch.from_numpy(keep_mask_ref(B, S, cfg.hidden_size, 0, K.SITE_EMBED, thr, seed)), sc)
    nh = cfg.num_attention_heads
    probs_z = []
    for i, layer in enumerate(ref.layers):
        layer.mlp.drop = _MaskDrop(torch.from_numpy(keep_mask_ref(B, S, cfg.intermediate_size, i, K.SITE_MLP, thr, seed)), sc)
        layer.attn.out_drop = _MaskDrop(torch.from_numpy(keep_mask_ref(B, S, cfg.hidden_size, i, K.SITE_ATTN_OUT, thr, seed)), sc)
        probs_z.append(K.dropout_keep(B * nh, S, S, i, K.SITE_ATTN_PROBS, thr, seed, DEV).cpu().view(B, nh, S, S).float() * sc)

    def masked_dropout_attention(module, query, key, value, attention_mask, scaling, dropout=0.0, **kwargs):
        # TF eager_attention_forward with nn.functional.dropout replaced by the materialised mask of this layer (patched in under the
        # eager name, so that the model keeps building the eager path's additive padding / sliding-window masks)
        w = torch.matmul(query, key.transpose(2, 3)) * scaling
        if attention_mask is not None:
            w = w + attention_mask
        w = nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(query.dtype)
        assert dropout == 0.1 and module.training
        w = w * probs_z[module.layer_idx]
        return torch.matmul(w, value).transpose(1, 2).contiguous(), w

    from transformers.models.modernbert import modeling_modernbert

    monkeypatch.setattr(modeling_modernbert, "eager_attention_forward", masked_dropout_attention)
    yr = ref(input_ids=ids.cpu(), attention_mask=mask.cpu()).last_hidden_state
    lr = (yr * w.cpu())[valid.cpu()].sum()
    lr.backward()

    assert _rel(y[valid], yr[valid.cpu()]) <= 2e-2
    # the loss as a relative quantity: a positive-weighted energy of the valid hidden states (no cancelling terms)
    wp = w.abs().cpu()[valid.cpu()]
    e, er = (y.detach().cpu()[valid.cpu()] ** 2 * wp).mean().item(), (yr.detach()[valid.cpu()] ** 2 * wp).mean().item()
    assert abs(e - er) <= 2e-2 * er, (e, er)
    # a dropout-free reference is far away: the masks matter at this tolerance
    monkeypatch.undo()
    ref0 = ModernBertModel(hc).float()
    ref0.load_state_dict(ref.state_dict(), strict=False)
    ref0.eval()
    assert _rel(y[valid], ref0(input_ids=ids.cpu(), attention_mask=mask.cpu()).last_hidden_state[valid.cpu()]) > 5e-2
    pr, pe = dict(ref.named_parameters()), dict(enc.named_parameters())
    names = ["embeddings.tok_embeddings.weight", "embeddings.norm.weight", "layers.0.attn.Wqkv.weight", "layers.1.attn.Wo.weight",
             "layers.1.mlp.Wi.weight", "layers.2.mlp.Wo.weight", "layers.3.mlp_norm.weight", "layers.3.attn_norm.weight", "final_norm.weight"]
    names = [n for n in names if n in pe]
    assert len(names) >= 6
    for n in names:
        assert _rel(pe[n].grad, pr[n].grad) <= 6e-2, n


def _step(enc, ids, mask, w, torch_seed, **kw):
    enc.zero_grad(set_to_none=True)
    torch.manual_seed(torch_seed)
    y = enc(input_ids=ids, attention_mask=mask, **kw)
    loss = (y * w)[mask.bool()].sum()
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in enc.named_parameters()}, y.detach()


def _assert_same(ga, gb):
    for n in ga:
        if "tok_embeddings" in n:  # float atomic scatter-add: order-dependent in the last bits
            torch.testing.assert_close(ga[n], gb[n], rtol=1e-5, atol=1e-6)
        else:
            assert torch.equal(ga[n], gb[n]), n


def test_eval_mode_is_dropout_free_and_train_mode_no_grad_drops():
    ids, mask, _ = _batch()
    a, b = _encoder(_tower_cfg()), _encoder(_tower_cfg(0.0, 0.0))
    a.eval(), b.eval()
    with torch.no_grad():
        assert torch.equal(a(input_ids=ids, attention_mask=mask), b(input_ids=ids, attention_mask=mask))
        a.train(), b.train()
        assert not torch.equal(a(input_ids=ids, attention_mask=mask), b(input_ids=ids, attention_mask=mask))  # torch semantics


def test_p0_training_step_launches_no_dropout_kernel():
    from cm3p_amd import _lib

    ids, mask, w = _batch()
    for p, want in ((0.0, False), (0.1, True)):
        enc = _encoder(_tower_cfg(p, p))
        _lib.profile_begin()
        _step(enc, ids, mask, w, 3)
        names = _lib.profile_end()
        assert any("drop" in n.lower() for n in names) == want, sorted(names)


def test_same_seed_reproduces_and_another_seed_differs():
    ids, mask, w = _batch()
    enc = _encoder(_tower_cfg())
    la, ga, _ = _step(enc, ids, mask, w, 5)
    lb, gb, _ = _step(enc, ids, mask, w, 5)
    assert torch.equal(la, lb)
    _assert_same(ga, gb)
    lc, _, _ = _step(enc, ids, mask, w, 6)
    assert not torch.equal(la, lc)


def test_gradient_checkpointing_recomputes_the_same_masks():
    ids, mask, w = _batch()
    a, b = _encoder(_tower_cfg()), _encoder(_tower_cfg())
    b.gradient_checkpointing = True
    la, ga, _ = _step(a, ids, mask, w, 9)
    lb, gb, _ = _step(b, ids, mask, w, 9)
    assert torch.equal(la, lb)
    _assert_same(ga, gb)


def test_unpadded_execution_agrees_with_padded_under_dropout():
    ids, mask, w = _batch(S=256, short=100)
    enc = _encoder(_tower_cfg())
    valid = mask.bool()
    la, ga, ya = _step(enc, ids, mask, w, 13)
    lb, gb, yb = _step(enc, ids, mask, w, 13, unpad=True)
    assert _rel(yb[valid], ya[valid]) <= 5e-3
    assert not yb[~valid].any()
    for n in ("layers.1.mlp.Wi.weight", "layers.0.attn.Wqkv.weight", "embeddings.norm.weight"):
        assert _rel(gb[n], ga[n]) <= 2e-2, n
    # a different mask is far away at this tolerance
    _, _, yc = _step(enc, ids, mask, w, 14, unpad=True)
    assert _rel(yc[valid], ya[valid]) > 2e-2


def test_cuda_graph_capture_with_dropout_is_refused():
    ids, mask, _ = _batch()
    enc = _encoder(_tower_cfg())
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), pytest.raises(NotImplementedError, match="graph"):
        with torch.cuda.graph(g, stream=s):
            enc(input_ids=ids, attention_mask=mask)
    torch.cuda.synchronize()


def test_trainer_steps_a_beatmap_classifier_with_dropout(tmp_path):
    from transformers import Trainer, TrainingArguments

    from cm3p_amd.modeling_cm3p import CM3PForBeatmapClassification

    bc = _tower_cfg()
    bc.num_labels = 5
    bc.problem_type = None
    torch.manual_seed(0)
    model = CM3PForBeatmapClassification(bc)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 190, (8, 192), generator=g)
    labels = torch.randint(0, 5, (8,), generator=g)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return {"input_ids": ids[i], "attention_mask": torch.ones_like(ids[i]), "labels": labels[i]}

    args = TrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=4, max_steps=2, bf16=True, report_to=[],
                             logging_steps=1, save_strategy="no", learning_rate=1e-4, dataloader_num_workers=0,
                             remove_unused_columns=False)
    result = Trainer(model=model, args=args, train_dataset=DS()).train()
    assert result.global_step == 2 and np.isfinite(result.training_loss)
