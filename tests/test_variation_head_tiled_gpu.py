"""The two routes of kernels.gemm_f32 seen from the model: the register-tiled fp32 GEMM changes no bit of a training step, and the
gathered-variation head takes it by default where its problems are large enough (no silent fall-back to the 16 x 16 kernel)."""
import os

import pytest
import torch
from safetensors.torch import load_file

from cases import CASES

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
NAME = "d64_variations"


def _build():
    from cm3p_amd import CM3PConfig, CM3PModel

    model = CM3PModel(CM3PConfig(**CASES[NAME]["cfg"]))
    sd = load_file(os.path.join(GOLD, "weights_d64.safetensors"))
    blob = load_file(os.path.join(GOLD, f"{NAME}.safetensors"))
    sd.update({k[2:]: v for k, v in blob.items() if k.startswith("w.")})
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train(), {k[3:]: v.to(DEV) for k, v in blob.items() if k.startswith("in.")}


def _step(K, monkeypatch, min_outputs):
    """One forward + backward of CM3PModel on the fixture with the routing constant set; -> (outputs, gradients, tags seen)."""
    from cm3p_amd import _lib

    monkeypatch.setattr(K, "GEMM_F32_TILED_MIN_OUTPUTS", min_outputs)
    model, inp = _build()
    _lib.profile_begin(only=set(K.GEMM_F32_TAGS.values()))
    out = model(**inp)
    out.loss.backward()
    tags = _lib.profile_end()
    outs = dict(loss=out.loss.detach(), logits_per_metadata=out.logits_per_metadata.detach(), logits_per_beatmap=out.logits_per_beatmap.detach(),
                metadata_embeds=out.metadata_embeds.detach(), beatmap_embeds=out.beatmap_embeds.detach())
    grads = {n: p.grad for n, p in model.named_parameters()}
    return outs, grads, tags


def test_a_training_step_has_the_same_bits_on_either_route(monkeypatch):
    """CM3PModel on the reference-made fixture d64_variations, forward and backward, once with every eligible fp32 GEMM of the head on
    the tiled kernel (threshold 0) and once with every one on the 16 x 16 kernel: loss, both logits tensors, both embeddings and
    every parameter gradient are equal."""
    from cm3p_amd import kernels as K

    o_t, g_t, tags_t = _step(K, monkeypatch, 0)
    o_r, g_r, tags_r = _step(K, monkeypatch, 1 << 62)
    tiled, plain = K.GEMM_F32_TAGS[True], K.GEMM_F32_TAGS[False]
    assert tiled in tags_t and plain not in tags_t, tags_t  # (every head GEMM of the model has unit strides)
    assert plain in tags_r and tiled not in tags_r, tags_r
    assert tags_t[tiled][0] == tags_r[plain][0] and tags_t[tiled][2] == tags_r[plain][2]  # the same launches, the same work
    for k in o_r:
        assert torch.equal(o_t[k], o_r[k]), k
    assert set(g_t) == set(g_r)
    for n in g_r:
        assert (g_t[n] is None) == (g_r[n] is None), n
        if g_r[n] is not None:
            assert torch.equal(g_t[n], g_r[n]), n
    assert any(g is not None for g in g_r.values())


def test_the_gathered_variation_head_takes_the_tiled_route_by_default():
    """dist.variation_head as rank 0 of a simulated world of 8 at b = 8, V = 32, P = 512 (synthetic gathered buffers, as
    tools/bench_gathered_variations.py builds them), default routing constants: every one of its GEMMs is past the threshold, so
    all six launches carry the tiled tag, with their work, and none the 16 x 16 tag."""
    from cm3p_amd import _lib
    from cm3p_amd import kernels as K
    from cm3p_amd.dist import variation_head

    N, b, V, P = 8, 8, 32, 512
    gen = torch.Generator().manual_seed(0)

    def unit(*shape):
        x = torch.randn(*shape, generator=gen)
        return (x / x.norm(dim=-1, keepdim=True)).to(DEV).requires_grad_(True)

    me, be, m_all, b_all = unit(b, V, P), unit(b, P), unit(N * b * V, P), unit(N * b, P)
    scale = torch.tensor(2.6592600, device=DEV, requires_grad=True)
    classes = torch.randint(1, 3, (b, V), generator=gen)
    classes[torch.arange(b), torch.randint(0, V, (b,), generator=gen)] = 0
    idx = K.first_zero_index(classes.to(DEV))
    assert K.gemm_f32_route(N * b * V, P, (1, N * b * V), (1, P)) and K.gemm_f32_route(b, N * b * V, (P, 1), (P, 1))
    _lib.profile_begin()
    loss = variation_head(me, be, m_all, b_all, idx, 0, scale)[2]
    loss.backward()
    tags = _lib.profile_end()
    tiled, plain = K.GEMM_F32_TAGS[True], K.GEMM_F32_TAGS[False]
    assert tiled in tags and plain not in tags, sorted(tags)
    assert tags[tiled][0] == 6  # two logits GEMMs, two gradients each
    assert tags[tiled][2] == 3 * (2.0 * b * V * N * b * P + 2.0 * b * N * b * V * P)  # each direction: logits, d rows, d gathered rows
    assert torch.isfinite(loss) and all(t.grad is not None and torch.isfinite(t.grad).all() for t in (me, be, m_all, b_all, scale))
