"""The wide-head golden case (head_dim 128 and 96), shared by make_golden_hd.py (which runs the reference on it) and
tests/test_attention_hd_gpu.py.  Pure data + seeded builders; nothing here imports the reference.

A 256-wide tower's weights alone are past the size limit of a committed file, so this case stores NO weights: both sides draw them
with `draw_weights` - one CPU generator per parameter, seeded by the parameter's name, so the values depend on neither the order in
which a model lists its parameters nor on any other parameter - at the O(1) activation scale of make_golden.build_model."""
from __future__ import annotations

import zlib

import torch

from cases import CASES, _cfg, make_inputs

NAME = "hd_mean_pad"

# beatmap tower: hidden 256 / 2 heads = head_dim 128; layer 0 global, layer 1 sliding (|q - k| <= 64).  Its audio encoder stays at head_dim 64.
_BEATMAP_HD = dict(
    vocab_size=200, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
    max_position_embeddings=1024, global_attn_every_n_layers=2, local_attention=128,
    global_rope_theta=160000.0, local_rope_theta=10000.0,
    audio_sos_token_id=197, audio_eos_token_id=198, audio_token_id=199, cls_embed=False,
    audio_config=dict(
        hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1,
        max_position_embeddings=1024, global_attn_every_n_layers=3, local_attention=128,
        projector_intermediate_size=128, projector_dim=256, n_mels=16,
    ),
)
# metadata tower: hidden 192 / 2 heads = head_dim 96, every layer global
_METADATA_HD = dict(
    vocab_size=100, hidden_size=192, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
    max_position_embeddings=128, global_attn_every_n_layers=1, local_attention=128, cls_embed=False,
)

# padded rows of an odd length > 200 (the band and the padding both matter; one row so short that the sliding layer's late queries
# see no key), mean pooling
CASE = dict(cfg=_cfg(_BEATMAP_HD, _METADATA_HD), B=3, S=203, L=32, pad=True, short_row=100)


def inputs() -> dict[str, torch.Tensor]:
    """cases.make_inputs on this case (it looks the case up by name: registered for the call only)."""
    CASES[NAME] = CASE
    try:
        return make_inputs(NAME)
    finally:
        del CASES[NAME]


def draw_weights(model: torch.nn.Module) -> None:
    """Overwrite every parameter but the logit scale in place: the rules of make_golden.build_model, one generator per name."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "logit_scale":
                continue
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            if "norm" in name:
                w = 1.0 + 0.2 * torch.randn(p.shape, generator=g)
            elif "tok_embeddings" in name:
                w = torch.randn(p.shape, generator=g)
                w[0].zero_()  # padding_idx row stays zero like nn.Embedding's init
            elif p.ndim >= 2:
                w = torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5
            else:
                w = 0.1 * torch.randn(p.shape, generator=g)
            p.copy_(w.to(p.dtype))
