"""cm3p_amd.lora on the CPU: what add_lora registers and freezes on every kind of model that carries an encoder stack, the selection by
`targets` / `layers`, every refusal, the adapter state dict, merge_lora / remove_lora, and the extension C ABI (include/cm3p_lora.h,
_lib.EXT_SIGNATURES) under the rules tests/test_cabi.py and tests/test_kernel_ledger.py apply to cm3p_hip.h.  (The kernels:
tests/test_lora_kernels_gpu.py; the models on them: tests/test_lora_model_gpu.py, `-m gpu`.)"""
import ctypes
import math
import os
import re
import struct

import pytest
import torch

import transformers  # noqa: F401  (a missing transformers is an error here, not a skip)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LORA_HEADER = os.path.join(ROOT, "include", "cm3p_lora.h")
FULL, SLIDE = "full_attention", "sliding_attention"

# Which test checks each entry point of cm3p_lora.h against a reference (the rule of tests/test_kernel_ledger.py), or why none does.
LEDGER = {
    "cm3p_lora_merge_cast_multi": ["tests/test_lora_kernels_gpu.py::test_merged_cast_against_float64",
                                   "tests/test_lora_kernels_gpu.py::test_merged_cast_table_of_several_matrices"],
    "cm3p_lora_grad": ["tests/test_lora_kernels_gpu.py::test_adapter_gradients_against_float64",
                       "tests/test_lora_kernels_gpu.py::test_adapter_gradients_over_three_row_blocks_and_pitched_rows"],
}
EXEMPT = {
    "cm3p_lora_abi_version": "host-only constant; test_lora_header_exports_and_binding_match_one_to_one compares it with the binding",
    "cm3p_lora_grad_workspace_bytes": "host-only size query; test_lora_host_only_queries restates its formula",
    "cm3p_lora_grad_row_block": "host-only query; test_lora_host_only_queries restates its rule",
}


def _cm3p_cfg():
    from cm3p_amd import CM3PConfig

    return CM3PConfig(
        beatmap_config=dict(vocab_size=300, hidden_size=128, intermediate_size=192, num_hidden_layers=3, num_attention_heads=2, cls_embed=False,
                            audio_sos_token_id=297, audio_eos_token_id=298, audio_token_id=299,
                            audio_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1,
                                              projector_intermediate_size=256, projector_dim=128, n_mels=16)),
        metadata_config=dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, cls_embed=False),
        projection_dim=64)


def _hf_cfg(**kw):
    from transformers import ModernBertConfig

    cfg = dict(vocab_size=200, hidden_size=128, intermediate_size=192, num_hidden_layers=4, num_attention_heads=2, max_position_embeddings=512,
               layer_types=[FULL, SLIDE, SLIDE, FULL], local_attention=128, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2)
    cfg.update(kw)
    return ModernBertConfig(**cfg)


def _models():
    from transformers import ModernBertForSequenceClassification

    from cm3p_amd import CM3PModel
    from cm3p_amd.hf_modernbert import FusedModernBertModel, fuse
    from cm3p_amd.modeling_cm3p import CM3PForMaskedLM

    cfg = _cm3p_cfg()
    return [("CM3PModel", CM3PModel(cfg), 3 + 2), ("CM3PForMaskedLM", CM3PForMaskedLM(cfg.beatmap_config), 3),
            ("FusedModernBertModel", FusedModernBertModel(_hf_cfg()), 4),
            ("fused ModernBertForSequenceClassification", fuse(ModernBertForSequenceClassification(_hf_cfg(num_labels=3))), 4)]


@pytest.mark.parametrize("which", range(4))
def test_add_lora_registers_initialises_and_freezes(which):
    from cm3p_amd import lora

    name, model, n_layers = _models()[which]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = {k: p.requires_grad for k, p in model.named_parameters()}
    encs = lora.find_encoders(model)
    assert sum(len(e.layers) for e in encs) == n_layers, name  # (every stack but the audio encoder's, the unregistered one included)
    assert lora.add_lora(model, r=8, alpha=16) is model
    sd = model.state_dict()
    new = sorted(set(sd) - set(before))
    assert len(new) == 2 * 4 * n_layers and all(k.endswith((".lora_A", ".lora_B")) for k in new), name
    params = dict(model.named_parameters())
    assert set(new) <= set(params)  # parameters(): what an optimizer and DDP see
    enc_ids = {id(p) for e in encs for p in e.parameters()}
    for k, p in params.items():
        if k in new:
            lin_w = params[k.rsplit(".", 1)[0] + ".weight"]
            assert p.requires_grad and p.dtype == torch.float32 and p.device == lin_w.device
            if k.endswith("lora_A"):
                assert tuple(p.shape) == (8, lin_w.shape[1])
                bound = 1.0 / math.sqrt(lin_w.shape[1])  # kaiming_uniform_(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
                q = p.detach()
                assert float(q.abs().max()) <= bound and float(q.abs().max()) > 0.5 * bound and abs(float(q.mean())) < 0.2 * bound
            else:
                assert tuple(p.shape) == (lin_w.shape[0], 8) and not bool(p.any())
        elif id(p) in enc_ids:
            assert not p.requires_grad, (name, k)  # the encoders' own parameters are frozen
        else:
            assert p.requires_grad == flags[k], (name, k)  # heads, pooling, the audio encoder: untouched
    assert all(torch.equal(sd[k], v) for k, v in before.items())
    for e in encs:
        assert e.has_lora()
        for layer in e.layers:
            assert layer.attn.Wqkv.lora_scale == 2.0
    # merge_lora: with B = 0 the weights do not move; the base's own keys and flags are back
    lora.merge_lora(model)
    assert set(model.state_dict()) == set(before) and all(torch.equal(model.state_dict()[k], v) for k, v in before.items())
    assert {k: p.requires_grad for k, p in model.named_parameters()} == flags
    assert not any(e.has_lora() for e in encs)


def test_targets_and_layers_select():
    from cm3p_amd import lora
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    m = FusedModernBertModel(_hf_cfg())
    lora.add_lora(m, r=16, alpha=32, targets=("attn.Wqkv", "mlp.Wo"), layers=[1, 3], freeze_base=False)
    assert sorted(lora.lora_state_dict(m)) == sorted(f"layers.{i}.{t}.lora_{ab}" for i in (1, 3) for t in ("attn.Wqkv", "mlp.Wo") for ab in "AB")
    assert all(p.requires_grad for p in m.parameters())  # freeze_base=False
    spec = m.encoder._stack_lora()
    assert [[a is not None for a in row] for row in spec] == [[False] * 4, [True, False, False, True], [False] * 4, [True, False, False, True]]
    lora.remove_lora(m)
    assert lora.lora_state_dict(m) == {} and m.encoder._stack_lora() is None


def test_every_refusal_comes_before_anything_is_registered():
    from cm3p_amd import lora
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    def clean(m):
        return lora.lora_state_dict(m) == {} and all(p.requires_grad for p in m.parameters())

    m = FusedModernBertModel(_hf_cfg())
    for r in (0, 4, 12, 128, 16.5):
        with pytest.raises(ValueError, match="r must be one of"):
            lora.add_lora(m, r=r)
    with pytest.raises(ValueError, match="targets"):
        lora.add_lora(m, targets=("attn.Wq",))
    with pytest.raises(ValueError, match="layers"):
        lora.add_lora(m, layers=[4])
    with pytest.raises(ValueError, match="no CM3PEncoder"):
        lora.add_lora(torch.nn.Linear(8, 8))
    with pytest.raises(TypeError):
        lora.add_lora(m, lora_dropout=0.1)  # not offered: the merged form has no place for it
    assert clean(m)
    # bf16 master weights
    mb = FusedModernBertModel(_hf_cfg()).to(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp32 master"):
        lora.add_lora(mb)
    assert clean(mb)
    # the bf16 residual stream of training steps: at add_lora, and at the call when it is switched on afterwards
    mt = FusedModernBertModel(_hf_cfg()).set_residual_dtype(torch.bfloat16, training=True)
    with pytest.raises(NotImplementedError, match="bf16 residual stream"):
        lora.add_lora(mt)
    assert clean(mt)
    mt.set_residual_dtype(None, training=True)
    lora.add_lora(mt)
    mt.set_residual_dtype(torch.bfloat16, training=True)
    with pytest.raises(NotImplementedError, match="bf16 residual stream"):
        mt.encoder._bf16_stream(None)  # (what every forward asks before its first launch)
    # extents that are not multiples of 8: refused with the layer named (a weight replaced after construction; the constructor refuses
    # such configurations itself)
    mo = FusedModernBertModel(_hf_cfg())
    mo.layers[2].mlp.Wo.weight = torch.nn.Parameter(torch.zeros(128, 196))
    with pytest.raises(NotImplementedError, match=r"layers\.2\.mlp\.Wo.*multiples of 8"):
        lora.add_lora(mo)
    assert clean(mo)
    # twice
    lora.add_lora(m, layers=[0])
    with pytest.raises(ValueError, match="already carries"):
        lora.add_lora(m)


def test_state_dict_round_trip_and_merge_folds_the_product():
    from cm3p_amd import lora
    from cm3p_amd.hf_modernbert import FusedModernBertModel

    torch.manual_seed(0)
    a, b = FusedModernBertModel(_hf_cfg()), FusedModernBertModel(_hf_cfg())
    b.load_state_dict(a.state_dict())
    lora.add_lora(a, r=8, alpha=4)
    with torch.no_grad():
        for k, v in lora.lora_state_dict(a).items():
            if k.endswith("lora_B"):
                v.normal_(std=0.02)
    sd = {k: v.clone() for k, v in lora.lora_state_dict(a).items()}
    with pytest.raises(KeyError):
        lora.load_lora_state_dict(b, sd)  # no adapters there yet
    lora.add_lora(b, r=8, alpha=4)
    with pytest.raises(KeyError):
        lora.load_lora_state_dict(b, {k: v for k, v in sd.items() if "layers.0." not in k})
    with pytest.raises(ValueError):
        lora.load_lora_state_dict(b, {k: v[:4] if k.endswith("lora_A") else v for k, v in sd.items()})
    ver = b.layers[0].attn.Wqkv.lora_B._version
    lora.load_lora_state_dict(b, sd)
    assert b.layers[0].attn.Wqkv.lora_B._version > ver  # (the forward-only weight cache sees the load)
    assert all(torch.equal(v, lora.lora_state_dict(b)[k]) for k, v in sd.items())
    w0 = b.layers[1].mlp.Wi.weight.detach().clone()
    A, B = sd["layers.1.mlp.Wi.lora_A"], sd["layers.1.mlp.Wi.lora_B"]
    lora.merge_lora(b)
    assert torch.equal(b.layers[1].mlp.Wi.weight, w0 + 0.5 * (B @ A))
    assert set(b.state_dict()) == set(FusedModernBertModel(_hf_cfg()).state_dict()) and all(p.requires_grad for p in b.parameters())


# ---- the extension ABI --------------------------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)  # (the parse of tests/test_cabi.py)
    return sorted(set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text))), text


@pytest.fixture(scope="module")
def lib():
    from cm3p_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_lora_header_exports_and_binding_match_one_to_one(lib):
    from cm3p_amd import _lib

    names, text = _declared(LORA_HEADER)
    assert names == sorted(_lib.EXT_SIGNATURES) and len(names) == 5
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    for name, argtypes in _lib.EXT_SIGNATURES.items():
        m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(argtypes), (name, n, len(argtypes))
        assert (m.group(0).split()[0] == "int64_t") == (name in _lib._RETURNS_INT64), name
    assert lib.cm3p_lora_abi_version() == _lib.LORA_ABI_VERSION == int(re.search(r"#define CM3P_LORA_ABI_VERSION (\d+)", text).group(1))
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)


def test_cm3p_hip_h_and_its_abi_version_are_unchanged(lib):
    from cm3p_amd import _lib

    names, text = _declared(os.path.join(ROOT, "include", "cm3p_hip.h"))
    assert names == sorted(_lib.SIGNATURES) and not [n for n in names if "lora" in n]
    assert _lib.ABI_VERSION == 20 == lib.cm3p_abi_version() and "#define CM3P_ABI_VERSION 20" in text


def test_lora_ledger_covers_the_header_and_names_real_tests():
    names, _ = _declared(LORA_HEADER)
    assert sorted(set(LEDGER) | set(EXEMPT)) == names and not set(LEDGER) & set(EXEMPT)
    assert all(LEDGER.values()) and all(r.strip() for r in EXEMPT.values())
    for ids in LEDGER.values():
        for tid in ids:
            path, fn = tid.split("::")
            assert re.search(r"^def " + fn + r"\(", open(os.path.join(ROOT, path)).read(), flags=re.M), tid


def test_lora_host_only_queries(lib):
    from cm3p_amd import _lib

    assert [_lib.query("cm3p_lora_grad_row_block", T) for T in (1, 256, 16384, 16385, 131072)] == [256, 256, 256, 512, 2048]
    assert _lib.query("cm3p_lora_grad_row_block", 0) == -1
    T, K, N, r = 552, 72, 216, 64
    Tp, nrb = 576, 3
    assert _lib.query("cm3p_lora_grad_workspace_bytes", T, K, N, r) == 2 * r * (K + N) + 2 * 2 * r * Tp + 4 * nrb * r * (K + N)
    for bad in ((0, 64, 64, 8), (8, 60, 64, 8), (8, 64, 68, 8), (8, 64, 64, 12), (8, 64, 64, 128)):
        assert _lib.query("cm3p_lora_grad_workspace_bytes", *bad) == -1, bad


def test_null_and_unsupported_arguments_are_refused_without_a_gpu(lib):
    """Validation happens before any HIP call: CM3P_ERR_INVALID (-1), nothing launched."""
    from cm3p_amd import _lib

    fake = 4096  # an aligned, never dereferenced address
    need = _lib.query("cm3p_lora_grad_workspace_bytes", 65, 64, 192, 8)
    args = dict(X=fake, ldx=64, DY=fake, ldy=192, A=fake, B=fake, s=2.0, dA=fake, dB=fake, T=65, K=64, N=192, r=8, ws=fake, ws_bytes=need, stream=None)

    def grad(**kw):
        a = dict(args, **kw)
        return lib.cm3p_lora_grad(*[a[k] for k in args])

    for k in ("X", "DY", "A", "B", "dA", "dB", "ws"):
        assert grad(**{k: None}) == -1, k
    assert grad(r=12) == -1 and grad(r=0) == -1 and grad(r=128) == -1
    assert grad(T=0) == -1 and grad(K=60) == -1 and grad(N=100) == -1
    assert grad(ldx=56) == -1 and grad(ldy=196) == -1 and grad(ws_bytes=need - 1) == -1 and grad(X=fake + 2) == -1

    def table(**kw):
        e = dict(W=fake, A=fake, B=fake, s=int.from_bytes(struct.pack("<f", 2.0), "little"), rows=64, cols=64, r=8, out=fake, out_t=fake, first=0)
        e.update(kw)
        return (ctypes.c_int64 * 10)(*e.values())

    def merge(host, dev=fake, n=1):
        return lib.cm3p_lora_merge_cast_multi(host, dev, n, None)

    assert merge(None) == -1 and merge(table(), dev=None) == -1 and merge(table(), n=0) == -1
    for k in ("W", "A", "B", "out", "out_t"):
        assert merge(table(**{k: 0})) == -1 and merge(table(**{k: fake + 4})) == -1, k
    assert merge(table(r=12)) == -1 and merge(table(rows=60)) == -1 and merge(table(cols=0)) == -1 and merge(table(first=1)) == -1
    assert merge(table(rows=-96)) == -1  # interleaved GeGLU rows need 2 I a multiple of 64
