"""Dropout without a GPU: the configs that set embedding_dropout / attention_dropout / mlp_dropout build, out-of-range probabilities fail like
nn.Dropout, and the RNG contract of cm3p_amd/csrc/dropout_rng.h (Philox4x32-10, thresholds, 16-bit halves) agrees with a plain
Python restatement.  The restatement here (keep_mask_ref) is also what tests/test_dropout_gpu.py compares the kernels against."""
import copy

import numpy as np
import pytest

from cases import CASES

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox_ref(ctr, key):
    """Philox4x32-10 (Random123), one counter, scalar Python."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK32, p1 & MASK32, ((p0 >> 32) ^ c3 ^ k1) & MASK32, p0 & MASK32
    return c0, c1, c2, c3


def philox_np(c0, c1, c2, c3, k0, k1):
    """The same, vectorised over numpy uint32 arrays (broadcasting)."""
    u64 = np.uint64
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)
    for r in range(10):
        if r:
            k0, k1 = (k0 + u64(W0)) & u64(MASK32), (k1 + u64(W1)) & u64(MASK32)
        p0, p1 = c[0] * u64(M0), c[2] * u64(M1)
        c = [((p1 >> u64(32)) ^ c[1] ^ k0) & u64(MASK32), p1 & u64(MASK32), ((p0 >> u64(32)) ^ c[3] ^ k1) & u64(MASK32), p0 & u64(MASK32)]
    return c


def threshold_ref(p):
    return int(np.floor(p * 65536.0 + 0.5))


def scale_ref(thr):
    return 0.0 if thr >= 65536 else float(np.float32(65536.0) / np.float32(65536 - thr))


def keep_mask_ref(n2, n1, n0, layer, site, thr, seed):
    """keep[i2, i1, i0] of the contract: counter (i0 >> 3, i1, i2, 4 layer + site), key (seed low, seed high), decision i0 & 7 =
    16-bit half (i0 & 7) of the output, kept iff >= thr."""
    i2, i1, g = np.meshgrid(np.arange(n2), np.arange(n1), np.arange((n0 + 7) // 8), indexing="ij")
    w = philox_np(g, i1, i2, np.full_like(g, 4 * layer + site), seed & MASK32, seed >> 32)
    halves = np.stack([(w[j >> 1] >> np.uint64(16 * (j & 1))) & np.uint64(0xFFFF) for j in range(8)], axis=-1)  # [n2, n1, groups, 8]
    return (halves >= thr).reshape(n2, n1, -1)[:, :, :n0].astype(np.uint8)


def _cfg(**tower_over):
    cfg = copy.deepcopy(CASES["d64_cls_nopad"]["cfg"])
    for tower in ("beatmap_config", "metadata_config"):
        cfg[tower].update(tower_over)
    cfg["beatmap_config"]["audio_config"].update(tower_over)
    return cfg


@pytest.mark.parametrize("field", ["embedding_dropout", "attention_dropout", "mlp_dropout"])
def test_models_with_dropout_construct(field):
    from cm3p_amd import CM3PConfig, CM3PModel

    m = CM3PModel(CM3PConfig(**_cfg(**{field: 0.1})))
    assert getattr(m.beatmap_model.encoder.config, field) == 0.1
    assert getattr(m.metadata_model.encoder.config, field) == 0.1
    CM3PModel(CM3PConfig(**_cfg(embedding_dropout=1.0, attention_dropout=0.3, mlp_dropout=0.5)))


@pytest.mark.parametrize("field", ["embedding_dropout", "mlp_dropout", "attention_dropout"])
@pytest.mark.parametrize("p", [-0.1, 1.5])
def test_out_of_range_probabilities_raise_value_error(field, p):
    from cm3p_amd import CM3PConfig, CM3PModel

    with pytest.raises(ValueError, match=field):
        CM3PModel(CM3PConfig(**_cfg(**{field: p})))


def test_head_dim_16_towers_take_every_dropout_field():
    """The reference's tiny configuration (head_dim 16, the generic attention kernels) builds with all three fields set."""
    from cm3p_amd import CM3PConfig, CM3PModel

    cfg = copy.deepcopy(CASES["c1_tiny_nopad"]["cfg"])
    over = {"embedding_dropout": 0.1, "attention_dropout": 0.1, "mlp_dropout": 0.1}
    m = CM3PModel(CM3PConfig(**{**cfg, "beatmap_config": {**cfg["beatmap_config"], **over}, "metadata_config": {**cfg["metadata_config"], **over}}))
    assert m.beatmap_model.encoder.config.attention_dropout == 0.1


def test_philox_known_answers():
    from cm3p_amd import kernels as K

    ctr = [[0, 0, 0, 0], [MASK32] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]]
    key = [[0, 0], [MASK32] * 2, [0xA4093822, 0x299F31D0]]
    want = [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]
    assert K.philox4x32_10_host(ctr, key).tolist() == want
    assert [list(philox_ref(c, k)) for c, k in zip(ctr, key)] == want


def test_philox_matches_python_restatement():
    from cm3p_amd import kernels as K

    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, size=(1500, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, size=(1500, 2), dtype=np.uint64).astype(np.uint32)
    got = K.philox4x32_10_host(ctr, key)
    for i in range(0, 1500, 7):
        assert tuple(got[i]) == philox_ref(tuple(int(x) for x in ctr[i]), tuple(int(x) for x in key[i]))
    w = philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1])
    assert np.array_equal(np.stack(w, axis=1).astype(np.uint32), got)


def test_keep_rule():
    from cm3p_amd import kernels as K

    for p in (0.0, 1e-6, 0.1, 0.25, 0.5, 0.9, 1.0):
        assert K.dropout_threshold(p) == threshold_ref(p)
        assert K.dropout_scale(K.dropout_threshold(p)) == scale_ref(threshold_ref(p))
    assert K.dropout_threshold(0.1) == 6554 and K.dropout_scale(0) == 1.0 and K.dropout_scale(65536) == 0.0
    assert K.dropout_scale(32768) == 2.0
    # decision j of a call is the 16-bit half j of its output: j = 0 low half of word 0, j = 1 its high half, ...
    seed = 0x0123456789ABCDEF
    w = K.philox4x32_10_host([[5, 3, 2, 4 * 1 + 3]], [[seed & MASK32, seed >> 32]])[0]
    halves = [(int(w[j >> 1]) >> (16 * (j & 1))) & 0xFFFF for j in range(8)]
    for thr in (0, 6554, 32768, 65536):
        keep = keep_mask_ref(3, 4, 48, 1, 3, thr, seed)[2, 3, 40:48]
        assert keep.tolist() == [int(h >= thr) for h in halves]
    assert keep_mask_ref(2, 2, 16, 0, 0, 0, seed).all() and not keep_mask_ref(2, 2, 16, 0, 0, 65536, seed).any()
