"""The low-rank adapter kernels (csrc/lora.hip) against the float64 references of tests/lora_refs.py: the merged cast bit for bit
wherever the reference is clear of a bf16 rounding boundary (either neighbour elsewhere), with guard bytes around every output, and the
adapter gradients under the node bound |got - R| <= M_NODE |E - R| at every token-count seam of the kernels (one 64-token block of
the down stage short, exact and over; a short last row block of the token reduction; pitched rows), run twice for equal bits.
tests/test_lora_refs_host.py shows on the CPU that a correct kernel fits these checks and that wrong ones do not.

Each check prints its figures (`pytest -rP`).  CM3P_LORA_ERRORS_OUT=<file>: write the node ratios this run measured there."""
import json
import os
import struct

import pytest
import torch

import lora_refs as LR

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64        # sentinel elements before and after a caller-owned output (128 bytes: the outputs stay 16-byte aligned)
SENTINEL = 777.0  # (exact in bf16)
_SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    path = os.environ.get("CM3P_LORA_ERRORS_OUT")
    if _SEEN and path:
        with open(path, "w") as f:
            json.dump(dict(measured=_SEEN, margin=LR.M_NODE), f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def K():
    from cm3p_amd import kernels

    return kernels


def _merge(entries):
    """entries: [(W, A, B, s, interleave)] CPU fp32 -> [(out, out_t)] CPU, through cm3p_lora_merge_cast_multi with caller-owned outputs
    between sentinels (checked here)."""
    from cm3p_amd import _lib

    keep, table, outs, blocks = [], [], [], 0
    for W, A, B, s, il in entries:
        rows, cols = W.shape
        w, a, b = W.to(DEV), A.to(DEV), B.to(DEV)
        bufs = [torch.full((rows * cols + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        for q in bufs:
            q[GUARD:GUARD + rows * cols] = float("nan")
        keep += [w, a, b, *bufs]
        s_bits = int.from_bytes(struct.pack("<f", float(s)), "little")
        table += [w.data_ptr(), a.data_ptr(), b.data_ptr(), s_bits, -rows if il else rows, cols, A.shape[0],
                  bufs[0].data_ptr() + 2 * GUARD, bufs[1].data_ptr() + 2 * GUARD, blocks]
        blocks += (-(-rows // 64)) * (-(-cols // 64))
        outs.append((bufs, rows, cols))
    host = torch.tensor(table, dtype=torch.int64)
    tab = host.to(DEV)
    _lib.call("cm3p_lora_merge_cast_multi", host.data_ptr(), _lib.ptr(tab, torch.int64), len(entries), _lib.stream())
    torch.cuda.synchronize()
    res = []
    for bufs, rows, cols in outs:
        for q in bufs:
            assert bool((q[:GUARD] == SENTINEL).all()) and bool((q[GUARD + rows * cols:] == SENTINEL).all()), "guard bytes were written"
        res.append((bufs[0][GUARD:GUARD + rows * cols].view(rows, cols).cpu(), bufs[1][GUARD:GUARD + rows * cols].view(cols, rows).cpu()))
    return res


@pytest.mark.parametrize("case", range(len(LR.MERGE_SHAPES)))
def test_merged_cast_against_float64(case):
    W, A, B, s, il = LR.merge_single_cases()[case]
    (out, out_t), = _merge([(W, A, B, s, il)])
    frac = LR.merge_check(out, out_t, W, A, B, s, il, f"merge {tuple(W.shape)} r{A.shape[0]}")
    print(f"merge {tuple(W.shape)} r{A.shape[0]} interleave {il}: {frac:.4%} of elements on the either-neighbour branch")


def test_merged_cast_table_of_several_matrices():
    cases = LR.merge_table_cases()
    for i, ((W, A, B, s, il), (out, out_t)) in enumerate(zip(cases, _merge(cases))):
        LR.merge_check(out, out_t, W, A, B, s, il, f"table entry {i}")


@pytest.mark.parametrize("il", (False, True))
def test_merged_cast_with_zero_b_is_the_plain_cast_in_bits(K, il):
    W, A, B = LR.merge_case(128, 72, 16, seed=7, zero_b=True)
    W[0, 0], W[5, 3] = -0.0, 0.0
    (out, out_t), = _merge([(W, A, B, 2.0, il)])
    (y, yt), = K.cast_bf16_with_transpose_many([W.to(DEV)], [il])
    LR.bits_equal(out, y, "merged copy against the plain cast")
    LR.bits_equal(out_t, yt, "merged transpose against the plain cast")
    (y2, yt2), = K.lora_merge_cast_many([(W.to(DEV), A.to(DEV), B.to(DEV), 2.0, il)])  # (the wrapper: same launch, its own buffers)
    LR.bits_equal(y2, y, "wrapper's copy")
    LR.bits_equal(yt2, yt, "wrapper's transpose")


def _row_block_T(K):
    """A token count that spans three row blocks of the token reduction with a short last one."""
    tb = K.lora_grad_row_block(1000)
    T = 2 * tb + 40
    assert K.lora_grad_row_block(T) == tb and -(-T // tb) == 3
    return T


GRAD_T = (1, 63, 64, 65, 200)


def _grad_check(K, T, Kd, N, r, s, seed, pitch_x=None):
    X, DY, A, B = LR.grad_case(T, Kd, N, r, seed, pitch_x)
    Xd = X.to(DEV) if pitch_x is None else X._base.to(DEV)[:, :Kd]
    args = (Xd, DY.to(DEV), A.to(DEV), B.to(DEV), s)
    dA, dB = K.lora_grad(*args)
    dA2, dB2 = K.lora_grad(*args)
    LR.bits_equal(dA2, dA, "dA of a second run")
    LR.bits_equal(dB2, dB, "dB of a second run")
    R, E = LR.grad_ref(X, DY, A, B, s), LR.grad_rounded(X, DY, A, B, s)
    tag = f"T{T} K{Kd} N{N} r{r}" + (f" pitch {pitch_x}" if pitch_x else "")
    for name, got in (("dA", dA), ("dB", dB)):
        _SEEN[f"{name} {tag}"] = LR.node_check(got, R[name], E[name], f"{name} {tag}")


@pytest.mark.parametrize("T", GRAD_T)
@pytest.mark.parametrize("Kd", (64, 72))
@pytest.mark.parametrize("mult", (1, 3))
@pytest.mark.parametrize("r", (8, 64))
def test_adapter_gradients_against_float64(K, T, Kd, mult, r):
    _grad_check(K, T, Kd, mult * Kd, r, 32.0 / r, seed=T * 7 + Kd + r)


def test_adapter_gradients_over_three_row_blocks_and_pitched_rows(K):
    T = _row_block_T(K)
    _grad_check(K, T, 72, 216, 64, 0.5, seed=3)
    _grad_check(K, T, 64, 64, 8, 4.0, seed=4)
    _grad_check(K, 200, 72, 72, 8, 4.0, seed=5, pitch_x=88)
    _grad_check(K, 65, 64, 192, 64, 0.5, seed=6, pitch_x=72)


def test_adapter_gradients_with_zero_scale_are_exact_zeros(K):
    X, DY, A, B = LR.grad_case(65, 72, 216, 8, seed=9)
    dA, dB = K.lora_grad(X.to(DEV), DY.to(DEV), A.to(DEV), B.to(DEV), 0.0)
    assert bool((dA == 0).all()) and bool((dB == 0).all())
