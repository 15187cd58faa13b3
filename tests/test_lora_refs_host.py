"""tests/lora_refs.py on the CPU: the rounded restatements E of the adapter kernels fit the checks tests/test_lora_kernels_gpu.py applies
to the kernels (so the bounds are attainable), the chosen seeds keep the merged cast's reference clear of bf16 rounding boundaries
within the cap, and evaluations that are wrong in one place are refused (so the bounds are sharp)."""
import pytest
import torch

import lora_refs as LR



def _fails(what, fn):
    with pytest.raises(AssertionError):
        fn()
    print(f"refused: {what}")


def test_bf16_rne64_is_torchs_rounding_and_the_interleave_is_a_permutation():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g)  # (fp32 values: one rounding either way)
    assert torch.equal(LR.bf16_rne64(x.double()), x.to(torch.bfloat16).double())
    ties = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8)], dtype=torch.float64)
    assert LR.bf16_rne64(ties).tolist() == [1.0, 1.0 + 2 ** -6, -1.0]
    idx = LR.interleave_index(64)
    assert sorted(idx.tolist()) == list(range(128)) and idx[:3].tolist() == [0, 1, 2] and idx[32:34].tolist() == [64, 65] and idx[64] == 32


def test_merged_cast_restatement_fits_and_seeds_stay_under_the_cap():
    """Every case the GPU test runs: E passes the check the kernel gets, and the reference is clear of rounding boundaries within the cap."""
    for i, (W, A, B, s, il) in enumerate(LR.merge_single_cases() + LR.merge_table_cases()):
        out, out_t = LR.merge_rounded(W, A, B, s, il)
        frac = LR.merge_check(out, out_t, W, A, B, s, il, f"E case {i}")
        print(f"case {i}: {tuple(W.shape)} r {A.shape[0]} s {s}: {frac:.4%} either-neighbour")
        assert frac <= LR.AMBIGUOUS_CAP


def test_merged_cast_with_zero_b_is_the_plain_cast():
    W, A, B = LR.merge_case(128, 72, 16, seed=7, zero_b=True)
    out, out_t = LR.merge_rounded(W, A, B, 2.0)
    assert torch.equal(out, W.to(torch.bfloat16).double()) and torch.equal(out_t, out.t())
    assert LR.merge_check(out, out_t, W, A, B, 2.0, False, "B = 0") == 0.0


def test_wrong_merged_casts_are_refused():
    W, A, B = LR.merge_case(128, 64, 8, seed=1)
    for wrong, il in (("s_twice", False), ("interleave_on_transpose", True)):
        out, out_t = LR.merge_rounded(W, A, B, 4.0, il, wrong=wrong)
        _fails(wrong, lambda: LR.merge_check(out, out_t, W, A, B, 4.0, il, wrong))
    out, out_t = LR.merge_rounded(W, A, B, 4.0, True)
    _fails("canonical rows where interleaved ones belong", lambda: LR.merge_check(out_t.t(), out_t, W, A, B, 4.0, True, "rows"))
    # the adapter as a separate bf16 product added to bf16(W): two roundings more than the kernel makes
    two = (W.to(torch.bfloat16).float() + (4.0 * (B @ A)).to(torch.bfloat16).float()).to(torch.bfloat16).double()
    _fails("separate bf16 product", lambda: LR.merge_check(two, two.t(), W, A, B, 4.0, False, "two roundings"))


GRAD_SHAPES = ((1, 64, 64, 8), (63, 64, 192, 64), (65, 72, 72, 64), (200, 72, 216, 8), (552, 64, 64, 64))


@pytest.mark.parametrize("T,K,N,r", GRAD_SHAPES)
def test_gradient_restatement_sits_at_ratio_one(T, K, N, r):
    X, DY, A, B = LR.grad_case(T, K, N, r, seed=T)
    R, E = LR.grad_ref(X, DY, A, B, 2.0), LR.grad_rounded(X, DY, A, B, 2.0)
    for k in ("dA", "dB"):
        LR.node_check(E[k], R[k], E[k], k, m=1.0)


@pytest.mark.parametrize("wrong", ("s_twice", "u_unrounded_swapped_with_v", "a_for_a_t", "last_row_dropped"))
def test_wrong_gradients_are_refused(wrong):
    T, K, N, r = 65, 64, 192, 64  # (K = r: A stands where A^T belongs without a shape error)
    X, DY, A, B = LR.grad_case(T, K, N, r, seed=11)
    R, E, Wr = LR.grad_ref(X, DY, A, B, 2.0), LR.grad_rounded(X, DY, A, B, 2.0), LR.grad_rounded(X, DY, A, B, 2.0, wrong=wrong)
    refused = 0
    for k in ("dA", "dB"):
        try:
            LR.node_check(Wr[k], R[k], E[k], f"{wrong}: {k}")
        except AssertionError:
            refused += 1
    # a_for_a_t touches u only, so dB alone moves; every other variant moves both
    assert refused == (1 if wrong == "a_for_a_t" else 2), (wrong, refused)


def test_pitched_case_keeps_its_pad_columns_out_of_the_values():
    X, DY, A, B = LR.grad_case(9, 72, 72, 8, seed=5, pitch_x=88)
    assert X.shape == (9, 72) and X.stride(0) == 88 and bool((X._base[:, 72:] > 1e38).all()) and bool(torch.isfinite(X.float()).all())
