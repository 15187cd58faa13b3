"""Which test checks each C-ABI entry point against a reference.  Every function the public headers (include/cm3p_hip.h, cm3p_lora.h,
cm3p_attn_row.h, cm3p_attn_qrows.h) declare is either in LEDGER, with the test functions that compare its results with a reference
restatement (node ids without parameters), or in EXEMPT with the reason it has none (host-side size and version queries, ablation and
audit hooks).  A new entry point cannot land without one or the other; every header under include/ is read, so neither can a new header.
No GPU needed: the tests named here are found by parsing their files."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))  # every public header, also one a later change adds

KG = "tests/test_kernels_gpu.py::"
CH = "tests/test_conv_head_kernels_gpu.py::"
DR = "tests/test_dropout_gpu.py::"
DK = "tests/test_dropout_kernels_gpu.py::"
MU = "tests/test_muon_gpu.py::"
MG = "tests/test_model_gpu.py::"
RK = "tests/test_row_kernels_gpu.py::"
GK = "tests/test_gemm_kernels_gpu.py::"
AD = "tests/test_attention_d64_gpu.py::"
AF = "tests/test_attention_fused_gpu.py::"
MK = "tests/test_muon_kernels_gpu.py::"
LH = "tests/test_loss_head_gpu.py::"
AG = "tests/test_attn_generic_gpu.py::"
LK = "tests/test_lora_kernels_gpu.py::"
AW = "tests/test_attn_row_kernels_gpu.py::"
AQ = "tests/test_attn_qrows_kernels_gpu.py::"

LEDGER = {
    "cm3p_layernorm_fwd": [KG + "test_layernorm_fwd_bwd", CH + "test_layernorm_with_many_rows_per_wave",
                           RK + "test_layernorm_forward_every_instance_and_output_form", RK + "test_layernorm_forward_on_rows_that_break_a_careless_variance"],
    "cm3p_layernorm_bwd": [KG + "test_layernorm_fwd_bwd", CH + "test_layernorm_with_many_rows_per_wave",
                           RK + "test_layernorm_backward_every_form"],
    "cm3p_embed_ln_fwd": [KG + "test_embed_ln_with_audio_override",
                          RK + "test_embed_ln_forward_is_layernorm_of_the_gathered_rows"],
    "cm3p_embed_ln_bwd": [KG + "test_embed_ln_with_audio_override",
                          RK + "test_embed_ln_backward_against_float64_autograd"],
    "cm3p_embed_ln_bwd_sorted": [KG + "test_embed_ln_with_audio_override", KG + "test_embedding_backward_in_id_order_is_reproducible_and_matches_autograd",
                                 RK + "test_embed_ln_backward_against_float64_autograd"],
    "cm3p_token_order": [KG + "test_token_order_is_the_stable_sort_of_the_ids"],
    "cm3p_audio_slots": [KG + "test_embed_ln_with_audio_override",
                         RK + "test_audio_slots_is_the_exclusive_cumsum"],
    "cm3p_gemm_bf16": [KG + "test_gemm_forward_layout", KG + "test_gemm_dgrad_layout", KG + "test_gemm_wgrad_layout",
                       KG + "test_gemm256_forward_and_dgrad_layout", KG + "test_gemm256_wgrad_layout", KG + "test_gemm_bias_epilogue",
                       GK + "test_forward_every_epilogue_at_one_to_five_k_tiles", GK + "test_forward_edge_tiles",
                       GK + "test_k_strided_operands_with_ragged_tiles", GK + "test_wgrad_split_k_with_a_short_last_split",
                       GK + "test_linear_wgrad_reaches_the_big_kernel_by_the_librarys_own_split", GK + "test_small_kernel_natively",
                       GK + "test_pitched_operands_and_output", GK + "test_random_data_within_the_derived_bound"],
    "cm3p_gemm8p_set_grid": [KG + "test_ring_gemm_with_more_workgroups_than_cus_is_the_same_gemm",
                             GK + "test_forward_every_epilogue_at_one_to_five_k_tiles"],
    "cm3p_gemm8p_get_grid": [KG + "test_ring_gemm_with_more_workgroups_than_cus_is_the_same_gemm",
                             GK + "test_forward_every_epilogue_at_one_to_five_k_tiles"],
    "cm3p_qkv_gemm_rope": [KG + "test_fused_qkv_rope_gemm_and_inverse_in_attention_backward",
                           GK + "test_rope_epilogue_against_its_kernels_specification"],
    "cm3p_cast_f32_bf16": [CH + "test_cast_f32_bf16_is_rne"],
    "cm3p_cast_f32_bf16_t": [KG + "test_cast_with_transpose"],
    "cm3p_cast_f32_bf16_t_multi": [KG + "test_cast_with_transpose_of_many_matrices_in_one_launch"],
    "cm3p_add_f32": [CH + "test_add_f32_is_the_fp32_add_then_rne", CH + "test_add_f32_with_no_elements"],
    "cm3p_rope_table": [KG + "test_rope_matches_reference_formula",
                        RK + "test_rope_table_is_cos_sin_of_the_fp32_product"],
    "cm3p_rope_apply": [KG + "test_rope_matches_reference_formula",
                        RK + "test_rope_apply_against_the_float64_rotation"],
    "cm3p_attn_fwd": [KG + "test_attention_global_nopad", KG + "test_attention_random_shapes", KG + "test_attention_sliding_window",
                      AD + "test_matches_float64", AD + "test_exact_conditions", AD + "test_count_probe", AD + "test_window0_copies_v_and_dout",
                      AD + "test_the_largest_window_is_the_window_s_in_bits",
                      AF + "test_matches_float64", AF + "test_count_probe", AF + "test_the_length_rule_picks_four_key_blocks_per_slab"],
    "cm3p_attn_probs": [MG + "test_output_attentions_matches_the_reference_eager_probabilities",
                        AD + "test_probs"],
    "cm3p_attn_bwd": [KG + "test_attention_global_backward_both_implementations", KG + "test_attention_random_shapes",
                      AD + "test_matches_float64", AD + "test_exact_conditions", AD + "test_count_probe", AD + "test_band_equals_global_when_the_window_covers_everything",
                      AD + "test_the_largest_window_is_the_window_s_in_bits"],
    "cm3p_attn_fwd_generic": [KG + "test_generic_attention_matches_fp32_reference",
                              AG + "test_matches_float64", AG + "test_count_probe", AG + "test_window0_copies_v_and_dout",
                              AG + "test_a_window_that_covers_the_axis_is_the_global_mask_in_bits",
                              AG + "test_head_64_both_kernel_families_meet_their_own_float64_bounds"],
    "cm3p_attn_bwd_generic": [KG + "test_generic_attention_matches_fp32_reference",
                              AG + "test_matches_float64", AG + "test_count_probe", AG + "test_window0_copies_v_and_dout",
                              AG + "test_a_window_that_covers_the_axis_is_the_global_mask_in_bits",
                              AG + "test_head_64_both_kernel_families_meet_their_own_float64_bounds"],
    "cm3p_attn_fwd_generic_dropout": [DR + "test_generic_attention_dropout_matches_fp32_restatement",
                                      AG + "test_dropout", AG + "test_dropout_at_a_window_that_covers_the_axis"],
    "cm3p_attn_bwd_generic_dropout": [DR + "test_generic_attention_dropout_matches_fp32_restatement",
                                      AG + "test_dropout", AG + "test_dropout_at_a_window_that_covers_the_axis"],
    "cm3p_rope_apply_generic": [KG + "test_generic_rope_is_the_reference_rotation_and_its_transpose",
                                RK + "test_rope_apply_against_the_float64_rotation"],
    "cm3p_attn_bwd_fused": [KG + "test_attention_global_backward_both_implementations",
                            AD + "test_matches_float64",
                            AF + "test_matches_float64", AF + "test_same_bits", AF + "test_one_valid_key_block_moved_along_the_sequence",
                            AF + "test_rope_epilogues_match_float64", AF + "test_packed_equals_padded_and_matches_float64", AF + "test_count_probe",
                            AF + "test_the_length_rule_picks_four_key_blocks_per_slab"],
    "cm3p_attn_fwd_dropout": [DR + "test_attention_dropout_matches_fp32_restatement",
                              AD + "test_dropout_at_other_windows",
                              DK + "test_attention_dropout_matches_float64", DK + "test_attention_dropout_with_a_top_bit_seed_and_another_layer"],
    "cm3p_attn_bwd_dropout": [DR + "test_attention_dropout_matches_fp32_restatement",
                              AD + "test_dropout_at_other_windows",
                              DK + "test_attention_dropout_matches_float64", DK + "test_attention_dropout_with_a_top_bit_seed_and_another_layer"],
    "cm3p_attn_fwd_dropout_varlen": [DR + "test_attention_dropout_varlen_equals_padded",
                                     DK + "test_packed_attention_dropout_matches_float64"],
    "cm3p_attn_bwd_dropout_varlen": [DR + "test_attention_dropout_varlen_equals_padded",
                                     DK + "test_packed_attention_dropout_matches_float64"],
    "cm3p_geglu_fwd": [KG + "test_geglu_and_gelu",
                       RK + "test_geglu_against_float64"],
    "cm3p_gemm_geglu": [KG + "test_wi_gemm_with_geglu_in_its_store_phase_equals_the_two_kernels",
                        GK + "test_geglu_epilogue_against_float64_and_the_two_kernel_chain"],
    "cm3p_geglu_bwd": [KG + "test_geglu_and_gelu",
                       RK + "test_geglu_against_float64"],
    "cm3p_dropout_f32": [DR + "test_dropout_f32_matches_the_mask_and_packed_equals_padded",
                         DK + "test_dropout_f32_every_output_form_at_one_group_per_row", DK + "test_dropout_f32_past_the_grid",
                         DK + "test_dropout_f32_every_site_and_the_edge_thresholds", DK + "test_dropout_f32_packed_layouts"],
    "cm3p_geglu_fwd_dropout": [DR + "test_geglu_dropout_forward_and_backward",
                               DK + "test_geglu_dropout_against_float64", DK + "test_geglu_dropout_at_the_edge_thresholds"],
    "cm3p_geglu_bwd_dropout": [DR + "test_geglu_dropout_forward_and_backward",
                               DK + "test_geglu_dropout_against_float64", DK + "test_geglu_dropout_at_the_edge_thresholds"],
    "cm3p_dropout_keep": [DR + "test_materialiser_equals_the_restatement",
                          DK + "test_materialiser_in_bits"],
    "cm3p_philox4x32_10_host": ["tests/test_dropout_host.py::test_philox_known_answers", "tests/test_dropout_host.py::test_philox_matches_python_restatement"],
    "cm3p_gelu_fwd": [KG + "test_gelu_on_every_finite_bf16_input_against_float64",
                      RK + "test_gelu_element_kernels_past_the_grid"],
    "cm3p_gelu_bwd": [KG + "test_gelu_on_every_finite_bf16_input_against_float64",
                      RK + "test_gelu_element_kernels_past_the_grid"],
    "cm3p_im2col_k3": [CH + "test_im2col_is_the_padded_gather_bit_for_bit", CH + "test_conv_front_end_refuses_what_it_cannot_do"],
    "cm3p_col2im_k3": [CH + "test_col2im_is_the_ordered_sum_and_the_adjoint_of_im2col", CH + "test_conv_gelu_stages_against_float64"],
    "cm3p_bias_gelu_fwd": [CH + "test_bias_gelu_forward_against_float64", CH + "test_conv_gelu_stages_against_float64"],
    "cm3p_bias_gelu_bwd": [CH + "test_bias_gelu_backward_against_float64"],
    "cm3p_pool_fwd": [KG + "test_pooling",
                      RK + "test_pooling_against_float64"],
    "cm3p_pool_bwd": [KG + "test_pooling",
                      RK + "test_pooling_against_float64"],
    "cm3p_gemm_f32": [CH + "test_gemm_f32_all_stride_forms", KG + "test_head_kernels"],
    "cm3p_l2norm_fwd": [KG + "test_head_kernels", LH + "test_l2norm_forward_and_backward_against_float64"],
    "cm3p_l2norm_bwd": [KG + "test_head_kernels", LH + "test_l2norm_forward_and_backward_against_float64"],
    "cm3p_cross_entropy": [CH + "test_cross_entropy_with_the_specs_of_the_contrastive_loss", KG + "test_head_kernels"],
    "cm3p_scale_exp": [CH + "test_scale_exp_dot_and_sum_against_float64"],
    "cm3p_scale_by": [KG + "test_masked_lm_loss_kernels", CH + "test_cross_entropy_masked_against_float64",
                      LH + "test_scale_by_is_the_fp32_product_in_bits"],
    "cm3p_dot_f32": [CH + "test_scale_exp_dot_and_sum_against_float64"],
    "cm3p_sum_f32": [CH + "test_scale_exp_dot_and_sum_against_float64", KG + "test_masked_lm_loss_kernels",
                     LH + "test_sum_f32_against_float64", LH + "test_add_scaled_node_in_bits"],
    "cm3p_cross_entropy_masked": [CH + "test_cross_entropy_masked_against_float64", CH + "test_single_label_classifier_ignores_minus_100_rows"],
    "cm3p_inv_valid_count": [KG + "test_masked_lm_loss_kernels", LH + "test_inv_valid_count_is_the_fp32_quotient_in_bits"],
    "cm3p_ce_masked_stats": [KG + "test_masked_lm_loss_kernels",
                             LH + "test_masked_ce_stats_and_dlogits_at_every_seam", LH + "test_masked_ce_with_a_whole_row_block_ignored_into_guarded_buffers"],
    "cm3p_ce_masked_dlogits_bf16": [KG + "test_masked_lm_loss_kernels",
                                    LH + "test_masked_ce_stats_and_dlogits_at_every_seam", LH + "test_masked_ce_with_a_whole_row_block_ignored_into_guarded_buffers"],
    "cm3p_add_bias_f32": [CH + "test_add_bias_is_the_fp32_add_bit_for_bit"],
    "cm3p_colsum_f32": [CH + "test_colsum_against_float64"],
    "cm3p_pointwise_loss": [CH + "test_pointwise_loss_against_float64"],
    "cm3p_first_zero_index": [KG + "test_head_kernels", LH + "test_first_zero_index_is_the_argmax_of_the_zero_mask"],
    "cm3p_attn_fwd_varlen": [KG + "test_attention_varlen_equals_padded_on_valid_rows",
                             AD + "test_varlen_equals_padded", AF + "test_packed_equals_padded_and_matches_float64"],
    "cm3p_attn_bwd_varlen": [KG + "test_attention_varlen_equals_padded_on_valid_rows",
                             AD + "test_varlen_equals_padded", AF + "test_packed_equals_padded_and_matches_float64"],
    "cm3p_gather_rows_f32": [KG + "test_gather_scatter_rows",
                             RK + "test_gather_and_scatter_rows_bit_for_bit"],
    "cm3p_scatter_rows_f32": [KG + "test_gather_scatter_rows",
                              RK + "test_gather_and_scatter_rows_bit_for_bit"],
    "cm3p_gemm_bf16_batched": [MU + "test_batched_gemm_axpby",
                               MK + "test_one_newton_schulz_iteration_against_float64", MK + "test_six_iterations_keep_the_padding_zero_and_everything_finite"],
    "cm3p_muon_partials": [MU + "test_steps_match_the_reference_fixture", MU + "test_model_sized_group_against_the_oracle",
                           MK + "test_stage_kernels_against_their_references", MK + "test_an_all_zero_matrix_stays_zero_and_leaves_its_group_alone", MK + "test_two_steps_of_the_class_at_the_block_seams_aligned_and_not"],
    "cm3p_muon_momentum": [MU + "test_steps_match_the_reference_fixture", MU + "test_model_sized_group_against_the_oracle",
                           MK + "test_stage_kernels_against_their_references", MK + "test_float4_and_scalar_momentum_kernels_give_the_same_bits", MK + "test_an_all_zero_matrix_stays_zero_and_leaves_its_group_alone", MK + "test_two_steps_of_the_class_at_the_block_seams_aligned_and_not"],
    "cm3p_muon_normalize": [MU + "test_steps_match_the_reference_fixture", MU + "test_model_sized_group_against_the_oracle",
                            MK + "test_stage_kernels_against_their_references", MK + "test_an_all_zero_matrix_stays_zero_and_leaves_its_group_alone", MK + "test_two_steps_of_the_class_at_the_block_seams_aligned_and_not"],
    "cm3p_muon_apply": [MU + "test_steps_match_the_reference_fixture", MU + "test_model_sized_group_against_the_oracle",
                        MK + "test_stage_kernels_against_their_references", MK + "test_an_all_zero_matrix_stays_zero_and_leaves_its_group_alone", MK + "test_two_steps_of_the_class_at_the_block_seams_aligned_and_not"],
    "cm3p_adamw_multi": [MU + "test_steps_match_the_reference_fixture", MK + "test_adamw_multi_against_float64"],
    # include/cm3p_lora.h
    "cm3p_lora_merge_cast_multi": [LK + "test_merged_cast_against_float64", LK + "test_merged_cast_table_of_several_matrices",
                                   LK + "test_merged_cast_with_zero_b_is_the_plain_cast_in_bits"],
    "cm3p_lora_grad": [LK + "test_adapter_gradients_against_float64", LK + "test_adapter_gradients_over_three_row_blocks_and_pitched_rows",
                       LK + "test_adapter_gradients_with_zero_scale_are_exact_zeros"],
    # include/cm3p_attn_row.h
    "cm3p_attn_row_fwd": [AW + "test_row_kernels_against_float64", AW + "test_row_kernels_exact_conditions",
                          AW + "test_row_forward_agrees_with_row_0_of_the_full_forward"],
    "cm3p_attn_row_bwd": [AW + "test_row_kernels_against_float64", AW + "test_row_kernels_exact_conditions",
                          AW + "test_row_backward_agrees_with_the_full_backward_fed_a_one_row_dout"],
    # include/cm3p_attn_qrows.h
    "cm3p_attn_qrows_fwd": [AQ + "test_qrows_kernels_against_float64", AQ + "test_qrows_kernels_exact_conditions",
                            AQ + "test_every_row_listed_agrees_with_the_full_kernels"],
    "cm3p_attn_qrows_bwd": [AQ + "test_qrows_kernels_against_float64", AQ + "test_qrows_kernels_exact_conditions",
                            AQ + "test_backward_agrees_with_the_full_backward_fed_a_dout_that_is_zero_off_the_list"],
}

EXEMPT = {
    "cm3p_abi_version": "host query: the header's version number (tests/test_cabi.py compares it with the binding)",
    "cm3p_layernorm_bwd_blocks": "host query: workspace rows of cm3p_layernorm_bwd",
    "cm3p_embed_ln_bwd_sorted_chunk": "host query: the id-order backward's chunk size",
    "cm3p_token_order_workspace_ints": "host query: workspace size of cm3p_token_order",
    "cm3p_gemm_wgrad_splits": "host query: split-K factor the wrapper picks",
    "cm3p_gemm_route": "host query: the kernel, instance and split count a bf16 GEMM call lands on (tests/test_gemm_refs_host.py)",
    "cm3p_build_ablation_flags": "ablation hook: tests/test_cabi.py and _lib.load() require 0 from a product library",
    "cm3p_debug_set_dma_audit": "audit hook of the debug twin (tests/test_dma_audit_gpu.py)",
    "cm3p_attn_fwd_impl": "host query: which forward kernel a shape takes",
    "cm3p_attn_generic_supported": "host query: head dims the generic kernels take",
    "cm3p_attn_bwd_fused_workspace_bytes": "host query: workspace size of cm3p_attn_bwd_fused",
    "cm3p_attn_bwd_fused_slab_group": "host query: slab grouping of cm3p_attn_bwd_fused",
    "cm3p_bias_gelu_bwd_blocks": "host query: partial rows of cm3p_bias_gelu_bwd",
    "cm3p_pool_chunks": "host query: workspace size of cm3p_pool_fwd",
    "cm3p_ce_masked_dlogits_blocks": "host query: partial rows of cm3p_ce_masked_dlogits_bf16",
    "cm3p_colsum_blocks": "host query: partial rows of cm3p_colsum_f32",
    "cm3p_lora_abi_version": "host query: cm3p_lora.h's version number (tests/test_lora_host.py compares it with the binding)",
    "cm3p_lora_grad_workspace_bytes": "host query: workspace size of cm3p_lora_grad (tests/test_lora_host.py restates its formula)",
    "cm3p_lora_grad_row_block": "host query: row block of cm3p_lora_grad (tests/test_lora_host.py restates its rule)",
    "cm3p_attn_row_abi_version": "host query: cm3p_attn_row.h's version number (tests/test_attn_row_refs_host.py compares it with the binding)",
    "cm3p_attn_qrows_abi_version": "host query: cm3p_attn_qrows.h's version number (tests/test_attn_qrows_refs_host.py compares it with the binding)",
}


def _declared():
    """The same parse as tests/test_cabi.py::_declared."""
    declared = set()
    assert {os.path.basename(h) for h in HEADERS} >= {"cm3p_hip.h", "cm3p_lora.h", "cm3p_attn_row.h", "cm3p_attn_qrows.h"}
    for header in HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        found = set(re.findall(r"\b(?:int|int64_t)\s+(cm3p_[a-z0-9_]+)\s*\(", text))
        assert found, f"no entry point parsed from {header}"
        declared |= found
    return declared


def _test_functions(relpath):
    tree = ast.parse(open(os.path.join(ROOT, relpath)).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_declared_entry_point_is_in_the_ledger_or_exempt():
    declared = _declared()
    covered = set(LEDGER) | set(EXEMPT)
    assert not declared - covered, f"entry points with neither a test nor an exemption: {sorted(declared - covered)}"
    assert not covered - declared, f"ledger names no longer in a header: {sorted(covered - declared)}"
    assert {"cm3p_attn_fwd", "cm3p_lora_grad", "cm3p_attn_row_fwd", "cm3p_attn_qrows_bwd"} <= declared  # one of each header


def test_ledger_and_exempt_are_disjoint_and_nonempty():
    assert not set(LEDGER) & set(EXEMPT), sorted(set(LEDGER) & set(EXEMPT))
    assert all(LEDGER.values()) and all(r.strip() for r in EXEMPT.values())


def test_every_named_test_exists():
    cache = {}
    missing = []
    for name, ids in LEDGER.items():
        for node in ids:
            path, func = node.split("::")
            if path not in cache:
                cache[path] = _test_functions(path) if os.path.exists(os.path.join(ROOT, path)) else set()
            if func not in cache[path]:
                missing.append((name, node))
    assert not missing, missing
