"""ctypes binding of libaudiolm_hip.so (C ABI declared in include/audiolm_hip.h).

This is the reference-side binding a maintainer would add.  There is NO fallback: if the shared
library is missing / cannot be built the import fails loudly, and every op refuses non-CUDA tensors.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_longlong, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ALM_LIB_PATH') or os.path.join(_HERE, 'libaudiolm_hip.so')      # ALM_LIB_PATH: A/B runs of an alternative build

_P, _I, _L, _F, _U = c_void_p, c_int, c_longlong, c_float, c_ulonglong

# name -> argtypes (all return int).  Kept in sync with include/audiolm_hip.h (tests/test_cabi.py checks both directions).
SIGNATURES = {
    'alm_gemm_bf16_nt': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _I, _L, _L, _L, _L, _L, _L, _F, _I, _I, _P],
    'alm_gemm_bf16_nt_ws': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _I, _L, _L, _L, _L, _L, _L, _F, _I, _I, _P, _L, _P],
    'alm_gemm_bf16_nt_inl': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _F, _I, _I, _I, _P, _L, _P],
    'alm_gemm_nt_plan': [_I, _I, _I, _I, _I, _P],
    'alm_gemm_nt_ws_bytes': [],
    'alm_gemm_splitk_slices': [_I, _I, _I, _I],
    'alm_gemm_splitk_ws_floats': [_I, _I, _I, _I],
    'alm_gemm_splitk_tile': [_I, _I, _I, _I],
    'alm_gemm_nt_tile_choice': [_I, _I, _I],
    'alm_gemm_tn_batched_plan': [_I, _I, _I, _I, _P],
    'alm_gemm_bf16_nt_splitk': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _L, _L, _L, _F, _I, _P],
    'alm_gemm_bf16_tn_splitk': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _L, _L, _L, _F, _I, _P],
    'alm_gemm_bf16_tn_batched': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _I, _L, _L, _L, _L, _L, _L, _F, _I, _P],
    'alm_gemm_bf16_tn_batched_panels': [_P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _I, _L, _L, _L, _L, _L, _L, _F, _I, _P, _P],
    'alm_gemm_bf16_tn_grouped': [_P, _I, _P, _I, _P],
    'alm_gemm_tn_grouped_plan': [_P, _I, _I, _P],
    'alm_gemm_tn_grouped_ws_floats': [_P, _I, _I],
    'alm_gemm_bf16_nt_group2': [_P, _P, _P, _I, _I, _I, _L, _L, _L, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _P],
    'alm_gemm_bf16_nt_tile': [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _F, _I, _I, _I, _P],
    'alm_transpose_bf16': [_P, _P, _I, _I, _L, _L, _I, _P],
    'alm_transpose_bf16_batched': [_P, _P, _I, _I, _L, _L, _I, _I, _L, _L, _P],
    'alm_pack_weights_multi': [_P, _I, _P],
    'alm_pack_weight': [_P, _I, _I, _L, _P, _L, _I, _I, _P, _L, _P],
    'alm_ln_partial_blocks': [_I],
    'alm_layernorm_fwd': [_P, _I, _L, _P, _P, _I, _L, _P, _L, _P, _P, _I, _I, _P],
    'alm_layernorm_bwd': [_P, _I, _L, _P, _I, _L, _P, _P, _P, _P, _L, _P, _I, _L, _P, _I, _I, _P],
    'alm_colsum': [_P, _I, _L, _I, _I, _P, _F, _I, _P, _P],
    'alm_colsum_chunks': [_I],
    'alm_colsum_partial': [_P, _L, _I, _I, _P, _P],
    'alm_geglu_fwd': [_P, _P, _L, _I, _P],
    'alm_geglu_bwd': [_P, _P, _P, _L, _I, _P],
    'alm_geglu_partial_blocks': [_I],
    'alm_geglu_ln_fwd': [_P, _L, _I, _P, _P, _L, _P, _P, _I, _I, _I, _P],
    'alm_geglu_ln_bwd': [_P, _L, _P, _L, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    'alm_mqa_attn_fwd': [_P, _L, _P, _L, _P, _L, _P, _P, _L, _P, _I, _I, _I, _I, _F, _F, _U, _P, _P],
    'alm_mqa_attn_bwd': [_P, _L, _P, _L, _P, _L, _P, _P, _L, _P, _P, _L, _P, _L, _P, _P, _L, _L, _P, _I, _I, _I, _I, _F, _F, _U, _P, _P],
    'alm_mqa_attn_bias_fwd': [_P, _L, _P, _L, _P, _L, _P, _P, _L, _P, _I, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _F, _U, _P, _P],
    'alm_mqa_attn_bias_bwd': [_P, _L, _P, _L, _P, _L, _P, _P, _L, _P, _P, _L, _P, _L, _P, _P, _L, _L, _P, _I, _I, _I, _I, _F,
                              _P, _I, _P, _P, _P, _P, _P, _F, _U, _P, _P],
    'alm_attn_bias_part_rows': [_I, _I, _I],
    'alm_attn_bias_grad_reduce': [_P, _P, _I, _I, _I, _I, _F, _P],
    'alm_posmlp_in_fwd': [_P, _P, _P, _P, _P, _I, _I, _I, _P],
    'alm_posmlp_in_bwd_chunks': [_I],
    'alm_posmlp_in_bwd': [_P, _P, _P, _I, _I, _I, _P],
    'alm_silu_fwd': [_P, _P, _L, _P],
    'alm_silu_bwd': [_P, _P, _P, _L, _P],
    'alm_posmlp_out_fwd': [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    'alm_posmlp_out_bwd': [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    'alm_xattn_softmax_fwd': [_P, _L, _P, _P, _F, _P, _L, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    'alm_xattn_dbias': [_P, _L, _P, _L, _P, _P, _L, _I, _I, _I, _I, _P],
    'alm_xattn_combine': [_P, _L, _P, _P, _P, _L, _L, _I, _I, _P],
    'alm_xattn_softmax_bwd': [_P, _L, _P, _L, _P, _F, _P, _L, _I, _I, _I, _I, _P],
    'alm_xattn_delta': [_P, _L, _P, _L, _P, _I, _I, _I, _I, _P],
    'alm_value_residual_mix': [_P, _L, _P, _L, _P, _L, _L, _I, _P],
    'alm_kv_grad_pack': [_P, _P, _L, _I, _L, _P, _P, _L, _L, _I, _I, _P],
    'alm_forgetful_mask': [_P, _L, _P, _L, _I, _I, _I, _P],
    'alm_coarse_prepare': [_P, _L, _P, _L, _I, _I, _I, _L, _L, _L, _I, _I, _P, _P, _P, _P, _I, _P],
    'alm_semantic_prepare': [_P, _L, _I, _I, _L, _L, _P, _P, _I, _P],
    'alm_unique_consecutive_i64': [_P, _L, _I, _I, _I, _L, _L, _P, _L, _P, _P],
    'alm_fine_prepare': [_P, _L, _P, _L, _I, _I, _I, _L, _L, _I, _I, _I, _P, _P, _P],
    'alm_loss_combine': [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _L, _F, _F, _F, _F, _I, _L, _P, _P, _P],
    'alm_mqa_head_groups': [_I],
    'alm_mqa_bwd_parts': [_I, _I, _I],
    'alm_hc_coef_width': [_I],
    'alm_hc_partial_width': [_I, _I],
    'alm_hc_grads_width': [_I, _I],
    'alm_hc_partial_rows': [_I, _I, _I, _I, _L, _I],
    'alm_hc_fwd_prefetch': [_I, _I, _I],
    'alm_hc_bwd_variant': [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _L, _I],
    'alm_hc_fwd': [_P, _I, _I, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'alm_hc_bwd': [_P, _I, _I, _P, _L, _P, _L, _P, _L, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _L, _P, _P, _L, _P, _I, _I, _I, _I, _I, _P],
    'alm_hc_param_grads': [_P, _I, _P, _P, _P, _P, _I, _I, _P],
    'alm_hc_param_grads_batched': [_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P],
    'alm_streams_expand': [_P, _P, _I, _I, _L, _P],
    'alm_streams_reduce': [_P, _P, _I, _I, _L, _P],
    'alm_residual_add': [_P, _P, _L, _P, _L, _I, _P],
    'alm_f32_to_bf16': [_P, _P, _P, _L, _L, _I, _P],
    'alm_add_f32': [_P, _P, _P, _L, _F, _P],
    'alm_embed_assemble': [_P, _P, _I, _P, _P, _P, _L, _I, _P, _P],
    'alm_embed_scatter_add': [_P, _P, _I, _P, _P, _P, _F, _L, _I, _P],
    'alm_embed_scatter_ws_floats': [_P, _I, _L, _I],
    'alm_embed_scatter_owned': [_P, _P, _I, _P, _P, _P, _F, _L, _I, _P, _P],
    'alm_gather_split_bf16': [_P, _L, _L, _P, _P, _P, _L, _L, _I, _P],
    'alm_gather_rows_bf16': [_P, _L, _P, _P, _L, _L, _I, _P],
    'alm_scatter_rows_bf16': [_P, _L, _P, _P, _L, _L, _I, _P],
    'alm_cross_entropy_fwd': [_P, _L, _P, _P, _P, _L, _I, _I, _P],
    'alm_cross_entropy_bwd': [_P, _L, _P, _P, _P, _P, _L, _L, _I, _I, _I, _P],
    'alm_reduce_sum': [_P, _L, _P, _F, _P],
    'alm_mqa_decode_attn': [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _I, _I, _F, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    'alm_opt_chunk_elems': [],
    'alm_opt_grad_sumsq': [_P, _I, _P, _I, _P, _P],
    'alm_opt_adam_step': [_P, _I, _P, _I, _F, _F, _F, _F, _I, _I, _P, _F, _P],
    'alm_opt_adam_pack_step': [_P, _I, _F, _F, _F, _F, _I, _I, _P, _F, _P],
    'alm_conv1d_packed_floats': [_I, _I, _I],
    'alm_conv1d_pack': [_P, _P, _I, _I, _I, _P],
    'alm_conv1d_causal': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_resunit_causal': [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'alm_phase_interleave': [_P, _P, _I, _I, _I, _I, _P],
    'alm_rvq_decode': [_P, _L, _P, _P, _L, _I, _I, _I, _I, _P],
    'alm_rvq_padded_codes': [_I],
    'alm_rvq_padded_dim': [_I],
    'alm_rvq_pack': [_P, _P, _P, _I, _I, _I, _P],
    'alm_rvq_encode': [_P, _L, _P, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _P],
    'alm_bct_to_btc': [_P, _P, _I, _I, _I, _P],
    'alm_rvq_code_stats_chunk': [],
    'alm_rvq_code_stats_ws_floats': [_I, _I, _I],
    'alm_rvq_code_stats': [_P, _L, _P, _L, _P, _P, _P, _L, _I, _I, _I, _P],
    'alm_rvq_train_quantize_blocks': [_I],
    'alm_rvq_train_quantize': [_P, _L, _P, _L, _P, _P, _L, _P, _P, _F, _I, _I, _I, _I, _P],
    'alm_rvq_ema_update': [_P, _P, _P, _P, _P, _F, _F, _F, _P, _P, _I, _I, _P],
    'alm_rvq_expire': [_P, _I, _P, _P, _L, _P, _L, _P, _I, _I, _F, _P, _P, _P, _I, _I, _I, _P],
    'alm_rvq_kmeans_update': [_P, _P, _P, _P, _P, _P, _I, _I, _P],
    'alm_rvq_train_bwd': [_P, _L, _P, _L, _P, _P, _L, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    'alm_conv1d_wgrad_chunk': [_I, _I],
    'alm_conv1d_wgrad_ws_floats': [_I, _I, _I, _I, _I],
    'alm_conv1d_dgrad': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_conv1d_wgrad': [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_phase_deinterleave': [_P, _P, _I, _I, _I, _I, _P],
    'alm_resample_sinc': [_P, _L, _P, _L, _P, _I, _L, _L, _L, _I, _I, _I, _P],
    'alm_resample_sinc_bwd': [_P, _L, _P, _L, _P, _I, _L, _L, _L, _I, _I, _I, _P],
    'alm_hubert_conv0_chunks': [_L],
    'alm_hubert_conv0_stats': [_P, _L, _P, _P, _P, _I, _I, _L, _L, _I, _I, _F, _P],
    'alm_hubert_conv0_apply': [_P, _L, _P, _P, _P, _P, _P, _I, _I, _L, _L, _I, _I, _P],
    'alm_conv1d_valid': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_layernorm_bct_split': [_P, _P, _P, _P, _I, _I, _I, _F, _P],
    'alm_mha_attn_fwd': [_P, _P, _I, _I, _I, _I, _F, _P],
    'alm_vqw2v_group_chunks': [_I, _I, _I],
    'alm_vqw2v_group_stats': [_P, _P, _P, _I, _I, _I, _I, _F, _P],
    'alm_vqw2v_group_apply': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P],
    'alm_vqw2v_group_apply_t': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    'alm_vqw2v_conv0_stats': [_P, _L, _P, _P, _P, _I, _I, _L, _L, _I, _I, _F, _P],
    'alm_vqw2v_conv0_apply': [_P, _L, _P, _P, _P, _P, _P, _I, _I, _L, _L, _I, _I, _I, _P],
    'alm_t5_embed':[_P, _P, _P, _I, _I, _L, _P, _P],
    'alm_t5_rmsnorm': [_P, _P, _P, _P, _I, _I, _F, _I, _P],
    'alm_t5_gate': [_P, _P, _L, _L, _I, _P],
    'alm_t5_attn_fwd': [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    'alm_layernorm_bct': [_P, _P, _P, _P, _I, _I, _I, _F, _P],
    'alm_geglu_bct': [_P, _P, _I, _I, _I, _P],
    'alm_local_attn': [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    'alm_local_attn_bwd_supported': [_I, _I],
    'alm_local_attn_bwd_ws_floats': [_I, _I, _I, _I, _I],
    'alm_local_attn_bwd': [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _F, _P],
    'alm_layernorm_bct_bwd_ws_floats': [_I, _I],
    'alm_layernorm_bct_bwd': [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    'alm_geglu_bct_bwd': [_P, _P, _P, _I, _I, _I, _P],
    'alm_conv1d_causal_pre': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_lstm_launches': [_I, _I],
    'alm_lstm_seq': [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    'alm_gconv1d_out_len': [_I, _I, _I, _I],
    'alm_gconv1d_fwd': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_gconv1d_dgrad': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_gconv1d_fwd_masked': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_gconv1d_wgrad_ws_floats': [_I, _I, _I, _I, _I, _I, _I, _I],
    'alm_gconv1d_wgrad': [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_avgpool1d_out_len': [_I, _I],
    'alm_avgpool1d_fwd': [_P, _P, _L, _I, _I, _P],
    'alm_avgpool1d_bwd': [_P, _P, _L, _I, _I, _P],
    'alm_loss_ws_floats': [],
    'alm_loss_mean_fwd': [_P, _P, _P, _P, _L, _I, _P],
    'alm_loss_mean_bwd': [_P, _P, _P, _P, _P, _L, _I, _P],
    'alm_grad_penalty_ws_floats': [_I, _L],
    'alm_grad_penalty_fwd': [_P, _P, _P, _P, _L, _I, _L, _F, _F, _P],
    'alm_grad_penalty_bwd': [_P, _P, _P, _P, _I, _L, _F, _F, _P],
    'alm_stft_frames': [_I, _I, _I],
    'alm_stft_fwd': [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    'alm_stft_bwd_ws_floats': [_I, _I, _I, _I],
    'alm_stft_bwd': [_P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    'alm_cconv2d_out_hw': [_I, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    'alm_cconv2d_fwd': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_cconv2d_dgrad': [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_cconv2d_wgrad_ws_floats': [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I],
    'alm_cconv2d_wgrad': [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_modrelu_ws_floats': [],
    'alm_modrelu_fwd': [_P, _P, _P, _L, _P],
    'alm_modrelu_bwd': [_P, _P, _P, _P, _P, _P, _L, _P],
    'alm_cabs_fwd': [_P, _P, _L, _P],
    'alm_cabs_bwd': [_P, _P, _P, _L, _P],
    'alm_modrelu_bwd2': [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    'alm_cabs_bwd2': [_P, _P, _P, _P, _P, _L, _P],
    'alm_mel_power_fwd': [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'alm_mel_project_fwd': [_P, _P, _P, _I, _I, _I, _I, _P],
    'alm_mel_loss_ws_floats': [],
    'alm_mel_frame_loss_fwd': [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P],
    'alm_mel_frame_loss_bwd': [_P, _P, _P, _P, _I, _I, _I, _F, _P],
    'alm_mel_power_bwd': [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    'alm_se_gate_supported': [_I, _I],
    'alm_se_gate_fwd': [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    'alm_se_gate_bwd_ws_floats': [_I, _I, _I, _I],
    'alm_se_gate_bwd': [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    'alm_film_fwd': [_P, _P, _P, _P, _I, _I, _F, _F, _P],
    'alm_film_bwd_ws_floats': [_I, _I],
    'alm_film_bwd': [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _F, _F, _P],
    'alm_fsq_consts_floats': [_I],
    'alm_fsq_fwd': [_P, _L, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P, _I, _I, _I, _I, _I, _P],
    'alm_fsq_decode': [_P, _L, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    'alm_fsq_bwd_ws_floats': [_I, _I, _I],
    'alm_fsq_bwd': [_P, _L, _P, _L, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    'alm_lfq_fwd_ws_doubles': [_I, _I, _I],
    'alm_lfq_fwd': [_P, _L, _P, _P, _P, _P, _P, _L, _P, _L, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _F, _F, _F, _F, _P],
    'alm_lfq_decode': [_P, _L, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    'alm_lfq_bwd_ws_floats': [_I, _I, _I, _I],
    'alm_lfq_bwd': [_P, _L, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _F, _F, _F, _F, _P],
    'alm_gate_loop_chunk': [],
    'alm_gate_loop_norm_fwd': [_P, _P, _P, _I, _I, _I, _P],
    'alm_gate_loop_scan_ws_floats': [_I, _I, _I],
    'alm_gate_loop_scan_fwd': [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    'alm_gate_loop_scan_bwd': [_P, _P, _P, _P, _P, _L, _I, _I, _I, _P],
    'alm_gate_loop_norm_bwd_ws_floats': [_I, _I, _I],
    'alm_gate_loop_norm_bwd': [_P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P],
    'alm_memset_zero': [_P, _L, _P],
    'alm_list_op_id': [ctypes.c_char_p],
    'alm_list_op_nargs': [_I],
    'alm_list_run': [_P, _I, _P, _P, _I, _P, _I, _P, _P],
}

_lib = None


class AlmError(RuntimeError):
    pass


def load(build_if_missing: bool = True):
    """Loads (building in-tree with hipcc if necessary) the shared library.  Raises if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and not os.environ.get('ALM_LIB_PATH'):
        from . import build as _build
        try:
            _build.build(verbose=False)
        except Exception as e:  # no hipcc on the box: fine as long as the prebuilt .so that travelled with the tree matches the sources
            if not os.path.exists(LIB_PATH):
                raise ImportError(f'libaudiolm_hip.so is missing and could not be built: {e}') from e
            if not _build._fresh(_build._digest()):
                raise ImportError(f'libaudiolm_hip.so is stale (csrc/ or include/ changed since it was built) and could not be rebuilt: {e}') from e
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"`')
    # torch FIRST: its wheel bundles its own libamdhip64 / libhsa-runtime64, and whichever copy enters the process first serves both torch
    # and this library (same SONAME).  Loaded the other way round, torch ends up on the system runtime it was not built against and every
    # launch fails with hipErrorNoDevice (seen on MI355X when the package was imported before torch).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError(f'{LIB_PATH} does not export {name} (declared in include/audiolm_hip.h): stale or foreign library')
        fn.argtypes = argtypes
        fn.restype = c_int
    _lib = lib
    return lib


class AlmOptTensor(ctypes.Structure):
    """mirror of AlmOptTensor in include/audiolm_hip.h"""
    _fields_ = [('p', c_void_p), ('g', c_void_p), ('m', c_void_p), ('v', c_void_p), ('n', c_longlong), ('wd', c_float), ('step', c_int)]


class AlmOptPackJob(ctypes.Structure):
    """mirror of AlmOptPackJob in include/audiolm_hip.h"""
    _fields_ = [('p', c_void_p), ('g', c_void_p), ('m', c_void_p), ('v', c_void_p), ('rows', c_int), ('cols', c_int), ('ld', c_longlong),
                ('dst', c_void_p), ('ld_dst', c_longlong), ('rows_pad', c_int), ('cols_pad', c_int), ('dstT', c_void_p), ('ld_dstT', c_longlong),
                ('wd', c_float), ('step', c_int)]


class AlmListEntry(ctypes.Structure):
    """mirror of AlmListEntry in include/audiolm_hip.h"""
    _fields_ = [('op', c_int), ('nargs', c_int), ('first', c_int), ('reserved', c_int)]


class AlmPackJob(ctypes.Structure):
    """mirror of AlmPackJob in include/audiolm_hip.h"""
    _fields_ = [('src', c_void_p), ('rows', c_int), ('cols', c_int), ('ld_src', c_longlong), ('dst', c_void_p), ('ld_dst', c_longlong),
                ('rows_pad', c_int), ('cols_pad', c_int), ('dstT', c_void_p), ('ld_dstT', c_longlong)]


class AlmTnJob(ctypes.Structure):
    """mirror of AlmTnJob in include/audiolm_hip.h (16 eight-byte words; the launch-list recorder relocates the c_void_p ones)"""
    _fields_ = [('At', c_void_p), ('Bt', c_void_p), ('C', c_void_p), ('M', c_int), ('N', c_int), ('K', c_int), ('nb1', c_int), ('nb2', c_int),
                ('accumulate', c_int), ('alpha', c_float), ('reserved', c_int), ('lda', c_longlong), ('ldb', c_longlong), ('ldc', c_longlong),
                ('sA1', c_longlong), ('sA2', c_longlong), ('sB1', c_longlong), ('sB2', c_longlong), ('sC1', c_longlong), ('sC2', c_longlong)]


_BOUND = {}          # name -> bound ctypes function (one dict lookup per call instead of load() + getattr on the CDLL: ~150 calls per training step)
RECORDER = None      # launchlist.Recorder while a stack pass is being recorded (the launches still run: recording is an ordinary step that is also written down)


def call(name: str, *args):
    fn = _BOUND.get(name)
    if fn is None:
        fn = _BOUND[name] = getattr(load(), name)
    if RECORDER is not None:
        RECORDER.note(name, args)
    rc = fn(*args)
    if rc != 0:
        raise AlmError(f'{name} failed with code {rc}' + (' (ALM_ERR_BAD_ARG)' if rc == 10001 else ' (ALM_ERR_UNSUPPORTED)' if rc == 10002 else ' (hipError_t)'))
    return rc


def query(name: str, *args) -> int:
    """For the int-returning size queries (alm_*_blocks / alm_*_width)."""
    fn = _BOUND.get(name)
    if fn is None:
        fn = _BOUND[name] = getattr(load(), name)
    return fn(*args)
