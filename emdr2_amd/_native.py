"""ctypes binding of libemdr2_hip.so (C ABI: include/emdr2_mips.h, include/emdr2_assembly.h, include/emdr2_answers.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C emdr2_amd/csrc`.  If it is
missing this module raises at first use -- the product path never falls back to a CPU or eager
implementation.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libemdr2_hip.so")     # tools/ may point this at lib/libemdr2_hip_exp.so (`make exp`) before first use

EMDR2_ABI_VERSION = 4
FLAG_AMBIGUOUS = 1
FLAG_OVERFLOW = 2
MAX_TOPK = 120
AUDIT_WORDS = 16
# the report of emdr2_mips_audit, in word order (include/emdr2_mips.h); words 14 and 15 are reserved
AUDIT_NAMES = ("rows_checked", "pad_rows_nonzero", "nonfinite_rows", "rows_over_emax", "block_norm_low", "block_norm_noncanonical",
               "emax_noncanonical", "shadow_pad_rows_nonzero", "shadow_norm_low", "shadow_resid_low", "shadow_rows_noncanonical",
               "shadow_table_noncanonical", "first_bad_row", "first_bad_block")
AUDIT_SOUND_WORDS = (1, 2, 3, 4, 7, 8, 9)           # a non-zero count: a search result may be wrong (word 2 only while a shadow is in use)
AUDIT_CANONICAL_WORDS = (5, 6, 10, 11)              # a non-zero count: the image is not byte for byte a fresh build
AUDIT_NONE = (1 << 64) - 1                          # first_bad_row / first_bad_block: no offender
GEN_WORDS = 37                                      # the report of emdr2_mips_generation_stats: the five named words, then the 32 age bins
GEN_NAMES = ("count", "sum_age", "min_age", "max_age", "from_future")
GEN_MAX = (1 << 31) - 1                             # generations are below 2^31

_ERRORS = {-1: "bad argument", -2: "workspace too small", -3: "HIP launch/runtime error", -4: "unsupported shape"}

# name -> (restype, argtypes); mirrors include/emdr2_mips.h one to one
_vp, _i32, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
SIGNATURES = {
    "emdr2_abi_version": (_i32, []),
    "emdr2_device_cu_count": (_i32, []),
    "emdr2_mips_layout_bytes": (_i32, [_i64, _i32, ctypes.POINTER(_sz)]),
    "emdr2_mips_pack_rows": (_i32, [_vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp]),
    "emdr2_mips_unpack_rows": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    "emdr2_mips_gather_rows": (_i32, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _vp]),
    "emdr2_mips_export_rows": (_i32, [_vp, _i64, _i32, _i64, _i64, _vp, _vp]),
    "emdr2_mips_digest_rows": (_i32, [_vp, _i64, _i32, _i64, _i64, _i64, _vp, _vp]),
    "emdr2_mips_workspace_bytes": (_i32, [_i32, _i32, _i32, ctypes.POINTER(_sz)]),
    "emdr2_mips_search": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_exact_workspace_bytes": (_i32, [_i64, _i32, ctypes.POINTER(_sz)]),
    "emdr2_mips_search_exact": (_i32, [_vp, _i64, _i32, _i64, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_merge": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "emdr2_mips_search_f32": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_exact_workspace_bytes_f32": (_i32, [_i64, _i32, ctypes.POINTER(_sz)]),
    "emdr2_mips_search_exact_f32": (_i32, [_vp, _i64, _i32, _i64, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_merge_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "emdr2_mips_search_records": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_merge_records": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "emdr2_mips_pack_records": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "emdr2_mips_shadow_bytes": (_i32, [_i64, _i32, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "emdr2_mips_seal_shadow": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "emdr2_mips_search_shadow": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_shadow_launches": (_i32, []),
    "emdr2_mips_search_plan": (_i32, [_i64, _i32, _i32, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "emdr2_mips_block_norm_bytes": (_i32, [_i64, ctypes.POINTER(_sz)]),
    "emdr2_mips_block_norms": (_i32, [_vp, _i64, _i32, _i64, _i64, _vp, _vp]),
    "emdr2_mips_update_rows": (_i32, [_vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "emdr2_mips_scatter_workspace_bytes": (_i32, [_i64, _i64, ctypes.POINTER(_sz)]),
    "emdr2_mips_update_rows_scattered": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_update_rows_stamped": (_i32, [_vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _i32, _vp, _vp]),
    "emdr2_mips_update_rows_scattered_stamped": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, ctypes.c_uint32,
                                                         _i32, _vp, _vp]),
    "emdr2_mips_generation_stats": (_i32, [_vp, _i64, _i64, _vp, _i64, ctypes.c_uint32, _vp, _vp]),
    "emdr2_mips_oldest_rows_workspace_bytes": (_i32, [_i64, ctypes.POINTER(_sz)]),
    "emdr2_mips_oldest_rows": (_i32, [_vp, _i64, _i64, ctypes.c_uint32, _i64, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_digest_stamps": (_i32, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "emdr2_mips_row_keys": (_i32, [_vp, _i64, _i32, _i64, _i64, _i64, _vp, _vp, _vp]),
    "emdr2_mips_changed_rows_workspace_bytes": (_i32, [_i64, ctypes.POINTER(_sz)]),
    "emdr2_mips_changed_rows": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "emdr2_mips_audit": (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "emdr2_mips_debug_scores": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "emdr2_mips_set_timing": (_i32, [_i32]),
    "emdr2_mips_timing_collect": (_i32, [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_i64), _i32, ctypes.POINTER(_i32)]),
}

SIGNATURES["emdr2_assemble_evidence"] = (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32,
                                                  _vp, _vp, _vp, _vp, _vp, _vp])
# include/emdr2_answers.h: arena, doc_ids, n_b, k, ans_tokens, ans_off, q_ans_off, cont_bits, hit_pos, hit_ans, best_slot, slot_hist, stream
SIGNATURES["emdr2_answer_hits"] = (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])


_f32 = ctypes.c_float
_u32 = ctypes.c_uint32
SIGNATURES["emdr2_gemm_nt_bf16"] = (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _i64, _i64, _i64,
                                             _f32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _f32, _u32, _vp])
SIGNATURES["emdr2_gemm_tn_bf16"] = (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp])
SIGNATURES["emdr2_dropout"] = (_i32, [_vp, _vp, _i64, _i32, _f32, _u32, _vp])
SIGNATURES["emdr2_transpose_bf16"] = (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _i64, _i64, _vp, _vp])


SIGNATURES.update({
    "emdr2_layernorm_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "emdr2_layernorm_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_layernorm_bwd_mask": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _f32, _u32, _vp]),
    "emdr2_softmax_mask_fwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _f32, _u32, _vp]),
    "emdr2_softmax_mask_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _u32, _vp, _vp]),
    "emdr2_softmax_mask_t": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _u32, _vp]),
    "emdr2_gelu_bwd": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "emdr2_embedding_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _u32, _vp]),
    "emdr2_embedding_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _u32, _vp]),
    "emdr2_attention_fwd": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                   _f32, _f32, _u32, _vp, _vp, _vp]),
    "emdr2_attention_bwd": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64,
                                   _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _u32, _vp]),
    "emdr2_lse_gather_fwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_lse_gather_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_sumsq_f32": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "emdr2_adam_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _f32, _vp]),
    "emdr2_adam_step_flat": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _f32, _vp]),
    "emdr2_sumsq_census_f32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _vp]),
    "emdr2_step_verdict": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "emdr2_adam_step_flat_guarded": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _f32, _vp, _vp]),
    "emdr2_scale_cast_f32_to_bf16": (_i32, [_vp, _vp, _i64, _f32, _vp]),
    "emdr2_widen_bf16_to_f32": (_i32, [_vp, _vp, _i64, _vp]),
    "emdr2_cast_f32_to_bf16": (_i32, [_vp, _vp, _i64, _vp]),
    "emdr2_accum_bf16_to_f32": (_i32, [_vp, _vp, _i64, _f32, _vp]),
    # "State audit": master, m, v, work_bf16, n, block_keys, report, stream
    "emdr2_state_audit_ws_bytes": (_i32, [_i64, ctypes.POINTER(_sz)]),
    "emdr2_state_audit": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    # "Parameter statistics": the host-only plan (offsets, lengths, n_params, n, items, first, n_items); master, grad, m, v, n, items,
    # n_items, first, n_params, beta1, beta2, eps, step, workspace, out, stream
    "emdr2_param_stats_plan": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, ctypes.POINTER(_i64)]),
    "emdr2_param_stats_ws_bytes": (_i32, [_i64, ctypes.POINTER(_sz)]),
    "emdr2_param_stats": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32, _f32, _f32, _i32, _vp, _vp, _vp]),
})


SIGNATURES.update({
    "emdr2_seq_lengths": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "emdr2_seq_pack_ids": (_i32, [_vp, _vp, _vp, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "emdr2_gather_rows": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_scatter_rows": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_embedding_packed_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _u32, _vp]),
    "emdr2_embedding_packed_bwd": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _u32, _vp]),
    "emdr2_attention_varlen_fwd": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                          _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _u32, _vp, _vp, _vp]),
    "emdr2_attention_varlen_bwd": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64,
                                          _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _u32, _vp]),
})
SIGNATURES["emdr2_attention_splitkv_plan"] = (_i32, [_i32, _i32, _i32, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(_sz)])
SIGNATURES["emdr2_attention_fwd_splitkv"] = (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64,
                                                      _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _u32, _vp, _vp, _i32, _vp, _sz, _vp])
SIGNATURES["emdr2_attention_bwd_splitkv"] = (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                                                      _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _u32,
                                                      _i32, _vp, _sz, _vp])
# q + strides, k + strides, ids_q, ids_k, cu_k, m, l, seg, w, mass, batch, heads, sq, max_sk, n_seg, head_dim, scale, accumulate, stream
SIGNATURES["emdr2_attention_key_mass"] = (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp])
# ... seg, w, kw, kw_ld, mass, ... (the weighted form); x + strides, norm, ld, batch, sk, heads, head_dim, stream
SIGNATURES["emdr2_attention_key_mass_weighted"] = (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                                            _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp])
SIGNATURES["emdr2_head_row_norms"] = (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp])
SIGNATURES["emdr2_gemm_nt_lse_bf16"] = (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp])
SIGNATURES["emdr2_retriever_prior_fwd"] = (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp])
SIGNATURES["emdr2_retriever_prior_bwd"] = (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp])
SIGNATURES["emdr2_retriever_prior_h16_fwd"] = (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp])
SIGNATURES["emdr2_retriever_prior_h16_bwd"] = (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp])
SIGNATURES["emdr2_marginal_fwd"] = (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp])
SIGNATURES["emdr2_marginal_bwd"] = (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp])
SIGNATURES["emdr2_lse_combine"] = (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp])
# the ordered ("deterministic gradients") entries of include/emdr2_ops.h: each mirrors the entry named behind it, plus ws, ws_bytes
_psz = ctypes.POINTER(_sz)
SIGNATURES["emdr2_gemm_tn_ordered_ws_bytes"] = (_i32, [_i32, _i32, _i32, _i32, _psz])
SIGNATURES["emdr2_gemm_tn_bf16_ordered"] = (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp])     # emdr2_gemm_tn_bf16
SIGNATURES["emdr2_layernorm_bwd_ordered_ws_bytes"] = (_i32, [_i64, _i32, _psz])
SIGNATURES["emdr2_layernorm_bwd_ordered"] = (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _f32, _u32, _vp, _sz,
                                                      _vp])                                                               # emdr2_layernorm_bwd_mask
SIGNATURES["emdr2_embedding_bwd_ordered_ws_bytes"] = (_i32, [_i64, _i32, _i32, _i32, _i32, _psz])
SIGNATURES["emdr2_embedding_bwd_ordered"] = (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _u32, _vp, _sz,
                                                      _vp])                                                               # emdr2_embedding_packed_bwd
SIGNATURES["emdr2_ops_set_timing"] = (_i32, [_i32])
SIGNATURES["emdr2_ops_timing_collect"] = (_i32, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64), _i32])


# include/emdr2_ops_f32.h (ABI 4): the validation-only fp32 compute path
SIGNATURES.update({
    "emdr2_f32_gemm": (_i32, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32,
                              _vp, _vp, _i32, _vp]),
    "emdr2_f32_layernorm_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp]),
    "emdr2_f32_layernorm_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_f32_softmax_mask_fwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "emdr2_f32_softmax_mask_bwd": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "emdr2_f32_gelu_fwd": (_i32, [_vp, _vp, _i64, _vp]),
    "emdr2_f32_gelu_bwd": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "emdr2_f32_embedding_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "emdr2_f32_embedding_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "emdr2_f32_lse_gather_fwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_f32_lse_gather_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "emdr2_f32_retriever_prior_fwd": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "emdr2_f32_retriever_prior_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
})


class EvidenceArenaStruct(ctypes.Structure):
    """include/emdr2_assembly.h: emdr2_evidence_arena (device pointers)."""
    _fields_ = [("passage_tokens", _vp), ("passage_off", _vp), ("title_tokens", _vp), ("title_off", _vp),
                ("group_docs", _vp), ("group_off", _vp), ("doc_group", _vp), ("doc_pos", _vp), ("n_docs", _i64)]


_lib = None


class NativeError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raises NativeError when the library is absent."""
    global _lib
    if _lib is None:
        # torch first: PyTorch-ROCm ships its own libamdhip64; if this library were loaded before it, the dynamic linker would bind us to
        # the system HIP runtime and torch to its bundled one -- two runtimes in one process, torch's device pointers invalid in ours
        # (seen as "HIP launch/runtime error" on the first kernel when build() and smoke() ran in one interpreter).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                "libemdr2_hip.so not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C emdr2_amd/csrc`. There is no CPU fallback for the EMDR2 hot path." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)       # AttributeError here == header/library drift
            fn.restype, fn.argtypes = res, args
        if handle.emdr2_abi_version() != EMDR2_ABI_VERSION:
            raise NativeError("libemdr2_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        raise NativeError("%s failed: %s (%d)" % (what, _ERRORS.get(rc, "unknown error"), rc))


SCAN_ENGINES = ("DENSE", "LOCKSTEP", "PERSISTENT_F16", "PERSISTENT_I8")        # EMDR2_SCAN_* of include/emdr2_mips.h, in code order
PLAN_MAX_SEGMENTS = 32


def search_plan(n_rows, n_q, dim, k, shadow_min_rows=-1, cus=0):
    """emdr2_mips_search_plan: the segment schedule of one search pass of n_q <= 512 queries (csrc/mips_plan.h; host arithmetic, no GPU
    needed; cus = 0: this device's) -> ([(row_begin, row_end, engine name, select_after, prog_slot), ...], pack_q8)"""
    n, q8 = ctypes.c_int(), ctypes.c_int()
    end = (_i64 * PLAN_MAX_SEGMENTS)()
    eng, sel, slot = ((ctypes.c_int32 * PLAN_MAX_SEGMENTS)() for _ in range(3))
    check(lib().emdr2_mips_search_plan(n_rows, n_q, dim, k, shadow_min_rows, cus, PLAN_MAX_SEGMENTS, ctypes.byref(n), end, eng, sel, slot,
                                       ctypes.byref(q8)), "search_plan")
    begin = [0] + list(end[:n.value])
    return [(begin[i], end[i], SCAN_ENGINES[eng[i]], bool(sel[i]), slot[i]) for i in range(n.value)], bool(q8.value)


def stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)
