"""ctypes binding of the C ABI in include/flash_attn_gfx950.h (libflash_attn_gfx950.so).

This is the binding a non-PyTorch host (or the reference's maintainers)
would write: plain device pointers and sizes, a stream handle, integer status codes.  The
PyTorch host module (`_C`) is built on the same entry points in C++; this module exists so
tests and bench.py can drive and time the C ABI directly.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))


def _first_existing(*candidates):
    return next((c for c in candidates if os.path.exists(c)), candidates[-1])


# installed package (setup.py ships library and header inside it) first, then the in-tree build
LIBRARY_PATH = _first_existing(os.path.join(_HERE, "libflash_attn_gfx950.so"), os.path.join(os.path.dirname(_HERE), "csrc", "libflash_attn_gfx950.so"))
# development aid (tools/ only: A/B and error-distribution scripts drive a variant build through this binding); the host module `_C` links the product library
if os.environ.get("FA_GFX950_LIBRARY"):
    LIBRARY_PATH = os.path.abspath(os.environ["FA_GFX950_LIBRARY"])
HEADER_PATH = _first_existing(os.path.join(_HERE, "include", "flash_attn_gfx950.h"),
                              os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "flash_attn_gfx950.h"))

FA_FP16, FA_BF16 = 0, 1
FA_OK = 0
FA_ERR_NULL_POINTER, FA_ERR_BAD_SHAPE, FA_ERR_BAD_GQA, FA_ERR_BAD_HEADDIM, FA_ERR_BAD_DTYPE, FA_ERR_BAD_STRIDE = -1, -2, -3, -4, -5, -6
FA_ERR_BAD_ABI = -8
FA_PARAMS_MAGIC = 0xFA950A71      # include/flash_attn_gfx950.h

_vp, _i32, _fp = ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p


class Strides(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int64), ("row", ctypes.c_int64), ("head", ctypes.c_int64)]


class _Params(ctypes.Structure):
    """ABI 4: every params struct starts with {struct_size, magic}; the constructor fills them like FA_PARAMS_INIT"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size, self.magic = ctypes.sizeof(type(self)), FA_PARAMS_MAGIC


class FwdParams(_Params):
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("k", _vp), ("v", _vp), ("o", _vp), ("lse", _vp),
                ("cu_seqlens_q", _vp), ("cu_seqlens_k", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_k", _i32), ("h", _i32), ("h_k", _i32), ("d", _i32),
                ("dtype", _i32), ("is_causal", _i32),
                ("q_stride", Strides), ("k_stride", Strides), ("v_stride", Strides), ("o_stride", Strides),
                ("total_q", ctypes.c_int64), ("total_k", ctypes.c_int64)]      # ABI 2, optional (0 = unknown)


class BwdParams(_Params):
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("k", _vp), ("v", _vp), ("o", _vp), ("dout", _vp), ("lse", _vp),
                ("dq", _vp), ("dk", _vp), ("dv", _vp), ("dsoftmax_sum", _vp),
                ("cu_seqlens_q", _vp), ("cu_seqlens_k", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_k", _i32), ("h", _i32), ("h_k", _i32), ("d", _i32),
                ("dtype", _i32), ("is_causal", _i32),
                ("q_stride", Strides), ("k_stride", Strides), ("v_stride", Strides), ("o_stride", Strides),
                ("do_stride", Strides), ("dq_stride", Strides), ("dk_stride", Strides), ("dv_stride", Strides),
                ("total_q", ctypes.c_int64), ("total_k", ctypes.c_int64),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_int64)]


class KvcacheParams(_Params):
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("k_cache", _vp), ("v_cache", _vp), ("k_new", _vp), ("v_new", _vp),
                ("o", _vp), ("lse", _vp), ("cache_seqlens", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_cache", _i32), ("seqlen_new", _i32), ("h", _i32), ("h_k", _i32), ("d", _i32),
                ("dtype", _i32), ("is_causal", _i32), ("num_splits", _i32),
                ("q_stride", Strides), ("k_cache_stride", Strides), ("v_cache_stride", Strides), ("k_new_stride", Strides), ("v_new_stride", Strides),
                ("o_stride", Strides),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_int64),
                ("block_table", _vp), ("block_table_stride", ctypes.c_int64), ("page_block_size", _i32), ("num_blocks", _i32)]


class KvcacheOptions(_Params):
    """fa_kvcache_options: options of a decode call beyond fa_kvcache_params (the _ex entry points); zeroed = none"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("is_local", _i32), ("window_size_left", _i32),
                ("window_size_right", _i32)]


class KvcacheOptionsV2(_Params):
    """fa_kvcache_options_v2: fa_kvcache_options plus the 8-bit cache fields (passed to the _ex entry points through the same pointer)"""
    _fields_ = KvcacheOptions._fields_ + [("cache_dtype", _i32), ("k_descale", _vp), ("v_descale", _vp),
                                          ("k_descale_batch_stride", ctypes.c_int64), ("k_descale_head_stride", ctypes.c_int64),
                                          ("v_descale_batch_stride", ctypes.c_int64), ("v_descale_head_stride", ctypes.c_int64)]


class KvcacheOptionsV3(_Params):
    """fa_kvcache_options_v3: fa_kvcache_options_v2 plus the rotary embedding fields (same pointer, told apart by struct_size)"""
    _fields_ = KvcacheOptionsV2._fields_ + [("rotary_cos", _vp), ("rotary_sin", _vp), ("rotary_row_stride", ctypes.c_int64), ("seqlen_ro", _i32),
                                            ("rotary_dim", _i32), ("rotary_interleaved", _i32), ("reserved_", _i32)]


class KvcacheOptionsV4(_Params):
    """fa_kvcache_options_v4: fa_kvcache_options_v3 plus the ragged-batch fields (same pointer, told apart by struct_size)"""
    _fields_ = KvcacheOptionsV3._fields_ + [("cu_seqlens_q", _vp), ("cu_seqlens_k_new", _vp), ("total_q", ctypes.c_int64), ("total_k_new", ctypes.c_int64)]


class KvcacheOptionsV5(_Params):
    """fa_kvcache_options_v5: fa_kvcache_options_v4 plus softmax_scale / softcap and two reserved words (same pointer, told apart by struct_size)"""
    _fields_ = KvcacheOptionsV4._fields_ + [("softmax_scale", ctypes.c_float), ("softcap", ctypes.c_float), ("reserved", ctypes.c_int64 * 2)]


class KvcacheOptionsV6(_Params):
    """fa_kvcache_options_v6: fa_kvcache_options_v5 plus the attention sinks - a float32 device pointer, its element stride - and two reserved words"""
    _fields_ = KvcacheOptionsV5._fields_ + [("sinks", _vp), ("sinks_stride", ctypes.c_int64), ("reserved2", ctypes.c_int64 * 2)]


class KvcacheOptionsV7(_Params):
    """fa_kvcache_options_v7: fa_kvcache_options_v6 plus the tree mask - an int64 device pointer, its batch and row strides in elements - and two reserved words"""
    _fields_ = KvcacheOptionsV6._fields_ + [("tree_mask", _vp), ("tree_mask_batch_stride", ctypes.c_int64), ("tree_mask_row_stride", ctypes.c_int64),
                                            ("reserved3", ctypes.c_int64 * 2)]


class KvcacheOptionsV8(_Params):
    """fa_kvcache_options_v8: fa_kvcache_options_v7 plus row_tile (0 = the 16-row kernels, 64 = the 64-row kernels for prompt chunks) and six reserved words"""
    _fields_ = KvcacheOptionsV7._fields_ + [("row_tile", _i32), ("reserved4_", _i32), ("reserved4", ctypes.c_int64 * 5)]


class MlaParams(_Params):
    """fa_mla_params: MLA decode over a latent KV cache (fa_run_mla_fwd_kvcache)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("kv_cache", _vp), ("kv_new", _vp), ("o", _vp), ("lse", _vp),
                ("cache_seqlens", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_cache", _i32), ("seqlen_new", _i32), ("h", _i32), ("d_qk", _i32), ("d_v", _i32),
                ("dtype", _i32), ("is_causal", _i32), ("num_splits", _i32), ("softmax_scale", ctypes.c_float), ("reserved_", _i32),
                ("q_stride", Strides), ("kv_cache_stride", Strides), ("kv_new_stride", Strides), ("o_stride", Strides),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_int64),
                ("block_table", _vp), ("block_table_stride", ctypes.c_int64), ("page_block_size", _i32), ("num_blocks", _i32)]


class MlaSparseParams(_Params):
    """fa_mla_sparse_params: sparse MLA decode over a latent KV cache (fa_run_mla_sparse_fwd_kvcache)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("kv_cache", _vp), ("o", _vp), ("lse", _vp),
                ("cache_seqlens", _vp), ("indices", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_cache", _i32), ("topk", _i32), ("h", _i32), ("d_qk", _i32), ("d_v", _i32),
                ("dtype", _i32), ("num_splits", _i32), ("softmax_scale", ctypes.c_float), ("reserved_", ctypes.c_int64),
                ("q_stride", Strides), ("kv_cache_stride", Strides), ("o_stride", Strides),
                ("indices_batch_stride", ctypes.c_int64), ("indices_row_stride", ctypes.c_int64),
                ("workspace", _vp), ("workspace_bytes", ctypes.c_int64),
                ("block_table", _vp), ("block_table_stride", ctypes.c_int64), ("page_block_size", _i32), ("num_blocks", _i32)]


class MlaParamsV2(_Params):
    """fa_mla_params_v2: fa_mla_params plus kv_format (same pointer, told apart by struct_size)"""
    _fields_ = MlaParams._fields_ + [("kv_format", _i32), ("reserved2_", _i32)]


class MlaSparseParamsV2(_Params):
    """fa_mla_sparse_params_v2: fa_mla_sparse_params plus kv_format (same pointer, told apart by struct_size)"""
    _fields_ = MlaSparseParams._fields_ + [("kv_format", _i32), ("reserved2_", _i32)]


class MlaIndexerParams(_Params):
    """fa_mla_indexer_params: index logits of the DeepSeek-V3.2 indexer (fa_run_mla_indexer_logits)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q_idx", _vp), ("weights", _vp), ("k_idx_cache", _vp), ("k_scale", _vp), ("logits", _vp),
                ("cache_seqlens", _vp), ("block_table", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_cache", _i32), ("h", _i32), ("d", _i32), ("dtype", _i32), ("k_format", _i32), ("is_causal", _i32),
                ("page_block_size", _i32), ("num_blocks", _i32), ("reserved_", ctypes.c_int64),
                ("q_idx_stride", Strides), ("weights_stride", Strides),
                ("k_cache_batch_stride", ctypes.c_int64), ("k_cache_row_stride", ctypes.c_int64), ("k_scale_batch_stride", ctypes.c_int64),
                ("k_scale_row_stride", ctypes.c_int64), ("logits_batch_stride", ctypes.c_int64), ("logits_row_stride", ctypes.c_int64),
                ("block_table_stride", ctypes.c_int64)]


class MlaIndexerParamsV2(_Params):
    """fa_mla_indexer_params_v2: fa_mla_indexer_params plus q_format (the *_v2 entry points; run_mla_indexer_logits and its kin pick them by the class)"""
    _fields_ = MlaIndexerParams._fields_ + [("q_format", _i32), ("reserved2_", _i32)]


class MlaTopkParams(_Params):
    """fa_mla_topk_params: the top-k selection over index logits (fa_run_mla_indexer_topk)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("logits", _vp), ("indices", _vp), ("cache_seqlens", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_cache", _i32), ("topk", _i32), ("is_causal", _i32), ("reserved_", _i32),
                ("logits_batch_stride", ctypes.c_int64), ("logits_row_stride", ctypes.c_int64)]


class MlaPrefillParams(_Params):
    """fa_mla_prefill_params: MLA prefill attention, 192-wide q / k and 128-wide v, dense or packed (fa_run_mla_prefill_fwd)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("k", _vp), ("v", _vp), ("o", _vp), ("lse", _vp),
                ("cu_seqlens_q", _vp), ("cu_seqlens_k", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_k", _i32), ("h", _i32), ("h_k", _i32), ("d_qk", _i32), ("d_v", _i32),
                ("dtype", _i32), ("is_causal", _i32), ("softmax_scale", ctypes.c_float),
                ("q_stride", Strides), ("k_stride", Strides), ("v_stride", Strides), ("o_stride", Strides),
                ("total_q", ctypes.c_int64), ("total_k", ctypes.c_int64)]


class MlaPrefillBwdParams(_Params):
    """fa_mla_prefill_bwd_params: the backward of MLA prefill attention, dq / dk / dv from dout, q, k, v, o, lse (fa_run_mla_prefill_bwd)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("q", _vp), ("k", _vp), ("v", _vp), ("o", _vp), ("lse", _vp), ("dout", _vp),
                ("dq", _vp), ("dk", _vp), ("dv", _vp), ("dsoftmax_sum", _vp), ("cu_seqlens_q", _vp), ("cu_seqlens_k", _vp),
                ("b", _i32), ("seqlen_q", _i32), ("seqlen_k", _i32), ("h", _i32), ("h_k", _i32), ("d_qk", _i32), ("d_v", _i32),
                ("dtype", _i32), ("is_causal", _i32), ("softmax_scale", ctypes.c_float), ("phases", _i32), ("reserved_", _i32),
                ("q_stride", Strides), ("k_stride", Strides), ("v_stride", Strides), ("o_stride", Strides), ("dout_stride", Strides),
                ("dq_stride", Strides), ("dk_stride", Strides), ("dv_stride", Strides),
                ("total_q", ctypes.c_int64), ("total_k", ctypes.c_int64)]


FA_MERGE_MAX_PARTS = 8


class LseStrides(ctypes.Structure):
    """fa_lse_strides: the (batch, head, row) strides of an fp32 LSE, in elements"""
    _fields_ = [("batch", ctypes.c_int64), ("head", ctypes.c_int64), ("row", ctypes.c_int64)]


class MergeParams(_Params):
    """fa_merge_params: n_parts partial attention states (o_i, lse_i) of the same query rows into one (fa_run_merge_states)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("dtype", _i32), ("n_parts", _i32), ("b", _i32), ("rows", _i32), ("h", _i32), ("d_v", _i32),
                ("o", _vp * FA_MERGE_MAX_PARTS), ("o_stride", Strides * FA_MERGE_MAX_PARTS), ("lse", _vp * FA_MERGE_MAX_PARTS),
                ("lse_stride", LseStrides * FA_MERGE_MAX_PARTS), ("out", _vp), ("out_stride", Strides), ("lse_out", _vp), ("lse_out_stride", LseStrides),
                ("stream", _vp)]


class MlaCacheAppendParams(_Params):
    """fa_mla_cache_append_params: latent rows into the MLA latent cache, copied or quantised to 656-byte rows (fa_run_mla_cache_append)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("kv_cache", _vp), ("kv_new", _vp), ("k_pe", _vp), ("cache_seqlens", _vp),
                ("cu_seqlens_new", _vp), ("block_table", _vp),
                ("b", _i32), ("seqlen_new", _i32), ("seqlen_cache", _i32), ("dtype", _i32), ("kv_format", _i32), ("page_block_size", _i32), ("num_blocks", _i32),
                ("reserved_", _i32), ("total_new", ctypes.c_int64),
                ("kv_cache_stride", Strides), ("kv_new_stride", Strides), ("k_pe_stride", Strides), ("block_table_stride", ctypes.c_int64)]


class MlaCacheGatherParams(_Params):
    """fa_mla_cache_gather_params: rows of the MLA latent cache into the caller's buffer, dequantised from FP8 rows (fa_run_mla_cache_gather)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("kv_cache", _vp), ("out", _vp), ("cache_seqlens", _vp), ("cu_seqlens_out", _vp),
                ("seq_starts", _vp), ("block_table", _vp),
                ("b", _i32), ("seqlen_out", _i32), ("seqlen_cache", _i32), ("dtype", _i32), ("kv_format", _i32), ("page_block_size", _i32), ("num_blocks", _i32),
                ("reserved_", _i32), ("total_out", ctypes.c_int64),
                ("kv_cache_stride", Strides), ("out_batch_stride", ctypes.c_int64), ("out_row_stride", ctypes.c_int64), ("block_table_stride", ctypes.c_int64)]


class MlaIndexCacheAppendParams(_Params):
    """fa_mla_index_cache_append_params: index keys into the index-key cache, copied or quantised to e4m3 with one scale per token (fa_run_mla_index_cache_append)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("magic", ctypes.c_uint32), ("k_idx_cache", _vp), ("k_scale", _vp), ("k_idx_new", _vp), ("cache_seqlens", _vp),
                ("cu_seqlens_new", _vp), ("block_table", _vp),
                ("b", _i32), ("seqlen_new", _i32), ("seqlen_cache", _i32), ("dtype", _i32), ("k_format", _i32), ("scale_format", _i32), ("page_block_size", _i32),
                ("num_blocks", _i32), ("total_new", ctypes.c_int64), ("reserved_", ctypes.c_int64),
                ("k_cache_batch_stride", ctypes.c_int64), ("k_cache_row_stride", ctypes.c_int64), ("k_scale_batch_stride", ctypes.c_int64),
                ("k_scale_row_stride", ctypes.c_int64), ("k_new_batch_stride", ctypes.c_int64), ("k_new_row_stride", ctypes.c_int64),
                ("block_table_stride", ctypes.c_int64)]


FA_MLA_KV_16BIT = 0
FA_MLA_KV_FP8_ROWS656 = 1     # 656-byte latent rows: 512 e4m3 codes, four fp32 scales, 64 rope elements of q's dtype; kv_cache_stride in bytes
FA_CACHE_FP8_E4M3 = 1
FA_IDX_Q_16BIT = 0            # q_format of fa_mla_indexer_params_v2: index queries of `dtype`, strides in elements
FA_IDX_Q_FP8_E4M3 = 1         # ... as OCP e4m3 codes, strides in bytes (needs k_format = FA_IDX_K_FP8_E4M3)
FA_IDX_K_FP8_E4M3 = 1         # k_format of fa_mla_indexer_params: index keys as OCP e4m3 codes, strides in bytes
FA_IDX_SCALE_FP32, FA_IDX_SCALE_UE8M0 = 0, 1     # scale_format of fa_mla_index_cache_append_params


_lib = None


def declared_functions():
    """names of every function declared in the public header"""
    with open(HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fa_[a-z0-9_]+)\s*\(", text)))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIBRARY_PATH):
            raise ImportError(f"{LIBRARY_PATH} missing: run `python flash-attention-turing_amd/build.py`")
        L = ctypes.CDLL(LIBRARY_PATH)
        # a stale build of the same ABI number can lack the (additive) exports this binding needs: say so instead of failing on first use
        missing = [n for n in declared_functions() if not hasattr(L, n)]
        if missing:
            raise ImportError(f"{LIBRARY_PATH} lacks {missing}: stale build, run `python flash-attention-turing_amd/build.py --force`")
        L.fa_abi_version.restype = ctypes.c_int
        L.fa_last_error.restype = ctypes.c_char_p
        L.fa_build_info.restype = ctypes.c_char_p
        L.fa_run_mha_fwd.argtypes = [ctypes.POINTER(FwdParams), _vp]
        L.fa_run_mha_bwd.argtypes = [ctypes.POINTER(BwdParams), _vp]
        L.fa_bwd_dot_do_o.argtypes = [ctypes.POINTER(BwdParams), _vp]
        L.fa_bwd_dq.argtypes = [ctypes.POINTER(BwdParams), _vp]
        L.fa_bwd_dkdv.argtypes = [ctypes.POINTER(BwdParams), _vp]
        L.fa_bwd_workspace_bytes.argtypes = [ctypes.POINTER(BwdParams)]
        L.fa_bwd_workspace_bytes.restype = ctypes.c_int64
        L.fa_run_mha_fwd_kvcache.argtypes = [ctypes.POINTER(KvcacheParams), _vp]
        L.fa_run_mha_fwd_kvcache.restype = ctypes.c_int
        L.fa_kvcache_workspace_bytes.argtypes = [ctypes.POINTER(KvcacheParams)]
        L.fa_kvcache_workspace_bytes.restype = ctypes.c_int64
        L.fa_kvcache_num_splits.argtypes = [ctypes.POINTER(KvcacheParams)]
        L.fa_kvcache_num_splits.restype = ctypes.c_int32
        _op = ctypes.c_void_p                       # fa_kvcache_options, _v2 .. _v8 (told apart by struct_size)
        L.fa_run_mha_fwd_kvcache_ex.argtypes = [ctypes.POINTER(KvcacheParams), _op, _vp]
        L.fa_run_mha_fwd_kvcache_ex.restype = ctypes.c_int
        L.fa_kvcache_workspace_bytes_ex.argtypes = [ctypes.POINTER(KvcacheParams), _op]
        L.fa_kvcache_workspace_bytes_ex.restype = ctypes.c_int64
        L.fa_kvcache_num_splits_ex.argtypes = [ctypes.POINTER(KvcacheParams), _op]
        L.fa_kvcache_num_splits_ex.restype = ctypes.c_int32
        L.fa_kvcache_row_tile_ex.argtypes = [ctypes.POINTER(KvcacheParams), _op]
        L.fa_kvcache_row_tile_ex.restype = ctypes.c_int32
        # (fa_mla_params or fa_mla_params_v2, fa_mla_sparse_params or its _v2, through the same pointer: void*)
        L.fa_run_mla_fwd_kvcache.argtypes = [_vp, _vp]
        L.fa_run_mla_fwd_kvcache.restype = ctypes.c_int
        L.fa_mla_workspace_bytes.argtypes = [_vp]
        L.fa_mla_workspace_bytes.restype = ctypes.c_int64
        L.fa_mla_num_splits.argtypes = [_vp]
        L.fa_mla_num_splits.restype = ctypes.c_int32
        L.fa_run_mla_sparse_fwd_kvcache.argtypes = [_vp, _vp]
        L.fa_run_mla_sparse_fwd_kvcache.restype = ctypes.c_int
        L.fa_mla_sparse_workspace_bytes.argtypes = [_vp]
        L.fa_mla_sparse_workspace_bytes.restype = ctypes.c_int64
        L.fa_mla_sparse_num_splits.argtypes = [_vp]
        L.fa_mla_sparse_num_splits.restype = ctypes.c_int32
        L.fa_run_mla_indexer_logits.argtypes = [ctypes.POINTER(MlaIndexerParams), _vp]
        L.fa_run_mla_indexer_logits.restype = ctypes.c_int
        L.fa_run_mla_indexer_prefill_logits.argtypes = [ctypes.POINTER(MlaIndexerParams), _vp]
        L.fa_run_mla_indexer_prefill_logits.restype = ctypes.c_int
        L.fa_mla_indexer_prefill_launch.argtypes = [ctypes.POINTER(MlaIndexerParams)] + [ctypes.POINTER(ctypes.c_int32)] * 3
        # (fa_mla_indexer_params_v2 or fa_mla_indexer_params through the same pointer: void*)
        L.fa_run_mla_indexer_logits_v2.argtypes = [_vp, _vp]
        L.fa_run_mla_indexer_logits_v2.restype = ctypes.c_int
        L.fa_run_mla_indexer_prefill_logits_v2.argtypes = [_vp, _vp]
        L.fa_run_mla_indexer_prefill_logits_v2.restype = ctypes.c_int
        L.fa_mla_indexer_prefill_launch_v2.argtypes = [_vp] + [ctypes.POINTER(ctypes.c_int32)] * 3
        L.fa_mla_indexer_prefill_launch_v2.restype = ctypes.c_int
        L.fa_mla_indexer_prefill_launch.restype = ctypes.c_int
        L.fa_run_mla_indexer_topk.argtypes = [ctypes.POINTER(MlaTopkParams), _vp]
        L.fa_run_mla_indexer_topk.restype = ctypes.c_int
        L.fa_run_mla_prefill_fwd.argtypes = [ctypes.POINTER(MlaPrefillParams), _vp]
        L.fa_run_mla_prefill_fwd.restype = ctypes.c_int
        L.fa_run_mla_prefill_bwd.argtypes = [ctypes.POINTER(MlaPrefillBwdParams), _vp]
        L.fa_run_mla_prefill_bwd.restype = ctypes.c_int
        L.fa_run_merge_states.argtypes = [ctypes.POINTER(MergeParams)]
        L.fa_run_merge_states.restype = ctypes.c_int
        L.fa_run_mla_cache_append.argtypes = [ctypes.POINTER(MlaCacheAppendParams), _vp]
        L.fa_run_mla_cache_append.restype = ctypes.c_int
        L.fa_run_mla_cache_gather.argtypes = [ctypes.POINTER(MlaCacheGatherParams), _vp]
        L.fa_run_mla_cache_gather.restype = ctypes.c_int
        L.fa_run_mla_index_cache_append.argtypes = [ctypes.POINTER(MlaIndexCacheAppendParams), _vp]
        L.fa_run_mla_index_cache_append.restype = ctypes.c_int
        L.fa_mha_fwd.argtypes = [_vp] * 5 + [_i32] * 8 + [_vp]
        L.fa_mha_bwd.argtypes = [_vp] * 10 + [_i32] * 8 + [_vp]
        L.fa_mha_varlen_fwd.argtypes = [_vp] * 7 + [_i32] * 8 + [_vp]
        L.fa_mha_varlen_bwd.argtypes = [_vp] * 12 + [_i32] * 8 + [_vp]
        for n in ("fa_run_mha_fwd", "fa_run_mha_bwd", "fa_bwd_dot_do_o", "fa_bwd_dq", "fa_bwd_dkdv", "fa_mha_fwd", "fa_mha_bwd",
                  "fa_mha_varlen_fwd", "fa_mha_varlen_bwd"):
            getattr(L, n).restype = ctypes.c_int
        L.fa_fwd_flops.argtypes = [_i32] * 6
        L.fa_fwd_flops.restype = ctypes.c_double
        L.fa_fwd_bytes.argtypes = [_i32] * 6
        L.fa_fwd_bytes.restype = ctypes.c_double
        L.fa_device_clock_khz.argtypes = [_i32]
        L.fa_device_clock_khz.restype = ctypes.c_int
        L.fa_fwd_kernel_name.argtypes = [_i32]
        L.fa_fwd_kernel_name.restype = ctypes.c_char_p
        L.fa_kernel_name.argtypes = [_i32] * 7
        L.fa_kernel_name.restype = ctypes.c_char_p
        L.fa_kernel_name_dtype.argtypes = [_i32] * 8
        L.fa_kernel_name_dtype.restype = ctypes.c_char_p
        L.fa_set_kernel_policy.argtypes = [_i32]
        L.fa_set_kernel_policy.restype = _i32
        L.fa_set_policy_problem_heads.argtypes = [ctypes.c_int64]
        L.fa_set_policy_problem_heads.restype = ctypes.c_int64
        _lib = L
    return _lib


def device_clock_khz(device_index=0) -> int:
    return int(lib().fa_device_clock_khz(int(device_index)))


def fwd_kernel_name(d) -> str:
    return lib().fa_fwd_kernel_name(int(d)).decode()


STAGES = {"fwd": 0, "dq": 1, "dkdv": 2}


DTYPES = {"fp16": 0, "bf16": 1}


def kernel_name(stage, b, seqlen_q, seqlen_k, h, d, causal, dtype="fp16") -> str:
    """fa_kernel_name_dtype: the kernel a launch of this shape goes to under the current policy (stage: "fwd", "dq", "dkdv"; dtype "fp16" / "bf16")"""
    return lib().fa_kernel_name_dtype(STAGES[stage], DTYPES[dtype], int(b), int(seqlen_q), int(seqlen_k), int(h), int(d), int(bool(causal))).decode()


POLICY_MFMA32, POLICY_MFMA16, POLICY_AUTO = 0, 1, 2


def set_kernel_policy(policy) -> int:
    """fa_set_kernel_policy: which head_dim-128 kernel set (32x32x16 / 16x16x32 MFMA tiles) serves a launch; returns the previous policy"""
    prev = lib().fa_set_kernel_policy(int(policy))
    if prev < 0:
        raise ValueError(f"unknown kernel policy {policy}")
    return prev


def set_policy_problem_heads(batch_times_heads) -> int:
    """fa_set_policy_problem_heads: the batch x heads FA_POLICY_AUTO sizes the following launches with (0 = each launch's own); returns the previous value"""
    prev = lib().fa_set_policy_problem_heads(int(batch_times_heads))
    if prev < 0:
        raise ValueError(f"batch x heads must be >= 0, got {batch_times_heads}")
    return prev


def last_error() -> str:
    return lib().fa_last_error().decode()


def check(rc: int):
    if rc != FA_OK:
        raise RuntimeError(f"flash_attn_gfx950: {last_error()} [code {rc}]")


def dtype_code(torch_dtype) -> int:
    import torch

    return {torch.float16: FA_FP16, torch.bfloat16: FA_BF16}[torch_dtype]


def mha_fwd(q, k, v, o, lse, causal, stream=None):
    """Contiguous torch tensors in, kernels enqueued on `stream` (default: torch's current stream)."""
    import torch

    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    s = torch.cuda.current_stream(q.device).cuda_stream if stream is None else stream
    check(lib().fa_mha_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                           b, sq, sk, h, hk, d, dtype_code(q.dtype), int(causal), s))


def mha_bwd(q, k, v, o, lse, dout, dq, dk, dv, dsum, causal, stream=None):
    import torch

    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    s = torch.cuda.current_stream(q.device).cuda_stream if stream is None else stream
    check(lib().fa_mha_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), dout.data_ptr(),
                           dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dsum.data_ptr(),
                           b, sq, sk, h, hk, d, dtype_code(q.dtype), int(causal), s))


def bwd_params(q, k, v, o, lse, dout, dq, dk, dv, dsum, causal):
    """fa_bwd_params for contiguous (b, s, h, d) torch tensors (stage-level entry points: fa_bwd_dot_do_o / fa_bwd_dq / fa_bwd_dkdv)"""
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    p = BwdParams()
    p.q, p.k, p.v, p.o, p.dout, p.lse = (t.data_ptr() for t in (q, k, v, o, dout, lse))
    p.dq, p.dk, p.dv, p.dsoftmax_sum = (t.data_ptr() for t in (dq, dk, dv, dsum))
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d = b, sq, sk, h, hk, d
    p.dtype, p.is_causal = dtype_code(q.dtype), int(causal)
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o), ("do_stride", dout),
                    ("dq_stride", dq), ("dk_stride", dk), ("dv_stride", dv)):
        setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def bwd_workspace_bytes(params):
    """bytes of fp32 scratch the dK/dV launch of these params would use to split a KV head's query-head group (0: no split)"""
    n = lib().fa_bwd_workspace_bytes(ctypes.byref(params))
    if n < 0:
        check(int(n))
    return int(n)


def attach_workspace(params, like):
    """allocate the scratch fa_bwd_workspace_bytes asks for (torch, on `like`'s device) and hang it on params; returns the tensor
    (keep it alive until the launch has run) or None"""
    import torch

    n = bwd_workspace_bytes(params)
    if n == 0:
        return None
    ws = torch.empty(n // 4, device=like.device, dtype=torch.float32)
    params.workspace, params.workspace_bytes = ws.data_ptr(), n
    return ws


def run_bwd(params, stream=None):
    """the whole backward from a parameter struct, e.g. one with a workspace attached: dQ (which also computes D = rowsum(dO * O)
    into dsoftmax_sum), then dK/dV (+ the plane sum when the head group was split through the workspace)"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mha_bwd(ctypes.byref(params), s))


def bwd_stage(name, params, stream=None):
    """run one backward launch: name in {'dot_do_o', 'dq', 'dkdv'}"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(getattr(lib(), "fa_bwd_" + name)(ctypes.byref(params), s))


def fwd_params(q, k, v, o, lse, causal):
    """fa_fwd_params for (b, s, h, d) torch tensors with arbitrary batch / row / head strides (e.g. shard views)"""
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    p = FwdParams()
    p.q, p.k, p.v, p.o, p.lse = (t.data_ptr() for t in (q, k, v, o, lse))
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d = b, sq, sk, h, hk, d
    p.dtype, p.is_causal = dtype_code(q.dtype), int(causal)
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o)):
        setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def run_fwd(params, stream=None):
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mha_fwd(ctypes.byref(params), s))


def kvcache_params(q, k_cache, v_cache, o, lse, cache_seqlens=None, k_new=None, v_new=None, causal=False, num_splits=0, block_table=None, *,
                   cu_seqlens_q=None, max_seqlen_q=None):
    """fa_kvcache_params for (b, s, h, d) torch tensors with arbitrary batch / row / head strides (caches may be views of larger buffers);
    with block_table (int32 (b, max_blocks_per_seq)) the caches are page pools (num_blocks, page_block_size, h_k, d).  With cu_seqlens_q
    (a ragged call; pass the same tensor to kvcache_options) q / o are packed (total_q, h, d), k_new / v_new (total_new, h_k, d), lse is
    (h, total_q), b = len(cu_seqlens_q) - 1 and seqlen_q = max_seqlen_q."""
    if cu_seqlens_q is not None:
        return _kvcache_params_ragged(q, k_cache, v_cache, o, lse, cache_seqlens, k_new, v_new, causal, num_splits, block_table, cu_seqlens_q, max_seqlen_q)
    b, sq, h, d = q.shape
    p = KvcacheParams()
    p.q, p.k_cache, p.v_cache, p.o, p.lse = (t.data_ptr() for t in (q, k_cache, v_cache, o, lse))
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.h_k, p.d = b, sq, k_cache.shape[1], h, k_cache.shape[2], d
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_block_size, p.num_blocks = k_cache.shape[1], k_cache.shape[0]
        p.seqlen_cache = block_table.shape[1] * k_cache.shape[1]
    p.dtype, p.is_causal, p.num_splits = dtype_code(q.dtype), int(causal), int(num_splits)
    tensors = [("q_stride", q), ("k_cache_stride", k_cache), ("v_cache_stride", v_cache), ("o_stride", o)]
    if k_new is not None:
        p.k_new, p.v_new, p.seqlen_new = k_new.data_ptr(), v_new.data_ptr(), k_new.shape[1]
        tensors += [("k_new_stride", k_new), ("v_new_stride", v_new)]
    for name, t in tensors:
        setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def _kvcache_params_ragged(q, k_cache, v_cache, o, lse, cache_seqlens, k_new, v_new, causal, num_splits, block_table, cu_seqlens_q, max_seqlen_q):
    total_q, h, d = q.shape
    p = KvcacheParams()
    p.q, p.k_cache, p.v_cache, p.o, p.lse = (t.data_ptr() for t in (q, k_cache, v_cache, o, lse))
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.h_k, p.d = cu_seqlens_q.shape[0] - 1, int(max_seqlen_q), k_cache.shape[1], h, k_cache.shape[2], d
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_block_size, p.num_blocks = k_cache.shape[1], k_cache.shape[0]
        p.seqlen_cache = block_table.shape[1] * k_cache.shape[1]
    p.dtype, p.is_causal, p.num_splits = dtype_code(q.dtype), int(causal), int(num_splits)
    for name, t in (("k_cache_stride", k_cache), ("v_cache_stride", v_cache)):
        setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    packed = [("q_stride", q), ("o_stride", o)]
    if k_new is not None:
        p.k_new, p.v_new, p.seqlen_new = k_new.data_ptr(), v_new.data_ptr(), min(k_new.shape[0], p.seqlen_cache)
        packed += [("k_new_stride", k_new), ("v_new_stride", v_new)]
    for name, t in packed:
        setattr(p, name, Strides(0, t.stride(0), t.stride(1)))         # (the batch stride of a packed tensor is not read)
    return p


def kvcache_options(window_size=(-1, -1), cache_dtype=0, k_descale=None, v_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=True, *,
                    cu_seqlens_q=None, cu_seqlens_k_new=None, total_q=0, total_k_new=0, softmax_scale=None, softcap=None, sinks=None, tree_mask=None, row_tile=None):
    """fa_kvcache_options with a sliding window (left, right); (-1, -1) gives a zeroed struct (no window).  With cache_dtype
    (FA_CACHE_FP8_E4M3) or a descale (float32 (b, h_k) torch tensors, any strides) the struct is fa_kvcache_options_v2; with rotary_cos /
    rotary_sin ((seqlen_ro, rotary_dim / 2) torch tensors of q's dtype with one row stride) it is fa_kvcache_options_v3; with cu_seqlens_q /
    cu_seqlens_k_new (int32 (b + 1,) torch tensors) and the packed row counts total_q / total_k_new it is fa_kvcache_options_v4; with softmax_scale or
    softcap (Python floats; None = not given) it is fa_kvcache_options_v5; with sinks (a float32 (nheads,) torch tensor, any stride) it is
    fa_kvcache_options_v6; with tree_mask (an int64 torch tensor, (b, seqlen_q) or, ragged, (total_q,), any strides) it is fa_kvcache_options_v7; with row_tile (a Python int; None = not given) it is
    fa_kvcache_options_v8."""
    v8 = row_tile is not None
    v7 = v8 or tree_mask is not None
    v6 = v7 or sinks is not None
    v5 = v6 or softmax_scale is not None or softcap is not None
    v4 = v5 or cu_seqlens_q is not None or cu_seqlens_k_new is not None
    v3 = rotary_cos is not None or rotary_sin is not None
    v2 = v3 or cache_dtype != 0 or k_descale is not None or v_descale is not None
    o = KvcacheOptionsV8() if v8 else KvcacheOptionsV7() if v7 else KvcacheOptionsV6() if v6 else KvcacheOptionsV5() if v5 else KvcacheOptionsV4() if v4 else KvcacheOptionsV3() if v3 else KvcacheOptionsV2() if v2 else KvcacheOptions()
    if v4:
        o.cu_seqlens_q = None if cu_seqlens_q is None else cu_seqlens_q.data_ptr()
        o.cu_seqlens_k_new = None if cu_seqlens_k_new is None else cu_seqlens_k_new.data_ptr()
        o.total_q, o.total_k_new = int(total_q), int(total_k_new)
        v2 = True
    if v5:
        o.softmax_scale = 0.0 if softmax_scale is None else float(softmax_scale)
        o.softcap = 0.0 if softcap is None else float(softcap)
    if v6 and sinks is not None:
        o.sinks, o.sinks_stride = sinks.data_ptr(), sinks.stride(0)
    if v8:
        o.row_tile = int(row_tile)
    if v7 and tree_mask is not None:
        o.tree_mask = tree_mask.data_ptr()
        o.tree_mask_batch_stride, o.tree_mask_row_stride = (0, tree_mask.stride(0)) if tree_mask.dim() == 1 else (tree_mask.stride(0), tree_mask.stride(1))
    left, right = window_size
    if (left, right) != (-1, -1):
        o.is_local, o.window_size_left, o.window_size_right = 1, int(left), int(right)
    if v2:
        o.cache_dtype = int(cache_dtype)
        if k_descale is not None:
            o.k_descale, o.k_descale_batch_stride, o.k_descale_head_stride = k_descale.data_ptr(), k_descale.stride(0), k_descale.stride(1)
        if v_descale is not None:
            o.v_descale, o.v_descale_batch_stride, o.v_descale_head_stride = v_descale.data_ptr(), v_descale.stride(0), v_descale.stride(1)
    if v3:
        t = rotary_cos if rotary_cos is not None else rotary_sin
        o.rotary_cos = None if rotary_cos is None else rotary_cos.data_ptr()
        o.rotary_sin = None if rotary_sin is None else rotary_sin.data_ptr()
        o.rotary_row_stride, o.seqlen_ro, o.rotary_dim = t.stride(0), t.shape[0], 2 * t.shape[1]
        o.rotary_interleaved = int(bool(rotary_interleaved))
    return o


def kvcache_workspace_bytes(params, options=None) -> int:
    """fa_kvcache_workspace_bytes[_ex]: fp32 scratch the split the library would choose needs (0: one split); options = KvcacheOptions"""
    n = lib().fa_kvcache_workspace_bytes(ctypes.byref(params)) if options is None else lib().fa_kvcache_workspace_bytes_ex(ctypes.byref(params), ctypes.byref(options))
    if n < 0:
        check(int(n))
    return int(n)


def kvcache_num_splits(params, options=None) -> int:
    """fa_kvcache_num_splits[_ex]: key splits the launch of these params would use (their workspace fields included)"""
    n = lib().fa_kvcache_num_splits(ctypes.byref(params)) if options is None else lib().fa_kvcache_num_splits_ex(ctypes.byref(params), ctypes.byref(options))
    if n < 0:
        check(int(n))
    return int(n)


def kvcache_row_tile(params, options=None) -> int:
    """fa_kvcache_row_tile_ex: packed query rows per workgroup of the attention launch these params and options would make (16 or 64)"""
    n = lib().fa_kvcache_row_tile_ex(ctypes.byref(params), None if options is None else ctypes.byref(options))
    if n < 0:
        check(int(n))
    return int(n)


def run_fwd_kvcache(params, stream=None, options=None):
    """fa_run_mha_fwd_kvcache, or fa_run_mha_fwd_kvcache_ex with options (KvcacheOptions)"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    if options is None:
        check(lib().fa_run_mha_fwd_kvcache(ctypes.byref(params), s))
    else:
        check(lib().fa_run_mha_fwd_kvcache_ex(ctypes.byref(params), ctypes.byref(options), s))


def mla_cache_is_fp8(kv_cache) -> bool:
    """a latent cache in the FP8 format of the two MLA calls: uint8 or float8_e4m3fn, 656 bytes a row"""
    import torch

    return kv_cache.dtype in (torch.uint8, torch.float8_e4m3fn) and kv_cache.shape[-1] == 656


def mla_params(q, kv_cache, o, lse, cache_seqlens=None, kv_new=None, causal=False, num_splits=0, block_table=None, softmax_scale=None):
    """fa_mla_params for q (b, sq, h, 576), kv_cache (b, capacity, 1, 576) - or, with block_table (int32 (b, max_blocks)), a page pool (num_blocks,
    page_block_size, 1, 576) - kv_new (b, s_new, 1, 576) and o (b, sq, h, 512) torch tensors with arbitrary batch / row / head strides.  An FP8 cache
    (uint8 / float8_e4m3fn, 656 wide) gives a MlaParamsV2 with kv_format = FA_MLA_KV_FP8_ROWS656."""
    b, sq, h, d_qk = q.shape
    p = MlaParams()
    if mla_cache_is_fp8(kv_cache):      # a 1-byte dtype: the strides below are in bytes, as the format asks
        p = MlaParamsV2()
        p.kv_format = FA_MLA_KV_FP8_ROWS656
    p.q, p.kv_cache, p.o, p.lse = (t.data_ptr() for t in (q, kv_cache, o, lse))
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.d_qk, p.d_v = b, sq, kv_cache.shape[1], h, d_qk, o.shape[-1]
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_block_size, p.num_blocks = kv_cache.shape[1], kv_cache.shape[0]
        p.seqlen_cache = block_table.shape[1] * kv_cache.shape[1]
    p.dtype, p.is_causal, p.num_splits = dtype_code(q.dtype), int(causal), int(num_splits)
    p.softmax_scale = 0.0 if softmax_scale is None else float(softmax_scale)
    tensors = [("q_stride", q), ("kv_cache_stride", kv_cache), ("o_stride", o)]
    if kv_new is not None:
        p.kv_new, p.seqlen_new = kv_new.data_ptr(), kv_new.shape[1]
        tensors.append(("kv_new_stride", kv_new))
    for name, t in tensors:
        setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def mla_workspace_bytes(params) -> int:
    """fa_mla_workspace_bytes: fp32 scratch the split the library would choose (or num_splits) needs (0: one split)"""
    n = lib().fa_mla_workspace_bytes(ctypes.byref(params))
    if n < 0:
        check(int(n))
    return int(n)


def mla_num_splits(params) -> int:
    """fa_mla_num_splits: key splits the launch of these params would use (their workspace fields included)"""
    n = lib().fa_mla_num_splits(ctypes.byref(params))
    if n < 0:
        check(int(n))
    return int(n)


def run_mla_fwd_kvcache(params, stream=None):
    """fa_run_mla_fwd_kvcache"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mla_fwd_kvcache(ctypes.byref(params), s))


def mla_sparse_params(q, kv_cache, o, lse, indices, cache_seqlens=None, num_splits=0, block_table=None, softmax_scale=None):
    """fa_mla_sparse_params for q (b, sq, h, 576), kv_cache (b, capacity, 1, 576) - or, with block_table (int32 (b, max_blocks)), a page pool (num_blocks,
    page_block_size, 1, 576) - indices int32 (b, sq, topk) with any batch / row strides, and o (b, sq, h, 512) torch tensors.  An FP8 cache (uint8 /
    float8_e4m3fn, 656 wide) gives a MlaSparseParamsV2 with kv_format = FA_MLA_KV_FP8_ROWS656."""
    b, sq, h, d_qk = q.shape
    p = MlaSparseParams()
    if mla_cache_is_fp8(kv_cache):      # a 1-byte dtype: the strides below are in bytes, as the format asks
        p = MlaSparseParamsV2()
        p.kv_format = FA_MLA_KV_FP8_ROWS656
    p.q, p.kv_cache, p.o, p.lse, p.indices = (t.data_ptr() for t in (q, kv_cache, o, lse, indices))
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.d_qk, p.d_v = b, sq, kv_cache.shape[1], h, d_qk, o.shape[-1]
    p.topk, p.indices_batch_stride, p.indices_row_stride = indices.shape[-1], indices.stride(0), indices.stride(1)
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_block_size, p.num_blocks = kv_cache.shape[1], kv_cache.shape[0]
        p.seqlen_cache = block_table.shape[1] * kv_cache.shape[1]
    p.dtype, p.num_splits = dtype_code(q.dtype), int(num_splits)
    p.softmax_scale = 0.0 if softmax_scale is None else float(softmax_scale)
    for name, t in (("q_stride", q), ("kv_cache_stride", kv_cache), ("o_stride", o)):
        setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def mla_sparse_workspace_bytes(params) -> int:
    """fa_mla_sparse_workspace_bytes: fp32 scratch the split the library would choose (or num_splits) needs (0: one split)"""
    n = lib().fa_mla_sparse_workspace_bytes(ctypes.byref(params))
    if n < 0:
        check(int(n))
    return int(n)


def mla_sparse_num_splits(params) -> int:
    """fa_mla_sparse_num_splits: slot splits the launch of these params would use (their workspace fields included)"""
    n = lib().fa_mla_sparse_num_splits(ctypes.byref(params))
    if n < 0:
        check(int(n))
    return int(n)


def run_mla_sparse_fwd_kvcache(params, stream=None):
    """fa_run_mla_sparse_fwd_kvcache"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mla_sparse_fwd_kvcache(ctypes.byref(params), s))


def mla_indexer_params(q_idx, weights, k_idx_cache, logits, cache_seqlens=None, k_scale=None, block_table=None, causal=True):
    """fa_mla_indexer_params for q_idx (b, sq, h, 128), weights fp32 (b, sq, h), k_idx_cache (b, capacity, 128) in q_idx's dtype or uint8 / float8_e4m3fn
    (e4m3 codes: a 1-byte dtype, so its strides are bytes, as the format asks) - or, with block_table, a pool (num_blocks, page_block_size, 128) - k_scale
    fp32 (b, capacity) / (num_blocks, page_block_size) or None, and the caller's fp32 buffer logits (b, sq, capacity): torch tensors with arbitrary strides."""
    return _fill_mla_indexer(MlaIndexerParams(), dtype_code(q_idx.dtype), q_idx, weights, k_idx_cache, logits, cache_seqlens, k_scale, block_table, causal)


def _fill_mla_indexer(p, dtype, q_idx, weights, k_idx_cache, logits, cache_seqlens, k_scale, block_table, causal):
    """the fields fa_mla_indexer_params and its _v2 share"""
    b, sq, h, d = q_idx.shape
    p.q_idx, p.weights, p.k_idx_cache, p.logits = (t.data_ptr() for t in (q_idx, weights, k_idx_cache, logits))
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.d = b, sq, k_idx_cache.shape[1], h, d
    p.dtype, p.is_causal = dtype, int(causal)
    p.k_format = FA_IDX_K_FP8_E4M3 if k_idx_cache.element_size() == 1 else FA_MLA_KV_16BIT
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_block_size, p.num_blocks = k_idx_cache.shape[1], k_idx_cache.shape[0]
        p.seqlen_cache = block_table.shape[1] * k_idx_cache.shape[1]
    if k_scale is not None:
        p.k_scale, p.k_scale_batch_stride, p.k_scale_row_stride = k_scale.data_ptr(), k_scale.stride(0), k_scale.stride(1)
    p.q_idx_stride = Strides(q_idx.stride(0), q_idx.stride(1), q_idx.stride(2))
    p.weights_stride = Strides(weights.stride(0), weights.stride(1), weights.stride(2))
    p.k_cache_batch_stride, p.k_cache_row_stride = k_idx_cache.stride(0), k_idx_cache.stride(1)
    p.logits_batch_stride, p.logits_row_stride = logits.stride(0), logits.stride(1)
    return p


def mla_indexer_params_v2(q_idx, weights, k_idx_cache, logits, cache_seqlens=None, k_scale=None, block_table=None, causal=True):
    """fa_mla_indexer_params_v2 for the tensors of mla_indexer_params.  A uint8 / float8_e4m3fn q_idx gives q_format = FA_IDX_Q_FP8_E4M3 (a 1-byte dtype, so its
    strides are bytes, as the format asks) and dtype = FA_BF16, a valid value that is not used; an fp16 / bf16 q_idx gives q_format = FA_IDX_Q_16BIT."""
    q8 = q_idx.element_size() == 1
    p = _fill_mla_indexer(MlaIndexerParamsV2(), FA_BF16 if q8 else dtype_code(q_idx.dtype), q_idx, weights, k_idx_cache, logits, cache_seqlens, k_scale, block_table, causal)
    p.q_format = FA_IDX_Q_FP8_E4M3 if q8 else FA_IDX_Q_16BIT
    return p


def run_mla_indexer_logits(params, stream=None):
    """fa_run_mla_indexer_logits"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check((lib().fa_run_mla_indexer_logits_v2 if isinstance(params, MlaIndexerParamsV2) else lib().fa_run_mla_indexer_logits)(ctypes.byref(params), s))


def run_mla_indexer_prefill_logits(params, stream=None):
    """fa_run_mla_indexer_prefill_logits: the fa_mla_indexer_params of run_mla_indexer_logits, a workgroup per tile of tokens"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check((lib().fa_run_mla_indexer_prefill_logits_v2 if isinstance(params, MlaIndexerParamsV2) else lib().fa_run_mla_indexer_prefill_logits)(ctypes.byref(params), s))


def mla_indexer_prefill_launch(params):
    """fa_mla_indexer_prefill_launch: (tokens of a workgroup's tile, keys of a workgroup's range, ranges per tile) of the launch these params would make; host only"""
    tq, wg, nc = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    fn = lib().fa_mla_indexer_prefill_launch_v2 if isinstance(params, MlaIndexerParamsV2) else lib().fa_mla_indexer_prefill_launch
    check(fn(ctypes.byref(params), ctypes.byref(tq), ctypes.byref(wg), ctypes.byref(nc)))
    return tq.value, wg.value, nc.value


def mla_topk_params(logits, indices, cache_seqlens=None, causal=True):
    """fa_mla_topk_params for logits fp32 (b, sq, capacity), any batch / row strides, and the contiguous int32 buffer indices (b, sq, topk)"""
    p = MlaTopkParams()
    p.logits, p.indices = logits.data_ptr(), indices.data_ptr()
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.b, p.seqlen_q, p.seqlen_cache, p.topk, p.is_causal = logits.shape[0], logits.shape[1], logits.shape[2], indices.shape[-1], int(causal)
    p.logits_batch_stride, p.logits_row_stride = logits.stride(0), logits.stride(1)
    return p


def run_mla_indexer_topk(params, stream=None):
    """fa_run_mla_indexer_topk"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mla_indexer_topk(ctypes.byref(params), s))


def mla_prefill_params(q, k, v, o, lse, cu_seqlens_q=None, cu_seqlens_k=None, causal=False, softmax_scale=None):
    """fa_mla_prefill_params for dense q (b, sq, h, 192), k (b, sk, h_k, 192), v (b, sk, h_k, 128), o (b, sq, h, 128), lse (b, h, sq) or, with both
    cu_seqlens (int32 (b + 1,)), packed q (total_q, h, 192), k (total_k, h_k, 192), v (total_k, h_k, 128), o (total_q, h, 128), lse (h, total_q): torch
    tensors with arbitrary batch / row / head strides, the caller's o and lse."""
    p = MlaPrefillParams()
    p.q, p.k, p.v, p.o, p.lse = (t.data_ptr() for t in (q, k, v, o, lse))
    packed = cu_seqlens_q is not None or cu_seqlens_k is not None
    p.h, p.h_k, p.d_qk, p.d_v = q.shape[-2], k.shape[-2], q.shape[-1], v.shape[-1]
    p.dtype, p.is_causal = dtype_code(q.dtype), int(causal)
    p.softmax_scale = 0.0 if softmax_scale is None else float(softmax_scale)
    if packed:
        p.cu_seqlens_q = None if cu_seqlens_q is None else cu_seqlens_q.data_ptr()
        p.cu_seqlens_k = None if cu_seqlens_k is None else cu_seqlens_k.data_ptr()
        p.b = (cu_seqlens_q if cu_seqlens_q is not None else cu_seqlens_k).numel() - 1
        p.total_q, p.total_k = q.shape[0], k.shape[0]
        for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o)):
            setattr(p, name, Strides(0, t.stride(0), t.stride(1)))
    else:
        p.b, p.seqlen_q, p.seqlen_k = q.shape[0], q.shape[1], k.shape[1]
        for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o)):
            setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def run_mla_prefill_fwd(params, stream=None):
    """fa_run_mla_prefill_fwd"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mla_prefill_fwd(ctypes.byref(params), s))


def mla_prefill_bwd_params(dout, q, k, v, o, lse, dq, dk, dv, dsoftmax_sum, cu_seqlens_q=None, cu_seqlens_k=None, causal=False, softmax_scale=None, phases=0):
    """fa_mla_prefill_bwd_params for the tensors of mla_prefill_params plus dout (like o), the caller's dq / dk / dv (like q / k / v, strides of their own)
    and dsoftmax_sum (fp32, like lse)."""
    p = MlaPrefillBwdParams()
    p.q, p.k, p.v, p.o, p.lse, p.dout, p.dq, p.dk, p.dv, p.dsoftmax_sum = (t.data_ptr() for t in (q, k, v, o, lse, dout, dq, dk, dv, dsoftmax_sum))
    packed = cu_seqlens_q is not None or cu_seqlens_k is not None
    p.h, p.h_k, p.d_qk, p.d_v = q.shape[-2], k.shape[-2], q.shape[-1], v.shape[-1]
    p.dtype, p.is_causal, p.phases = dtype_code(q.dtype), int(causal), int(phases)
    p.softmax_scale = 0.0 if softmax_scale is None else float(softmax_scale)
    tensors = (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o), ("dout_stride", dout), ("dq_stride", dq), ("dk_stride", dk), ("dv_stride", dv))
    if packed:
        p.cu_seqlens_q = None if cu_seqlens_q is None else cu_seqlens_q.data_ptr()
        p.cu_seqlens_k = None if cu_seqlens_k is None else cu_seqlens_k.data_ptr()
        p.b = (cu_seqlens_q if cu_seqlens_q is not None else cu_seqlens_k).numel() - 1
        p.total_q, p.total_k = q.shape[0], k.shape[0]
        for name, t in tensors:
            setattr(p, name, Strides(0, t.stride(0), t.stride(1)))
    else:
        p.b, p.seqlen_q, p.seqlen_k = q.shape[0], q.shape[1], k.shape[1]
        for name, t in tensors:
            setattr(p, name, Strides(t.stride(0), t.stride(1), t.stride(2)))
    return p


def run_mla_prefill_bwd(params, stream=None):
    """fa_run_mla_prefill_bwd"""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(lib().fa_run_mla_prefill_bwd(ctypes.byref(params), s))


def merge_params(outs, lses, out, lse_out, stream=None):
    """fa_merge_params for parts outs[i] (b, rows, h, d_v) / lses[i] (b, h, rows), or packed outs[i] (total, h, d_v) / lses[i] (h, total): torch tensors with
    strides of their own (an LSE may be any view of those shapes), the caller's out and lse_out.  stream: a raw stream handle, None = the default stream."""
    p = MergeParams()
    p.n_parts, p.dtype = len(outs), dtype_code(out.dtype)
    packed = out.dim() == 3
    p.b, p.rows, p.h, p.d_v = (1 if packed else out.shape[0]), out.shape[-3], out.shape[-2], out.shape[-1]
    ostr = (lambda t: Strides(0, t.stride(0), t.stride(1))) if packed else (lambda t: Strides(t.stride(0), t.stride(1), t.stride(2)))
    lstr = (lambda t: LseStrides(0, t.stride(0), t.stride(1))) if packed else (lambda t: LseStrides(t.stride(0), t.stride(1), t.stride(2)))
    for i, (o, l) in enumerate(zip(outs, lses)):
        p.o[i], p.lse[i], p.o_stride[i], p.lse_stride[i] = o.data_ptr(), l.data_ptr(), ostr(o), lstr(l)
    p.out, p.lse_out, p.out_stride, p.lse_out_stride = out.data_ptr(), lse_out.data_ptr(), ostr(out), lstr(lse_out)
    p.stream = stream
    return p


def run_merge_states(params):
    """fa_run_merge_states (the stream is a field of the struct)"""
    check(lib().fa_run_merge_states(ctypes.byref(params)))


def _attach_paging(p, block_table, pool):
    """the four paging fields of a cache-io struct over the page pool ``pool``; seqlen_cache becomes the table's capacity"""
    p.seqlen_cache = pool.shape[1]
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_block_size, p.num_blocks = pool.shape[1], pool.shape[0]
        p.seqlen_cache = block_table.shape[1] * pool.shape[1]


def mla_cache_append_params(kv_cache, kv_new, cache_seqlens, k_pe=None, block_table=None, cu_seqlens_new=None):
    """fa_mla_cache_append_params for kv_cache (b, capacity, 1, 576) 16-bit or (.., 656) uint8 / float8_e4m3fn (or a pool with block_table), kv_new dense
    (b, s_new, 1, w) or packed (total_new, 1, w) with cu_seqlens_new, w = 576 or 512 with k_pe (.., 1, 64): torch tensors with arbitrary strides."""
    packed = cu_seqlens_new is not None
    p = MlaCacheAppendParams()
    p.kv_cache, p.kv_new, p.cache_seqlens = kv_cache.data_ptr(), kv_new.data_ptr(), cache_seqlens.data_ptr()
    p.b, p.dtype = cache_seqlens.shape[0], dtype_code(kv_new.dtype)
    p.kv_format = FA_MLA_KV_FP8_ROWS656 if kv_cache.element_size() == 1 else FA_MLA_KV_16BIT
    _attach_paging(p, block_table, kv_cache)
    rows = (lambda t: Strides(0, t.stride(0), 0)) if packed else (lambda t: Strides(t.stride(0), t.stride(1), 0))
    p.kv_cache_stride, p.kv_new_stride = Strides(kv_cache.stride(0), kv_cache.stride(1), 0), rows(kv_new)
    if k_pe is not None:
        p.k_pe, p.k_pe_stride = k_pe.data_ptr(), rows(k_pe)
    if packed:
        p.cu_seqlens_new, p.total_new = cu_seqlens_new.data_ptr(), kv_new.shape[0]
    else:
        p.seqlen_new = kv_new.shape[1]
    return p


def mla_cache_gather_params(kv_cache, out, cache_seqlens=None, block_table=None, cu_seqlens_out=None, seq_starts=None):
    """fa_mla_cache_gather_params for kv_cache as in mla_cache_append_params and out dense (b, n, 576) or packed (total, 576) with cu_seqlens_out"""
    packed = cu_seqlens_out is not None
    p = MlaCacheGatherParams()
    p.kv_cache, p.out = kv_cache.data_ptr(), out.data_ptr()
    p.cache_seqlens = None if cache_seqlens is None else cache_seqlens.data_ptr()
    p.seq_starts = None if seq_starts is None else seq_starts.data_ptr()
    p.b, p.dtype = (cu_seqlens_out.shape[0] - 1 if packed else out.shape[0]), dtype_code(out.dtype)
    p.kv_format = FA_MLA_KV_FP8_ROWS656 if kv_cache.element_size() == 1 else FA_MLA_KV_16BIT
    _attach_paging(p, block_table, kv_cache)
    p.kv_cache_stride = Strides(kv_cache.stride(0), kv_cache.stride(1), 0)
    if packed:
        p.cu_seqlens_out, p.total_out, p.out_row_stride = cu_seqlens_out.data_ptr(), out.shape[0], out.stride(0)
    else:
        p.seqlen_out, p.out_batch_stride, p.out_row_stride = out.shape[1], out.stride(0), out.stride(1)
    return p


def mla_index_cache_append_params(k_idx_cache, k_idx_new, cache_seqlens, k_scale=None, block_table=None, cu_seqlens_new=None, scale_format=FA_IDX_SCALE_FP32):
    """fa_mla_index_cache_append_params for k_idx_cache / k_scale as in mla_indexer_params and k_idx_new dense (b, s_new, 128) or packed (total_new, 128)"""
    packed = cu_seqlens_new is not None
    p = MlaIndexCacheAppendParams()
    p.k_idx_cache, p.k_idx_new, p.cache_seqlens = k_idx_cache.data_ptr(), k_idx_new.data_ptr(), cache_seqlens.data_ptr()
    p.b, p.dtype, p.scale_format = cache_seqlens.shape[0], dtype_code(k_idx_new.dtype), scale_format
    p.k_format = FA_IDX_K_FP8_E4M3 if k_idx_cache.element_size() == 1 else FA_MLA_KV_16BIT
    _attach_paging(p, block_table, k_idx_cache)
    p.k_cache_batch_stride, p.k_cache_row_stride = k_idx_cache.stride(0), k_idx_cache.stride(1)
    if k_scale is not None:
        p.k_scale, p.k_scale_batch_stride, p.k_scale_row_stride = k_scale.data_ptr(), k_scale.stride(0), k_scale.stride(1)
    if packed:
        p.cu_seqlens_new, p.total_new, p.k_new_row_stride = cu_seqlens_new.data_ptr(), k_idx_new.shape[0], k_idx_new.stride(0)
    else:
        p.seqlen_new, p.k_new_batch_stride, p.k_new_row_stride = k_idx_new.shape[1], k_idx_new.stride(0), k_idx_new.stride(1)
    return p


def _run_io(name, params, stream):
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    check(getattr(lib(), name)(ctypes.byref(params), s))


def run_mla_cache_append(params, stream=None):
    """fa_run_mla_cache_append"""
    _run_io("fa_run_mla_cache_append", params, stream)


def run_mla_cache_gather(params, stream=None):
    """fa_run_mla_cache_gather"""
    _run_io("fa_run_mla_cache_gather", params, stream)


def run_mla_index_cache_append(params, stream=None):
    """fa_run_mla_index_cache_append"""
    _run_io("fa_run_mla_index_cache_append", params, stream)
