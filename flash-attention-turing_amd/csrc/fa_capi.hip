// fa_capi.hip — the C-ABI boundary (include/flash_attn_gfx950.h).
// Host-side validation + parameter fill + dispatch; the counterpart of the reference's
// set_params_fprop / set_params_dgrad / run_mha_fwd / run_mha_bwd
// (csrc/flash_attn/flash_api.cpp:5-153) without any torch type in sight.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "fa_params.hpp"
#include "fa_mla_indexer.hpp"
#include "fa_merge_states.hpp"
#include "fa_mla_cache_io.hpp"
#include "flash_attn_gfx950.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

fa::TStride conv(const fa_strides& s) { return fa::TStride{s.batch, s.row, s.head}; }

fa_strides contiguous_bshd(int64_t s, int64_t h, int64_t d) { return fa_strides{s * h * d, h * d, d}; }

// Rows must be 16-byte aligned for the 128-bit loads; one sequence of one batch entry must fit
// a 32-bit byte offset (the kernels address rows through buffer descriptors).
int check_tensor(const char* name, const void* ptr, const fa_strides& st, int64_t rows, int d, bool varlen) {
    if (ptr == nullptr) return fail(FA_ERR_NULL_POINTER, "%s is NULL", name);
    if (((uintptr_t)ptr & 15) != 0) return fail(FA_ERR_BAD_STRIDE, "%s base pointer must be 16-byte aligned", name);
    if (st.row < d || st.head < 0 || (st.row % 8) != 0 || (st.head % 8) != 0 || (!varlen && (st.batch % 8) != 0))
        return fail(FA_ERR_BAD_STRIDE, "%s strides (batch=%lld,row=%lld,head=%lld) must be multiples of 8 elements with row >= head_dim",
                    name, (long long)st.batch, (long long)st.row, (long long)st.head);
    if (rows * st.row * 2 >= ((int64_t)1 << 31))
        return fail(FA_ERR_BAD_STRIDE, "%s: one sequence spans %lld bytes (limit 2^31)", name, (long long)(rows * st.row * 2));
    return FA_OK;
}

// The same for an 8-bit (e4m3) cache, strides in 1-byte elements: the kernels keep 16-byte loads, so everything is a multiple of 16 elements.
int check_cache8(const char* name, const void* ptr, const fa_strides& st, int64_t rows, int d) {
    if (ptr == nullptr) return fail(FA_ERR_NULL_POINTER, "%s is NULL", name);
    if (((uintptr_t)ptr & 15) != 0) return fail(FA_ERR_BAD_STRIDE, "%s base pointer must be 16-byte aligned", name);
    if (st.row < d || st.head < 0 || (st.row % 16) != 0 || (st.head % 16) != 0 || (st.batch % 16) != 0)
        return fail(FA_ERR_BAD_STRIDE, "%s (8-bit cache) strides (batch=%lld,row=%lld,head=%lld) must be multiples of 16 elements (16-byte loads) with row >= head_dim",
                    name, (long long)st.batch, (long long)st.row, (long long)st.head);
    if (rows * st.row >= ((int64_t)1 << 31))
        return fail(FA_ERR_BAD_STRIDE, "%s: one sequence spans %lld bytes (limit 2^31)", name, (long long)(rows * st.row));
    return FA_OK;
}

// ---- rules that several entry points share: each is stated once, and an entry point calls it at ITS place in ITS order of checks.  The code, the words and
// the place of a refusal are part of the interface (callers and tests match on them); where the entry points differ, the difference is an argument.

int check_dtype(int dtype) {
    if (dtype != FA_FP16 && dtype != FA_BF16) return fail(FA_ERR_BAD_DTYPE, "dtype %d unsupported (0=fp16, 1=bf16)", dtype);
    return FA_OK;
}

int check_num_splits(int num_splits) {
    if (num_splits < 0) return fail(FA_ERR_BAD_SHAPE, "num_splits must be >= 0 (0 = the library's choice), got %d", num_splits);
    return FA_OK;
}

// The workspace pair.  empty_unaligned: fa_bwd_params does not look at the pointer of an empty workspace; the decode structs refuse a misaligned one of any size.
int check_workspace(const void* workspace, int64_t workspace_bytes, bool empty_unaligned = false) {
    if (workspace_bytes < 0) return fail(FA_ERR_BAD_SHAPE, "workspace_bytes must be >= 0");
    if (workspace != nullptr && !(empty_unaligned && workspace_bytes == 0) && (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return fail(FA_ERR_BAD_STRIDE, "workspace must be 16-byte aligned");
    return FA_OK;
}

// dflt: what 0 stands for, in the struct's own words ("576 ** -0.5")
int check_softmax_scale(float softmax_scale, const char* dflt) {
    if (!(softmax_scale >= 0.f) || isinf(softmax_scale))
        return fail(FA_ERR_BAD_SHAPE, "softmax_scale %g must be finite and > 0 (0 = the default %s)", (double)softmax_scale, dflt);
    return FA_OK;
}

// A reserved field.  code: FA_ERR_BAD_ABI in fa_mla_params and fa_mla_sparse_params, FA_ERR_BAD_SHAPE in the structs that came after them - as each shipped.
int check_reserved(int64_t reserved, const char* what, int code) {
    if (reserved != 0) return fail(code, "%s: reserved_ is not zero (a field of a newer header that this library does not know)", what);
    return FA_OK;
}

// Both cu_seqlens or neither.  prefill_words: the MLA prefill structs name the missing one and check the alignment; fa_fwd_params / fa_bwd_params do neither.
int check_cu_seqlens(const int32_t* cu_q, const int32_t* cu_k, bool prefill_words) {
    if (cu_q == nullptr && cu_k == nullptr) return FA_OK;
    if (!prefill_words) {
        if (cu_q == nullptr || cu_k == nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_q and cu_seqlens_k must both be given for varlen");
        return FA_OK;
    }
    if (cu_q == nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_q is NULL but cu_seqlens_k is given (both or neither)");
    if (cu_k == nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_k is NULL but cu_seqlens_q is given (both or neither)");
    if (((reinterpret_cast<uintptr_t>(cu_q) | reinterpret_cast<uintptr_t>(cu_k)) & 3u) != 0)
        return fail(FA_ERR_BAD_STRIDE, "cu_seqlens_q / cu_seqlens_k must be 4-byte aligned");
    return FA_OK;
}

// The paged-cache fields of fa_kvcache_params, fa_mla_params, fa_mla_sparse_params and fa_mla_indexer_params (block_table = NULL: a contiguous cache)
int check_paged(const int32_t* block_table, int64_t block_table_stride, int page_block_size, int num_blocks, int seqlen_cache) {
    const int P = page_block_size;
    if (block_table == nullptr) {
        if (P != 0) return fail(FA_ERR_NULL_POINTER, "page_block_size = %d given without block_table", P);
        return FA_OK;
    }
    if (P == 0) return fail(FA_ERR_BAD_SHAPE, "block_table given without page_block_size");
    if (P < 0 || P % 16 != 0) return fail(FA_ERR_BAD_SHAPE, "page_block_size %d must be a positive multiple of 16", P);
    if (num_blocks < 1) return fail(FA_ERR_BAD_SHAPE, "num_blocks %d: a paged cache needs at least one page", num_blocks);
    if (seqlen_cache <= 0 || seqlen_cache % P != 0)
        return fail(FA_ERR_BAD_SHAPE, "seqlen_cache (%d) must be a positive multiple of page_block_size (%d) with block_table", seqlen_cache, P);
    if (block_table_stride < seqlen_cache / P)
        return fail(FA_ERR_BAD_STRIDE, "block_table_stride %lld is below the table's %d columns (seqlen_cache / page_block_size)", (long long)block_table_stride, seqlen_cache / P);
    if ((reinterpret_cast<uintptr_t>(block_table) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "block_table must be 4-byte aligned");
    return FA_OK;
}

// kvcache: the decode call, which has head_dim 256 as well (fa_fwd_kvcache_d256.hip); fwd / bwd / varlen have 64 and 128
int check_common(int b, int sq, int sk, int h, int hk, int d, int dtype, bool kvcache = false) {
    if (b < 0 || sq < 0 || sk < 0 || h <= 0 || hk <= 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d seqlen_k=%d h=%d h_k=%d", b, sq, sk, h, hk);
    if (h % hk != 0) return fail(FA_ERR_BAD_GQA, "num_heads_q (%d) must be divisible by num_heads_k (%d) for GQA/MQA", h, hk);
    if (kvcache) {
        if (d != 64 && d != 128 && d != 256) return fail(FA_ERR_BAD_HEADDIM, "head_dim %d unsupported (64, 128 or 256 over a KV cache)", d);
    } else if (d != 64 && d != 128) return fail(FA_ERR_BAD_HEADDIM, "head_dim %d unsupported (64 or 128)", d);
    return check_dtype(dtype);
}

// The head of every import_* form below: the pointer and the magic.  init_words: the one-size structs (import_exact) word a wrong magic in their own way.
template <typename P>
int check_header(const P* user, const char* what, bool init_words = false) {
    if (user == nullptr) return fail(FA_ERR_NULL_POINTER, "params is NULL");
    if (user->magic == FA_PARAMS_MAGIC) return FA_OK;
    if (init_words)
        return fail(FA_ERR_BAD_ABI, "%s: magic is not FA_PARAMS_MAGIC - no {struct_size, magic} header; initialise the struct with FA_PARAMS_INIT (ABI %d)", what, FA_ABI_VERSION);
    return fail(FA_ERR_BAD_ABI, "%s: no {struct_size, magic} header - caller was compiled against an ABI < 4 header; recompile against include/flash_attn_gfx950.h (ABI %d)",
                what, FA_ABI_VERSION);
}

// ABI 4: the caller's struct -> a zeroed local one, min(caller's size, ours) bytes.  Fields appended after the caller's header was
// written stay 0 / NULL ("not given"); a struct without the {size, magic} header (ABI 1-3 callers) or longer than ours is an error.
template <typename P>
int import_params(const P* user, P& local, const char* what, size_t base = offsetof(P, total_q)) {   // base: everything up to the first appended (optional) field is mandatory
    if (int rc = check_header(user, what)) return rc;
    if (user->struct_size < base || user->struct_size > sizeof(P))
        return fail(FA_ERR_BAD_ABI, "%s: struct_size %u outside [%zu, %zu] - header / library mismatch", what, user->struct_size, base, sizeof(P));
    memset(&local, 0, sizeof(P));
    memcpy(&local, user, user->struct_size);
    return FA_OK;
}

// The MLA structs come in two sizes, fa_mla*_params and fa_mla*_params_v2 (kv_format appended), through one pointer: exactly those two sizes are
// accepted, and the first arrives as a _v2 with kv_format = 0.  (The layouts share their prefix: static_asserts below.)
template <typename P1, typename P2>
int import_mla(const P1* user, P2& local, const char* what) {
    static_assert(sizeof(P2) == sizeof(P1) + 8 && offsetof(P2, kv_format) == sizeof(P1), "the _v2 struct is the first one with two int32 appended");
    if (int rc = check_header(user, what)) return rc;
    if (user->struct_size != sizeof(P1) && user->struct_size != sizeof(P2))
        return fail(FA_ERR_BAD_ABI, "%s: struct_size %u is neither %zu nor %zu (%s_v2) - header / library mismatch", what, user->struct_size, sizeof(P1), sizeof(P2), what);
    memset(&local, 0, sizeof(P2));
    memcpy(&local, user, user->struct_size);
    return FA_OK;
}

// The indexer structs (fa_mla_indexer_params, fa_mla_topk_params) have one size each: struct_size must be it.
template <typename P>
int import_exact(const P* user, P& local, const char* what) {
    if (int rc = check_header(user, what, true)) return rc;
    if (user->struct_size != sizeof(P))
        return fail(FA_ERR_BAD_ABI, "%s: struct_size %u is not %zu - header / library mismatch", what, user->struct_size, sizeof(P));
    memcpy(&local, user, sizeof(P));
    return FA_OK;
}

int check_mla_format(int32_t kv_format, int32_t reserved2) {
    if (kv_format != FA_MLA_KV_16BIT && kv_format != FA_MLA_KV_FP8_ROWS656)
        return fail(FA_ERR_BAD_SHAPE, "kv_format %d unknown (0 = a 16-bit latent cache, 1 = FP8 rows of 656 bytes)", kv_format);
    if (reserved2 != 0) return fail(FA_ERR_BAD_SHAPE, "reserved2_ is not zero (%d)", reserved2);
    return FA_OK;
}

// kv_cache of kv_format = FA_MLA_KV_FP8_ROWS656: strides in bytes, 16-byte loads and stores; one sequence (one page) fits a 32-bit byte offset
int check_mla_cache8(const void* ptr, const fa_strides& st, int64_t rows) {
    if (ptr == nullptr) return fail(FA_ERR_NULL_POINTER, "kv_cache is NULL");
    if (((uintptr_t)ptr & 15) != 0) return fail(FA_ERR_BAD_STRIDE, "kv_cache base pointer must be 16-byte aligned");
    if (st.row < 656 || (st.row % 16) != 0 || (st.batch % 16) != 0)
        return fail(FA_ERR_BAD_STRIDE, "kv_cache (FP8 rows of 656 bytes) strides (batch=%lld,row=%lld) must be multiples of 16 bytes with row >= 656", (long long)st.batch,
                    (long long)st.row);
    if (rows * st.row >= ((int64_t)1 << 31)) return fail(FA_ERR_BAD_STRIDE, "kv_cache: one sequence spans %lld bytes (limit 2^31)", (long long)(rows * st.row));
    return FA_OK;
}

template <typename K>
void set_scale(K& kp, float scale) {
    kp.scale = scale;
    kp.scale_log2e = scale * 1.4426950408889634f;
}

// p.block_table (NULL = contiguous: the four fields stay 0) -> kp
template <typename P>
void fill_paged(const P& p, fa::KvcacheKernelParams& kp) {
    if (p.block_table == nullptr) return;
    kp.block_table = p.block_table; kp.bt_stride = p.block_table_stride;
    kp.page_size = p.page_block_size; kp.num_blocks = p.num_blocks;
}

// ---- what fa_mla_params and fa_mla_sparse_params share (P: the _v2 form of either): fill_mla / fill_mla_sparse call these between their own checks
int check_mla_dims(int d_qk, int d_v, int dtype) {
    if (d_qk != 576) return fail(FA_ERR_BAD_HEADDIM, "d_qk %d unsupported (the latent row is 576 wide: 512 compressed + 64 rope elements)", d_qk);
    if (d_v != 512) return fail(FA_ERR_BAD_HEADDIM, "d_v %d unsupported (the value is the first 512 elements of the latent row)", d_v);
    return check_dtype(dtype);
}

// num_splits, softmax_scale, reserved_, kv_format / reserved2_, then the workspace pair (with_workspace = false: not looked at).  what: the struct, for reserved_
template <typename P>
int check_mla_tail(const P& p, const char* what, bool with_workspace) {
    int rc;
    if ((rc = check_num_splits(p.num_splits))) return rc;
    if ((rc = check_softmax_scale(p.softmax_scale, "576 ** -0.5"))) return rc;
    if ((rc = check_reserved(p.reserved_, what, FA_ERR_BAD_ABI))) return rc;
    if ((rc = check_mla_format(p.kv_format, p.reserved2_))) return rc;
    return with_workspace ? check_workspace(p.workspace, p.workspace_bytes) : FA_OK;
}

// kv_cache under kv_format.  kvc: kv_cache_stride with head = 0 (one KV head).  Paged: the descriptors span at most one page, so the 2^31-byte limit applies per
// page (page offsets are 64-bit); contiguous: one descriptor per sequence
template <typename P>
int check_mla_cache(const P& p, const fa_strides& kvc) {
    const int64_t rows = p.block_table != nullptr ? p.page_block_size : p.seqlen_cache;
    if (p.kv_format == FA_MLA_KV_FP8_ROWS656) return check_mla_cache8(p.kv_cache, kvc, rows);
    return check_tensor("kv_cache", p.kv_cache, kvc, rows, p.d_qk, false);
}

// The fields of a zeroed kp that both structs state alike: q, the cache (key and value are the same rows), o, lse, lengths, sizes, one KV head, scale, paging.
// kp.d = 512 is the width of V, of o and of the partial planes.
template <typename P>
void fill_mla_kp(const P& p, const fa_strides& kvc, fa::KvcacheKernelParams& kp) {
    kp.q_ptr = p.q; kp.k_cache = kp.v_cache = const_cast<void*>(static_cast<const void*>(p.kv_cache));
    kp.o_ptr = p.o; kp.lse_ptr = p.lse; kp.cache_seqlens = p.cache_seqlens;
    kp.q = conv(p.q_stride); kp.kc = kp.vc = conv(kvc); kp.o = conv(p.o_stride);
    kp.b = p.b; kp.seqlen_q = p.seqlen_q; kp.seqlen_cache = p.seqlen_cache;
    kp.h = p.h; kp.h_k = 1; kp.h_ratio = p.h; kp.d = p.d_v;
    kp.cache_fp8 = p.kv_format == FA_MLA_KV_FP8_ROWS656 ? 1 : 0;     // kc / vc are in bytes then
    set_scale(kp, p.softmax_scale > 0.f ? p.softmax_scale : 1.0f / sqrtf((float)p.d_qk));
    fill_paged(p, kp);
}

// The split of an MLA decode call (kp: the dense call's own, the sparse call's `split` copy).  sized = false: without a limit, what the workspace query sizes for
template <typename P>
int32_t mla_split(const fa::KvcacheKernelParams& kp, const P& local, bool sized) {
    const int64_t avail = !sized ? -1 : local.workspace != nullptr ? local.workspace_bytes : 0;
    return fa::kvcache_split(kp, avail, local.num_splits, -1, fa::kKvcPrefillRows);
}

// ---- what the MLA prefill forward and backward share
// What fa_mla_prefill_params and fa_mla_prefill_bwd_params (P) check alike and first: sizes, GQA, widths, dtype, cu_seqlens, softmax_scale, the packed totals.
// Behind it a call is packed iff cu_seqlens_q is given.
template <typename P>
int check_mla_prefill_front(const P& p) {
    if (p.b < 0 || p.seqlen_q < 0 || p.seqlen_k < 0 || p.h <= 0 || p.h_k <= 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d seqlen_k=%d h=%d h_k=%d", p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k);
    if (p.h % p.h_k != 0) return fail(FA_ERR_BAD_GQA, "h (%d) must be divisible by h_k (%d) for GQA/MQA", p.h, p.h_k);
    if (p.d_qk != 192) return fail(FA_ERR_BAD_HEADDIM, "d_qk %d unsupported (q and k are 192 wide: 128 no-rope + 64 rope elements)", p.d_qk);
    if (p.d_v != 128) return fail(FA_ERR_BAD_HEADDIM, "d_v %d unsupported (v and o are 128 wide)", p.d_v);
    int rc;
    if ((rc = check_dtype(p.dtype))) return rc;
    if ((rc = check_cu_seqlens(p.cu_seqlens_q, p.cu_seqlens_k, true))) return rc;
    if ((rc = check_softmax_scale(p.softmax_scale, "192 ** -0.5"))) return rc;
    if (p.cu_seqlens_q != nullptr && (p.total_q < 0 || p.total_k < 0))
        return fail(FA_ERR_BAD_SHAPE, "total_q (%lld) / total_k (%lld) must be >= 0 with cu_seqlens", (long long)p.total_q, (long long)p.total_k);
    return FA_OK;
}

// The launch grids: h_k x tiles (dense: per batch entry; packed: of all rows, plus one slot per sequence), counted in tiles of 64 - the smaller of the two row
// tiles fa_fwd_mla_prefill.hip can be built with - and a packed row index is an int.  key_grid: the backward's dK / dV launch runs over key tiles as well.
template <typename P>
int check_mla_prefill_grid(const P& p, bool key_grid) {
    const bool packed = p.cu_seqlens_q != nullptr;
    const int64_t rows_q = packed ? p.total_q : p.seqlen_q, rows_k = packed ? p.total_k : p.seqlen_k, h_ratio = p.h / p.h_k;
    auto grid = [&](int64_t rows) {
        const int64_t tiles = (rows + fa::kKvcPrefillRows - 1) / fa::kKvcPrefillRows;
        return (packed ? tiles + p.b : tiles * p.b) * p.h_k;
    };
    if (rows_q * h_ratio >= ((int64_t)1 << 31) || rows_k >= ((int64_t)1 << 31) || grid(rows_q * h_ratio) >= ((int64_t)1 << 31) || (key_grid && grid(rows_k) >= ((int64_t)1 << 31)))
        return fail(FA_ERR_BAD_SHAPE, "call too large: b = %d sequences, %lld query rows x h = %d heads, %lld keys exceed the launch grid", p.b, (long long)rows_q, p.h,
                    (long long)rows_k);
    return FA_OK;
}

// The fields that MlaPrefillParams and MlaPrefillBwdParams (K, zeroed) name alike: q / k / v / o / lse, cu_seqlens, sizes, the scale
template <typename P, typename K>
void fill_mla_prefill_kp(const P& p, K& kp) {
    const bool packed = p.cu_seqlens_q != nullptr;
    kp.q_ptr = p.q; kp.k_ptr = p.k; kp.v_ptr = p.v; kp.o_ptr = p.o; kp.lse_ptr = p.lse;
    kp.cu_q = p.cu_seqlens_q; kp.cu_k = p.cu_seqlens_k;
    kp.q = conv(p.q_stride); kp.k = conv(p.k_stride); kp.v = conv(p.v_stride); kp.o = conv(p.o_stride);
    kp.b = p.b; kp.seqlen_q = p.seqlen_q; kp.seqlen_k = p.seqlen_k;
    kp.h = p.h; kp.h_k = p.h_k; kp.h_ratio = p.h / p.h_k;
    kp.is_causal = p.is_causal ? 1 : 0;
    kp.total_q = packed ? p.total_q : 0; kp.total_k = packed ? p.total_k : 0;
    set_scale(kp, p.softmax_scale > 0.f ? p.softmax_scale : 1.0f / sqrtf((float)p.d_qk));        // (the default = 192 ** -0.5 rounded once to fp32)
}

// k_idx_cache of fa_mla_indexer_params and fa_mla_index_cache_append_params (P): strides in bytes (FA_IDX_K_FP8_E4M3) or elements, 16-byte accesses either way
template <typename P>
int check_idx_cache(const P& p) {
    const bool fp8 = p.k_format == FA_IDX_K_FP8_E4M3, paged = p.block_table != nullptr;
    const int es = fp8 ? 1 : 2, unit = 16 / es;
    if (p.k_idx_cache == nullptr) return fail(FA_ERR_NULL_POINTER, "k_idx_cache is NULL");
    if ((reinterpret_cast<uintptr_t>(p.k_idx_cache) & 15u) != 0) return fail(FA_ERR_BAD_STRIDE, "k_idx_cache base pointer must be 16-byte aligned");
    if (p.k_cache_row_stride < fa::kIdxD || p.k_cache_row_stride % unit != 0 || p.k_cache_batch_stride % unit != 0 || p.k_cache_batch_stride < 0)
        return fail(FA_ERR_BAD_STRIDE, "k_idx_cache strides (k_cache_batch_stride=%lld, k_cache_row_stride=%lld) must be multiples of %d %s (16-byte loads) with rows at least 128 apart",
                    (long long)p.k_cache_batch_stride, (long long)p.k_cache_row_stride, unit, fp8 ? "bytes" : "elements");
    // one descriptor per sequence (per page): below 2^31 bytes, the prefetched step past the end included
    const int64_t span = ((int64_t)(paged ? p.page_block_size : p.seqlen_cache) + 2 * fa::kIdxStep) * p.k_cache_row_stride * es;
    if (span >= ((int64_t)1 << 31)) return fail(FA_ERR_BAD_STRIDE, "k_idx_cache: one %s spans %lld bytes (limit 2^31)", paged ? "page" : "sequence", (long long)span);
    return FA_OK;
}

// ---- what the three cache-io structs (fa_mla_cache_append_params, fa_mla_cache_gather_params, fa_mla_index_cache_append_params) share
// Sizes, the form (dense rows / packed total under cu) and the grid.  rows, total, cu: the struct's own fields under their own names.  Returns through n_rows the
// rows of the launch (0: nothing to move).
int check_io_rows(int b, int seqlen_cache, const char* rows_name, int rows, const char* total_name, int64_t total, const char* cu_name, const int32_t* cu,
                  int64_t& n_rows) {
    if (b < 0 || seqlen_cache < 0 || rows < 0) return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d %s=%d seqlen_cache=%d", b, rows_name, rows, seqlen_cache);
    if (cu != nullptr) {
        if (total < 0) return fail(FA_ERR_BAD_SHAPE, "%s (%lld) must be >= 0 with %s", total_name, (long long)total, cu_name);
        if ((reinterpret_cast<uintptr_t>(cu) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "%s must be 4-byte aligned", cu_name);
    }
    n_rows = cu != nullptr ? total : (int64_t)b * rows;
    if (n_rows >= ((int64_t)1 << 31)) return fail(FA_ERR_BAD_SHAPE, "call too large: %lld rows exceed the launch grid", (long long)n_rows);
    if (b == 0) n_rows = 0;
    return FA_OK;
}

// A 16-bit row tensor the movers address with 16-byte accesses through 64-bit offsets (no extent rule): strides in elements.  width: the least row stride (0: any)
int check_io_rows16(const char* name, const void* ptr, int64_t batch, int64_t row, int width, bool dense) {
    if (ptr == nullptr) return fail(FA_ERR_NULL_POINTER, "%s is NULL", name);
    if (((uintptr_t)ptr & 15) != 0) return fail(FA_ERR_BAD_STRIDE, "%s base pointer must be 16-byte aligned", name);
    if ((row % 8) != 0 || row < width || (dense && (batch % 8) != 0))
        return fail(FA_ERR_BAD_STRIDE, "%s strides (batch=%lld,row=%lld) must be multiples of 8 elements%s", name, (long long)batch, (long long)row,
                    width ? " with rows at least their width apart" : "");
    return FA_OK;
}

// The latent cache of the append and the gather (P): kv_format, then the view under it, the rules of fa_mla_params_v2
template <typename P>
int check_io_latent_cache(const P& p) {
    fa_strides kvc = p.kv_cache_stride;
    kvc.head = 0;
    const int64_t rows = p.block_table != nullptr ? p.page_block_size : p.seqlen_cache;
    if (p.kv_format == FA_MLA_KV_FP8_ROWS656) return check_mla_cache8(p.kv_cache, kvc, rows);
    return check_tensor("kv_cache", p.kv_cache, kvc, rows, 576, false);
}

// cache_seqlens / block_table / the cache view of a zeroed MlaCacheIoParams.  es: bytes per unit of the cache strides
template <typename P>
void fill_io_cache(const P& p, const void* cache, int64_t batch, int64_t row, int es, fa::MlaCacheIoParams& io) {
    io.cache = const_cast<void*>(cache); io.c_batch = batch * es; io.c_row = row * es;
    io.cache_seqlens = p.cache_seqlens; io.b = p.b; io.seqlen_cache = p.seqlen_cache;
    if (p.block_table != nullptr) {
        io.block_table = p.block_table; io.bt_stride = p.block_table_stride; io.page_size = p.page_block_size; io.num_blocks = p.num_blocks;
    }
}

int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return FA_OK;
    fail((int)e, "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

}  // namespace

extern "C" {

int fa_abi_version(void) { return FA_ABI_VERSION; }
const char* fa_last_error(void) { return g_err; }

#define FA_STR2(x) #x
#define FA_STR(x) FA_STR2(x)
#ifndef FA_SOURCE_DIGEST
#define FA_SOURCE_DIGEST "unstamped"      // build.py passes the first 12 hex digits of the sha256 over kernel sources, headers and flags
#endif
const char* fa_build_info(void) { return "flash_attn_gfx950 abi=" FA_STR(FA_ABI_VERSION) " arch=gfx950 mfma=32x32x16+16x16x32 wave64 src=" FA_SOURCE_DIGEST " built " __DATE__; }

double fa_fwd_flops(int32_t b, int32_t sq, int32_t sk, int32_t h, int32_t d, int32_t is_causal) {
    double pairs;
    if (!is_causal) {
        pairs = (double)sq * (double)sk;
    } else {
        // visible (i, j) pairs with j <= i + (sk - sq), 0 <= j < sk
        const int64_t delta = (int64_t)sk - sq;
        double acc = 0.0;
        // rows i with i + delta < 0 see nothing; rows with i + delta >= sk-1 see sk
        int64_t i0 = delta < 0 ? -delta : 0;        // first row that sees key 0
        if (i0 < sq) {
            int64_t n = sq - i0;                     // rows i0..sq-1 see (i + delta + 1) keys (<= sk always since i<=sq-1)
            double first = (double)(i0 + delta + 1), last = (double)(sq - 1 + delta + 1);
            acc = (first + last) * (double)n / 2.0;
        }
        pairs = acc;
    }
    return 4.0 * (double)b * (double)h * pairs * (double)d;
}

double fa_fwd_bytes(int32_t b, int32_t sq, int32_t sk, int32_t h, int32_t hk, int32_t d) {
    return 2.0 * ((double)b * sq * h * d * 2.0 + (double)b * sk * hk * d * 2.0) + (double)b * h * sq * 4.0;
}

const char* fa_fwd_kernel_name(int32_t d) { return fa::fwd_kernel_name(d); }
int32_t fa_set_kernel_policy(int32_t policy) { return fa::set_kernel_policy(policy); }
int64_t fa_set_policy_problem_heads(int64_t batch_times_heads) { return fa::set_policy_problem_heads(batch_times_heads); }
const char* fa_kernel_name(int32_t stage, int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t d, int32_t is_causal) {
    return fa_kernel_name_dtype(stage, FA_FP16, b, seqlen_q, seqlen_k, h, d, is_causal);
}
const char* fa_kernel_name_dtype(int32_t stage, int32_t dtype, int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t d, int32_t is_causal) {
    if (dtype != FA_FP16 && dtype != FA_BF16) return "";
    if (stage == FA_STAGE_FWD) {
        fa::FwdKernelParams kp{};
        kp.b = b; kp.seqlen_q = seqlen_q; kp.seqlen_k = seqlen_k; kp.h = h; kp.d = d; kp.is_causal = is_causal;
        return fa::fwd_kernel_name_for(kp, dtype);
    }
    if (stage != FA_STAGE_DQ && stage != FA_STAGE_DKDV) return "";
    fa::BwdKernelParams kp{};
    kp.b = b; kp.seqlen_q = seqlen_q; kp.seqlen_k = seqlen_k; kp.h = h; kp.d = d; kp.is_causal = is_causal;
    return fa::bwd_kernel_name_for(kp, stage == FA_STAGE_DKDV);
}

int fa_device_clock_khz(int32_t device) {
    int khz = 0;
    const hipError_t e = hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device);
    return e == hipSuccess ? khz : -(int)e;
}

int fa_run_mha_fwd(const fa_fwd_params* user, void* stream) {
    fa_fwd_params local;
    int rc = import_params(user, local, "fa_fwd_params");
    if (rc) return rc;
    const fa_fwd_params* p = &local;
    rc = check_common(p->b, p->seqlen_q, p->seqlen_k, p->h, p->h_k, p->d, p->dtype);
    if (rc) return rc;
    const bool varlen = p->cu_seqlens_q != nullptr || p->cu_seqlens_k != nullptr;
    if ((rc = check_cu_seqlens(p->cu_seqlens_q, p->cu_seqlens_k, false))) return rc;
    if (p->b == 0 || p->seqlen_q == 0) return FA_OK;   // nothing to write
    if (p->lse == nullptr) return fail(FA_ERR_NULL_POINTER, "lse is NULL");
    if ((rc = check_tensor("q", p->q, p->q_stride, p->seqlen_q, p->d, varlen))) return rc;
    if ((rc = check_tensor("o", p->o, p->o_stride, p->seqlen_q, p->d, varlen))) return rc;
    if (p->seqlen_k > 0) {
        if ((rc = check_tensor("k", p->k, p->k_stride, p->seqlen_k, p->d, varlen))) return rc;
        if ((rc = check_tensor("v", p->v, p->v_stride, p->seqlen_k, p->d, varlen))) return rc;
    }
    fa::FwdKernelParams kp;
    memset(&kp, 0, sizeof(kp));
    kp.q_ptr = p->q; kp.k_ptr = p->k; kp.v_ptr = p->v; kp.o_ptr = p->o; kp.lse_ptr = p->lse;
    kp.cu_seqlens_q = p->cu_seqlens_q; kp.cu_seqlens_k = p->cu_seqlens_k;
    kp.q = conv(p->q_stride); kp.k = conv(p->k_stride); kp.v = conv(p->v_stride); kp.o = conv(p->o_stride);
    kp.lse_row_stride = p->seqlen_q;
    kp.b = p->b; kp.seqlen_q = p->seqlen_q; kp.seqlen_k = p->seqlen_k;
    kp.h = p->h; kp.h_k = p->h_k; kp.h_ratio = p->h / p->h_k; kp.d = p->d;
    kp.is_causal = p->is_causal ? 1 : 0;
    if (p->total_q < 0 || p->total_k < 0) return fail(FA_ERR_BAD_SHAPE, "total_q / total_k must be >= 0 (0 = unknown)");
    kp.total_q = varlen ? p->total_q : 0;          // sizes the varlen launch grid by the tokens present (fa_device.hpp)
    set_scale(kp, 1.0f / sqrtf((float)p->d));      // hard-wired like the reference (flash_fwd_kernel.h:351)
    return hip_status(fa::launch_fwd(kp, p->dtype, (hipStream_t)stream), "fa_fwd launch");
}

// with_workspace = false: the `workspace` fields are not looked at (fa_bwd_workspace_bytes, and the launches that never use it)
static int fill_bwd(const fa_bwd_params* user, fa::BwdKernelParams& kp, fa_bwd_params& local, bool with_workspace) {
    int rc = import_params(user, local, "fa_bwd_params");
    if (rc) return rc;
    const fa_bwd_params* p = &local;
    rc = check_common(p->b, p->seqlen_q, p->seqlen_k, p->h, p->h_k, p->d, p->dtype);
    if (rc) return rc;
    const bool varlen = p->cu_seqlens_q != nullptr || p->cu_seqlens_k != nullptr;
    if ((rc = check_cu_seqlens(p->cu_seqlens_q, p->cu_seqlens_k, false))) return rc;
    if (p->b > 0 && p->seqlen_q > 0) {
        if (p->lse == nullptr || p->dsoftmax_sum == nullptr) return fail(FA_ERR_NULL_POINTER, "lse / dsoftmax_sum is NULL");
        if ((rc = check_tensor("q", p->q, p->q_stride, p->seqlen_q, p->d, varlen))) return rc;
        if ((rc = check_tensor("o", p->o, p->o_stride, p->seqlen_q, p->d, varlen))) return rc;
        if ((rc = check_tensor("dout", p->dout, p->do_stride, p->seqlen_q, p->d, varlen))) return rc;
        if ((rc = check_tensor("dq", p->dq, p->dq_stride, p->seqlen_q, p->d, varlen))) return rc;
    }
    if (p->b > 0 && p->seqlen_k > 0) {
        if ((rc = check_tensor("k", p->k, p->k_stride, p->seqlen_k, p->d, varlen))) return rc;
        if ((rc = check_tensor("v", p->v, p->v_stride, p->seqlen_k, p->d, varlen))) return rc;
        if ((rc = check_tensor("dk", p->dk, p->dk_stride, p->seqlen_k, p->d, varlen))) return rc;
        if ((rc = check_tensor("dv", p->dv, p->dv_stride, p->seqlen_k, p->d, varlen))) return rc;
    }
    memset(&kp, 0, sizeof(kp));
    kp.q_ptr = p->q; kp.k_ptr = p->k; kp.v_ptr = p->v; kp.o_ptr = p->o; kp.do_ptr = p->dout;
    kp.lse_ptr = p->lse; kp.dsum_ptr = p->dsoftmax_sum;
    kp.dq_ptr = p->dq; kp.dk_ptr = p->dk; kp.dv_ptr = p->dv;
    kp.cu_seqlens_q = p->cu_seqlens_q; kp.cu_seqlens_k = p->cu_seqlens_k;
    kp.q = conv(p->q_stride); kp.k = conv(p->k_stride); kp.v = conv(p->v_stride); kp.o = conv(p->o_stride);
    kp.dout = conv(p->do_stride); kp.dq = conv(p->dq_stride); kp.dk = conv(p->dk_stride); kp.dv = conv(p->dv_stride);
    kp.lse_row_stride = p->seqlen_q;
    kp.b = p->b; kp.seqlen_q = p->seqlen_q; kp.seqlen_k = p->seqlen_k;
    kp.h = p->h; kp.h_k = p->h_k; kp.h_ratio = p->h / p->h_k; kp.d = p->d;
    kp.is_causal = p->is_causal ? 1 : 0;
    if (p->total_q < 0 || p->total_k < 0) return fail(FA_ERR_BAD_SHAPE, "total_q / total_k must be >= 0 (0 = unknown)");
    if (p->cu_seqlens_q != nullptr) { kp.total_q = p->total_q; kp.total_k = p->total_k; }
    set_scale(kp, 1.0f / sqrtf((float)p->d));
    if (with_workspace && (rc = check_workspace(p->workspace, p->workspace_bytes, true))) return rc;
    if (with_workspace && p->workspace != nullptr && p->workspace_bytes > 0) { kp.ws = (float*)p->workspace; kp.ws_bytes = p->workspace_bytes; }
    kp.n_split = 1;
    return FA_OK;
}

int64_t fa_bwd_workspace_bytes(const fa_bwd_params* user) {
    fa::BwdKernelParams kp;
    fa_bwd_params local;
    int rc = fill_bwd(user, kp, local, false);
    if (rc) return rc;
    const fa_bwd_params* p = &local;
    if (p->b == 0 || p->seqlen_k == 0 || p->seqlen_q == 0) return 0;
    return fa::dkdv_workspace_bytes(kp, fa::dkdv_split(kp, -1));
}

int fa_bwd_dot_do_o(const fa_bwd_params* user, void* stream) {
    fa::BwdKernelParams kp;
    fa_bwd_params local;
    int rc = fill_bwd(user, kp, local, false);
    if (rc) return rc;
    const fa_bwd_params* p = &local;
    if (p->b == 0 || p->seqlen_q == 0) return FA_OK;
    return hip_status(fa::launch_bwd_dot_do_o(kp, p->dtype, (hipStream_t)stream), "fa_bwd_dot_do_o launch");
}

int fa_bwd_dq(const fa_bwd_params* user, void* stream) {
    fa::BwdKernelParams kp;
    fa_bwd_params local;
    int rc = fill_bwd(user, kp, local, false);
    if (rc) return rc;
    const fa_bwd_params* p = &local;
    if (p->b == 0 || p->seqlen_q == 0) return FA_OK;
    return hip_status(fa::launch_bwd_dq(kp, p->dtype, (hipStream_t)stream), "fa_bwd_dq launch");
}

int fa_bwd_dkdv(const fa_bwd_params* user, void* stream) {
    fa::BwdKernelParams kp;
    fa_bwd_params local;
    int rc = fill_bwd(user, kp, local, true);
    if (rc) return rc;
    const fa_bwd_params* p = &local;
    if (p->b == 0 || p->seqlen_k == 0) return FA_OK;
    return hip_status(fa::launch_bwd_dkdv(kp, p->dtype, (hipStream_t)stream), "fa_bwd_dkdv launch");
}

int fa_run_mha_bwd(const fa_bwd_params* user, void* stream) {
    fa::BwdKernelParams kp;
    fa_bwd_params local;
    int rc = fill_bwd(user, kp, local, true);
    if (rc) return rc;
    const fa_bwd_params* p = &local;
    if (p->b == 0) return FA_OK;
    hipStream_t s = (hipStream_t)stream;
    // The reference's run_flash_bwd launches dot_do_o, dQ, dK/dV (flash_bwd_launch_template.h:69-146).  Here the dQ kernel computes
    // D = rowsum(dO * O) for its own rows in its prologue and leaves it in dsoftmax_sum for the dK/dV launch: two launches, same
    // stream, no host sync in between.  (fa_bwd_dot_do_o stays available as a stand-alone entry point.)
    if (p->seqlen_q > 0) {
        if ((rc = hip_status(fa::launch_bwd_dq(kp, p->dtype, s), "fa_bwd_dq launch"))) return rc;
    }
    if (p->seqlen_k > 0) {
        if ((rc = hip_status(fa::launch_bwd_dkdv(kp, p->dtype, s), "fa_bwd_dkdv launch"))) return rc;
    }
    return FA_OK;
}

int fa_mha_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
               int32_t b, int32_t sq, int32_t sk, int32_t h, int32_t hk, int32_t d,
               int32_t dtype, int32_t is_causal, void* stream) {
    fa_fwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse;
    p.b = b; p.seqlen_q = sq; p.seqlen_k = sk; p.h = h; p.h_k = hk; p.d = d; p.dtype = dtype; p.is_causal = is_causal;
    p.q_stride = contiguous_bshd(sq, h, d); p.o_stride = p.q_stride;
    p.k_stride = contiguous_bshd(sk, hk, d); p.v_stride = p.k_stride;
    return fa_run_mha_fwd(&p, stream);
}

int fa_mha_varlen_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                      const int32_t* cu_q, const int32_t* cu_k,
                      int32_t b, int32_t max_sq, int32_t max_sk, int32_t h, int32_t hk, int32_t d,
                      int32_t dtype, int32_t is_causal, void* stream) {
    if (cu_q == nullptr || cu_k == nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_q/cu_seqlens_k must not be NULL");
    fa_fwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse; p.cu_seqlens_q = cu_q; p.cu_seqlens_k = cu_k;
    p.b = b; p.seqlen_q = max_sq; p.seqlen_k = max_sk; p.h = h; p.h_k = hk; p.d = d; p.dtype = dtype; p.is_causal = is_causal;
    p.q_stride = fa_strides{0, (int64_t)h * d, d}; p.o_stride = p.q_stride;
    p.k_stride = fa_strides{0, (int64_t)hk * d, d}; p.v_stride = p.k_stride;
    return fa_run_mha_fwd(&p, stream);
}

int fa_mha_bwd(const void* q, const void* k, const void* v, const void* o, const float* lse,
               const void* dout, void* dq, void* dk, void* dv, float* dsum,
               int32_t b, int32_t sq, int32_t sk, int32_t h, int32_t hk, int32_t d,
               int32_t dtype, int32_t is_causal, void* stream) {
    fa_bwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse; p.dout = dout; p.dq = dq; p.dk = dk; p.dv = dv; p.dsoftmax_sum = dsum;
    p.b = b; p.seqlen_q = sq; p.seqlen_k = sk; p.h = h; p.h_k = hk; p.d = d; p.dtype = dtype; p.is_causal = is_causal;
    p.q_stride = contiguous_bshd(sq, h, d); p.o_stride = p.do_stride = p.dq_stride = p.q_stride;
    p.k_stride = contiguous_bshd(sk, hk, d); p.v_stride = p.dk_stride = p.dv_stride = p.k_stride;
    return fa_run_mha_bwd(&p, stream);
}

int fa_mha_varlen_bwd(const void* q, const void* k, const void* v, const void* o, const float* lse,
                      const void* dout, void* dq, void* dk, void* dv, float* dsum,
                      const int32_t* cu_q, const int32_t* cu_k,
                      int32_t b, int32_t max_sq, int32_t max_sk, int32_t h, int32_t hk, int32_t d,
                      int32_t dtype, int32_t is_causal, void* stream) {
    if (cu_q == nullptr || cu_k == nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_q/cu_seqlens_k must not be NULL");
    fa_bwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse; p.dout = dout; p.dq = dq; p.dk = dk; p.dv = dv; p.dsoftmax_sum = dsum;
    p.cu_seqlens_q = cu_q; p.cu_seqlens_k = cu_k;
    p.b = b; p.seqlen_q = max_sq; p.seqlen_k = max_sk; p.h = h; p.h_k = hk; p.d = d; p.dtype = dtype; p.is_causal = is_causal;
    p.q_stride = fa_strides{0, (int64_t)h * d, d}; p.o_stride = p.do_stride = p.dq_stride = p.q_stride;
    p.k_stride = fa_strides{0, (int64_t)hk * d, d}; p.v_stride = p.dk_stride = p.dv_stride = p.k_stride;
    return fa_run_mha_bwd(&p, stream);
}

// The options pointer of the _ex entry points -> a zeroed fa_kvcache_options_v8 filled with what the caller's struct carries: struct_size says
// which of the eight layouts it is (fa_kvcache_options: the window alone; fa_kvcache_options_v2: plus the 8-bit cache fields;
// fa_kvcache_options_v3: plus the rotary fields; fa_kvcache_options_v4: plus the ragged-batch fields; fa_kvcache_options_v5: plus softmax_scale
// and softcap; fa_kvcache_options_v6: plus the attention sinks;
// fa_kvcache_options_v7: plus the tree mask; fa_kvcache_options_v8: plus row_tile).  NULL = all zero.
static int import_kvcache_options(const fa_kvcache_options* user, fa_kvcache_options_v8& o) {
    memset(&o, 0, sizeof(o));
    if (user == nullptr) return FA_OK;
    if (user->magic != FA_PARAMS_MAGIC)
        return fail(FA_ERR_BAD_ABI, "fa_kvcache_options: no {struct_size, magic} header (FA_PARAMS_INIT); recompile against include/flash_attn_gfx950.h (ABI %d)", FA_ABI_VERSION);
    if (user->struct_size != sizeof(fa_kvcache_options) && user->struct_size != sizeof(fa_kvcache_options_v2) && user->struct_size != sizeof(fa_kvcache_options_v3) &&
        user->struct_size != sizeof(fa_kvcache_options_v4) && user->struct_size != sizeof(fa_kvcache_options_v5) && user->struct_size != sizeof(fa_kvcache_options_v6) &&
        user->struct_size != sizeof(fa_kvcache_options_v7) && user->struct_size != sizeof(fa_kvcache_options_v8))
        return fail(FA_ERR_BAD_ABI, "fa_kvcache_options: struct_size %u is none of sizeof(fa_kvcache_options) = %zu, sizeof(fa_kvcache_options_v2) = %zu, sizeof(fa_kvcache_options_v3) = %zu, sizeof(fa_kvcache_options_v4) = %zu, sizeof(fa_kvcache_options_v5) = %zu, sizeof(fa_kvcache_options_v6) = %zu, sizeof(fa_kvcache_options_v7) = %zu, sizeof(fa_kvcache_options_v8) = %zu - header / library mismatch",
                    user->struct_size, sizeof(fa_kvcache_options), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v4),
                    sizeof(fa_kvcache_options_v5), sizeof(fa_kvcache_options_v6), sizeof(fa_kvcache_options_v7), sizeof(fa_kvcache_options_v8));
    memcpy(&o, user, user->struct_size);
    if (o.cache_dtype != 0 && o.cache_dtype != FA_CACHE_FP8_E4M3)
        return fail(FA_ERR_BAD_DTYPE, "cache_dtype %d unsupported (0 = the dtype of q, %d = FA_CACHE_FP8_E4M3; e4m3fnuz and e5m2 caches are not supported)", o.cache_dtype,
                    FA_CACHE_FP8_E4M3);
    if (o.cache_dtype == 0 && (o.k_descale != nullptr || o.v_descale != nullptr))
        return fail(FA_ERR_BAD_DTYPE, "k_descale / v_descale need cache_dtype = FA_CACHE_FP8_E4M3 (a 16-bit cache has no descale)");
    return FA_OK;
}

// with_workspace = false: the `workspace` fields are not looked at (fa_kvcache_workspace_bytes)
static int fill_kvcache(const fa_kvcache_params* user, fa::KvcacheKernelParams& kp, fa_kvcache_params& local, bool with_workspace,
                        const fa_kvcache_options_v8& o) {
    // the paged-cache fields are optional: a caller built before them passes struct_size = offsetof(block_table) and gets NULL / 0
    int rc = import_params(user, local, "fa_kvcache_params", offsetof(fa_kvcache_params, block_table));
    if (rc) return rc;
    const fa_kvcache_params* p = &local;
    const bool paged = p->block_table != nullptr;
    const bool ragged = o.cu_seqlens_q != nullptr;      // q, o, k_new, v_new are packed: their batch strides are not read (seqlen_q = max_seqlen_q)
    if (p->b < 0 || p->seqlen_q < 1 || p->seqlen_cache < 0 || p->seqlen_new < 0 || p->h <= 0 || p->h_k <= 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d (>= 1) seqlen_cache=%d seqlen_new=%d h=%d h_k=%d", p->b, p->seqlen_q, p->seqlen_cache,
                    p->seqlen_new, p->h, p->h_k);
    if ((rc = check_common(p->b, p->seqlen_q, p->seqlen_cache, p->h, p->h_k, p->d, p->dtype, true))) return rc;
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    if (p->seqlen_new > p->seqlen_cache)
        return fail(FA_ERR_BAD_SHAPE, "seqlen_new (%d) exceeds the cache capacity seqlen_cache (%d)", p->seqlen_new, p->seqlen_cache);
    if ((p->k_new == nullptr) != (p->v_new == nullptr)) return fail(FA_ERR_NULL_POINTER, "k_new and v_new must both be given or both be NULL");
    if (p->k_new != nullptr && p->cache_seqlens == nullptr)
        return fail(FA_ERR_NULL_POINTER, "k_new / v_new need cache_seqlens (the rows they are appended at)");
    if (p->k_new == nullptr && p->seqlen_new != 0) return fail(FA_ERR_BAD_SHAPE, "seqlen_new = %d without k_new / v_new", p->seqlen_new);
    if ((rc = check_num_splits(p->num_splits))) return rc;
    if (with_workspace && (rc = check_workspace(p->workspace, p->workspace_bytes))) return rc;
    if (p->b > 0) {
        if (p->lse == nullptr) return fail(FA_ERR_NULL_POINTER, "lse is NULL");
        if ((rc = check_tensor("q", p->q, p->q_stride, p->seqlen_q, p->d, ragged))) return rc;
        if ((rc = check_tensor("o", p->o, p->o_stride, p->seqlen_q, p->d, ragged))) return rc;
        // paged: the descriptors span at most one page, so the 2^31-byte limit applies per page (page offsets are 64-bit)
        const int64_t cache_rows = paged ? p->page_block_size : p->seqlen_cache;
        if (o.cache_dtype == FA_CACHE_FP8_E4M3) {
            if ((rc = check_cache8("k_cache", p->k_cache, p->k_cache_stride, cache_rows, p->d))) return rc;
            if ((rc = check_cache8("v_cache", p->v_cache, p->v_cache_stride, cache_rows, p->d))) return rc;
            if (((uintptr_t)o.k_descale & 3) != 0 || ((uintptr_t)o.v_descale & 3) != 0) return fail(FA_ERR_BAD_STRIDE, "k_descale / v_descale must be 4-byte aligned");
        } else {
            if ((rc = check_tensor("k_cache", p->k_cache, p->k_cache_stride, cache_rows, p->d, false))) return rc;
            if ((rc = check_tensor("v_cache", p->v_cache, p->v_cache_stride, cache_rows, p->d, false))) return rc;
        }
        if (p->k_new != nullptr) {
            if ((rc = check_tensor("k_new", p->k_new, p->k_new_stride, p->seqlen_new, p->d, ragged))) return rc;
            if ((rc = check_tensor("v_new", p->v_new, p->v_new_stride, p->seqlen_new, p->d, ragged))) return rc;
        }
    }
    memset(&kp, 0, sizeof(kp));
    kp.q_ptr = p->q; kp.k_cache = p->k_cache; kp.v_cache = p->v_cache; kp.k_new = p->k_new; kp.v_new = p->v_new;
    kp.o_ptr = p->o; kp.lse_ptr = p->lse; kp.cache_seqlens = p->cache_seqlens;
    kp.q = conv(p->q_stride); kp.kc = conv(p->k_cache_stride); kp.vc = conv(p->v_cache_stride);
    kp.kn = conv(p->k_new_stride); kp.vn = conv(p->v_new_stride); kp.o = conv(p->o_stride);
    kp.b = p->b; kp.seqlen_q = p->seqlen_q; kp.seqlen_cache = p->seqlen_cache; kp.seqlen_new = p->k_new != nullptr ? p->seqlen_new : 0;
    kp.h = p->h; kp.h_k = p->h_k; kp.h_ratio = p->h / p->h_k; kp.d = p->d;
    kp.is_causal = p->is_causal ? 1 : 0;
    set_scale(kp, 1.0f / sqrtf((float)p->d));
    fill_paged(*p, kp);
    if (o.cache_dtype == FA_CACHE_FP8_E4M3) {
        kp.cache_fp8 = 1;
        kp.k_descale = o.k_descale; kp.kds_batch = o.k_descale_batch_stride; kp.kds_head = o.k_descale_head_stride;
        kp.v_descale = o.v_descale; kp.vds_batch = o.v_descale_batch_stride; kp.vds_head = o.v_descale_head_stride;
    }
    return FA_OK;
}

// fa_kvcache_options (NULL = none) -> the window fields of kp, normalised: right = 0 under causal, and a side that cannot bind is -1 (left >=
// seqlen_cache - 1: lo_t <= L - 1 - left <= 0 for every row; right >= seqlen_q - 1: lim_t >= L for every row).  A window whose left side is
// unbounded and whose right side is unbounded or the causal limit is exactly the plain call: is_local stays 0 (the plain kernels, split and bits).
static int fill_kvcache_window(const fa_kvcache_options_v8& o, fa::KvcacheKernelParams& kp) {
    if (!o.is_local) return FA_OK;
    if (o.window_size_left < -1 || o.window_size_right < -1)
        return fail(FA_ERR_BAD_SHAPE, "window_size (%d, %d): each side must be >= -1 (-1 = unbounded)", o.window_size_left, o.window_size_right);
    int left = o.window_size_left, right = kp.is_causal ? 0 : o.window_size_right;
    if (left >= kp.seqlen_cache - 1) left = -1;
    if (right >= kp.seqlen_q - 1) right = -1;
    kp.is_local = (left >= 0 || (right >= 0 && !kp.is_causal)) ? 1 : 0;
    kp.window_left = kp.is_local ? left : -1;
    kp.window_right = kp.is_local ? right : -1;
    return FA_OK;
}

// The rotary fields of the options (rotary_cos = rotary_sin = NULL: off, rp.cos stays NULL and nothing else is looked at) -> rp, validated.
// The query-position rule is decided from what the caller stated (is_causal, a window other than (-1, -1)), not from the normalised window.
static int fill_kvcache_rotary(const fa_kvcache_options_v8& o, const fa::KvcacheKernelParams& kp, fa::KvcacheRotaryParams& rp) {
    memset(&rp, 0, sizeof(rp));
    if (o.rotary_cos == nullptr && o.rotary_sin == nullptr) return FA_OK;
    if (o.rotary_cos == nullptr || o.rotary_sin == nullptr) return fail(FA_ERR_BAD_SHAPE, "rotary_cos and rotary_sin must both be given or both be NULL");
    if (o.rotary_dim < 16 || o.rotary_dim > kp.d || o.rotary_dim % 16 != 0)
        return fail(FA_ERR_BAD_SHAPE, "rotary_dim %d must be a multiple of 16 with 16 <= rotary_dim <= head_dim (%d)", o.rotary_dim, kp.d);
    if (o.seqlen_ro < 1 || o.seqlen_ro < kp.seqlen_cache)
        return fail(FA_ERR_BAD_SHAPE, "seqlen_ro (%d rows of rotary_cos / rotary_sin) must be >= 1 and cover the cache capacity seqlen_cache (%d)", o.seqlen_ro, kp.seqlen_cache);
    if (kp.k_new == nullptr)
        return fail(FA_ERR_BAD_SHAPE, "rotary_cos / rotary_sin need k_new / v_new (the rotation is applied to q and to the appended rows)");
    if (((uintptr_t)o.rotary_cos & 15) != 0 || ((uintptr_t)o.rotary_sin & 15) != 0)
        return fail(FA_ERR_BAD_STRIDE, "rotary_cos / rotary_sin base pointers must be 16-byte aligned");
    if (o.rotary_row_stride % 8 != 0 || (o.seqlen_ro > 1 && o.rotary_row_stride < o.rotary_dim / 2))
        return fail(FA_ERR_BAD_STRIDE, "rotary_row_stride %lld must be a multiple of 8 elements (16-byte loads) and at least rotary_dim / 2 = %d", (long long)o.rotary_row_stride,
                    o.rotary_dim / 2);
    rp.cos = o.rotary_cos; rp.sin = o.rotary_sin; rp.row_stride = o.rotary_row_stride;
    rp.seqlen_ro = o.seqlen_ro; rp.rotary_dim = o.rotary_dim; rp.interleaved = o.rotary_interleaved ? 1 : 0;
    rp.q_pos_per_row = (kp.is_causal || (o.is_local && (o.window_size_left != -1 || o.window_size_right != -1))) ? 1 : 0;
    return FA_OK;
}

// The ragged-batch fields of the options (cu_seqlens_q = NULL: off, rg.cu_q stays NULL and only a stray cu_seqlens_k_new is looked at) -> rg,
// validated.  rg.kp is left to the caller (the launch takes the finished kp).
static int fill_kvcache_ragged(const fa_kvcache_options_v8& o, const fa::KvcacheKernelParams& kp, const fa::KvcacheRotaryParams& rp, fa::KvcacheRaggedParams& rg) {
    memset(&rg, 0, sizeof(rg));
    if (o.cu_seqlens_q == nullptr) {
        if (o.cu_seqlens_k_new != nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_k_new given without cu_seqlens_q (packed k_new / v_new belong to a ragged call)");
        return FA_OK;
    }
    if (rp.cos != nullptr)
        return fail(FA_ERR_BAD_SHAPE, "rotary_cos / rotary_sin together with cu_seqlens_q are not supported (rotary with ragged queries is out of scope of this library version)");
    if (o.cu_seqlens_k_new != nullptr && kp.k_new == nullptr) return fail(FA_ERR_NULL_POINTER, "cu_seqlens_k_new given without k_new / v_new");
    if (kp.k_new != nullptr && o.cu_seqlens_k_new == nullptr)
        return fail(FA_ERR_NULL_POINTER, "k_new / v_new in a ragged call (cu_seqlens_q) are packed and need cu_seqlens_k_new");
    if (o.total_q < 0 || o.total_k_new < 0)
        return fail(FA_ERR_BAD_SHAPE, "total_q (%lld) and total_k_new (%lld) must be >= 0", (long long)o.total_q, (long long)o.total_k_new);
    if (((uintptr_t)o.cu_seqlens_q & 3) != 0 || ((uintptr_t)o.cu_seqlens_k_new & 3) != 0)
        return fail(FA_ERR_BAD_STRIDE, "cu_seqlens_q / cu_seqlens_k_new must be 4-byte aligned");
    // the attention grid is slots x h_k x n_split workgroups (n_split <= 128) and a tile index is an int
    if (o.total_q * kp.h_ratio >= ((int64_t)1 << 31) || (fa::kvcache_ragged_slots(kp, o.total_q, nullptr) * kp.h_k) >= ((int64_t)1 << 24))
        return fail(FA_ERR_BAD_SHAPE, "ragged call too large: total_q = %lld rows x %d heads per KV head over %d sequences exceeds the launch grid", (long long)o.total_q,
                    kp.h_ratio, kp.b);
    rg.cu_q = o.cu_seqlens_q;
    rg.cu_kn = kp.k_new != nullptr ? o.cu_seqlens_k_new : nullptr;
    rg.total_q = o.total_q;
    rg.total_kn = kp.k_new != nullptr ? o.total_k_new : 0;
    return FA_OK;
}

// softmax_scale / softcap of the options -> kp.scale / kp.scale_log2e and cap_pre (0 = no cap: the kernels, hence the bits, of the call without
// the two fields whenever the scale is the default's value).  With a cap the attention kernels of fa_fwd_kvcache_softcap.hip keep tanh(s * pre)
// and read the cap where the scale was: scale = softcap, scale_log2e = softcap * log2(e), cap_pre = 2 log2(e) * softmax_scale / softcap.
static int fill_kvcache_softcap(const fa_kvcache_options_v8& o, fa::KvcacheKernelParams& kp, float& cap_pre) {
    cap_pre = 0.f;
    if (int rc = check_softmax_scale(o.softmax_scale, "1 / sqrt(head_dim)")) return rc;
    if (!(o.softcap >= 0.f) || isinf(o.softcap)) return fail(FA_ERR_BAD_SHAPE, "softcap %g must be finite and >= 0 (0 = no cap)", (double)o.softcap);
    if (o.reserved[0] != 0 || o.reserved[1] != 0)
        return fail(FA_ERR_BAD_ABI, "fa_kvcache_options_v5: reserved fields are not zero (a field of a newer header that this library does not know)");
    if (o.softmax_scale > 0.f) set_scale(kp, o.softmax_scale);
    if (o.softcap > 0.f) {
        cap_pre = (kp.scale / o.softcap) * 2.8853900817779268f;
        if (!(cap_pre > 0.f) || isinf(cap_pre))
            return fail(FA_ERR_BAD_SHAPE, "softmax_scale %g over softcap %g is outside the fp32 range", (double)kp.scale, (double)o.softcap);
        set_scale(kp, o.softcap);
    }
    return FA_OK;
}

// The sink fields of the options (sinks = NULL: off, sink.ptr stays NULL and only the reserved words are looked at - a v6 struct
// with a zeroed tail is a v5 call) -> sink, validated; behind every older field.  Sinks with a soft cap and sinks at head_dim 256 have no kernels.
static int fill_kvcache_sinks(const fa_kvcache_options_v8& o, const fa::KvcacheKernelParams& kp, float cap_pre, fa::KvcacheSink& sink) {
    sink.ptr = nullptr;
    sink.stride = 0;
    if (o.sinks != nullptr) {
        if (((uintptr_t)o.sinks & 3) != 0) return fail(FA_ERR_BAD_STRIDE, "sinks must be 4-byte aligned (fp32 logits, one per query head)");
        if (cap_pre > 0.f) return fail(FA_ERR_BAD_SHAPE, "sinks together with softcap > 0 are not supported");
        if (kp.d == 256) return fail(FA_ERR_BAD_SHAPE, "sinks at head_dim d = 256 are not supported (d must be 64 or 128 with sinks)");
        sink.ptr = o.sinks;
        sink.stride = o.sinks_stride;
    }
    if (o.reserved2[0] != 0 || o.reserved2[1] != 0)
        return fail(FA_ERR_BAD_ABI, "fa_kvcache_options_v6: reserved2 fields are not zero (a field of a newer header that this library does not know)");
    return FA_OK;
}

// The tree-mask fields of the options (tree_mask = NULL: off, tree.ptr stays NULL and only the reserved words are looked at - a v7 struct with a
// zeroed tail is a v6 call) -> tree, validated; behind every older field.  The mask is a select of its own: it does not combine with the causal
// limit, a window, a soft cap, sinks or rotary (a node's position is its depth, not its index: the engine rotates), has no head_dim-256 kernels,
// and a row's word holds 64 draft tokens.  What the caller stated decides, not the normalised window.
static int fill_kvcache_tree(const fa_kvcache_options_v8& o, const fa::KvcacheKernelParams& kp, const fa::KvcacheRotaryParams& rp, float cap_pre,
                             const fa::KvcacheSink& sink, fa::KvcacheTree& tree) {
    tree.ptr = nullptr;
    tree.batch_stride = tree.row_stride = 0;
    if (o.tree_mask != nullptr) {
        if (((uintptr_t)o.tree_mask & 7) != 0) return fail(FA_ERR_BAD_STRIDE, "tree_mask must be 8-byte aligned (int64 words, one per query row)");
        if (kp.is_causal) return fail(FA_ERR_BAD_SHAPE, "tree_mask together with is_causal is not supported (the lower-triangle mask is the causal call)");
        if (o.is_local && (o.window_size_left != -1 || o.window_size_right != -1))
            return fail(FA_ERR_BAD_SHAPE, "tree_mask together with window_size (%d, %d) is not supported", o.window_size_left, o.window_size_right);
        if (cap_pre > 0.f) return fail(FA_ERR_BAD_SHAPE, "tree_mask together with softcap > 0 is not supported");
        if (sink.ptr != nullptr) return fail(FA_ERR_BAD_SHAPE, "tree_mask together with sinks is not supported");
        if (rp.cos != nullptr)
            return fail(FA_ERR_BAD_SHAPE, "tree_mask together with rotary_cos / rotary_sin is not supported (a node's position is its depth: rotate before the call)");
        if (kp.d == 256) return fail(FA_ERR_BAD_SHAPE, "tree_mask at head_dim d = 256 is not supported (d must be 64 or 128 with tree_mask)");
        if (kp.seqlen_q > 64)
            return fail(FA_ERR_BAD_SHAPE, "tree_mask: seqlen_q (ragged: max_seqlen_q) = %d exceeds 64, the draft tokens one mask word holds", kp.seqlen_q);
        tree.ptr = o.tree_mask;
        tree.batch_stride = o.tree_mask_batch_stride;
        tree.row_stride = o.tree_mask_row_stride;
    }
    if (o.reserved3[0] != 0 || o.reserved3[1] != 0)
        return fail(FA_ERR_BAD_ABI, "fa_kvcache_options_v7: reserved3 fields are not zero (a field of a newer header that this library does not know)");
    return FA_OK;
}

// row_tile of the options (0: the 16-row kernels, and only the reserved words are looked at - a v8 struct with a zeroed tail is a v7 call) ->
// row_tile as the launchers take it (kKvcRows / kKvcPrefillRows), validated; behind every older field.  The wide kernels are the plain and the
// causal body alone: no window, soft cap, sinks, tree mask or rotary image, and no head_dim 256.  What the caller stated decides, not the normalised window.
static int fill_kvcache_prefill(const fa_kvcache_options_v8& o, const fa::KvcacheKernelParams& kp, const fa::KvcacheRotaryParams& rp, float cap_pre,
                                const fa::KvcacheSink& sink, const fa::KvcacheTree& tree, int32_t& row_tile) {
    row_tile = fa::kKvcRows;
    if (o.row_tile != 0) {
        if (o.row_tile != fa::kKvcPrefillRows)
            return fail(FA_ERR_BAD_SHAPE, "row_tile %d unsupported (0 = the 16-row kernels, 64 = the 64-row kernels for prompt chunks)", o.row_tile);
        if (o.is_local && (o.window_size_left != -1 || o.window_size_right != -1))
            return fail(FA_ERR_BAD_SHAPE, "row_tile = 64 together with window_size (%d, %d) is not supported", o.window_size_left, o.window_size_right);
        if (cap_pre > 0.f) return fail(FA_ERR_BAD_SHAPE, "row_tile = 64 together with softcap > 0 is not supported");
        if (sink.ptr != nullptr) return fail(FA_ERR_BAD_SHAPE, "row_tile = 64 together with sinks is not supported");
        if (tree.ptr != nullptr) return fail(FA_ERR_BAD_SHAPE, "row_tile = 64 together with tree_mask is not supported");
        if (rp.cos != nullptr) return fail(FA_ERR_BAD_SHAPE, "row_tile = 64 together with rotary_cos / rotary_sin is not supported");
        if (kp.d == 256) return fail(FA_ERR_BAD_SHAPE, "row_tile = 64 at head_dim d = 256 is not supported (d must be 64 or 128 with row_tile = 64)");
        row_tile = fa::kKvcPrefillRows;
    }
    if (o.reserved4_ != 0 || o.reserved4[0] != 0 || o.reserved4[1] != 0 || o.reserved4[2] != 0 || o.reserved4[3] != 0 || o.reserved4[4] != 0)
        return fail(FA_ERR_BAD_ABI, "fa_kvcache_options_v8: reserved4 fields are not zero (a field of a newer header that this library does not know)");
    return FA_OK;
}

struct KvcacheCall {        // what the four _ex entry points derive from their two structs
    fa::KvcacheKernelParams kp;
    fa_kvcache_params local;
    fa_kvcache_options_v8 o;
    fa::KvcacheRotaryParams rp;
    fa::KvcacheRaggedParams rg;
    float cap_pre;
    fa::KvcacheSink sink;
    fa::KvcacheTree tree;
    int32_t row_tile;

    int64_t total_q() const { return rg.cu_q != nullptr ? rg.total_q : -1; }      // (-1: not a ragged call)
    // the split of the call over `avail` bytes for the partials (-1: without a limit, what the workspace query sizes for)
    int32_t split(int64_t avail) const { return fa::kvcache_split(kp, avail, local.num_splits, total_q(), row_tile); }
    // Workspace for the split partials: all of it, or in a rotary call what is left once the image of the rotated q has taken its part; a workspace
    // that cannot hold the image is an error (the attention kernels read q from it: there is no path without it)
    int64_t split_bytes() const {
        const int64_t have = local.workspace != nullptr ? local.workspace_bytes : 0;
        if (rp.cos == nullptr) return have;
        const int64_t need = fa::kvcache_rotary_image_bytes(kp);
        if (have < need)
            return fail(FA_ERR_BAD_SHAPE, "rotary: the workspace (%lld bytes) cannot hold the image of the rotated q: %lld bytes needed (fa_kvcache_workspace_bytes_ex)", (long long)have,
                        (long long)need);
        return have - need;
    }
};

// Params first, as before the options existed (their errors win), except that the cache tensors are checked under the cache dtype the
// options state; then the options' own values.
static int fill_kvcache_all(const fa_kvcache_params* user, const fa_kvcache_options* options, KvcacheCall& c, bool with_workspace) {
    fa_kvcache_options_v8 none;
    memset(&none, 0, sizeof(none));
    const int orc = import_kvcache_options(options, c.o);
    char oerr[sizeof(g_err)];
    memcpy(oerr, g_err, sizeof(oerr));
    int rc = fill_kvcache(user, c.kp, c.local, with_workspace, orc ? none : c.o);
    if (rc) return rc;
    if (orc) {
        memcpy(g_err, oerr, sizeof(g_err));
        return orc;
    }
    if ((rc = fill_kvcache_window(c.o, c.kp))) return rc;
    if ((rc = fill_kvcache_rotary(c.o, c.kp, c.rp))) return rc;
    if ((rc = fill_kvcache_ragged(c.o, c.kp, c.rp, c.rg))) return rc;
    if ((rc = fill_kvcache_softcap(c.o, c.kp, c.cap_pre))) return rc;
    if ((rc = fill_kvcache_sinks(c.o, c.kp, c.cap_pre, c.sink))) return rc;
    if ((rc = fill_kvcache_tree(c.o, c.kp, c.rp, c.cap_pre, c.sink, c.tree))) return rc;
    return fill_kvcache_prefill(c.o, c.kp, c.rp, c.cap_pre, c.sink, c.tree, c.row_tile);
}

int64_t fa_kvcache_workspace_bytes_ex(const fa_kvcache_params* user, const fa_kvcache_options* options) {
    KvcacheCall c;
    int rc = fill_kvcache_all(user, options, c, false);
    if (rc) return rc;
    if (c.kp.b == 0) return 0;
    return (c.rp.cos != nullptr ? fa::kvcache_rotary_image_bytes(c.kp) : 0) + fa::kvcache_workspace_bytes(c.kp, c.split(-1), c.total_q());
}

int32_t fa_kvcache_num_splits_ex(const fa_kvcache_params* user, const fa_kvcache_options* options) {
    KvcacheCall c;
    int rc = fill_kvcache_all(user, options, c, true);
    if (rc) return rc;
    if (c.kp.b == 0) return 1;
    const int64_t avail = c.split_bytes();
    if (avail < 0) return (int32_t)avail;
    return c.split(avail);
}

int32_t fa_kvcache_row_tile_ex(const fa_kvcache_params* user, const fa_kvcache_options* options) {
    KvcacheCall c;
    int rc = fill_kvcache_all(user, options, c, false);
    if (rc) return rc;
    return c.row_tile;
}

int fa_run_mha_fwd_kvcache_ex(const fa_kvcache_params* user, const fa_kvcache_options* options, void* stream) {
    KvcacheCall c;
    int rc = fill_kvcache_all(user, options, c, true);
    if (rc) return rc;
    fa::KvcacheKernelParams& kp = c.kp;
    if (kp.b == 0) return FA_OK;
    const int64_t avail = c.split_bytes();
    if (avail < 0) return (int)avail;
    char* ws = (char*)c.local.workspace;
    if (c.rp.cos != nullptr) {
        // the fused rotary launch takes the place of the append: it writes the cache rows and the image of the rotated q at the head of the
        // workspace; the attention kernels then run as without rotary, with the image as their q and nothing left to append
        c.rp.kp = kp;
        c.rp.q_image = ws;
        ws += fa::kvcache_rotary_image_bytes(kp);
        if ((rc = hip_status(fa::launch_kvcache_rotary(c.rp, c.local.dtype, (hipStream_t)stream), "fa_kvcache_rotary launch"))) return rc;
        kp.q_ptr = c.rp.q_image;
        kp.q = conv(contiguous_bshd(kp.seqlen_q, kp.h, kp.d));
        kp.k_new = kp.v_new = nullptr;          // (seqlen_new stays: the appended rows count into the valid length)
    }
    kp.n_split = c.split(avail);
    kp.ws_o = kp.n_split > 1 ? (float*)ws : nullptr;
    if (c.rg.cu_q == nullptr)
        return hip_status(fa::launch_fwd_kvcache(kp, c.local.dtype, (hipStream_t)stream, c.cap_pre, c.sink, c.tree, c.row_tile), "fa_fwd_kvcache launch");
    // ragged queries: the append, attention and combine kernels of fa_fwd_kvcache_ragged.hip (no rotary: refused by fill_kvcache_ragged)
    c.rg.kp = kp;
    return hip_status(fa::launch_fwd_kvcache_ragged(c.rg, c.local.dtype, (hipStream_t)stream, c.cap_pre, c.sink, c.tree, c.row_tile), "fa_fwd_kvcache (ragged) launch");
}

int64_t fa_kvcache_workspace_bytes(const fa_kvcache_params* user) { return fa_kvcache_workspace_bytes_ex(user, nullptr); }
int32_t fa_kvcache_num_splits(const fa_kvcache_params* user) { return fa_kvcache_num_splits_ex(user, nullptr); }
int fa_run_mha_fwd_kvcache(const fa_kvcache_params* user, void* stream) { return fa_run_mha_fwd_kvcache_ex(user, nullptr, stream); }

// ---- MLA decode over a latent KV cache -------------------------------------------------------------------------------------------------------
// fa_mla_params -> KvcacheMlaParams, validated.  kp.d = 512 is the width of V, of o and of the partial planes; the split and the workspace are the
// decode call's rules over the grid of 64-row tiles.  with_workspace = false: the `workspace` fields are not looked at.
static int fill_mla(const fa_mla_params* user, fa::KvcacheMlaParams& mp, fa_mla_params_v2& local, bool with_workspace) {
    int rc = import_mla(user, local, "fa_mla_params");
    if (rc) return rc;
    const fa_mla_params_v2* p = &local;
    if (p->b < 0 || p->seqlen_q < 1 || p->seqlen_cache < 0 || p->seqlen_new < 0 || p->h <= 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d (>= 1) seqlen_cache=%d seqlen_new=%d h=%d", p->b, p->seqlen_q, p->seqlen_cache, p->seqlen_new, p->h);
    if ((rc = check_mla_dims(p->d_qk, p->d_v, p->dtype))) return rc;
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    if (p->seqlen_new > p->seqlen_cache)
        return fail(FA_ERR_BAD_SHAPE, "seqlen_new (%d) exceeds the cache capacity seqlen_cache (%d)", p->seqlen_new, p->seqlen_cache);
    if (p->kv_new != nullptr && p->cache_seqlens == nullptr) return fail(FA_ERR_NULL_POINTER, "kv_new needs cache_seqlens (the rows it is appended at)");
    if (p->kv_new == nullptr && p->seqlen_new != 0) return fail(FA_ERR_BAD_SHAPE, "seqlen_new = %d without kv_new", p->seqlen_new);
    if ((rc = check_mla_tail(*p, "fa_mla_params", with_workspace))) return rc;
    // the attention grid is b x 64-row tiles x n_split workgroups (n_split <= 128), and a packed row index is an int
    const int64_t tiles = ((int64_t)p->seqlen_q * p->h + fa::kKvcPrefillRows - 1) / fa::kKvcPrefillRows;
    if ((int64_t)p->seqlen_q * p->h >= ((int64_t)1 << 31) || (int64_t)p->b * tiles >= ((int64_t)1 << 24))
        return fail(FA_ERR_BAD_SHAPE, "call too large: b = %d sequences x seqlen_q = %d rows x h = %d heads exceeds the launch grid", p->b, p->seqlen_q, p->h);
    fa_strides kvc = p->kv_cache_stride, kvn = p->kv_new_stride;
    kvc.head = kvn.head = 0;        // one KV head
    if (p->b > 0) {
        if (p->lse == nullptr) return fail(FA_ERR_NULL_POINTER, "lse is NULL");
        if ((rc = check_tensor("q", p->q, p->q_stride, p->seqlen_q, p->d_qk, false))) return rc;
        if ((rc = check_tensor("o", p->o, p->o_stride, p->seqlen_q, p->d_v, false))) return rc;
        if ((rc = check_mla_cache(*p, kvc))) return rc;
        if (p->kv_new != nullptr && (rc = check_tensor("kv_new", p->kv_new, kvn, p->seqlen_new, p->d_qk, false))) return rc;
    }
    memset(&mp, 0, sizeof(mp));
    fa::KvcacheKernelParams& kp = mp.kp;
    mp.d_qk = p->d_qk;
    fill_mla_kp(*p, kvc, kp);
    kp.k_new = kp.v_new = p->kv_new; kp.kn = kp.vn = conv(kvn); kp.seqlen_new = p->kv_new != nullptr ? p->seqlen_new : 0;
    kp.is_causal = p->is_causal ? 1 : 0;
    return FA_OK;
}

int64_t fa_mla_workspace_bytes(const fa_mla_params* user) {
    fa::KvcacheMlaParams mp;
    fa_mla_params_v2 local;
    int rc = fill_mla(user, mp, local, false);
    if (rc) return rc;
    if (mp.kp.b == 0) return 0;
    return fa::kvcache_workspace_bytes(mp.kp, mla_split(mp.kp, local, false));
}

int32_t fa_mla_num_splits(const fa_mla_params* user) {
    fa::KvcacheMlaParams mp;
    fa_mla_params_v2 local;
    int rc = fill_mla(user, mp, local, true);
    if (rc) return rc;
    if (mp.kp.b == 0) return 1;
    return mla_split(mp.kp, local, true);
}

int fa_run_mla_fwd_kvcache(const fa_mla_params* user, void* stream) {
    fa::KvcacheMlaParams mp;
    fa_mla_params_v2 local;
    int rc = fill_mla(user, mp, local, true);
    if (rc) return rc;
    if (mp.kp.b == 0) return FA_OK;
    mp.kp.n_split = mla_split(mp.kp, local, true);
    mp.kp.ws_o = mp.kp.n_split > 1 ? (float*)local.workspace : nullptr;
    if (mp.kp.cache_fp8) return hip_status(fa::launch_fwd_kvcache_mla_fp8(mp, local.dtype, (hipStream_t)stream), "fa_fwd_kvcache_mla_fp8 launch");
    return hip_status(fa::launch_fwd_kvcache_mla(mp, local.dtype, (hipStream_t)stream), "fa_fwd_kvcache_mla launch");
}

// ---- sparse MLA decode over a latent KV cache ------------------------------------------------------------------------------------------------
// fa_mla_sparse_params -> KvcacheMlaSparseParams, validated: the checks and words of fill_mla without kv_new / is_causal, plus indices and topk.  split: what
// kvcache_split / kvcache_workspace_bytes are asked with - the grid is b x seqlen_q x ceil(h / 64) workgroups a split and the split runs over the slots
// [0, topk), so the copy states b x seqlen_q "sequences" of one token and topk in the place of seqlen_cache (rows = b * h * seqlen_q either way).
static int fill_mla_sparse(const fa_mla_sparse_params* user, fa::KvcacheMlaSparseParams& sp, fa::KvcacheKernelParams& split, fa_mla_sparse_params_v2& local, bool with_workspace) {
    int rc = import_mla(user, local, "fa_mla_sparse_params");
    if (rc) return rc;
    const fa_mla_sparse_params_v2* p = &local;
    if (p->b < 0 || p->seqlen_q < 1 || p->seqlen_cache < 0 || p->h <= 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d (>= 1) seqlen_cache=%d h=%d", p->b, p->seqlen_q, p->seqlen_cache, p->h);
    if ((rc = check_mla_dims(p->d_qk, p->d_v, p->dtype))) return rc;
    if (p->topk < fa::kKvcStep || p->topk % fa::kKvcStep != 0)
        return fail(FA_ERR_BAD_SHAPE, "topk %d must be a positive multiple of %d (pad the lists with -1)", p->topk, fa::kKvcStep);
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    if ((rc = check_mla_tail(*p, "fa_mla_sparse_params", with_workspace))) return rc;
    // the attention grid is b x seqlen_q x 64-head tiles x n_split workgroups (n_split <= 128), and a row index is an int
    const int64_t tiles = ((int64_t)p->h + fa::kKvcPrefillRows - 1) / fa::kKvcPrefillRows;
    if ((int64_t)p->seqlen_q * p->h >= ((int64_t)1 << 31) || (int64_t)p->b * p->seqlen_q * tiles >= ((int64_t)1 << 24))
        return fail(FA_ERR_BAD_SHAPE, "call too large: b = %d sequences x seqlen_q = %d rows x h = %d heads exceeds the launch grid", p->b, p->seqlen_q, p->h);
    fa_strides kvc = p->kv_cache_stride;
    kvc.head = 0;        // one KV head
    if (p->b > 0) {
        if (p->lse == nullptr) return fail(FA_ERR_NULL_POINTER, "lse is NULL");
        if (p->indices == nullptr) return fail(FA_ERR_NULL_POINTER, "indices is NULL");
        if ((reinterpret_cast<uintptr_t>(p->indices) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "indices must be 4-byte aligned");
        if (p->indices_batch_stride < 0 || p->indices_row_stride < 0)
            return fail(FA_ERR_BAD_STRIDE, "indices strides (indices_batch_stride=%lld, indices_row_stride=%lld) must be >= 0 elements", (long long)p->indices_batch_stride,
                        (long long)p->indices_row_stride);
        if ((rc = check_tensor("q", p->q, p->q_stride, p->seqlen_q, p->d_qk, false))) return rc;
        if ((rc = check_tensor("o", p->o, p->o_stride, p->seqlen_q, p->d_v, false))) return rc;
        if ((rc = check_mla_cache(*p, kvc))) return rc;
    }
    memset(&sp, 0, sizeof(sp));
    sp.d_qk = p->d_qk; sp.topk = p->topk;
    sp.indices = p->indices; sp.idx_batch = p->indices_batch_stride; sp.idx_row = p->indices_row_stride;
    fill_mla_kp(*p, kvc, sp.kp);
    split = sp.kp;
    split.b = p->b * p->seqlen_q; split.seqlen_q = 1; split.seqlen_cache = p->topk;
    return FA_OK;
}

int64_t fa_mla_sparse_workspace_bytes(const fa_mla_sparse_params* user) {
    fa::KvcacheMlaSparseParams sp;
    fa::KvcacheKernelParams split;
    fa_mla_sparse_params_v2 local;
    int rc = fill_mla_sparse(user, sp, split, local, false);
    if (rc) return rc;
    if (sp.kp.b == 0) return 0;
    return fa::kvcache_workspace_bytes(split, mla_split(split, local, false));
}

int32_t fa_mla_sparse_num_splits(const fa_mla_sparse_params* user) {
    fa::KvcacheMlaSparseParams sp;
    fa::KvcacheKernelParams split;
    fa_mla_sparse_params_v2 local;
    int rc = fill_mla_sparse(user, sp, split, local, true);
    if (rc) return rc;
    if (sp.kp.b == 0) return 1;
    return mla_split(split, local, true);
}

int fa_run_mla_sparse_fwd_kvcache(const fa_mla_sparse_params* user, void* stream) {
    fa::KvcacheMlaSparseParams sp;
    fa::KvcacheKernelParams split;
    fa_mla_sparse_params_v2 local;
    int rc = fill_mla_sparse(user, sp, split, local, true);
    if (rc) return rc;
    if (sp.kp.b == 0) return FA_OK;
    sp.kp.n_split = mla_split(split, local, true);
    sp.kp.ws_o = sp.kp.n_split > 1 ? (float*)local.workspace : nullptr;
    if (sp.kp.cache_fp8) return hip_status(fa::launch_fwd_kvcache_mla_sparse_fp8(sp, local.dtype, (hipStream_t)stream), "fa_fwd_kvcache_mla_sparse_fp8 launch");
    return hip_status(fa::launch_fwd_kvcache_mla_sparse(sp, local.dtype, (hipStream_t)stream), "fa_fwd_kvcache_mla_sparse launch");
}

// ---- the indexer in front of sparse MLA decode -------------------------------------------------------------------------------------------------
// fa_mla_indexer_params (216 bytes) and fa_mla_indexer_params_v2 (q_format appended) share their prefix.  v2_entry: one of the _v2 entry points, which take either
// struct and tell them apart by struct_size (the shorter one arrives as a _v2 with q_format = FA_IDX_Q_16BIT); the entry points without _v2 take the 216-byte
// struct alone (import_exact).  With FA_IDX_Q_FP8_E4M3 q_idx holds e4m3 codes, its strides count bytes and the launch is one of the _fp8q ones.
static_assert(sizeof(fa_mla_indexer_params_v2) == sizeof(fa_mla_indexer_params) + 8 && offsetof(fa_mla_indexer_params_v2, q_format) == sizeof(fa_mla_indexer_params) &&
                  offsetof(fa_mla_indexer_params_v2, block_table_stride) == offsetof(fa_mla_indexer_params, block_table_stride),
              "fa_mla_indexer_params_v2 is fa_mla_indexer_params with two int32 appended");
static int fill_mla_indexer(const void* user_, bool v2_entry, fa::MlaIndexerParams& ip, fa_mla_indexer_params_v2& local) {
    memset(&local, 0, sizeof(local));
    int rc;
    if (!v2_entry) {
        rc = import_exact(static_cast<const fa_mla_indexer_params*>(user_), reinterpret_cast<fa_mla_indexer_params&>(local), "fa_mla_indexer_params");
        if (rc) return rc;
    } else {
        const fa_mla_indexer_params_v2* user = static_cast<const fa_mla_indexer_params_v2*>(user_);
        if ((rc = check_header(user, "fa_mla_indexer_params_v2", true))) return rc;
        if (user->struct_size != sizeof(fa_mla_indexer_params) && user->struct_size != sizeof(fa_mla_indexer_params_v2))
            return fail(FA_ERR_BAD_ABI, "fa_mla_indexer_params_v2: struct_size %u is neither %zu (fa_mla_indexer_params) nor %zu - header / library mismatch", user->struct_size,
                        sizeof(fa_mla_indexer_params), sizeof(fa_mla_indexer_params_v2));
        memcpy(&local, user, user->struct_size);
    }
    const fa_mla_indexer_params_v2* p = &local;
    const bool paged = p->block_table != nullptr;
    if (p->b < 0 || p->seqlen_q < 1 || p->seqlen_cache < 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d (>= 1) seqlen_cache=%d", p->b, p->seqlen_q, p->seqlen_cache);
    if (p->h != 16 && p->h != 32 && p->h != 64) return fail(FA_ERR_BAD_HEADDIM, "h %d unsupported (16, 32 or 64 index heads)", p->h);
    if (p->d != fa::kIdxD) return fail(FA_ERR_BAD_HEADDIM, "d %d unsupported (index heads and index keys are 128 wide)", p->d);
    if ((rc = check_dtype(p->dtype))) return rc;
    if (p->k_format != FA_MLA_KV_16BIT && p->k_format != FA_IDX_K_FP8_E4M3)
        return fail(FA_ERR_BAD_DTYPE, "k_format %d unknown (0 = keys of dtype, 1 = OCP e4m3 codes)", p->k_format);
    if ((rc = check_reserved(p->reserved_, "fa_mla_indexer_params", FA_ERR_BAD_SHAPE))) return rc;
    if (p->q_format != FA_IDX_Q_16BIT && p->q_format != FA_IDX_Q_FP8_E4M3)
        return fail(FA_ERR_BAD_DTYPE, "q_format %d unknown (0 = queries of dtype, 1 = OCP e4m3 codes)", p->q_format);
    if (p->reserved2_ != 0) return fail(FA_ERR_BAD_SHAPE, "reserved2_ is not zero (%d)", p->reserved2_);
    const bool q8 = p->q_format == FA_IDX_Q_FP8_E4M3;
    if (q8 && p->k_format != FA_IDX_K_FP8_E4M3)
        return fail(FA_ERR_BAD_DTYPE, "k_format %d: e4m3 index queries (q_format = 1) need an e4m3 index-key cache (k_format = 1)", p->k_format);
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    // a workgroup's key range ends at most kIdxMaxWgKeys past the capacity, and the grid is one-dimensional
    if (p->seqlen_cache > INT32_MAX - 2 * fa::kIdxMaxWgKeys) return fail(FA_ERR_BAD_SHAPE, "seqlen_cache %d too large", p->seqlen_cache);
    if ((int64_t)p->b * p->seqlen_q >= ((int64_t)1 << 24))
        return fail(FA_ERR_BAD_SHAPE, "call too large: b = %d sequences x seqlen_q = %d tokens exceeds the launch grid", p->b, p->seqlen_q);
    const bool fp8 = p->k_format == FA_IDX_K_FP8_E4M3;
    const int es = fp8 ? 1 : 2;     // strides of the cache: bytes (FP8) or elements; 16-byte loads either way (check_idx_cache)
    if (p->b > 0) {
        if (p->logits == nullptr) return fail(FA_ERR_NULL_POINTER, "logits is NULL");
        if ((reinterpret_cast<uintptr_t>(p->logits) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "logits must be 4-byte aligned");
        if (p->logits_row_stride < p->seqlen_cache || p->logits_batch_stride < 0)
            return fail(FA_ERR_BAD_STRIDE, "logits strides (logits_batch_stride=%lld, logits_row_stride=%lld): rows must be at least seqlen_cache = %d elements apart",
                        (long long)p->logits_batch_stride, (long long)p->logits_row_stride, p->seqlen_cache);
        if (p->weights == nullptr) return fail(FA_ERR_NULL_POINTER, "weights is NULL");
        if ((reinterpret_cast<uintptr_t>(p->weights) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "weights must be 4-byte aligned");
        if (p->q_idx == nullptr) return fail(FA_ERR_NULL_POINTER, "q_idx is NULL");
        const fa_strides& qs = p->q_idx_stride;
        if ((reinterpret_cast<uintptr_t>(p->q_idx) & 15u) != 0) return fail(FA_ERR_BAD_STRIDE, "q_idx base pointer must be 16-byte aligned");
        const int qunit = q8 ? 16 : 8;  // 16-byte loads: bytes of codes, or elements of dtype
        if (qs.head % qunit != 0 || qs.row % qunit != 0 || qs.batch % qunit != 0)
            return fail(FA_ERR_BAD_STRIDE, "q_idx strides (batch=%lld,row=%lld,head=%lld) must be multiples of %d %s", (long long)qs.batch, (long long)qs.row, (long long)qs.head,
                        qunit, q8 ? "bytes" : "elements");
        if ((rc = check_idx_cache(*p))) return rc;
        if (p->k_scale != nullptr && (reinterpret_cast<uintptr_t>(p->k_scale) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "k_scale must be 4-byte aligned");
    }
    memset(&ip, 0, sizeof(ip));
    ip.q_ptr = p->q_idx; ip.w_ptr = p->weights; ip.k_cache = p->k_idx_cache; ip.k_scale = p->k_scale; ip.logits = p->logits;
    ip.cache_seqlens = p->cache_seqlens; ip.block_table = p->block_table;
    ip.q_batch = p->q_idx_stride.batch; ip.q_row = p->q_idx_stride.row; ip.q_head = p->q_idx_stride.head;
    ip.w_batch = p->weights_stride.batch; ip.w_row = p->weights_stride.row; ip.w_head = p->weights_stride.head;
    ip.k_batch = p->k_cache_batch_stride * es; ip.k_row = p->k_cache_row_stride * es;
    ip.ks_batch = p->k_scale_batch_stride; ip.ks_row = p->k_scale_row_stride;
    ip.lg_batch = p->logits_batch_stride; ip.lg_row = p->logits_row_stride;
    ip.bt_stride = p->block_table_stride;
    ip.b = p->b; ip.seqlen_q = p->seqlen_q; ip.seqlen_cache = p->seqlen_cache; ip.h = p->h;
    ip.is_causal = p->is_causal ? 1 : 0; ip.cache_fp8 = fp8 ? 1 : 0;
    ip.page_size = paged ? p->page_block_size : 0; ip.num_blocks = paged ? p->num_blocks : 0;
    return FA_OK;
}

static int run_mla_indexer_logits(const void* user, bool v2_entry, bool prefill, void* stream) {
    fa::MlaIndexerParams ip;
    fa_mla_indexer_params_v2 local;
    int rc = fill_mla_indexer(user, v2_entry, ip, local);
    if (rc) return rc;
    if (ip.b == 0 || ip.seqlen_cache == 0) return FA_OK;        // nothing to write
    hipStream_t s = (hipStream_t)stream;
    if (local.q_format == FA_IDX_Q_FP8_E4M3)
        return prefill ? hip_status(fa::launch_mla_indexer_prefill_logits_fp8q(ip, s), "fa_mla_indexer_prefill_logits_fp8q launch")
                       : hip_status(fa::launch_mla_indexer_logits_fp8q(ip, s), "fa_mla_indexer_logits_fp8q launch");
    return prefill ? hip_status(fa::launch_mla_indexer_prefill_logits(ip, local.dtype, s), "fa_mla_indexer_prefill_logits launch")
                   : hip_status(fa::launch_mla_indexer_logits(ip, local.dtype, s), "fa_mla_indexer_logits launch");
}

static int mla_indexer_prefill_launch(const void* user, bool v2_entry, int32_t* tokens_per_wg, int32_t* wg_keys, int32_t* n_chunks) {
    fa::MlaIndexerParams ip;
    fa_mla_indexer_params_v2 local;
    int rc = fill_mla_indexer(user, v2_entry, ip, local);
    if (rc) return rc;
    fa::mla_indexer_prefill_shape(ip);
    if (tokens_per_wg != nullptr) *tokens_per_wg = fa::kIdxpTQ;
    if (wg_keys != nullptr) *wg_keys = ip.wg_keys;
    if (n_chunks != nullptr) *n_chunks = ip.n_chunks;
    return FA_OK;
}

int fa_run_mla_indexer_logits(const fa_mla_indexer_params* user, void* stream) { return run_mla_indexer_logits(user, false, false, stream); }
// the prompt-chunk form of fa_run_mla_indexer_logits: the same struct through the same fill_mla_indexer
int fa_run_mla_indexer_prefill_logits(const fa_mla_indexer_params* user, void* stream) { return run_mla_indexer_logits(user, false, true, stream); }
int fa_mla_indexer_prefill_launch(const fa_mla_indexer_params* user, int32_t* tokens_per_wg, int32_t* wg_keys, int32_t* n_chunks) {
    return mla_indexer_prefill_launch(user, false, tokens_per_wg, wg_keys, n_chunks);
}
// the same three for fa_mla_indexer_params_v2 (or, by struct_size, the 216-byte struct)
int fa_run_mla_indexer_logits_v2(const fa_mla_indexer_params_v2* user, void* stream) { return run_mla_indexer_logits(user, true, false, stream); }
int fa_run_mla_indexer_prefill_logits_v2(const fa_mla_indexer_params_v2* user, void* stream) { return run_mla_indexer_logits(user, true, true, stream); }
int fa_mla_indexer_prefill_launch_v2(const fa_mla_indexer_params_v2* user, int32_t* tokens_per_wg, int32_t* wg_keys, int32_t* n_chunks) {
    return mla_indexer_prefill_launch(user, true, tokens_per_wg, wg_keys, n_chunks);
}

int fa_run_mla_indexer_topk(const fa_mla_topk_params* user, void* stream) {
    fa_mla_topk_params local;
    int rc = import_exact(user, local, "fa_mla_topk_params");
    if (rc) return rc;
    const fa_mla_topk_params* p = &local;
    if (p->b < 0 || p->seqlen_q < 1 || p->seqlen_cache < 0)
        return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d seqlen_q=%d (>= 1) seqlen_cache=%d", p->b, p->seqlen_q, p->seqlen_cache);
    if (p->topk < 32 || p->topk % 32 != 0) return fail(FA_ERR_BAD_SHAPE, "topk %d must be a positive multiple of 32", p->topk);
    if ((rc = check_reserved(p->reserved_, "fa_mla_topk_params", FA_ERR_BAD_SHAPE))) return rc;
    if ((int64_t)p->b * p->seqlen_q >= ((int64_t)1 << 31))
        return fail(FA_ERR_BAD_SHAPE, "call too large: b = %d sequences x seqlen_q = %d tokens exceeds the launch grid", p->b, p->seqlen_q);
    if (p->b == 0) return FA_OK;
    if (p->indices == nullptr) return fail(FA_ERR_NULL_POINTER, "indices is NULL");
    if ((reinterpret_cast<uintptr_t>(p->indices) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "indices must be 4-byte aligned");
    if (p->seqlen_cache > 0) {
        if (p->logits == nullptr) return fail(FA_ERR_NULL_POINTER, "logits is NULL");
        if ((reinterpret_cast<uintptr_t>(p->logits) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "logits must be 4-byte aligned");
        if (p->logits_row_stride < 0 || p->logits_batch_stride < 0)
            return fail(FA_ERR_BAD_STRIDE, "logits strides (logits_batch_stride=%lld, logits_row_stride=%lld) must be >= 0 elements", (long long)p->logits_batch_stride,
                        (long long)p->logits_row_stride);
    }
    fa::MlaTopkParams tp;
    memset(&tp, 0, sizeof(tp));
    tp.logits = p->logits; tp.indices = p->indices; tp.cache_seqlens = p->cache_seqlens;
    tp.lg_batch = p->logits_batch_stride; tp.lg_row = p->logits_row_stride;
    tp.b = p->b; tp.seqlen_q = p->seqlen_q; tp.seqlen_cache = p->seqlen_cache; tp.topk = p->topk; tp.is_causal = p->is_causal ? 1 : 0;
    return hip_status(fa::launch_mla_indexer_topk(tp, (hipStream_t)stream), "fa_mla_indexer_topk launch");
}

// ---- MLA prefill attention -------------------------------------------------------------------------------------------------------------------
// fa_mla_prefill_params -> MlaPrefillParams, validated.  The tensor checks are those of fa_run_mha_fwd (check_tensor: alignment, strides, the 2^31-byte
// extent of one sequence); a packed call states no max_seqlen, so there the extent is the whole packed tensor's.
int fa_run_mla_prefill_fwd(const fa_mla_prefill_params* user, void* stream) {
    fa_mla_prefill_params local;
    int rc = import_exact(user, local, "fa_mla_prefill_params");
    if (rc) return rc;
    const fa_mla_prefill_params* p = &local;
    if ((rc = check_mla_prefill_front(*p))) return rc;
    if ((rc = check_mla_prefill_grid(*p, false))) return rc;
    const bool packed = p->cu_seqlens_q != nullptr;
    const int64_t rows_q = packed ? p->total_q : p->seqlen_q, rows_k = packed ? p->total_k : p->seqlen_k;
    if (p->b == 0 || rows_q == 0) return FA_OK;     // nothing to write
    if (p->lse == nullptr) return fail(FA_ERR_NULL_POINTER, "lse is NULL");
    if ((rc = check_tensor("q", p->q, p->q_stride, rows_q, p->d_qk, packed))) return rc;
    if ((rc = check_tensor("o", p->o, p->o_stride, rows_q, p->d_v, packed))) return rc;
    if (rows_k > 0) {
        if ((rc = check_tensor("k", p->k, p->k_stride, rows_k, p->d_qk, packed))) return rc;
        if ((rc = check_tensor("v", p->v, p->v_stride, rows_k, p->d_v, packed))) return rc;
    }
    fa::MlaPrefillParams kp;
    memset(&kp, 0, sizeof(kp));
    fill_mla_prefill_kp(*p, kp);
    return hip_status(fa::launch_fwd_mla_prefill(kp, p->dtype, (hipStream_t)stream), "fa_fwd_mla_prefill launch");
}

// fa_mla_prefill_bwd_params -> MlaPrefillBwdParams, validated: the forward's checks (phases and reserved_ in front of the grids), then the tensors of the backward.
int fa_run_mla_prefill_bwd(const fa_mla_prefill_bwd_params* user, void* stream) {
    fa_mla_prefill_bwd_params local;
    int rc = import_exact(user, local, "fa_mla_prefill_bwd_params");
    if (rc) return rc;
    const fa_mla_prefill_bwd_params* p = &local;
    if ((rc = check_mla_prefill_front(*p))) return rc;
    if (p->phases < 0 || p->phases > 2) return fail(FA_ERR_BAD_SHAPE, "phases %d unknown (0 = both launches, 1 = dq, 2 = dk / dv)", p->phases);
    if ((rc = check_reserved(p->reserved_, "fa_mla_prefill_bwd_params", FA_ERR_BAD_SHAPE))) return rc;
    if ((rc = check_mla_prefill_grid(*p, true))) return rc;
    const bool packed = p->cu_seqlens_q != nullptr;
    const int64_t rows_q = packed ? p->total_q : p->seqlen_q, rows_k = packed ? p->total_k : p->seqlen_k;
    if (p->b == 0 || rows_q == 0) return FA_OK;     // nothing to launch
    if (p->lse == nullptr) return fail(FA_ERR_NULL_POINTER, "lse is NULL");
    if (p->dsoftmax_sum == nullptr) return fail(FA_ERR_NULL_POINTER, "dsoftmax_sum is NULL");
    if (((reinterpret_cast<uintptr_t>(p->lse) | reinterpret_cast<uintptr_t>(p->dsoftmax_sum)) & 3u) != 0)
        return fail(FA_ERR_BAD_STRIDE, "lse / dsoftmax_sum must be 4-byte aligned");
    if ((rc = check_tensor("q", p->q, p->q_stride, rows_q, p->d_qk, packed))) return rc;
    if ((rc = check_tensor("o", p->o, p->o_stride, rows_q, p->d_v, packed))) return rc;
    if ((rc = check_tensor("dout", p->dout, p->dout_stride, rows_q, p->d_v, packed))) return rc;
    if ((rc = check_tensor("dq", p->dq, p->dq_stride, rows_q, p->d_qk, packed))) return rc;
    if (rows_k > 0) {
        if ((rc = check_tensor("k", p->k, p->k_stride, rows_k, p->d_qk, packed))) return rc;
        if ((rc = check_tensor("v", p->v, p->v_stride, rows_k, p->d_v, packed))) return rc;
        if ((rc = check_tensor("dk", p->dk, p->dk_stride, rows_k, p->d_qk, packed))) return rc;
        if ((rc = check_tensor("dv", p->dv, p->dv_stride, rows_k, p->d_v, packed))) return rc;
    }
    fa::MlaPrefillBwdParams kp;
    memset(&kp, 0, sizeof(kp));
    fill_mla_prefill_kp(*p, kp);
    kp.do_ptr = p->dout; kp.dq_ptr = p->dq; kp.dk_ptr = p->dk; kp.dv_ptr = p->dv; kp.dsum_ptr = p->dsoftmax_sum;
    kp.dout = conv(p->dout_stride); kp.dq = conv(p->dq_stride); kp.dk = conv(p->dk_stride); kp.dv = conv(p->dv_stride);
    // (with query rows but no key anywhere the dQ launch still runs: every row is dead and is written as zeros)
    return hip_status(fa::launch_bwd_mla_prefill(kp, p->dtype, p->phases ? p->phases : 3, (hipStream_t)stream), "fa_bwd_mla_prefill launch");
}

// ---- merging attention states ----------------------------------------------------------------------------------------------------------------
// fa_merge_params -> MergeStatesParams, validated.  The parts are streamed once through 64-bit addresses, so there is no 2^31-byte extent rule here; the lse
// strides may take any value (a stride of 0 or a negative one is a view like any other), the o strides follow the rule of every 16-byte load of the library.
int fa_run_merge_states(const fa_merge_params* user) {
    fa_merge_params local;
    int rc = import_exact(user, local, "fa_merge_params");
    if (rc) return rc;
    const fa_merge_params* p = &local;
    if (p->n_parts < 2 || p->n_parts > FA_MERGE_MAX_PARTS) return fail(FA_ERR_BAD_SHAPE, "n_parts %d unsupported (2 .. %d parts)", p->n_parts, FA_MERGE_MAX_PARTS);
    if (p->d_v != 64 && p->d_v != 128 && p->d_v != 256 && p->d_v != 512) return fail(FA_ERR_BAD_HEADDIM, "d_v %d unsupported (64, 128, 256 or 512)", p->d_v);
    if ((rc = check_dtype(p->dtype))) return rc;
    if (p->b < 0 || p->rows < 0 || p->h < 0) return fail(FA_ERR_BAD_SHAPE, "bad sizes b=%d rows=%d h=%d", p->b, p->rows, p->h);
    const int64_t all_rows = (int64_t)p->b * p->rows;
    const int64_t total = all_rows < ((int64_t)1 << 31) ? all_rows * p->h : 0;       // (three int32 factors fit an int64 only once two of them fit an int32)
    if (all_rows >= ((int64_t)1 << 31) || total / (fa::kMergeThreads / (p->d_v / 8)) >= ((int64_t)1 << 31) - 1)
        return fail(FA_ERR_BAD_SHAPE, "call too large: b = %d x rows = %d x h = %d (row, head) pairs exceed the launch grid", p->b, p->rows, p->h);
    if (total == 0) return FA_OK;       // nothing to write
    auto check_o = [&](const char* name, int i, const void* ptr, const fa_strides& st) -> int {
        char nm[32];
        if (i >= 0) snprintf(nm, sizeof(nm), "%s[%d]", name, i);
        else snprintf(nm, sizeof(nm), "%s", name);
        if (ptr == nullptr) return fail(FA_ERR_NULL_POINTER, "%s is NULL", nm);
        if (((uintptr_t)ptr & 15) != 0) return fail(FA_ERR_BAD_STRIDE, "%s base pointer must be 16-byte aligned", nm);
        if ((st.batch % 8) != 0 || (st.row % 8) != 0 || (st.head % 8) != 0)
            return fail(FA_ERR_BAD_STRIDE, "%s strides (batch=%lld,row=%lld,head=%lld) must be multiples of 8 elements (16-byte loads)", nm, (long long)st.batch,
                        (long long)st.row, (long long)st.head);
        return FA_OK;
    };
    auto check_l = [&](const char* name, int i, const float* ptr) -> int {
        char nm[32];
        if (i >= 0) snprintf(nm, sizeof(nm), "%s[%d]", name, i);
        else snprintf(nm, sizeof(nm), "%s", name);
        if (ptr == nullptr) return fail(FA_ERR_NULL_POINTER, "%s is NULL", nm);
        if (((uintptr_t)ptr & 3) != 0) return fail(FA_ERR_BAD_STRIDE, "%s must be 4-byte aligned", nm);
        return FA_OK;
    };
    fa::MergeStatesParams kp;
    memset(&kp, 0, sizeof(kp));
    for (int i = 0; i < p->n_parts; ++i) {
        if ((rc = check_o("o", i, p->o[i], p->o_stride[i]))) return rc;
        if ((rc = check_l("lse", i, p->lse[i]))) return rc;
        kp.o_ptr[i] = p->o[i]; kp.lse_ptr[i] = p->lse[i];
        kp.o_batch[i] = p->o_stride[i].batch; kp.o_row[i] = p->o_stride[i].row; kp.o_head[i] = p->o_stride[i].head;
        kp.l_batch[i] = p->lse_stride[i].batch; kp.l_head[i] = p->lse_stride[i].head; kp.l_row[i] = p->lse_stride[i].row;
    }
    if ((rc = check_o("out", -1, p->out, p->out_stride))) return rc;
    if ((rc = check_l("lse_out", -1, p->lse_out))) return rc;
    kp.out_ptr = p->out; kp.lse_out_ptr = p->lse_out;
    kp.out_batch = p->out_stride.batch; kp.out_row = p->out_stride.row; kp.out_head = p->out_stride.head;
    kp.lo_batch = p->lse_out_stride.batch; kp.lo_head = p->lse_out_stride.head; kp.lo_row = p->lse_out_stride.row;
    kp.total = total; kp.n_parts = p->n_parts; kp.rows = p->rows; kp.h = p->h;
    return hip_status(fa::launch_merge_states(kp, p->dtype, p->d_v, (hipStream_t)p->stream), "fa_merge_states launch");
}

// ---- stand-alone append and gather for the MLA caches ----------------------------------------------------------------------------------------
// The three structs -> MlaCacheIoParams (every stride in bytes), validated.  The movers use 64-bit offsets, so kv_new, k_pe, k_idx_new and out have no
// 2^31-byte extent rule; the caches keep the rules of the calls that read them.
int fa_run_mla_cache_append(const fa_mla_cache_append_params* user, void* stream) {
    fa_mla_cache_append_params local;
    int rc = import_exact(user, local, "fa_mla_cache_append_params");
    if (rc) return rc;
    const fa_mla_cache_append_params* p = &local;
    int64_t n_rows;
    if ((rc = check_io_rows(p->b, p->seqlen_cache, "seqlen_new", p->seqlen_new, "total_new", p->total_new, "cu_seqlens_new", p->cu_seqlens_new, n_rows))) return rc;
    if ((rc = check_dtype(p->dtype))) return rc;
    if ((rc = check_mla_format(p->kv_format, 0))) return rc;
    if ((rc = check_reserved(p->reserved_, "fa_mla_cache_append_params", FA_ERR_BAD_SHAPE))) return rc;
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    if (n_rows == 0) return FA_OK;      // nothing to write
    const bool dense = p->cu_seqlens_new == nullptr, fp8 = p->kv_format == FA_MLA_KV_FP8_ROWS656;
    if (p->cache_seqlens == nullptr) return fail(FA_ERR_NULL_POINTER, "cache_seqlens is NULL (the rows kv_new is appended at)");
    if ((rc = check_io_latent_cache(*p))) return rc;
    if ((rc = check_io_rows16("kv_new", p->kv_new, p->kv_new_stride.batch, p->kv_new_stride.row, 0, dense))) return rc;
    if (p->k_pe != nullptr && (rc = check_io_rows16("k_pe", p->k_pe, p->k_pe_stride.batch, p->k_pe_stride.row, 0, dense))) return rc;
    fa::MlaCacheIoParams io;
    memset(&io, 0, sizeof(io));
    fill_io_cache(*p, p->kv_cache, p->kv_cache_stride.batch, p->kv_cache_stride.row, fp8 ? 1 : 2, io);
    io.src = p->kv_new; io.s_batch = 2 * p->kv_new_stride.batch; io.s_row = 2 * p->kv_new_stride.row;
    if (p->k_pe != nullptr) {
        io.src_pe = p->k_pe; io.pe_batch = 2 * p->k_pe_stride.batch; io.pe_row = 2 * p->k_pe_stride.row;
    } else {
        io.src_pe = (const char*)p->kv_new + 2 * 512; io.pe_batch = io.s_batch; io.pe_row = io.s_row;
    }
    io.cu = p->cu_seqlens_new; io.n = p->seqlen_new; io.total = n_rows;
    return hip_status(fa::launch_mla_cache_append(io, p->dtype, fp8, (hipStream_t)stream), "fa_mla_cache_append launch");
}

int fa_run_mla_cache_gather(const fa_mla_cache_gather_params* user, void* stream) {
    fa_mla_cache_gather_params local;
    int rc = import_exact(user, local, "fa_mla_cache_gather_params");
    if (rc) return rc;
    const fa_mla_cache_gather_params* p = &local;
    int64_t n_rows;
    if ((rc = check_io_rows(p->b, p->seqlen_cache, "seqlen_out", p->seqlen_out, "total_out", p->total_out, "cu_seqlens_out", p->cu_seqlens_out, n_rows))) return rc;
    if ((rc = check_dtype(p->dtype))) return rc;
    if ((rc = check_mla_format(p->kv_format, 0))) return rc;
    if ((rc = check_reserved(p->reserved_, "fa_mla_cache_gather_params", FA_ERR_BAD_SHAPE))) return rc;
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    if (n_rows == 0) return FA_OK;      // nothing to write
    const bool dense = p->cu_seqlens_out == nullptr, fp8 = p->kv_format == FA_MLA_KV_FP8_ROWS656;
    if (p->seq_starts != nullptr && (reinterpret_cast<uintptr_t>(p->seq_starts) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "seq_starts must be 4-byte aligned");
    if (p->seqlen_cache > 0 && (rc = check_io_latent_cache(*p))) return rc;       // (an empty cache is never read: every row is +0)
    if ((rc = check_io_rows16("out", p->out, p->out_batch_stride, p->out_row_stride, 576, dense))) return rc;
    fa::MlaCacheIoParams io;
    memset(&io, 0, sizeof(io));
    fill_io_cache(*p, p->kv_cache, p->kv_cache_stride.batch, p->kv_cache_stride.row, fp8 ? 1 : 2, io);
    io.out = p->out; io.o_batch = 2 * p->out_batch_stride; io.o_row = 2 * p->out_row_stride;
    io.cu = p->cu_seqlens_out; io.seq_starts = p->seq_starts; io.n = p->seqlen_out; io.total = n_rows;
    return hip_status(fa::launch_mla_cache_gather(io, p->dtype, fp8, (hipStream_t)stream), "fa_mla_cache_gather launch");
}

int fa_run_mla_index_cache_append(const fa_mla_index_cache_append_params* user, void* stream) {
    fa_mla_index_cache_append_params local;
    int rc = import_exact(user, local, "fa_mla_index_cache_append_params");
    if (rc) return rc;
    const fa_mla_index_cache_append_params* p = &local;
    int64_t n_rows;
    if ((rc = check_io_rows(p->b, p->seqlen_cache, "seqlen_new", p->seqlen_new, "total_new", p->total_new, "cu_seqlens_new", p->cu_seqlens_new, n_rows))) return rc;
    if ((rc = check_dtype(p->dtype))) return rc;
    if (p->k_format != FA_MLA_KV_16BIT && p->k_format != FA_IDX_K_FP8_E4M3)
        return fail(FA_ERR_BAD_DTYPE, "k_format %d unknown (0 = keys of dtype, 1 = OCP e4m3 codes)", p->k_format);
    if (p->scale_format != FA_IDX_SCALE_FP32 && p->scale_format != FA_IDX_SCALE_UE8M0)
        return fail(FA_ERR_BAD_DTYPE, "scale_format %d unknown (0 = fp32 scales, 1 = scales rounded up to powers of two, UE8M0)", p->scale_format);
    if ((rc = check_reserved(p->reserved_, "fa_mla_index_cache_append_params", FA_ERR_BAD_SHAPE))) return rc;
    if ((rc = check_paged(p->block_table, p->block_table_stride, p->page_block_size, p->num_blocks, p->seqlen_cache))) return rc;
    const bool dense = p->cu_seqlens_new == nullptr, fp8 = p->k_format == FA_IDX_K_FP8_E4M3;
    if (!fp8 && p->k_scale != nullptr) return fail(FA_ERR_BAD_SHAPE, "k_scale given with k_format = 0 (a 16-bit index cache has no scales)");
    if (n_rows == 0) return FA_OK;      // nothing to write
    if (p->cache_seqlens == nullptr) return fail(FA_ERR_NULL_POINTER, "cache_seqlens is NULL (the rows k_idx_new is appended at)");
    if ((rc = check_idx_cache(*p))) return rc;
    if (fp8 && p->k_scale == nullptr) return fail(FA_ERR_NULL_POINTER, "k_scale is NULL (k_format = 1 writes one scale per token)");
    if (fp8 && (reinterpret_cast<uintptr_t>(p->k_scale) & 3u) != 0) return fail(FA_ERR_BAD_STRIDE, "k_scale must be 4-byte aligned");
    if ((rc = check_io_rows16("k_idx_new", p->k_idx_new, p->k_new_batch_stride, p->k_new_row_stride, 0, dense))) return rc;
    fa::MlaCacheIoParams io;
    memset(&io, 0, sizeof(io));
    fill_io_cache(*p, p->k_idx_cache, p->k_cache_batch_stride, p->k_cache_row_stride, fp8 ? 1 : 2, io);
    io.k_scale = p->k_scale; io.ks_batch = p->k_scale_batch_stride; io.ks_row = p->k_scale_row_stride;
    io.src = p->k_idx_new; io.s_batch = 2 * p->k_new_batch_stride; io.s_row = 2 * p->k_new_row_stride;
    io.cu = p->cu_seqlens_new; io.n = p->seqlen_new; io.total = n_rows;
    return hip_status(fa::launch_mla_index_cache_append(io, p->dtype, fp8 ? 1 + p->scale_format : 0, (hipStream_t)stream), "fa_mla_index_cache_append launch");
}

}  // extern "C"
