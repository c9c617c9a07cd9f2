// fa_mla_indexer.hpp — kernel parameters and launchers of the DeepSeek-V3.2 indexer (fa_mla_indexer.hip): FP8 / 16-bit index logits over an index-key
// cache, and the top-k selection that turns a row of logits into the `indices` of fa_run_mla_sparse_fwd_kvcache.  Filled and validated by fa_capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.hpp"

namespace fa {

constexpr int kIdxD = 128;          // width of an index head and of an index key
constexpr int kIdxStep = 32;        // keys a wave takes per step (two 16-key MFMA column blocks)
constexpr int kIdxWaves = 4;        // waves of a logits workgroup; each walks its own steps, nothing is shared
constexpr int kIdxThreads = 64 * kIdxWaves;
constexpr int kIdxMaxWgKeys = 4096; // the longest key range of one logits workgroup
constexpr int kTopkThreads = 1024;  // one selection workgroup per (sequence, token) row

struct MlaIndexerParams {
    const void* q_ptr;              // (b, sq, h, 128) of `dtype`
    const float* w_ptr;             // (b, sq, h) fp32
    const void* k_cache;            // (b, capacity, 128) or a pool (num_blocks, page, 128): elements of `dtype`, or e4m3 codes (cache_fp8)
    const float* k_scale;           // nullptr = 1.0; one fp32 per cached token, addressed like the cache
    float* logits;                  // (b, sq, capacity) fp32
    const int32_t* cache_seqlens;   // nullptr: every sequence holds seqlen_cache keys
    const int32_t* block_table;     // nullptr: contiguous
    int64_t q_batch, q_row, q_head;             // elements
    int64_t w_batch, w_row, w_head;             // elements
    int64_t k_batch, k_row;                     // BYTES (batch = page when paged)
    int64_t ks_batch, ks_row;                   // elements
    int64_t lg_batch, lg_row;                   // elements
    int64_t bt_stride;
    int b, seqlen_q, seqlen_cache, h;
    int is_causal, cache_fp8;
    int page_size, num_blocks;
    int wg_keys, n_chunks;          // keys of a workgroup's range (a multiple of kIdxStep * kIdxWaves; prefill: of kIdxStep) and ranges per token / tile: set by the launcher
};

struct MlaTopkParams {
    const float* logits;            // (b, sq, capacity) fp32, last dimension contiguous
    int32_t* indices;               // (b, sq, topk) int32, contiguous
    const int32_t* cache_seqlens;
    int64_t lg_batch, lg_row;       // elements
    int b, seqlen_q, seqlen_cache, topk;
    int is_causal;
};

// keys token t of a sequence with L cached keys sees: the rule of the dense MLA call
__host__ __device__ inline int idx_visible(int L, int seqlen_q, int t, int is_causal) {
    if (!is_causal) return L;
    const int n = L - seqlen_q + t + 1;
    return n < 0 ? 0 : (n < L ? n : L);
}

// ---- device helpers the logits kernels of fa_mla_indexer.hip and fa_mla_indexer_prefill.hip share ------------------------------------------------
// eight e4m3 codes -> eight elements of T, exactly (every e4m3 value is an fp16 and a bf16 value)
template <typename T>
FA_DEV u32x4 idx_widen8(uint32_t w0, uint32_t w1) {
    if constexpr (__is_same(T, _Float16)) {
        return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true))};
    } else {
        return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true))};
    }
}

// relu(x) that keeps a NaN: the IEEE 754-2019 maximum (v_maximum3_f32), where the fmaxf of fa_mla_indexer.hip (v_max_f32, maximumNumber) returns 0 for a NaN
// dot product.  For every x that is not a NaN both give the same bits, so the bit relation to the decode call holds wherever no visible key holds a NaN; a
// NaN key gives NaN in its column here and 0 there.  (The 16-bit q_idx prefill kernels and both FP8 q_idx kernels use this one.)
FA_DEV float idxp_relu(float x) { return __builtin_elementwise_maximum(x, 0.f); }

// ---- FP8 q_idx (fa_mla_indexer_fp8q.hip, fa_mla_indexer_prefill_fp8q.hip): a whole 128-wide index head in one MFMA ------------------------------------
// acc += A B on v_mfma_f32_16x16x128_f8f6f4, both operands OCP e4m3 (format selectors 0 / 0), no block scales (the scale operands are literal zeros: the
// unscaled encoding).  A lane's operand is 32 codes: lo = bytes 16 g .. 16 g + 15, hi = bytes 64 + 16 g .. of row lane & 15 (g = lane >> 4), for A (a head of Q)
// and B (a key) alike.  Nothing is assumed about which contraction index the instruction gives each of those 32 bytes beyond "A and B of one lane group use
// the same ones": both sides permute the 128 columns identically, so the sum covers every column once.  C / D: lane = column (key) lane & 15, register r =
// row (head) 4 g + r, as for 16x16x32.
typedef int i32x8 __attribute__((ext_vector_type(8)));
FA_DEV f32x4 idx_mfma_e4m3(const u32x4& alo, const u32x4& ahi, const u32x4& blo, const u32x4& bhi, f32x4 acc) {
    const i32x8 a = {(int)alo.x, (int)alo.y, (int)alo.z, (int)alo.w, (int)ahi.x, (int)ahi.y, (int)ahi.z, (int)ahi.w};
    const i32x8 b = {(int)blo.x, (int)blo.y, (int)blo.z, (int)blo.w, (int)bhi.x, (int)bhi.y, (int)bhi.z, (int)bhi.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, 0, 0, 0);
}

FA_DEV int idx_len(const int32_t* cache_seqlens, int bidx, int seqlen_cache) {
    int L = seqlen_cache;
    if (cache_seqlens != nullptr) {
        const int cs = cache_seqlens[bidx];
        L = min(cs > 0 ? cs : 0, seqlen_cache);
    }
    return __builtin_amdgcn_readfirstlane(L);
}

int64_t mla_indexer_logits_shape(MlaIndexerParams& p);    // wg_keys, n_chunks -> the grid; 0: not launchable (host only)
hipError_t launch_mla_indexer_logits(MlaIndexerParams p, int dtype, hipStream_t s);
hipError_t launch_mla_indexer_topk(const MlaTopkParams& p, hipStream_t s);

// ---- the prefill logits launch (fa_mla_indexer_prefill.hip): a workgroup serves kIdxpTQ consecutive tokens of one sequence and wg_keys keys ----------
#ifndef FA_IDXP_TQ
#define FA_IDXP_TQ 8
#endif
constexpr int kIdxpTQ = FA_IDXP_TQ;         // tokens of a tile: 4 = one a wave, 8 = two a wave
constexpr int kIdxpMinWgKeys = 256;         // the shortest key range of a prefill workgroup: eight steps over which the tile's Q load is spread

// wg_keys and n_chunks of a prefill launch over p.b x ceil(p.seqlen_q / kIdxpTQ) tiles (host only; p.seqlen_q >= 1)
void mla_indexer_prefill_shape(MlaIndexerParams& p);
hipError_t launch_mla_indexer_prefill_logits(MlaIndexerParams p, int dtype, hipStream_t s);

// ---- FP8 (e4m3) q_idx over an FP8 cache: the launches above with q_ptr holding codes and q_batch / q_row / q_head in bytes (p.cache_fp8 is set) ----------
hipError_t launch_mla_indexer_logits_fp8q(MlaIndexerParams p, hipStream_t s);             // fa_mla_indexer_fp8q.hip
hipError_t launch_mla_indexer_prefill_logits_fp8q(MlaIndexerParams p, hipStream_t s);     // fa_mla_indexer_prefill_fp8q.hip

}  // namespace fa
