// fa_mla_indexer.hpp — kernel parameters and launchers of the DeepSeek-V3.2 indexer (fa_mla_indexer.hip): FP8 / 16-bit index logits over an index-key
// cache, and the top-k selection that turns a row of logits into the `indices` of fa_run_mla_sparse_fwd_kvcache.  Filled and validated by fa_capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
    int wg_keys, n_chunks;          // keys of a workgroup's range (a multiple of kIdxStep * kIdxWaves) and ranges per token: set by the launcher
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

hipError_t launch_mla_indexer_logits(MlaIndexerParams p, int dtype, hipStream_t s);
hipError_t launch_mla_indexer_topk(const MlaTopkParams& p, hipStream_t s);

}  // namespace fa
