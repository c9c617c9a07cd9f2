// fa_params.hpp — kernel-side parameter blocks (passed by value in the kernarg segment).
// Counterpart of the reference's Flash_fwd_params / Flash_bwd_params (src/flash.h:6-76), with
// real element strides and 64-bit offsets (the reference's int32 offsets in block_info.h:15-21
// overflow at b=32, s=16k, h=32, d=128 = 2^31 elements).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

struct TStride {
    int64_t batch, row, head;   // in elements
};

struct FwdKernelParams {
    const void* q_ptr;
    const void* k_ptr;
    const void* v_ptr;
    void* o_ptr;
    float* lse_ptr;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    TStride q, k, v, o;
    int64_t lse_row_stride;     // elements between consecutive (batch, head) rows of lse
    int32_t b, seqlen_q, seqlen_k, h, h_k, h_ratio, d;
    int32_t is_causal;
    uint32_t n_q_tiles;         // filled by the launcher
    uint32_t varlen_slots;      // filled by the launcher: != 0 -> compact varlen grid (fa_device.hpp), 0 -> plain grid
    uint32_t group_heads;       // filled by the launcher: dispatch order of a plain causal grid (fa_device.hpp:decode_block), 0 = one head after the other
    int64_t total_q;            // packed token count of q (0 = unknown)
    float scale_log2e;          // log2(e) / sqrt(d)
    float scale;                // 1 / sqrt(d)
};

struct BwdKernelParams {
    const void* q_ptr;
    const void* k_ptr;
    const void* v_ptr;
    const void* o_ptr;
    const void* do_ptr;
    const float* lse_ptr;
    float* dsum_ptr;            // D = rowsum(dO * O), layout of lse
    void* dq_ptr;
    void* dk_ptr;
    void* dv_ptr;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    TStride q, k, v, o, dout, dq, dk, dv;
    int64_t lse_row_stride;
    int32_t b, seqlen_q, seqlen_k, h, h_k, h_ratio, d;
    int32_t is_causal;
    uint32_t n_q_tiles, n_k_tiles;
    uint32_t varlen_slots;      // per launch, like FwdKernelParams
    uint32_t group_heads;       // per launch, like FwdKernelParams
    int64_t total_q, total_k;   // packed token counts (0 = unknown)
    float scale_log2e;
    float scale;
    // dK/dV with the query-head group of a KV head split over n_split workgroups (fa_bwd.hip): fp32 partial sums
    // ws[tensor 0 = dK, 1 = dV][split][key row of the whole batch][kv head][d]; n_split = 1: no workspace, direct output
    float* ws;
    int64_t ws_bytes;
    int64_t ws_rows;            // key rows of the whole batch: b * seqlen_k, or total_k for packed tensors
    int32_t n_split;
};

// Dispatch order of a plain causal grid (fa_device.hpp:decode_block): how many (batch, head) streams of an XCD are walked together, tile index first.
// Only where the mask makes the tiles UNEVEN: seqlen_k < 2 * seqlen_q (with many more keys than queries - chunked prefill, sq 1k against sk 8k -
// every query tile sees nearly all keys, there is nothing to balance, and walking the heads together would stream each head's K / V once per
// tile instead of once: measured +23 %).  Up to 4096 rows and keys: all heads of the XCD together (longest-processing-time order across heads:
// -12..-30 % against one head after the other at 1k-4k).  Longer: ~2 workgroups per compute unit at a time, ceil(2 x 32 x wg_per_cu / tiles) heads (2
// heads at 8k rows and head_dim 128: -1..2 %; one head from 16k on = the order of rounds 1-3, where a head alone is two workgroups per unit and
// its K / V stays in the XCD's L2).  `tiles` / `rows` are those of the axis the grid walks (query tiles; key blocks for dK/dV), `wg_per_cu` the
// workgroups of this kernel a compute unit holds at a time (2 for the narrow head_dim-64 kernels); an XCD has 32 compute units.
// FA_CAUSAL_ORDER 0 = one head after the other everywhere (A/B).  profiles/r4_causal_tile_order_ab.log, r4_causal_tile_order_long_ab.log, r4_causal_group_order_ab.log
#ifndef FA_BWD_DMA_SAVE_M0
#define FA_BWD_DMA_SAVE_M0 0  // backward kernels: 1 = save / restore M0 around every hand-issued LDS-DMA piece (fa_device.hpp:dma16_to_lds_hidden).  Like the forward
                              // kernels they hold no compiler-visible LDS-DMA and nothing hipcc generates for them touches M0 (tests/test_kernel_resources_cpu.py keeps
                              // that true), so the two SALU per piece are dropped: -0.1..-1.4 %, bit-identical (profiles/r4_bwd_dma_no_m0_save_ab.log)
#endif
#ifndef FA_CAUSAL_ORDER
#define FA_CAUSAL_ORDER 1
#endif
// Packed batches on the compact grid (`compact_b` = number of sequences, 0 = plain grid): heaviest items first across sequences and heads
// (fa_device.hpp:varlen_slot_lookup_heavy_first) when there is one sequence per lane and at most 64 tiles per sequence.
#ifndef FA_VARLEN_HEAVY_FIRST
#define FA_VARLEN_HEAVY_FIRST 1
#endif
// FA_CAUSAL_GROUP_MB: up to 4096 rows the heads of an XCD are walked together only as far as the streams they re-read (K and V of a head for the
// forward / dQ, Q and dO for dK/dV) stay in reach of the cache behind the L2s: 16 x 32 heads at 2k rows in ONE group stream 4 GB per launch and
// run at 0.91 of the head-after-head time where groups of 12-24 MiB reach 0.79-0.80 (profiles/r4_causal_group_footprint_ab.log).
#ifndef FA_CAUSAL_GROUP_MB
#define FA_CAUSAL_GROUP_MB 16
#endif
inline uint32_t causal_group_heads(bool causal, int64_t compact_b, int64_t n_bh, int64_t seqlen_q, int64_t seqlen_k, int64_t tiles, int wg_per_cu,
                                   int64_t stream_bytes_per_head = 0) {
    if (FA_CAUSAL_ORDER == 0 || !causal || tiles < 2 || seqlen_k >= 2 * seqlen_q) return 0u;
    if (compact_b != 0)      // (n_bh = heads of the grid here: the XCD rule needs a multiple of 8)
        return (FA_VARLEN_HEAVY_FIRST && compact_b <= 64 && tiles <= 64 && (n_bh & 7) == 0) ? 0xffffffffu : 0u;
    if ((n_bh & 7) != 0) return 0u;
    const int64_t per_xcd = n_bh >> 3;
    int64_t g = (2 * 32 * (int64_t)wg_per_cu + tiles - 1) / tiles;                  // ~2 workgroups per compute unit
    if (seqlen_q <= 4096 && seqlen_k <= 4096) {
        // all heads together, as far as their streams fit; groups of equal size (a short last group runs unbalanced)
        int64_t cap = stream_bytes_per_head > 0 ? ((int64_t)FA_CAUSAL_GROUP_MB << 20) / stream_bytes_per_head : per_xcd;
        if (cap < g) cap = g;
        if (cap >= per_xcd) return (uint32_t)per_xcd;
        // equal groups (a short last group runs unbalanced: 8 % in profiles/r4_causal_group_order_ab.log): the largest divisor of the heads per
        // XCD within the cap, unless that is less than half of it - then near-equal groups of ceil(heads / groups)
        int64_t div = 1;
        for (int64_t c = cap; c >= 1; --c)
            if (per_xcd % c == 0) { div = c; break; }
        const int64_t n_groups = (per_xcd + cap - 1) / cap;
        g = 2 * div >= cap ? div : (per_xcd + n_groups - 1) / n_groups;
    }
    return g <= 1 ? 0u : (uint32_t)(g < per_xcd ? g : per_xcd);
}

// Decode attention over a KV cache (fa_fwd_kvcache.hip, fa_run_mha_fwd_kvcache).  The seqlen_q x h_ratio query rows of one KV head are packed
// into row tiles of kKvcRows; a workgroup serves one (batch, KV head, row tile, key split).
struct KvcacheKernelParams {
    const void* q_ptr;
    void* k_cache;
    void* v_cache;
    const void* k_new;          // NULL: no append
    const void* v_new;
    void* o_ptr;
    float* lse_ptr;             // (b, h, seqlen_q)
    const int32_t* cache_seqlens;   // (b,) or NULL = every sequence is seqlen_cache long
    TStride q, kc, vc, kn, vn, o;
    int32_t b, seqlen_q, seqlen_cache, seqlen_new, h, h_k, h_ratio, d;
    int32_t is_causal;
    int32_t n_row_tiles;        // filled by the launcher
    int32_t n_split;            // key splits (1: the attention kernel writes o / lse itself)
    int32_t split_keys;         // keys per split, a multiple of kKvcStep
    int64_t rows_total;         // b * h * seqlen_q: rows of the partial planes
    float* ws_o;                // n_split x rows_total x d fp32 partial O (normalised), n_split > 1 only
    float* ws_lse;              // n_split x rows_total partial LSE (natural log, -inf = no visible key in the split)
    float scale_log2e;
    float scale;
    // paged cache (block_table != NULL): k_cache / v_cache are pools of num_blocks pages of page_size rows, kc.batch / vc.batch the page
    // strides; logical key j of sequence i is row j % page_size of page block_table[i * bt_stride + j / page_size] (clamped to the pool)
    const int32_t* block_table;
    int64_t bt_stride;
    int32_t page_size;          // a multiple of 16: the 16 keys of an MFMA block share a page
    int32_t num_blocks;
    // sliding window (fa_kvcache_options; is_local = 0: the plain kernels, the two fields are not read).  Key j is visible to query t of a
    // sequence of length L when L - seqlen_q + t - window_left <= j <= L - seqlen_q + t + window_right; -1 = unbounded on that side.
    // Normalised by the host: window_right is 0 under causal, and a side that cannot bind (left >= seqlen_cache - 1, right >= seqlen_q - 1) is -1.
    int32_t is_local;
    int32_t window_left;
    int32_t window_right;
    // 8-bit cache (fa_kvcache_options.cache_dtype = FA_CACHE_FP8_E4M3; cache_fp8 = 0: the 16-bit kernels, the fields below are not read).
    // k_cache / v_cache hold e4m3 codes and kc / vc are strides in those 1-byte elements; element (i, j, g, :) stands for
    // code x k_descale[i * kds_batch + g * kds_head] (fp32 device arrays, NULL = 1.0), likewise V.
    int32_t cache_fp8;
    const float* k_descale;
    const float* v_descale;
    int64_t kds_batch, kds_head, vds_batch, vds_head;
};
constexpr int kKvcRows = 16;    // packed query rows of a workgroup (one 16x16x32 MFMA tile)
constexpr int kKvcStep = 32;    // keys of one wave step (the split granularity)
constexpr int kKvcPrefillRows = 64;     // packed query rows of a workgroup of the wide kernels (fa_fwd_kvcache_prefill.hip): 16 per wave
// the row tiles a launch can be sized with; launch_fwd_kvcache / launch_fwd_kvcache_ragged return hipErrorInvalidValue for anything else,
// so that a grid is never sized by one value and run by the kernels of another
inline bool kvcache_row_tile_ok(int32_t row_tile) { return row_tile == kKvcRows || row_tile == kKvcPrefillRows; }
// total_q >= 0: a ragged call (below) with that many packed query rows - the partial planes have h * total_q rows and the automatic split
// counts the compact grid's tile slots in place of b x row tiles; -1: the dense call
// row_tile: the packed query rows of a workgroup the launch is sized with - kKvcRows, or kKvcPrefillRows for the 64-row kernels of
// fa_fwd_kvcache_prefill.hip (fa_kvcache_options_v8.row_tile); the automatic split counts that grid's workgroups
int32_t kvcache_split(const KvcacheKernelParams& kp, int64_t avail_bytes, int32_t requested, int64_t total_q = -1, int32_t row_tile = kKvcRows);   // key splits of a launch (>= 1)
int64_t kvcache_workspace_bytes(const KvcacheKernelParams& kp, int32_t n_split, int64_t total_q = -1);
// Attention sinks (fa_fwd_kvcache_sink.hip, fa_kvcache_options_v6.sinks): query head hq has the logit ptr[hq * stride] (fp32, device memory,
// natural-log units of the final scores) in the softmax denominator; ptr = NULL: off.
struct KvcacheSink {
    const float* ptr;
    int64_t stride;             // in elements
};
// Tree attention mask (fa_fwd_kvcache_tree.hip, fa_kvcache_options_v7.tree_mask): query row t of sequence i reads the 64-bit word
// ptr[i * batch_stride + t * row_stride] (ragged: ptr[(packed row) * row_stride]); bit u = "sees draft token u", the key L_i - sq_i + u.
// ptr = NULL: off.
struct KvcacheTree {
    const int64_t* ptr;
    int64_t batch_stride, row_stride;   // in elements
};
// cap_pre > 0: soft-capped scores (below) - the attention launch goes to fa_fwd_kvcache_softcap.hip, the append and the combine stay
// sink.ptr != NULL: attention sinks (below) - an unsplit attention launch and the combine of a split one go to fa_fwd_kvcache_sink.hip
// tree.ptr != NULL: a tree mask (below) - the attention launch goes to fa_fwd_kvcache_tree.hip, the append and the combine stay
// row_tile = kKvcPrefillRows: the attention launch goes to fa_fwd_kvcache_prefill.hip on a grid of 64-row tiles, the append and the combine stay
hipError_t launch_fwd_kvcache(KvcacheKernelParams kp, int dtype, hipStream_t stream, float cap_pre = 0.f, KvcacheSink sink = KvcacheSink{nullptr, 0},
                              KvcacheTree tree = KvcacheTree{nullptr, 0, 0}, int32_t row_tile = kKvcRows);

// Ragged query batches (fa_fwd_kvcache_ragged.hip, fa_kvcache_options_v4): q / o are packed (total_q, h, d), sequence i owns rows cu_q[i] ..
// cu_q[i + 1] - 1 and is tiled on its own (packed row r = t * h_ratio + j in tiles of kKvcRows from the sequence's first row), k_new / v_new are
// packed the same way under cu_kn.  In kp: b = sequences, seqlen_q = max_seqlen_q (sizes the launch and the split, never what a row sees),
// seqlen_new = the largest append allowed, rows_total = h * total_q, lse_ptr (h, total_q); the batch strides of q, o, kn, vn are not read.  A block
// of its own and not fields of KvcacheKernelParams: the kernarg segment of the dense kernels stays what it was.
struct KvcacheRaggedParams {
    KvcacheKernelParams kp;
    const int32_t* cu_q;        // (b + 1,)
    const int32_t* cu_kn;       // (b + 1,) or NULL = nothing appended
    int64_t total_q;            // rows of q / o (>= cu_q[b]; the rows past it are never touched)
    int64_t total_kn;           // rows of k_new / v_new
    int32_t slots;              // filled by the launcher: tile slots per KV head of the attention grid
    int32_t compact;            // filled by the launcher: 1 = slots are looked up in cu_q (kvc_slot_lookup), 0 = slot = sequence x tiles(max_seqlen_q) + tile
};
// tile slots per KV head of a ragged launch: min(ceil(total_q * h_ratio / row_tile) + b, b * tiles(max_seqlen_q)); *compact says which
int64_t kvcache_ragged_slots(const KvcacheKernelParams& kp, int64_t total_q, int32_t* compact, int32_t row_tile = kKvcRows);
hipError_t launch_fwd_kvcache_ragged(KvcacheRaggedParams rp, int dtype, hipStream_t stream, float cap_pre = 0.f, KvcacheSink sink = KvcacheSink{nullptr, 0},
                                     KvcacheTree tree = KvcacheTree{nullptr, 0, 0}, int32_t row_tile = kKvcRows);

// The family files below each wrap instantiations of one attention body (kvcache_attn of fa_kvcache_attn.hpp, or the 64-row body of
// fa_fwd_kvcache_prefill.hip) in kernels of their own and export the launch of their attention kernel, overloaded on the dense and the ragged
// params; kvc_route_attn of fa_kvcache_launch.hpp calls them in the place of the caller's own attention launch.
// Soft-capped scores (fa_fwd_kvcache_softcap.hip, fa_kvcache_options_v5.softcap > 0): score = softcap * tanh(q . k * softmax_scale / softcap).
// The kernels are kvcache_attn with SOFTCAP = true and read kp.scale = softcap, kp.scale_log2e = softcap * log2(e) (the host puts the cap where
// the scale was) and pre = 2 log2(e) * softmax_scale / softcap, which travels in a block of its own and not in KvcacheKernelParams: the kernarg
// segment of every other kernel stays what it was.  One sliding-window instantiation serves plain, causal and windowed calls: the launchers
// below state the plain call as the window (-1, -1) and the causal one as (-1, 0), which is exactly its limit.  They launch the attention
// kernel alone, on the grid the dense / ragged launcher computed; the append in front and the combine behind are the unchanged ones.
struct KvcacheSoftcapParams {
    KvcacheKernelParams kp;
    float pre;
};
struct KvcacheRaggedSoftcapParams {
    KvcacheRaggedParams rp;
    float pre;
};
hipError_t launch_kvcache_softcap_attn(const KvcacheKernelParams& kp, float pre, int dtype, unsigned grid, hipStream_t stream);
hipError_t launch_kvcache_softcap_attn(const KvcacheRaggedParams& rp, float pre, int dtype, unsigned grid, hipStream_t stream);

// Attention sinks (fa_fwd_kvcache_sink.hip): out = sum_j exp(s_j - M) v_j / (sum_j exp(s_j - M) + exp(sink - M)) with M = max(max_j s_j, sink), and
// the LSE includes the sink.  Unsplit (n_split = 1): the kernels are kvcache_attn with SINK = true, which adds the term in the per-row epilogue;
// as with the soft cap one sliding-window instantiation serves plain, causal and windowed calls.  Split: the attention launch is the one of the
// call without sinks - same kernels, same partial planes - and the sink combine adds the term once per row as one more part of the merge.  The
// sink travels in blocks of their own and not in KvcacheKernelParams: the kernarg segment of every other kernel stays what it was.  The four
// launchers take kp / rp as the dense / ragged launcher finished them; sinks with a soft cap or at head_dim 256 are refused by the C ABI.
struct KvcacheSinkParams {
    KvcacheKernelParams kp;
    KvcacheSink sink;
};
struct KvcacheRaggedSinkParams {
    KvcacheRaggedParams rp;
    KvcacheSink sink;
};
hipError_t launch_kvcache_sink_attn(const KvcacheKernelParams& kp, const KvcacheSink& sink, int dtype, unsigned grid, hipStream_t stream);
hipError_t launch_kvcache_sink_attn(const KvcacheRaggedParams& rp, const KvcacheSink& sink, int dtype, unsigned grid, hipStream_t stream);
hipError_t launch_kvcache_sink_combine(const KvcacheKernelParams& kp, const KvcacheSink& sink, int dtype, hipStream_t stream);
hipError_t launch_kvcache_sink_combine(const KvcacheRaggedParams& rp, const KvcacheSink& sink, int dtype, hipStream_t stream);

// Tree attention masks (fa_fwd_kvcache_tree.hip): the kernels are kvcache_attn with TREE = true - the plain (non-causal) body over the steps
// [0, L) whose select tests a bit of the row's mask word for the last sq keys.  They launch the attention kernel alone, split or not, on the grid
// the dense / ragged launcher computed: the append in front, the partial planes and the combine behind are the unchanged ones, so the split count
// and the workspace do not know about the mask.  The mask travels in blocks of their own and not in KvcacheKernelParams: the kernarg segment of
// every other kernel stays what it was.  A tree mask with causal, a window, a soft cap, sinks, rotary or head_dim 256 is refused by the C ABI.
struct KvcacheTreeParams {
    KvcacheKernelParams kp;
    KvcacheTree tree;
};
struct KvcacheRaggedTreeParams {
    KvcacheRaggedParams rp;
    KvcacheTree tree;
};
hipError_t launch_kvcache_tree_attn(const KvcacheKernelParams& kp, const KvcacheTree& tree, int dtype, unsigned grid, hipStream_t stream);
hipError_t launch_kvcache_tree_attn(const KvcacheRaggedParams& rp, const KvcacheTree& tree, int dtype, unsigned grid, hipStream_t stream);

// 64-row workgroups for prompt chunks (fa_fwd_kvcache_prefill.hip, fa_kvcache_options_v8.row_tile = 64): four waves of 16 rows each walk the same
// 32-key steps over K / V images staged once per workgroup in LDS, double-buffered; no merge of waves, the epilogue writes o / lse or the partial
// planes of the decode kernels.  The kernels read KvcacheKernelParams / KvcacheRaggedParams as they are, with n_row_tiles / slots counted in tiles
// of kKvcPrefillRows.  They launch the attention kernel alone, split or not; the append in front and the combine behind are the unchanged ones.
// A window, a soft cap, sinks, a tree mask, rotary and head_dim 256 are refused by the C ABI with row_tile = 64.
hipError_t launch_kvcache_prefill_attn(const KvcacheKernelParams& kp, int dtype, unsigned grid, hipStream_t stream);
hipError_t launch_kvcache_prefill_attn(const KvcacheRaggedParams& rp, int dtype, unsigned grid, hipStream_t stream);

// Multi-head latent attention over a latent KV cache (fa_fwd_kvcache_mla.hip, fa_run_mla_fwd_kvcache): MQA over one KV head whose key is the d_qk = 576
// wide latent row and whose value is the first kp.d = 512 columns of the same row.  In kp: k_cache = the latent cache (v_cache, vc, v_new, vn are not
// read), k_new / kn the new rows, h_k = 1, h_ratio = h, d = 512 - the width of o and of the partial planes, which kvcache_split and
// kvcache_workspace_bytes size (row_tile = kKvcPrefillRows).  A block of its own and not fields of KvcacheKernelParams: the kernarg segment of every
// other kernel stays what it was.  The launcher fills row tiles, split keys and the LSE plane like launch_fwd_kvcache.
struct KvcacheMlaParams {
    KvcacheKernelParams kp;
    int32_t d_qk;               // 576: 512 compressed columns, then 64 rope columns
};
hipError_t launch_fwd_kvcache_mla(KvcacheMlaParams mp, int dtype, hipStream_t stream);

// Sparse MLA decode (fa_fwd_kvcache_mla_sparse.hip, fa_run_mla_sparse_fwd_kvcache): the same latent cache, but query token t of sequence i attends to the
// rows its list names: indices[i * idx_batch + t * idx_row + s], s < topk (a positive multiple of kKvcStep), a logical key position that is valid iff
// 0 <= . < L_i.  kp as in KvcacheMlaParams without k_new / seqlen_new / is_causal; the split runs over the slots [0, topk) and the grid is
// b x seqlen_q x ceil(h / kKvcPrefillRows) x n_split, which the launcher states to kvcache_split / finish_params as seqlen_q = 1, seqlen_cache = topk.
struct KvcacheMlaSparseParams {
    KvcacheKernelParams kp;
    int32_t d_qk;               // 576
    int32_t topk;
    const int32_t* indices;
    int64_t idx_batch, idx_row; // in elements
};
hipError_t launch_fwd_kvcache_mla_sparse(KvcacheMlaSparseParams sp, int dtype, hipStream_t stream);

// The two MLA calls over an FP8 latent cache of 656-byte rows (fa_fwd_kvcache_mla_fp8.hip, kv_format = FA_MLA_KV_FP8_ROWS656): 512 e4m3 codes, four fp32
// scales (one per 128 codes), then the 64 rope elements in q's dtype.  The same params with kp.cache_fp8 = 1 and kp.kc in BYTES; k_new / kn stay 16-bit
// rows of 576 elements, quantised by the append.  Split, workspace and partial planes are those of the 16-bit launchers above.
hipError_t launch_fwd_kvcache_mla_fp8(KvcacheMlaParams mp, int dtype, hipStream_t stream);
hipError_t launch_fwd_kvcache_mla_sparse_fp8(KvcacheMlaSparseParams sp, int dtype, hipStream_t stream);

// MLA prefill attention (fa_fwd_mla_prefill.hip, fa_run_mla_prefill_fwd): multi-head attention with 192-wide q / k (128 no-rope columns, then 64 rope
// columns) and 128-wide v / o, before weight absorption.  Dense: q (b, seqlen_q, h, 192), k (b, seqlen_k, h_k, 192), v (b, seqlen_k, h_k, 128), lse
// (b, h, seqlen_q).  Packed (cu_q != NULL): q (total_q, h, 192), k / v (total_k, h_k, .), sequence i owns rows cu_q[i] .. cu_q[i + 1] - 1 of q / o and
// cu_k[i] .. cu_k[i + 1] - 1 of k / v, lse (h, total_q); seqlen_q / seqlen_k and the batch strides are not read.  The LDS-staged body of
// fa_fwd_kvcache_prefill.hip over plain tensors: no cache, no append, no key split.  A block of its own: no other kernel's kernarg segment changes.
struct MlaPrefillParams {
    const void* q_ptr;
    const void* k_ptr;
    const void* v_ptr;
    void* o_ptr;
    float* lse_ptr;
    const int32_t* cu_q;        // (b + 1,) or NULL = dense
    const int32_t* cu_k;
    TStride q, k, v, o;
    int32_t b, seqlen_q, seqlen_k, h, h_k, h_ratio;
    int32_t is_causal;
    int32_t n_row_tiles;        // filled by the launcher (dense): row tiles of a (batch, KV head)
    int32_t slots;              // filled by the launcher (packed): tile slots per KV head, ceil(total_q * h_ratio / rows of a tile) + b
    int64_t total_q, total_k;   // packed: rows of q / o and of k / v (>= cu_q[b] / cu_k[b]; the rows past them are never touched)
    float scale_log2e;
    float scale;
};
hipError_t launch_fwd_mla_prefill(MlaPrefillParams p, int dtype, hipStream_t stream);

// The backward of the above (fa_bwd_mla_prefill.hip, fa_run_mla_prefill_bwd): two launches on one stream, dQ (which also writes D = rowsum(dO * O) to
// dsum_ptr, fp32 in the layout of lse) and then dK / dV, which reads it.  Tensors, packing and strides as in MlaPrefillParams; dout is shaped like o, dq /
// dk / dv like q / k / v.  No atomics, no workspace besides dsum.  A block of its own: no other kernel's kernarg segment changes.
struct MlaPrefillBwdParams {
    const void* q_ptr;
    const void* k_ptr;
    const void* v_ptr;
    const void* o_ptr;
    const void* do_ptr;
    void* dq_ptr;
    void* dk_ptr;
    void* dv_ptr;
    const float* lse_ptr;
    float* dsum_ptr;
    const int32_t* cu_q;        // (b + 1,) or NULL = dense
    const int32_t* cu_k;
    TStride q, k, v, o, dout, dq, dk, dv;
    int32_t b, seqlen_q, seqlen_k, h, h_k, h_ratio;
    int32_t is_causal;
    int32_t n_row_tiles;        // filled by the launcher per launch (dense): row tiles (dQ) or key tiles (dK/dV) of a (batch, KV head)
    int32_t slots;              // filled by the launcher per launch (packed): tile slots per KV head, ceil(total * (h_ratio or 1) / 64) + b
    int64_t total_q, total_k;
    float scale_log2e;
    float scale;
};
hipError_t launch_bwd_mla_prefill(MlaPrefillBwdParams p, int dtype, int phases, hipStream_t stream);     // phases: 1 = dQ + D, 2 = dK / dV, 3 = both

// Rotary embedding on a decode call (fa_kvcache_rotary.hip, fa_kvcache_options_v3).  One fused launch takes the place of the append: it
// rotates k_new into the cache, copies / quantises v_new, and writes the rotated q into `q_image`, a contiguous (b, seqlen_q, h, d) buffer of
// q's dtype at the head of the caller's workspace; the attention kernels then read that image as their q.  A block of its own and not
// fields of KvcacheKernelParams: the kernarg segment of the attention, append and combine kernels stays what it was.
struct KvcacheRotaryParams {
    KvcacheKernelParams kp;     // the call as the append kernels see it (q_ptr / q: the caller's q)
    const void* cos;            // (seqlen_ro, rotary_dim / 2), q's dtype, rows `row_stride` elements apart
    const void* sin;
    int64_t row_stride;
    void* q_image;
    int32_t seqlen_ro;          // >= 1; positions are clamped to seqlen_ro - 1
    int32_t rotary_dim;         // a multiple of 16 in [16, d]
    int32_t interleaved;        // 0: pairs (i, i + rotary_dim / 2) (GPT-NeoX), else (2 i, 2 i + 1) (GPT-J)
    int32_t q_pos_per_row;      // query row t sits at cache_seqlens[i] + t (causal or windowed call), else every row at cache_seqlens[i]
};
int64_t kvcache_rotary_image_bytes(const KvcacheKernelParams& kp);     // bytes of q_image, rounded up to 16
hipError_t launch_kvcache_rotary(const KvcacheRotaryParams& rp, int dtype, hipStream_t stream);

// head_dim 256 (fa_fwd_kvcache_d256.hip): every kernel of a decode call at d = 256 - attention, append, combine, rotary - is instantiated in that file
// (from the same headers as at 64 / 128), built for ONE workgroup per compute unit.  The three launchers above finish kp / rp exactly as for 64 / 128 (row tiles, slots, split,
// workspace planes) and hand over here where they would pick their own instantiations.
hipError_t launch_kvcache_d256(const KvcacheKernelParams& kp, int dtype, hipStream_t stream, float cap_pre);
hipError_t launch_kvcache_ragged_d256(const KvcacheRaggedParams& rp, int dtype, hipStream_t stream, float cap_pre);
hipError_t launch_kvcache_rotary_d256(const KvcacheRotaryParams& rp, int dtype, hipStream_t stream);

// query-head group split chosen for a dK/dV launch (1 = none) and the workspace it needs
int32_t dkdv_split(const BwdKernelParams& kp, int64_t avail_bytes);
int64_t dkdv_workspace_bytes(const BwdKernelParams& kp, int32_t n_split);

hipError_t launch_fwd(FwdKernelParams kp, int dtype, hipStream_t stream);
const char* fwd_kernel_name(int d);
const char* fwd_kernel_name_for(const FwdKernelParams& kp, int dtype);                 // the kernel launch_fwd would pick for this problem
const char* bwd_kernel_name_for(const BwdKernelParams& kp, bool dkdv);      // ... launch_bwd_dq / launch_bwd_dkdv
int set_kernel_policy(int policy);      // FA_POLICY_* of the public header; returns the previous one, -1 for an unknown value
int kernel_policy();
// FA_POLICY_AUTO sizes a head_dim-128 launch by its workgroup count (round 6): (batch x heads) x tiles.  A caller that runs a (batch, head) SHARD of a problem and wants the
// kernels - hence the bits - of the whole problem states the whole problem's batch x heads here (0 = the launch's own); flash_attn_turing/sharding.py:problem_policy
int64_t set_policy_problem_heads(int64_t batch_times_heads);      // returns the previous value, -1 (and changes nothing) for a negative one
int64_t policy_bh(int64_t b, int64_t h);                          // the batch x heads FA_POLICY_AUTO sizes this launch with
int64_t device_cu_count();                                         // compute units of the current device (256 without one)
hipError_t launch_bwd_dot_do_o(BwdKernelParams kp, int dtype, hipStream_t stream);
hipError_t launch_bwd_dq(BwdKernelParams kp, int dtype, hipStream_t stream);
hipError_t launch_bwd_dkdv(BwdKernelParams kp, int dtype, hipStream_t stream);

}  // namespace fa
