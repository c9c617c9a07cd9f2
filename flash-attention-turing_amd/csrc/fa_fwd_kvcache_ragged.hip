// fa_fwd_kvcache_ragged.hip — decode attention over a KV cache for ragged query batches (fa_kvcache_options_v4: cu_seqlens_q / cu_seqlens_k_new).
//
// One scheduler step of a serving engine - sequences that decode one token, verify a few speculative ones or bring a chunk of their prompt - as
// ONE call: q / o are packed (total_q, h, d), k_new / v_new (total_k_new, h_k, d), sequence i owns the rows cu[i] .. cu[i + 1] - 1.
//   * The attention body is kvcache_attn of fa_fwd_kvcache.hip with RAGGED = true (this file includes that one for it): every sequence is tiled
//     on its own, packed row r = t * h_ratio + j in tiles of kKvcRows from the sequence's first row, exactly as the dense kernel tiles a batch
//     entry, and a lane owns one query row with private softmax statistics - so sequence i of a ragged call goes through the very steps of the
//     dense call on it alone and gives its bits.
//   * The grid is sized by the tokens present: slots x h_k x n_split workgroups with slots = ceil(total_q * h_ratio / kKvcRows) + b >= the sum
//     of the sequences' tiles; a workgroup finds its (sequence, tile) with kvc_slot_lookup (one round of loads and a wave prefix sum per 512
//     sequences) and slack slots exit without writing.  Where b x tiles(max_seqlen_q) is no larger - uniform decode batches - the slot is
//     decoded by a division and nothing is looked up.
//   * Rows of the LSE and of the split partials are (head, packed row): rows_total = h * total_q.  The combine skips packed rows at or past
//     cu_seqlens_q[b]: no split wrote them a partial, and their o / lse entries belong to the caller.
//   * The append finds a packed new row's sequence by bisection in cu_seqlens_k_new and writes cache row max(cache_seqlens[i], 0) + s, through
//     the table when paged, quantised when the cache is 8-bit.  Rows that would land at or past the capacity are dropped, as in the dense append.
#define FA_KVC_RAGGED_TU 1
#include "fa_fwd_kvcache.hip"

namespace fa {

namespace {

// MODE 0: every key below L, 1: causal, 2: sliding window (the causal limit arrives as window_right = 0)
template <typename T, int D, int MODE, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_kernel(const KvcacheRaggedParams rp) {
    kvcache_attn<T, D, MODE == 1, PAGED, MODE == 2, ES, true>(rp.kp, &rp);
}

// fa_kvcache_combine_kernel over the h * total_q rows of a ragged call: row R = hq * total_q + (packed query row)
template <typename T, int D>
__global__ __launch_bounds__(kKvcCombineThreads) void fa_kvcache_combine_ragged_kernel(const KvcacheRaggedParams rp) {
    const KvcacheKernelParams& p = rp.kp;
    constexpr int TPR = D / 8;                              // threads per row, 8 columns each
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)blockIdx.x * (kKvcCombineThreads / TPR) + tid / TPR;
    if (R >= p.rows_total) return;
    const int hq = (int)(R / rp.total_q);
    const int64_t row = R - (int64_t)hq * rp.total_q;
    if (row >= rp.cu_q[p.b]) return;                        // a surplus row of q: no partial was written, o / lse stay the caller's
    const int col = (tid % TPR) * 8;
    const int ns = p.n_split;
    float M = -INFINITY;
    bool nan_part = false;
    for (int s = 0; s < ns; ++s) {
        const float ls = p.ws_lse[(int64_t)s * p.rows_total + R];
        nan_part |= __builtin_isnan(ls);
        M = fmaxf(M, ls);
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float sum = 0.f;
    if (M != -INFINITY) {
        for (int s = 0; s < ns; ++s) {
            const float ls = p.ws_lse[(int64_t)s * p.rows_total + R];
            if (ls == -INFINITY) continue;
            const float w = __expf(ls - M);
            sum += w;
            const f32x4* src = (const f32x4*)(p.ws_o + ((int64_t)s * p.rows_total + R) * D + col);
            const f32x4 x0 = src[0], x1 = src[1];
            static_for<0, 4>([&](auto ee) {
                constexpr int e = decltype(ee)::value;
                acc[e] += w * x0[e];
                acc[4 + e] += w * x1[e];
            });
        }
    }
    if (nan_part) sum = __builtin_nanf("");
    const bool live = !(sum == 0.f);
    const float inv = live ? 1.0f / sum : 0.f;
    char* orow = (char*)p.o_ptr + 2 * (row * p.o.row + (int64_t)hq * p.o.head + col);
    *(u32x4*)orow = u32x4{LP<T>::pack2(acc[0] * inv, acc[1] * inv), LP<T>::pack2(acc[2] * inv, acc[3] * inv),
                          LP<T>::pack2(acc[4] * inv, acc[5] * inv), LP<T>::pack2(acc[6] * inv, acc[7] * inv)};
    if (tid % TPR == 0) p.lse_ptr[R] = live ? M + logf(sum) : 0.f;
}

// k_new / v_new (total_kn, h_k, d) -> the caches.  One thread per 8 elements of a packed new row r; its sequence is the i with cu_kn[i] <= r <
// cu_kn[i + 1] (bisection over the b + 1 entries; empty sequences share a value and are stepped over), rows at or past cu_kn[b] are not read.
// The row goes to cache row max(cache_seqlens[i], 0) + (r - cu_kn[i]); at or past the capacity seqlen_cache it is dropped, so nothing is written
// outside the sequence's capacity or, through a clamped table entry, outside the pool.  ES = 1: quantised as in fa_kvcache_append_fp8_kernel.
template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_kernel(const KvcacheRaggedParams rp) {
    const KvcacheKernelParams& p = rp.kp;
    constexpr int SLOTS = D / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = rp.total_kn * p.h_k * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    int64_t r = i / SLOTS;
    const int kvh = (int)(r % p.h_k);
    r /= p.h_k;
    int lo = 0, hi = p.b;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rp.cu_kn[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    if (lo >= p.b) return;                                  // a surplus row past cu_kn[b]
    const int bidx = lo;
    const int64_t t = r - rp.cu_kn[bidx];
    if (t < 0) return;                                      // (cu_kn[0] > 0: rows in front of the first sequence belong to nobody)
    const int cs = p.cache_seqlens[bidx];
    const int64_t row = (int64_t)(cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return;
    int64_t blk = bidx, prow = row;
    if constexpr (PAGED) {
        const int col = (int)(row / p.page_size);
        prow = row - (int64_t)col * p.page_size;
        blk = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
    }
    const u32x4 kx = *(const u32x4*)((const char*)p.k_new + 2 * (r * p.kn.row + (int64_t)kvh * p.kn.head + 8 * slot));
    const u32x4 vx = *(const u32x4*)((const char*)p.v_new + 2 * (r * p.vn.row + (int64_t)kvh * p.vn.head + 8 * slot));
    char* kdst = (char*)p.k_cache + ES * (blk * p.kc.batch + prow * p.kc.row + (int64_t)kvh * p.kc.head + 8 * slot);
    char* vdst = (char*)p.v_cache + ES * (blk * p.vc.batch + prow * p.vc.row + (int64_t)kvh * p.vc.head + 8 * slot);
    if constexpr (ES == 1) {
        const float kd = p.k_descale != nullptr ? p.k_descale[(int64_t)bidx * p.kds_batch + (int64_t)kvh * p.kds_head] : 1.f;
        const float vd = p.v_descale != nullptr ? p.v_descale[(int64_t)bidx * p.vds_batch + (int64_t)kvh * p.vds_head] : 1.f;
        *(u32x2*)kdst = quant8_e4m3<T>(kx, kd);
        *(u32x2*)vdst = quant8_e4m3<T>(vx, vd);
    } else {
        *(u32x4*)kdst = kx;
        *(u32x4*)vdst = vx;
    }
}

template <typename T, int D, bool PAGED, int ES>
void launch_ragged_attn(const KvcacheRaggedParams& rp, unsigned grid, hipStream_t s) {
    const KvcacheKernelParams& kp = rp.kp;
    if (kp.is_local) hipLaunchKernelGGL((fa_fwd_kvcache_ragged_kernel<T, D, 2, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, rp);
    else if (kp.is_causal) hipLaunchKernelGGL((fa_fwd_kvcache_ragged_kernel<T, D, 1, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, rp);
    else hipLaunchKernelGGL((fa_fwd_kvcache_ragged_kernel<T, D, 0, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, rp);
}

template <typename T, int D, int ES>
hipError_t launch_kvcache_ragged_t(const KvcacheRaggedParams& rp, hipStream_t s, float cap_pre, const KvcacheSink& sink, const KvcacheTree& tree, int32_t row_tile) {
    const KvcacheKernelParams& kp = rp.kp;
    const bool paged = kp.block_table != nullptr;
    if (kp.k_new != nullptr && rp.cu_kn != nullptr && rp.total_kn > 0) {
        const int64_t n = rp.total_kn * kp.h_k * (D / 8);
        const dim3 grid((unsigned)((n + 255) / 256));
        // (the 16-bit append copies bits: one instantiation serves both dtypes)
        using TA = std::conditional_t<ES == 1, T, _Float16>;
        if (paged) hipLaunchKernelGGL((fa_kvcache_append_ragged_kernel<TA, D, true, ES>), grid, dim3(256), 0, s, rp);
        else hipLaunchKernelGGL((fa_kvcache_append_ragged_kernel<TA, D, false, ES>), grid, dim3(256), 0, s, rp);
    }
    if (rp.total_q > 0) {
        const int64_t grid = (int64_t)rp.slots * kp.h_k * kp.n_split;
        if (row_tile == kKvcPrefillRows) {     // 64-row workgroups: the attention kernels of fa_fwd_kvcache_prefill.hip
            const hipError_t e = launch_kvcache_ragged_prefill_attn(rp, std::is_same_v<T, _Float16> ? 0 : 1, (unsigned)grid, s);
            if (e != hipSuccess) return e;
        } else if (cap_pre > 0.f) {    // soft-capped scores: the attention kernels of fa_fwd_kvcache_softcap.hip between this file's append and combine
            const hipError_t e = launch_kvcache_ragged_softcap_attn(rp, cap_pre, std::is_same_v<T, _Float16> ? 0 : 1, (unsigned)grid, s);
            if (e != hipSuccess) return e;
        } else if (sink.ptr != nullptr && kp.n_split == 1) {    // sinks, unsplit: the attention kernels of fa_fwd_kvcache_sink.hip
            const hipError_t e = launch_kvcache_ragged_sink_attn(rp, sink, std::is_same_v<T, _Float16> ? 0 : 1, (unsigned)grid, s);
            if (e != hipSuccess) return e;
        } else if (tree.ptr != nullptr) {      // a tree mask: the attention kernels of fa_fwd_kvcache_tree.hip
            const hipError_t e = launch_kvcache_ragged_tree_attn(rp, tree, std::is_same_v<T, _Float16> ? 0 : 1, (unsigned)grid, s);
            if (e != hipSuccess) return e;
        } else if (paged) launch_ragged_attn<T, D, true, ES>(rp, (unsigned)grid, s);
        else launch_ragged_attn<T, D, false, ES>(rp, (unsigned)grid, s);
        if (kp.n_split > 1) {
            // (sinks: the combine of fa_fwd_kvcache_sink.hip, which adds the sink as one more term of the merge)
            if (sink.ptr != nullptr) return launch_kvcache_ragged_sink_combine(rp, sink, std::is_same_v<T, _Float16> ? 0 : 1, s);
            const int64_t rows_per_block = kKvcCombineThreads / (D / 8);
            hipLaunchKernelGGL((fa_kvcache_combine_ragged_kernel<T, D>), dim3((unsigned)((kp.rows_total + rows_per_block - 1) / rows_per_block)),
                               dim3(kKvcCombineThreads), 0, s, rp);
        }
    }
    return hipGetLastError();
}

template <typename T, int D>
hipError_t launch_kvcache_ragged_es(const KvcacheRaggedParams& rp, hipStream_t s, float cap_pre, const KvcacheSink& sink, const KvcacheTree& tree, int32_t row_tile) {
    return rp.kp.cache_fp8 ? launch_kvcache_ragged_t<T, D, 1>(rp, s, cap_pre, sink, tree, row_tile) : launch_kvcache_ragged_t<T, D, 2>(rp, s, cap_pre, sink, tree, row_tile);
}

}  // namespace

#ifndef FA_KVC_D256_TU      // (fa_fwd_kvcache_d256.hip includes this file for the templates above)
// kp.seqlen_q = max_seqlen_q sizes the split exactly as the dense launcher does (kvcache_steps), so a forced split cuts the keys where the dense
// call with seqlen_q = max_seqlen_q cuts them.
hipError_t launch_fwd_kvcache_ragged(KvcacheRaggedParams rp, int dtype, hipStream_t s, float cap_pre, KvcacheSink sink, KvcacheTree tree, int32_t row_tile) {
    if (!kvcache_row_tile_ok(row_tile)) return hipErrorInvalidValue;
    KvcacheKernelParams& kp = rp.kp;
    kp.n_row_tiles = (int32_t)(((int64_t)kp.seqlen_q * kp.h_ratio + row_tile - 1) / row_tile);
    kp.rows_total = (int64_t)kp.h * rp.total_q;
    rp.slots = (int32_t)kvcache_ragged_slots(kp, rp.total_q, &rp.compact, row_tile);
    const int64_t steps = kvcache_steps(kp);
    if (kp.n_split < 1) kp.n_split = 1;
    kp.split_keys = (int32_t)(((steps + kp.n_split - 1) / kp.n_split) * kKvcStep);
    if (kp.split_keys <= 0) kp.split_keys = kKvcStep;
    if (kp.n_split > 1) kp.ws_lse = kp.ws_o + (int64_t)kp.n_split * kp.rows_total * kp.d;
    if (kp.d == 256) return launch_kvcache_ragged_d256(rp, dtype, s, cap_pre);
    if (dtype == 0) return kp.d == 64 ? launch_kvcache_ragged_es<_Float16, 64>(rp, s, cap_pre, sink, tree, row_tile) : launch_kvcache_ragged_es<_Float16, 128>(rp, s, cap_pre, sink, tree, row_tile);
    return kp.d == 64 ? launch_kvcache_ragged_es<__bf16, 64>(rp, s, cap_pre, sink, tree, row_tile) : launch_kvcache_ragged_es<__bf16, 128>(rp, s, cap_pre, sink, tree, row_tile);
}
#endif  // FA_KVC_D256_TU

}  // namespace fa
