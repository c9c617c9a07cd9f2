// fa_fwd_kvcache_ragged.hip — decode attention over a KV cache for ragged query batches (fa_kvcache_options_v4: cu_seqlens_q / cu_seqlens_k_new).
//
// One scheduler step of a serving engine - sequences that decode one token, verify a few speculative ones or bring a chunk of their prompt - as
// ONE call: q / o are packed (total_q, h, d), k_new / v_new (total_k_new, h_k, d), sequence i owns the rows cu[i] .. cu[i + 1] - 1.
//   * The attention body is kvcache_attn of fa_kvcache_attn.hpp with RAGGED = true: every sequence is tiled
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
//   * The append and combine kernels of a ragged call are the ragged templates of fa_kvcache_kernels.hpp, instantiated here; the launch sequence
//     and the routing to the family files are those of the dense call (fa_kvcache_launch.hpp).
#include "fa_kvcache_launch.hpp"

namespace fa {

namespace {

// MODE 0: every key below L, 1: causal, 2: sliding window (the causal limit arrives as window_right = 0)
template <typename T, int D, int MODE, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_kernel(const KvcacheRaggedParams rp) {
    kvcache_attn<T, D, MODE == 1, PAGED, MODE == 2, ES, true>(rp.kp, &rp);
}

// the window / causal / plain kernels of this file for a call no family file serves
void launch_own_attn(const KvcacheRaggedParams& rp, int dtype, unsigned grid, hipStream_t s) {
    kvc_dispatch<64, 128>(rp.kp, dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        auto launch = [&](auto* kernel) { kvc_launch_attn(kernel, grid, s, rp); };
        if (rp.kp.is_local) launch(fa_fwd_kvcache_ragged_kernel<T, K::D, 2, K::PAGED, K::ES>);
        else if (rp.kp.is_causal) launch(fa_fwd_kvcache_ragged_kernel<T, K::D, 1, K::PAGED, K::ES>);
        else launch(fa_fwd_kvcache_ragged_kernel<T, K::D, 0, K::PAGED, K::ES>);
    });
}

}  // namespace

// kp.seqlen_q = max_seqlen_q sizes the split exactly as the dense launcher does (kvcache_steps), so a forced split cuts the keys where the dense
// call with seqlen_q = max_seqlen_q cuts them.
hipError_t launch_fwd_kvcache_ragged(KvcacheRaggedParams rp, int dtype, hipStream_t s, float cap_pre, KvcacheSink sink, KvcacheTree tree, int32_t row_tile) {
    if (!kvcache_row_tile_ok(row_tile)) return hipErrorInvalidValue;
    KvcacheKernelParams& kp = rp.kp;
    finish_params(kp, (int64_t)kp.h * rp.total_q, row_tile);
    rp.slots = (int32_t)kvcache_ragged_slots(kp, rp.total_q, &rp.compact, row_tile);
    if (kp.d == 256) return launch_kvcache_ragged_d256(rp, dtype, s, cap_pre);
    return kvc_launch_call<64, 128>(rp, dtype, s, sink, [&](unsigned grid) {
        return kvc_route_attn(rp, dtype, grid, s, cap_pre, sink, tree, row_tile, [&] { launch_own_attn(rp, dtype, grid, s); });
    });
}

}  // namespace fa
