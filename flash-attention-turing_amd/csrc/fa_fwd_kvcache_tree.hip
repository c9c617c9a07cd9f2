// fa_fwd_kvcache_tree.hip — decode attention over a KV cache under a tree attention mask (fa_kvcache_options_v7: tree_mask != NULL).
//
//   Verifying a draft TREE of speculative tokens (EAGLE, Medusa, SpecInfer; the tree-attention backend of vLLM, the custom mask of SGLang and
//   FlashInfer): the sq query rows of a sequence are the nodes of a tree, every node sees the whole cached prefix, and among the draft tokens -
//   the last sq keys of the sequence, base = L - sq - a node sees only what its 64-bit word says.  Query row t sees key j iff 0 <= j < L and
//       j < base   or   bit (j - base) of tree_mask[i, t] is set.
//   * The attention body is kvcache_attn of fa_kvcache_attn.hpp with TREE = true: the plain, non-causal instantiation - steps [0, L), lim = L - whose
//     select tests the bit.  A lane owns one query row for the whole split and loads its word once in the prologue.  Nothing else differs, so
//     the lower-triangle mask gives the causal call bit for bit and the full mask the non-causal call, for every split count.
//   * The launchers run the attention kernel alone, split or not, on the grid the dense / ragged launcher computed.  Append, partial planes and
//     combine are the unchanged ones: the split count and the workspace do not know about the mask.
//   * The query heads of a token share its word (packed row r = t * h_ratio + j reads word t); bits at or above sq are never asked for (their
//     keys are at or past L), nor are bits of keys below 0 (L < sq).  Bit 63 is an ordinary bit: the word is shifted as an unsigned value.
//   * One instantiation per (dtype, head_dim, layout, cache element), dense and ragged: 32 attention kernels.  FA_KVC_TREE_UNIFORM = 1 builds
//     them with a wave-uniform branch that leaves the steps wholly inside the prefix on the plain select.
//   * A tree mask with causal, a window, a soft cap, sinks, rotary or head_dim 256 is refused by the C ABI: nothing here serves them.
#include "fa_kvcache_launch.hpp"

namespace fa {

namespace {

template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_tree_kernel(const KvcacheTreeParams tp) {
    kvcache_attn<T, D, false, PAGED, false, ES, false, false, false, true>(tp.kp, nullptr, 0.f, nullptr, 0, &tp.tree);
}

template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_tree_kernel(const KvcacheRaggedTreeParams tp) {
    kvcache_attn<T, D, false, PAGED, false, ES, true, false, false, true>(tp.rp.kp, &tp.rp, 0.f, nullptr, 0, &tp.tree);
}
// p as the dense / ragged launcher finished it (row tiles or slots, split, partial planes)
template <typename P>
hipError_t launch_tree_attn(const P& p, const KvcacheTree& tree, int dtype, unsigned grid, hipStream_t s) {
    const std::conditional_t<kKvcIsRagged<P>, KvcacheRaggedTreeParams, KvcacheTreeParams> tp{p, tree};
    kvc_dispatch<64, 128>(kvc_kp(p), dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_tree_kernel<T, K::D, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_tree_kernel<T, K::D, K::PAGED, K::ES>), grid, s, tp);
    });
    return hipGetLastError();
}

}  // namespace

// grid = b x h_k x row tiles x n_split (dense), slots x h_k x n_split (ragged)
hipError_t launch_kvcache_tree_attn(const KvcacheKernelParams& kp, const KvcacheTree& tree, int dtype, unsigned grid, hipStream_t s) { return launch_tree_attn(kp, tree, dtype, grid, s); }
hipError_t launch_kvcache_tree_attn(const KvcacheRaggedParams& rp, const KvcacheTree& tree, int dtype, unsigned grid, hipStream_t s) { return launch_tree_attn(rp, tree, dtype, grid, s); }

}  // namespace fa
