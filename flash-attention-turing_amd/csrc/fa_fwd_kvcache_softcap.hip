// fa_fwd_kvcache_softcap.hip — decode attention over a KV cache with soft-capped scores (fa_kvcache_options_v5: softcap > 0).
//
//   score = softcap * tanh((q . k) * softmax_scale / softcap), then the mask, then the softmax over the capped scores; LSE is their logsumexp.
//   * The attention body is kvcache_attn of fa_kvcache_attn.hpp with SOFTCAP = true: right behind the QK MFMAs every S^T element becomes
//     t = tanh(s * pre), and the rest of the step runs on t with c = softcap * log2(e) and the LSE factor softcap in the places of the scale.
//     The wave merge, the partial planes and the combine never read the scale: they are the code they were.
//   * gfx950 has no tanh instruction; kvc_tanh2 builds it from v_exp_f32 and v_rcp_f32, 8 of each per lane and 32-key step.
//   * pre = 2 log2(e) * softmax_scale / softcap comes from the host in a parameter block of its own; with an 8-bit cache the kernel multiplies
//     the K descale of its (batch, KV head) onto it (the descale belongs inside the tanh), and v_descale stays in the final normalisation.
//   * One instantiation per (dtype, head_dim, layout, cache element): the sliding-window code serves plain and causal calls as well, as the
//     windows (-1, -1) and (-1, 0) - an unbounded side is a case the window code already has, and right = 0 is exactly the causal limit.  16
//     dense and 16 ragged kernels instead of 96.  Dense and ragged calls share the body as before, so sequence i of a soft-capped ragged call
//     gives the bits of the soft-capped dense call on it alone.
//   * Only the attention launch lives here.  The append in front of it and the combine behind it are those of every call: kvc_route_attn
//     (fa_kvcache_launch.hpp) calls the function at the end of this file in the place of the caller's own attention launch.
#include "fa_kvcache_launch.hpp"

namespace fa {

namespace {

template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_softcap_kernel(const KvcacheSoftcapParams sp) {
    kvcache_attn<T, D, false, PAGED, true, ES, false, true>(sp.kp, nullptr, sp.pre);
}

template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_softcap_kernel(const KvcacheRaggedSoftcapParams sp) {
    kvcache_attn<T, D, false, PAGED, true, ES, true, true>(sp.rp.kp, &sp.rp, sp.pre);
}
// p as the dense / ragged launcher finished it (row tiles or slots, split, workspace planes)
template <typename P>
hipError_t launch_softcap_attn(const P& p, float pre, int dtype, unsigned grid, hipStream_t s) {
    const std::conditional_t<kKvcIsRagged<P>, KvcacheRaggedSoftcapParams, KvcacheSoftcapParams> sp{as_window(p), pre};
    kvc_dispatch<64, 128>(kvc_kp(p), dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_softcap_kernel<T, K::D, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_softcap_kernel<T, K::D, K::PAGED, K::ES>), grid, s, sp);
    });
    return hipGetLastError();
}

}  // namespace

// grid = b x h_k x row tiles x splits (dense), slots x h_k x splits (ragged)
hipError_t launch_kvcache_softcap_attn(const KvcacheKernelParams& kp, float pre, int dtype, unsigned grid, hipStream_t s) { return launch_softcap_attn(kp, pre, dtype, grid, s); }
hipError_t launch_kvcache_softcap_attn(const KvcacheRaggedParams& rp, float pre, int dtype, unsigned grid, hipStream_t s) { return launch_softcap_attn(rp, pre, dtype, grid, s); }

}  // namespace fa
