// fa_fwd_kvcache_softcap.hip — decode attention over a KV cache with soft-capped scores (fa_kvcache_options_v5: softcap > 0).
//
//   score = softcap * tanh((q . k) * softmax_scale / softcap), then the mask, then the softmax over the capped scores; LSE is their logsumexp.
//   * The attention body is kvcache_attn of fa_fwd_kvcache.hip with SOFTCAP = true (this file includes that one for it, with FA_KVC_RAGGED_TU
//     set so that the dense kernels and launchers are not compiled a second time): right behind the QK MFMAs every S^T element becomes
//     t = tanh(s * pre), and the rest of the step runs on t with c = softcap * log2(e) and the LSE factor softcap in the places of the scale.
//     The wave merge, the partial planes and the combine never read the scale: they are the code they were.
//   * gfx950 has no tanh instruction; kvc_tanh2 builds it from v_exp_f32 and v_rcp_f32, 8 of each per lane and 32-key step.
//   * pre = 2 log2(e) * softmax_scale / softcap comes from the host in a parameter block of its own; with an 8-bit cache the kernel multiplies
//     the K descale of its (batch, KV head) onto it (the descale belongs inside the tanh), and v_descale stays in the final normalisation.
//   * One instantiation per (dtype, head_dim, layout, cache element): the sliding-window code serves plain and causal calls as well, as the
//     windows (-1, -1) and (-1, 0) - an unbounded side is a case the window code already has, and right = 0 is exactly the causal limit.  16
//     dense and 16 ragged kernels instead of 96.  Dense and ragged calls share the body as before, so sequence i of a soft-capped ragged call
//     gives the bits of the soft-capped dense call on it alone.
//   * Only the attention launch lives here.  The append in front of it and the combine behind it are those of fa_fwd_kvcache.hip and
//     fa_fwd_kvcache_ragged.hip, whose launchers call the two functions at the end of this file in the place of their own attention launch.
#define FA_KVC_RAGGED_TU 1
#include "fa_fwd_kvcache.hip"

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

// a call without a window as the window code sees it: both sides unbounded, or the causal limit on the right
void softcap_window(KvcacheKernelParams& kp) {
    if (kp.is_local) return;
    kp.window_left = -1;
    kp.window_right = kp.is_causal ? 0 : -1;
}

template <typename T, int D>
void launch_softcap_t(const KvcacheSoftcapParams& sp, unsigned grid, hipStream_t s) {
    const bool paged = sp.kp.block_table != nullptr;
    if (sp.kp.cache_fp8) {
        if (paged) hipLaunchKernelGGL((fa_fwd_kvcache_softcap_kernel<T, D, true, 1>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
        else hipLaunchKernelGGL((fa_fwd_kvcache_softcap_kernel<T, D, false, 1>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
    } else {
        if (paged) hipLaunchKernelGGL((fa_fwd_kvcache_softcap_kernel<T, D, true, 2>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
        else hipLaunchKernelGGL((fa_fwd_kvcache_softcap_kernel<T, D, false, 2>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
    }
}

template <typename T, int D>
void launch_ragged_softcap_t(const KvcacheRaggedSoftcapParams& sp, unsigned grid, hipStream_t s) {
    const bool paged = sp.rp.kp.block_table != nullptr;
    if (sp.rp.kp.cache_fp8) {
        if (paged) hipLaunchKernelGGL((fa_fwd_kvcache_ragged_softcap_kernel<T, D, true, 1>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
        else hipLaunchKernelGGL((fa_fwd_kvcache_ragged_softcap_kernel<T, D, false, 1>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
    } else {
        if (paged) hipLaunchKernelGGL((fa_fwd_kvcache_ragged_softcap_kernel<T, D, true, 2>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
        else hipLaunchKernelGGL((fa_fwd_kvcache_ragged_softcap_kernel<T, D, false, 2>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
    }
}

}  // namespace

// kp as the dense launcher finished it (row tiles, split, workspace planes); grid = b x h_k x row tiles x splits
hipError_t launch_kvcache_softcap_attn(const KvcacheKernelParams& kp, float pre, int dtype, unsigned grid, hipStream_t s) {
    KvcacheSoftcapParams sp;
    sp.kp = kp;
    sp.pre = pre;
    softcap_window(sp.kp);
    if (dtype == 0) kp.d == 64 ? launch_softcap_t<_Float16, 64>(sp, grid, s) : launch_softcap_t<_Float16, 128>(sp, grid, s);
    else kp.d == 64 ? launch_softcap_t<__bf16, 64>(sp, grid, s) : launch_softcap_t<__bf16, 128>(sp, grid, s);
    return hipGetLastError();
}

// rp as the ragged launcher finished it (slots, compact, split); grid = slots x h_k x splits
hipError_t launch_kvcache_ragged_softcap_attn(const KvcacheRaggedParams& rp, float pre, int dtype, unsigned grid, hipStream_t s) {
    KvcacheRaggedSoftcapParams sp;
    sp.rp = rp;
    sp.pre = pre;
    softcap_window(sp.rp.kp);
    if (dtype == 0) rp.kp.d == 64 ? launch_ragged_softcap_t<_Float16, 64>(sp, grid, s) : launch_ragged_softcap_t<_Float16, 128>(sp, grid, s);
    else rp.kp.d == 64 ? launch_ragged_softcap_t<__bf16, 64>(sp, grid, s) : launch_ragged_softcap_t<__bf16, 128>(sp, grid, s);
    return hipGetLastError();
}

}  // namespace fa
