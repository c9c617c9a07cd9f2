// fa_fwd_kvcache_d256.hip — decode attention over a KV cache at head_dim 256 (Gemma 2 2B / 9B, Gemma 3): every kernel of such a call.
//
//   * The bodies are the ones head_dim 64 / 128 run - kvcache_attn, the append, combine and rotary kernels - instantiated at D = 256: this file
//     includes fa_fwd_kvcache_ragged.hip (and through it fa_fwd_kvcache.hip) and fa_kvcache_rotary.hip with FA_KVC_D256_TU set, which keeps
//     their templates and drops their launchers.  Everything the decode call supports at 128 is here: fp16 / bf16, contiguous / paged, 16-bit
//     / FP8 cache, dense / ragged, windows, softcap, rotary.  fwd / bwd / varlen_* have no head_dim 256.
//   * ONE workgroup per compute unit: __launch_bounds__(kKvcThreads, 1).  A lane holds Q^T (32 registers), O^T (64) and two prefetch sets of K
//     and V (4 x 64 with a 16-bit cache): about 390 registers, which the 256 of two workgroups per unit cannot place (the 16-bit kernels spill
//     170-200 registers there).  At one workgroup - one wave per SIMD, 512 registers - hipcc keeps the prefetch sets in AGPRs, loads them
//     there directly and feeds the MFMAs and the LDS image from there: no scratch, no v_accvgpr moves in the loop.  LDS: 67 072 bytes (the
//     merge planes; the four V images are 65 536).  Bytes in flight per unit are what two head_dim-128 workgroups hold: 4 waves x one
//     32-key step x 512 B x (K + V) = 128 KB; whether it streams like them is the measurement DESIGN.md 3.9 describes.
//   * One attention instantiation per (dtype, layout, cache element, dense / ragged, softcap): the sliding-window code serves plain and causal
//     calls as the windows (-1, -1) and (-1, 0), as in fa_fwd_kvcache_softcap.hip - an unbounded side is a case the window code already has,
//     and right = 0 is exactly the causal limit.  32 attention kernels instead of 64; FA_KVC_D256_PLAIN = 1 builds the plain and causal
//     instantiations of the calls without softcap as well (the A/B of DESIGN.md 3.9).
//   * Kernels of this file: 32 attention (16 dense: fa_fwd_kvcache_d256_kernel and _softcap_kernel, 16 ragged), 6 append + 6 ragged append,
//     2 combine + 2 ragged combine, 8 rotary = 56.
#define FA_KVC_D256_TU 1
#include "fa_fwd_kvcache_ragged.hip"
#include "fa_kvcache_rotary.hip"

#ifndef FA_KVC_D256_PLAIN
#define FA_KVC_D256_PLAIN 0
#endif

namespace fa {

namespace {

constexpr int kD256 = 256;

// MODE 0: every key below L, 1: causal, 2: sliding window (0 and 1 are built under FA_KVC_D256_PLAIN only)
template <typename T, int MODE, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_d256_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, kD256, MODE == 1, PAGED, MODE == 2, ES>(p);
}

template <typename T, int MODE, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_d256_ragged_kernel(const KvcacheRaggedParams rp) {
    kvcache_attn<T, kD256, MODE == 1, PAGED, MODE == 2, ES, true>(rp.kp, &rp);
}

template <typename T, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_d256_softcap_kernel(const KvcacheSoftcapParams sp) {
    kvcache_attn<T, kD256, false, PAGED, true, ES, false, true>(sp.kp, nullptr, sp.pre);
}

template <typename T, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_d256_ragged_softcap_kernel(const KvcacheRaggedSoftcapParams sp) {
    kvcache_attn<T, kD256, false, PAGED, true, ES, true, true>(sp.rp.kp, &sp.rp, sp.pre);
}

// a call without a window as the window code sees it: both sides unbounded, or the causal limit on the right
void as_window(KvcacheKernelParams& kp) {
    if (kp.is_local) return;
    kp.window_left = -1;
    kp.window_right = kp.is_causal ? 0 : -1;
}

template <typename T, bool PAGED, int ES>
void launch_attn(const KvcacheKernelParams& kp, float cap_pre, unsigned grid, hipStream_t s) {
    if (cap_pre > 0.f) {
        KvcacheSoftcapParams sp;
        sp.kp = kp;
        sp.pre = cap_pre;
        as_window(sp.kp);
        hipLaunchKernelGGL((fa_fwd_kvcache_d256_softcap_kernel<T, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
        return;
    }
#if FA_KVC_D256_PLAIN
    if (!kp.is_local) {
        if (kp.is_causal) hipLaunchKernelGGL((fa_fwd_kvcache_d256_kernel<T, 1, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, kp);
        else hipLaunchKernelGGL((fa_fwd_kvcache_d256_kernel<T, 0, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, kp);
        return;
    }
#endif
    KvcacheKernelParams wp = kp;
    as_window(wp);
    hipLaunchKernelGGL((fa_fwd_kvcache_d256_kernel<T, 2, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, wp);
}

template <typename T, bool PAGED, int ES>
void launch_ragged_attn_d256(const KvcacheRaggedParams& rp, float cap_pre, unsigned grid, hipStream_t s) {
    if (cap_pre > 0.f) {
        KvcacheRaggedSoftcapParams sp;
        sp.rp = rp;
        sp.pre = cap_pre;
        as_window(sp.rp.kp);
        hipLaunchKernelGGL((fa_fwd_kvcache_d256_ragged_softcap_kernel<T, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, sp);
        return;
    }
#if FA_KVC_D256_PLAIN
    if (!rp.kp.is_local) {
        if (rp.kp.is_causal) hipLaunchKernelGGL((fa_fwd_kvcache_d256_ragged_kernel<T, 1, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, rp);
        else hipLaunchKernelGGL((fa_fwd_kvcache_d256_ragged_kernel<T, 0, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, rp);
        return;
    }
#endif
    KvcacheRaggedParams wp = rp;
    as_window(wp.kp);
    hipLaunchKernelGGL((fa_fwd_kvcache_d256_ragged_kernel<T, 2, PAGED, ES>), dim3(grid), dim3(kKvcThreads), 0, s, wp);
}

// append, attention, combine of a dense call: launch_kvcache_t / launch_kvcache_fp8_t of fa_fwd_kvcache.hip at D = 256
template <typename T, bool PAGED, int ES>
hipError_t launch_dense(const KvcacheKernelParams& kp, hipStream_t s, float cap_pre) {
    if (kp.k_new != nullptr && kp.seqlen_new > 0) {
        const int64_t n = (int64_t)kp.b * kp.seqlen_new * kp.h_k * (kD256 / 8);
        const dim3 grid((unsigned)((n + 255) / 256));
        if constexpr (ES == 1) hipLaunchKernelGGL((fa_kvcache_append_fp8_kernel<T, kD256, PAGED>), grid, dim3(256), 0, s, kp);
        else if constexpr (PAGED) hipLaunchKernelGGL((fa_kvcache_append_paged_kernel<kD256>), grid, dim3(256), 0, s, kp);
        else hipLaunchKernelGGL((fa_kvcache_append_kernel<kD256>), grid, dim3(256), 0, s, kp);
    }
    const int64_t grid = (int64_t)kp.b * kp.h_k * kp.n_row_tiles * kp.n_split;
    launch_attn<T, PAGED, ES>(kp, cap_pre, (unsigned)grid, s);
    if (kp.n_split > 1) {
        const int64_t rows_per_block = kKvcCombineThreads / (kD256 / 8);
        hipLaunchKernelGGL((fa_kvcache_combine_kernel<T, kD256>), dim3((unsigned)((kp.rows_total + rows_per_block - 1) / rows_per_block)),
                           dim3(kKvcCombineThreads), 0, s, kp);
    }
    return hipGetLastError();
}

// ... and of a ragged call: launch_kvcache_ragged_t of fa_fwd_kvcache_ragged.hip at D = 256
template <typename T, bool PAGED, int ES>
hipError_t launch_ragged(const KvcacheRaggedParams& rp, hipStream_t s, float cap_pre) {
    const KvcacheKernelParams& kp = rp.kp;
    if (kp.k_new != nullptr && rp.cu_kn != nullptr && rp.total_kn > 0) {
        const int64_t n = rp.total_kn * kp.h_k * (kD256 / 8);
        using TA = std::conditional_t<ES == 1, T, _Float16>;        // (the 16-bit append copies bits: one instantiation serves both dtypes)
        hipLaunchKernelGGL((fa_kvcache_append_ragged_kernel<TA, kD256, PAGED, ES>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rp);
    }
    if (rp.total_q > 0) {
        const int64_t grid = (int64_t)rp.slots * kp.h_k * kp.n_split;
        launch_ragged_attn_d256<T, PAGED, ES>(rp, cap_pre, (unsigned)grid, s);
        if (kp.n_split > 1) {
            const int64_t rows_per_block = kKvcCombineThreads / (kD256 / 8);
            hipLaunchKernelGGL((fa_kvcache_combine_ragged_kernel<T, kD256>), dim3((unsigned)((kp.rows_total + rows_per_block - 1) / rows_per_block)),
                               dim3(kKvcCombineThreads), 0, s, rp);
        }
    }
    return hipGetLastError();
}

}  // namespace

// kp as launch_fwd_kvcache finished it (row tiles, split, workspace planes)
hipError_t launch_kvcache_d256(const KvcacheKernelParams& kp, int dtype, hipStream_t s, float cap_pre) {
    const bool paged = kp.block_table != nullptr;
    if (dtype == 0) {
        if (kp.cache_fp8) return paged ? launch_dense<_Float16, true, 1>(kp, s, cap_pre) : launch_dense<_Float16, false, 1>(kp, s, cap_pre);
        return paged ? launch_dense<_Float16, true, 2>(kp, s, cap_pre) : launch_dense<_Float16, false, 2>(kp, s, cap_pre);
    }
    if (kp.cache_fp8) return paged ? launch_dense<__bf16, true, 1>(kp, s, cap_pre) : launch_dense<__bf16, false, 1>(kp, s, cap_pre);
    return paged ? launch_dense<__bf16, true, 2>(kp, s, cap_pre) : launch_dense<__bf16, false, 2>(kp, s, cap_pre);
}

// rp as launch_fwd_kvcache_ragged finished it (slots, compact, split)
hipError_t launch_kvcache_ragged_d256(const KvcacheRaggedParams& rp, int dtype, hipStream_t s, float cap_pre) {
    const bool paged = rp.kp.block_table != nullptr;
    if (dtype == 0) {
        if (rp.kp.cache_fp8) return paged ? launch_ragged<_Float16, true, 1>(rp, s, cap_pre) : launch_ragged<_Float16, false, 1>(rp, s, cap_pre);
        return paged ? launch_ragged<_Float16, true, 2>(rp, s, cap_pre) : launch_ragged<_Float16, false, 2>(rp, s, cap_pre);
    }
    if (rp.kp.cache_fp8) return paged ? launch_ragged<__bf16, true, 1>(rp, s, cap_pre) : launch_ragged<__bf16, false, 1>(rp, s, cap_pre);
    return paged ? launch_ragged<__bf16, true, 2>(rp, s, cap_pre) : launch_ragged<__bf16, false, 2>(rp, s, cap_pre);
}

hipError_t launch_kvcache_rotary_d256(const KvcacheRotaryParams& rp, int dtype, hipStream_t s) {
    return dtype == 0 ? launch_rotary_t<_Float16, kD256>(rp, s) : launch_rotary_t<__bf16, kD256>(rp, s);
}

}  // namespace fa
