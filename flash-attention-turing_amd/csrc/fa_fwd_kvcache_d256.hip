// fa_fwd_kvcache_d256.hip — decode attention over a KV cache at head_dim 256 (Gemma 2 2B / 9B, Gemma 3): every kernel of such a call.
//
//   * The bodies are the ones head_dim 64 / 128 run - kvcache_attn (fa_kvcache_attn.hpp), the append and combine kernels (fa_kvcache_kernels.hpp) and
//     the rotary kernel (fa_kvcache_rotary.hpp) - instantiated at D = 256 through the launch helpers of fa_kvcache_launch.hpp, which the other
//     files call at 64 / 128.  Everything the decode call supports at 128 is here: fp16 / bf16, contiguous / paged, 16-bit
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
#include "fa_kvcache_rotary.hpp"

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
// append, attention, combine of a call as launch_fwd_kvcache / launch_fwd_kvcache_ragged finished it; no family file serves head_dim 256, the soft cap
// is this file's own
template <typename P>
hipError_t launch_d256(const P& p, int dtype, hipStream_t s, float cap_pre) {
    return kvc_launch_call<kD256>(p, dtype, s, KvcacheSink{nullptr, 0}, [&](unsigned grid) {
        kvc_dispatch<kD256>(kvc_kp(p), dtype, [&](auto leaf) {
            using K = decltype(leaf);
            using T = typename K::T;
            if (cap_pre > 0.f) {
                const std::conditional_t<kKvcIsRagged<P>, KvcacheRaggedSoftcapParams, KvcacheSoftcapParams> sp{as_window(p), cap_pre};
                kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_d256_softcap_kernel<T, K::PAGED, K::ES>, fa_fwd_kvcache_d256_ragged_softcap_kernel<T, K::PAGED, K::ES>), grid, s, sp);
                return;
            }
#if FA_KVC_D256_PLAIN
            if (!kvc_kp(p).is_local) {
                if (kvc_kp(p).is_causal) kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_d256_kernel<T, 1, K::PAGED, K::ES>, fa_fwd_kvcache_d256_ragged_kernel<T, 1, K::PAGED, K::ES>), grid, s, p);
                else kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_d256_kernel<T, 0, K::PAGED, K::ES>, fa_fwd_kvcache_d256_ragged_kernel<T, 0, K::PAGED, K::ES>), grid, s, p);
                return;
            }
#endif
            kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_d256_kernel<T, 2, K::PAGED, K::ES>, fa_fwd_kvcache_d256_ragged_kernel<T, 2, K::PAGED, K::ES>), grid, s, as_window(p));
        });
        return hipSuccess;
    });
}

}  // namespace

hipError_t launch_kvcache_d256(const KvcacheKernelParams& kp, int dtype, hipStream_t s, float cap_pre) { return launch_d256(kp, dtype, s, cap_pre); }
hipError_t launch_kvcache_ragged_d256(const KvcacheRaggedParams& rp, int dtype, hipStream_t s, float cap_pre) { return launch_d256(rp, dtype, s, cap_pre); }
hipError_t launch_kvcache_rotary_d256(const KvcacheRotaryParams& rp, int dtype, hipStream_t s) { return launch_rotary<kD256>(rp, dtype, s); }

}  // namespace fa
