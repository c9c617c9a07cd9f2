// fa_fwd_kvcache.hip — decode attention over a KV cache (fa_run_mha_fwd_kvcache, include/flash_attn_gfx950.h): the dense call.
//
//   * The attention body is kvcache_attn of fa_kvcache_attn.hpp (how a workgroup packs rows, splits keys and steps through them is described
//     there).  This file wraps its plain, causal and sliding-window instantiations over both layouts and both cache element sizes in kernels:
//     48 attention kernels.  The soft-capped, sink, tree-mask, 64-row and head_dim-256 instantiations live in the files named after them.
//   * The append and combine kernels of a dense call at head_dim 64 / 128 are instantiated here, from the templates of fa_kvcache_kernels.hpp.
//   * launch_fwd_kvcache finishes the params and runs append, attention, combine (kvc_launch_call of fa_kvcache_launch.hpp); which file's
//     attention kernels run is decided by kvc_route_attn there.  The split rule and the workspace size of every decode call are here too.
// Rotary embedding (fa_kvcache_options_v3) is not in this file: fa_kvcache_rotary.hip replaces the append launch by a fused one that also leaves
// the rotated q in an image these kernels read as their q (k_new = NULL then: nothing left to append, seqlen_new still counts into the length).
#include "fa_kvcache_launch.hpp"

namespace fa {

namespace {

template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, D, CAUSAL, false>(p);
}

template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_paged_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, D, CAUSAL, true>(p);
}

// Sliding window over either layout (the causal limit arrives as window_right = 0)
template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_local_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, D, false, PAGED, true>(p);
}

// The same three over an 8-bit (e4m3) cache
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_fp8_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, D, CAUSAL, false, false, 1>(p);
}

template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_fp8_paged_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, D, CAUSAL, true, false, 1>(p);
}

template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_fp8_local_kernel(const KvcacheKernelParams p) {
    kvcache_attn<T, D, false, PAGED, true, 1>(p);
}

// the window / paged / plain kernels of this file for a call no family file serves
void launch_own_attn(const KvcacheKernelParams& kp, int dtype, unsigned grid, hipStream_t s) {
    kvc_dispatch<64, 128>(kp, dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        constexpr int D = K::D;
        auto launch = [&](auto* kernel) { kvc_launch_attn(kernel, grid, s, kp); };
        if (kp.is_local) {
            if constexpr (K::ES == 1) launch(fa_fwd_kvcache_fp8_local_kernel<T, D, K::PAGED>);
            else launch(fa_fwd_kvcache_local_kernel<T, D, K::PAGED>);
        } else if constexpr (K::ES == 1 && K::PAGED) {
            kp.is_causal ? launch(fa_fwd_kvcache_fp8_paged_kernel<T, D, true>) : launch(fa_fwd_kvcache_fp8_paged_kernel<T, D, false>);
        } else if constexpr (K::ES == 1) {
            kp.is_causal ? launch(fa_fwd_kvcache_fp8_kernel<T, D, true>) : launch(fa_fwd_kvcache_fp8_kernel<T, D, false>);
        } else if constexpr (K::PAGED) {
            kp.is_causal ? launch(fa_fwd_kvcache_paged_kernel<T, D, true>) : launch(fa_fwd_kvcache_paged_kernel<T, D, false>);
        } else {
            kp.is_causal ? launch(fa_fwd_kvcache_kernel<T, D, true>) : launch(fa_fwd_kvcache_kernel<T, D, false>);
        }
    });
}

}  // namespace

// Split count: the host knows the capacity, not the lengths (they live on the device), so the split is sized from seqlen_cache (with a
// window: from the window's span, kvcache_steps; never more steps than without it, so the split and workspace never grow).  A launch
// of b x h_k x row tiles workgroups that already brings one per compute unit is not split; otherwise the key range is split until the
// launch holds two workgroups per unit (the occupancy of the attention kernel), keeping at least kKvcMinStepsPerSplit steps per split and
// at most kKvcMaxSplits splits.  An explicit request overrides the rule (never more splits than 32-key steps); a workspace smaller than
// the choice needs caps it (avail_bytes < 0: unlimited).
// A ragged call (total_q >= 0) counts the tile slots of its grid, kvcache_ragged_slots, in place of b x row tiles, and its partial planes
// have h x total_q rows.
// row_tile = the packed query rows of a workgroup: kKvcRows for the kernels of this file, kKvcPrefillRows for the 64-row kernels of
// fa_fwd_kvcache_prefill.hip - the same rule over that grid's workgroup count, and the same slot formula in tiles of 64.
int64_t kvcache_ragged_slots(const KvcacheKernelParams& kp, int64_t total_q, int32_t* compact, int32_t row_tile) {
    const int64_t packed = (total_q * kp.h_ratio + row_tile - 1) / row_tile + kp.b;
    const int64_t plain = (int64_t)kp.b * (((int64_t)kp.seqlen_q * kp.h_ratio + row_tile - 1) / row_tile);
    if (compact != nullptr) *compact = packed < plain ? 1 : 0;
    return packed < plain ? packed : plain;
}

int32_t kvcache_split(const KvcacheKernelParams& kp, int64_t avail_bytes, int32_t requested, int64_t total_q, int32_t row_tile) {
    const int64_t steps = kvcache_steps(kp);
    if (steps <= 1) return 1;
    int64_t n;
    if (requested > 0) {
        n = requested < steps ? requested : steps;
    } else {
        const int64_t wgs = total_q >= 0 ? kp.h_k * kvcache_ragged_slots(kp, total_q, nullptr, row_tile)
                                         : (int64_t)kp.b * kp.h_k * (((int64_t)kp.seqlen_q * kp.h_ratio + row_tile - 1) / row_tile);
        const int64_t cus = device_cu_count();
        if (wgs <= 0 || wgs >= cus) return 1;
        n = (2 * cus + wgs - 1) / wgs;
        const int64_t cap = steps / kKvcMinStepsPerSplit;
        if (n > cap) n = cap;
        if (n > kKvcMaxSplits) n = kKvcMaxSplits;
        if (n < 1) n = 1;
    }
    if (avail_bytes >= 0)
        while (n > 1 && kvcache_workspace_bytes(kp, (int32_t)n, total_q) > avail_bytes) --n;
    return (int32_t)n;
}

int64_t kvcache_workspace_bytes(const KvcacheKernelParams& kp, int32_t n_split, int64_t total_q) {
    if (n_split <= 1) return 0;
    const int64_t rows = total_q >= 0 ? kp.h * total_q : (int64_t)kp.b * kp.h * kp.seqlen_q;
    const int64_t o_bytes = (int64_t)n_split * rows * kp.d * 4;
    const int64_t l_bytes = ((int64_t)n_split * rows * 4 + 15) / 16 * 16;
    return o_bytes + l_bytes;
}

hipError_t launch_fwd_kvcache(KvcacheKernelParams kp, int dtype, hipStream_t s, float cap_pre, KvcacheSink sink, KvcacheTree tree, int32_t row_tile) {
    if (!kvcache_row_tile_ok(row_tile)) return hipErrorInvalidValue;
    finish_params(kp, (int64_t)kp.b * kp.h * kp.seqlen_q, row_tile);
    if (kp.d == 256) return launch_kvcache_d256(kp, dtype, s, cap_pre);
    return kvc_launch_call<64, 128>(kp, dtype, s, sink, [&](unsigned grid) {
        return kvc_route_attn(kp, dtype, grid, s, cap_pre, sink, tree, row_tile, [&] { launch_own_attn(kp, dtype, grid, s); });
    });
}

}  // namespace fa
