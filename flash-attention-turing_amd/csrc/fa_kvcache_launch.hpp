// fa_kvcache_launch.hpp — the host side of a decode call over a KV cache, written once for every fa_fwd_kvcache*.hip.
//
//   * kvc_dispatch turns the runtime values of a call (dtype, head_dim, paged, 8-bit cache) into one KvcLeaf type and calls a generic lambda with
//     it; the lambda names the kernel of its file for that leaf.  A file instantiates exactly the kernels its lambdas name.
//   * A call is append, attention, combine (kvc_launch_call).  The append and combine kernels are the templates of fa_kvcache_kernels.hpp,
//     instantiated by the files that call launch_append / launch_combine: fa_fwd_kvcache.hip (dense), fa_fwd_kvcache_ragged.hip (ragged) and
//     fa_fwd_kvcache_d256.hip (both, at head_dim 256).
//   * Which file's attention kernels a call at head_dim 64 / 128 runs is decided in one place, kvc_route_attn.
//   Every template takes P = KvcacheKernelParams (a dense call) or KvcacheRaggedParams (a ragged one); kvc_kp is the KvcacheKernelParams in it.
#pragma once
#include "fa_kvcache_kernels.hpp"

namespace fa {

namespace {

template <typename P>
constexpr bool kKvcIsRagged = std::is_same_v<P, KvcacheRaggedParams>;
inline const KvcacheKernelParams& kvc_kp(const KvcacheKernelParams& p) { return p; }
inline const KvcacheKernelParams& kvc_kp(const KvcacheRaggedParams& p) { return p.kp; }
inline KvcacheKernelParams& kvc_kp(KvcacheKernelParams& p) { return p; }
inline KvcacheKernelParams& kvc_kp(KvcacheRaggedParams& p) { return p.kp; }

// the kernel of a dense or of a ragged call (a file that owns both names both: both are instantiated, as both kinds of call need them)
template <typename P, typename KD, typename KR>
auto kvc_pick(KD* dense, KR* ragged) {
    if constexpr (kKvcIsRagged<P>) return ragged;
    else return dense;
}

// a call without a window as the window code sees it: both sides unbounded, or the causal limit on the right.  The families that keep one
// sliding-window instantiation for plain, causal and windowed calls (softcap, sinks, head_dim 256) launch on this copy.
template <typename P>
P as_window(P p) {
    KvcacheKernelParams& kp = kvc_kp(p);
    if (!kp.is_local) {
        kp.window_left = -1;
        kp.window_right = kp.is_causal ? 0 : -1;
    }
    return p;
}

// What the launchers fill in behind the caller: row tiles, rows of the partial planes, the keys of a split, the LSE plane behind the O planes.
inline void finish_params(KvcacheKernelParams& kp, int64_t rows_total, int32_t row_tile) {
    kp.n_row_tiles = (int32_t)(((int64_t)kp.seqlen_q * kp.h_ratio + row_tile - 1) / row_tile);
    kp.rows_total = rows_total;
    const int64_t steps = kvcache_steps(kp);
    if (kp.n_split < 1) kp.n_split = 1;
    kp.split_keys = (int32_t)(((steps + kp.n_split - 1) / kp.n_split) * kKvcStep);
    if (kp.split_keys <= 0) kp.split_keys = kKvcStep;
    if (kp.n_split > 1) kp.ws_lse = kp.ws_o + (int64_t)kp.n_split * kp.rows_total * kp.d;
}

// ---- runtime values -> compile-time leaf -------------------------------------------------------------------------------------------------
template <typename T_, int D_, bool PAGED_ = false, int ES_ = 2>
struct KvcLeaf {
    using T = T_;
    static constexpr int D = D_;
    static constexpr bool PAGED = PAGED_;
    static constexpr int ES = ES_;      // bytes per cache element
};

// f(KvcLeaf<T, D>) for the dtype (0 = fp16, else bf16) and the head_dim of the list that d names (the last one where it names none)
template <int D0, int... DS, typename F>
void kvc_dispatch_td(int dtype, int d, F&& f) {
    if constexpr (sizeof...(DS) > 0) {
        if (d != D0) return kvc_dispatch_td<DS...>(dtype, d, f);
    }
    if (dtype == 0) f(KvcLeaf<_Float16, D0>{});
    else f(KvcLeaf<__bf16, D0>{});
}

// ... and f(KvcLeaf<T, D, PAGED, ES>) with the layout and the element size of kp's cache
template <int... DS, typename F>
void kvc_dispatch(const KvcacheKernelParams& kp, int dtype, F&& f) {
    kvc_dispatch_td<DS...>(dtype, kp.d, [&](auto td) {
        using T = typename decltype(td)::T;
        constexpr int D = decltype(td)::D;
        const bool paged = kp.block_table != nullptr;
        if (kp.cache_fp8) paged ? f(KvcLeaf<T, D, true, 1>{}) : f(KvcLeaf<T, D, false, 1>{});
        else paged ? f(KvcLeaf<T, D, true, 2>{}) : f(KvcLeaf<T, D, false, 2>{});
    });
}

// ---- the three launches of a call ----------------------------------------------------------------------------------------------------------
template <typename A>
void kvc_launch_attn(void (*kernel)(A), unsigned grid, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kKvcThreads), 0, s, a);
}

// a combine kernel at head_dim D (the plain ones, and the sink combines of fa_fwd_kvcache_sink.hip) over rows_total output rows
template <int D, typename A>
void kvc_launch_combine(void (*kernel)(A), int64_t rows_total, hipStream_t s, const A& a) {
    const int64_t rows_per_block = kKvcCombineThreads / (D / 8);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((rows_total + rows_per_block - 1) / rows_per_block)), dim3(kKvcCombineThreads), 0, s, a);
}

template <int... DS, typename P>
void launch_combine(const P& p, int dtype, hipStream_t s) {
    kvc_dispatch_td<DS...>(dtype, kvc_kp(p).d, [&](auto td) {
        using T = typename decltype(td)::T;
        constexpr int D = decltype(td)::D;
        if constexpr (kKvcIsRagged<P>) kvc_launch_combine<D>(fa_kvcache_combine_ragged_kernel<T, D>, kvc_kp(p).rows_total, s, p);
        else kvc_launch_combine<D>(fa_kvcache_combine_kernel<T, D>, kvc_kp(p).rows_total, s, p);
    });
}

// k_new / v_new -> the cache, where the call brings any: one thread per 8 elements of a new row
template <int... DS, typename P>
void launch_append(const P& p, int dtype, hipStream_t s) {
    const KvcacheKernelParams& kp = kvc_kp(p);
    int64_t rows;       // new rows of the call
    bool any;
    if constexpr (kKvcIsRagged<P>) {
        rows = p.total_kn;
        any = p.cu_kn != nullptr && rows > 0;
    } else {
        rows = (int64_t)kp.b * kp.seqlen_new;
        any = kp.seqlen_new > 0;
    }
    if (kp.k_new == nullptr || !any) return;
    kvc_dispatch<DS...>(kp, dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        auto launch = [&](auto* kernel) {
            const int64_t n = rows * kp.h_k * (K::D / 8);
            hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
        };
        // (the 16-bit appends copy bits: they are not instantiated per dtype)
        if constexpr (kKvcIsRagged<P>) launch(fa_kvcache_append_ragged_kernel<std::conditional_t<K::ES == 1, T, _Float16>, K::D, K::PAGED, K::ES>);
        else if constexpr (K::ES == 1) launch(fa_kvcache_append_fp8_kernel<T, K::D, K::PAGED>);
        else if constexpr (K::PAGED) launch(fa_kvcache_append_paged_kernel<K::D>);
        else launch(fa_kvcache_append_kernel<K::D>);
    });
}

// One call behind finish_params at a head_dim of the list: the append, the attention launch `attn(grid)` (the caller's; grid = every workgroup of
// the call), and the combine of a split call - with sinks the sink combine, which adds the sink as one more term of the merge.
template <int... DS, typename P, typename Attn>
hipError_t kvc_launch_call(const P& p, int dtype, hipStream_t s, const KvcacheSink& sink, Attn&& attn) {
    const KvcacheKernelParams& kp = kvc_kp(p);
    launch_append<DS...>(p, dtype, s);
    int64_t grid;
    if constexpr (kKvcIsRagged<P>) {
        if (p.total_q <= 0) return hipGetLastError();
        grid = (int64_t)p.slots * kp.h_k * kp.n_split;
    } else {
        grid = (int64_t)kp.b * kp.h_k * kp.n_row_tiles * kp.n_split;
    }
    const hipError_t e = attn((unsigned)grid);
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) {
        if (sink.ptr != nullptr) return launch_kvcache_sink_combine(p, sink, dtype, s);
        launch_combine<DS...>(p, dtype, s);
    }
    return hipGetLastError();
}

// The attention launch of a call at head_dim 64 / 128, by family.  The order of the tests is behaviour: 64-row tiles, then a soft cap, then
// sinks on an unsplit call (a split one runs the kernels without sinks and the sink combine), then a tree mask, and last `own`, the caller's
// window / paged / plain kernels.  Each family file launches its attention kernel alone, on the grid it is given.
template <typename P, typename Own>
hipError_t kvc_route_attn(const P& p, int dtype, unsigned grid, hipStream_t s, float cap_pre, const KvcacheSink& sink, const KvcacheTree& tree,
                          int32_t row_tile, Own&& own) {
    if (row_tile == kKvcPrefillRows) return launch_kvcache_prefill_attn(p, dtype, grid, s);
    if (cap_pre > 0.f) return launch_kvcache_softcap_attn(p, cap_pre, dtype, grid, s);
    if (sink.ptr != nullptr && kvc_kp(p).n_split == 1) return launch_kvcache_sink_attn(p, sink, dtype, grid, s);
    if (tree.ptr != nullptr) return launch_kvcache_tree_attn(p, tree, dtype, grid, s);
    own();
    return hipSuccess;
}

}  // namespace

}  // namespace fa
