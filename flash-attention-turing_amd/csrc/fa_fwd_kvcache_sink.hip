// fa_fwd_kvcache_sink.hip — decode attention over a KV cache with attention sinks (fa_kvcache_options_v6: sinks != NULL).
//
//   Query head hq has one learned logit sink = sinks[hq * sinks_stride], in the units of the final scores (behind softmax_scale and k_descale; it
//   is never scaled).  With the visible scores s_j of a row and M = max(max_j s_j, sink):
//       out = sum_j exp(s_j - M) v_j / (sum_j exp(s_j - M) + exp(sink - M)),   lse = M + log(sum_j exp(s_j - M) + exp(sink - M))
//   - the sink is one more key of the row whose V row is zero, and the LSE includes it, so exp(s_j - lse) are the probabilities used.
//   * Unsplit launch (n_split = 1): the attention body is kvcache_attn of fa_kvcache_attn.hpp with SINK = true.  The sink enters in the per-row
//     epilogue, behind the merge of the four waves and in front of inv and lse: one load and a few fp32 operations per row; the 32-key loop is
//     the loop of the call without sinks.
//   * Split launch: the attention kernels are those of the call without sinks, launched by fa_fwd_kvcache.hip / fa_fwd_kvcache_ragged.hip as ever
//     - the partial planes hold what they held - and the combine kernels below take the place of theirs: the merge over the splits with the
//     sink as one more term, added once per row.  The split count and the workspace do not know about sinks.
//   * A sink of -inf changes nothing, bit for bit: fmaxf with -inf keeps M and the term is + 0.0f (the -inf - -inf cases are guarded).  A row
//     that sees no key gives O = 0 and LSE = the sink where it is finite, and stays dead (O = 0, LSE = 0) under -inf.  A NaN sink makes the
//     rows of its head NaN, O and LSE.
//   * One attention instantiation per (dtype, head_dim, layout, cache element), dense and ragged: the sliding-window code serves plain and causal
//     calls as the windows (-1, -1) and (-1, 0), as in fa_fwd_kvcache_softcap.hip.  32 attention kernels and 8 combines.  FA_KVC_SINK_PLAIN = 1
//     builds the plain and causal instantiations as well (64 more kernels) and sends calls without a window to them: the A / B of DESIGN.md
//     3.10 (tools/build_variant.py sinkplain -DFA_KVC_SINK_PLAIN=1, then tools/kvcache_bench.py --sinks --baseline-library).
//   * Sinks with a soft cap, and sinks at head_dim 256, are refused by the C ABI: nothing here serves them.
#include "fa_kvcache_launch.hpp"

#ifndef FA_KVC_SINK_PLAIN
#define FA_KVC_SINK_PLAIN 0
#endif

namespace fa {

namespace {

template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_sink_kernel(const KvcacheSinkParams sp) {
    kvcache_attn<T, D, false, PAGED, true, ES, false, false, true>(sp.kp, nullptr, 0.f, sp.sink.ptr, sp.sink.stride);
}

template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_sink_kernel(const KvcacheRaggedSinkParams sp) {
    kvcache_attn<T, D, false, PAGED, true, ES, true, false, true>(sp.rp.kp, &sp.rp, 0.f, sp.sink.ptr, sp.sink.stride);
}

#if FA_KVC_SINK_PLAIN
// every key below L (CAUSAL = false) or the causal limit, without the window code
template <typename T, int D, bool CAUSAL, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_sink_plain_kernel(const KvcacheSinkParams sp) {
    kvcache_attn<T, D, CAUSAL, PAGED, false, ES, false, false, true>(sp.kp, nullptr, 0.f, sp.sink.ptr, sp.sink.stride);
}

template <typename T, int D, bool CAUSAL, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_sink_plain_kernel(const KvcacheRaggedSinkParams sp) {
    kvcache_attn<T, D, CAUSAL, PAGED, false, ES, true, false, true>(sp.rp.kp, &sp.rp, 0.f, sp.sink.ptr, sp.sink.stride);
}
#endif

// fa_kvcache_combine_kernel / fa_kvcache_combine_ragged_kernel with the sink of the row's query head as one more term: M covers it, and it adds
// exp(sink - M) to the sum behind the splits' terms (in split order, as ever) and nothing to O.  The head of row R is found as those kernels find
// it for the output address.  All partials -inf and a finite sink: sum = 1, O = 0, LSE = the sink.
// (A third writing of the merge loop, like the two of fa_kvcache_kernels.hpp and for the reason given there.)
template <typename T, int D, bool RAGGED>
FA_DEV void kvcache_sink_combine(const KvcacheKernelParams& p, const KvcacheRaggedParams* rg, const KvcacheSink& sink) {
    constexpr int TPR = D / 8;                              // threads per row, 8 columns each
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)blockIdx.x * (kKvcCombineThreads / TPR) + tid / TPR;
    if (R >= p.rows_total) return;
    int hq;
    int64_t o_off;                                          // element offset of the row in o
    if constexpr (RAGGED) {
        hq = (int)(R / rg->total_q);
        const int64_t row = R - (int64_t)hq * rg->total_q;
        if (row >= rg->cu_q[p.b]) return;                   // a surplus row of q: no partial was written, o / lse stay the caller's
        o_off = row * p.o.row + (int64_t)hq * p.o.head;
    } else {
        const int t = (int)(R % p.seqlen_q);
        const int64_t bhq = R / p.seqlen_q;
        hq = (int)(bhq % p.h);
        o_off = (bhq / p.h) * p.o.batch + (int64_t)t * p.o.row + (int64_t)hq * p.o.head;
    }
    const int col = (tid % TPR) * 8;
    const int ns = p.n_split;
    const float sk = sink.ptr[(int64_t)hq * sink.stride];
    float M = -INFINITY;
    bool nan_part = false;
    for (int s = 0; s < ns; ++s) {
        const float ls = p.ws_lse[(int64_t)s * p.rows_total + R];
        nan_part |= __builtin_isnan(ls);
        M = fmaxf(M, ls);
    }
    M = fmaxf(M, sk);
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
    // (a sink of -inf adds + 0.0f and never meets M = -inf in the exponential; a NaN sink passes fmaxf unseen and makes the sum NaN here)
    sum += sk == -INFINITY ? 0.f : __expf(sk - M);
    if (nan_part) sum = __builtin_nanf("");
    const bool live = !(sum == 0.f);
    const float inv = live ? 1.0f / sum : 0.f;
    char* orow = (char*)p.o_ptr + 2 * (o_off + col);
    *(u32x4*)orow = u32x4{LP<T>::pack2(acc[0] * inv, acc[1] * inv), LP<T>::pack2(acc[2] * inv, acc[3] * inv),
                          LP<T>::pack2(acc[4] * inv, acc[5] * inv), LP<T>::pack2(acc[6] * inv, acc[7] * inv)};
    if (tid % TPR == 0) p.lse_ptr[R] = live ? M + logf(sum) : 0.f;
}

template <typename T, int D>
__global__ __launch_bounds__(kKvcCombineThreads) void fa_kvcache_sink_combine_kernel(const KvcacheSinkParams sp) {
    kvcache_sink_combine<T, D, false>(sp.kp, nullptr, sp.sink);
}

template <typename T, int D>
__global__ __launch_bounds__(kKvcCombineThreads) void fa_kvcache_sink_combine_ragged_kernel(const KvcacheRaggedSinkParams sp) {
    kvcache_sink_combine<T, D, true>(sp.rp.kp, &sp.rp, sp.sink);
}
template <typename P>
using KvcSinkBlock = std::conditional_t<kKvcIsRagged<P>, KvcacheRaggedSinkParams, KvcacheSinkParams>;

// p as the dense / ragged launcher finished it (row tiles or slots, n_split = 1)
template <typename P>
hipError_t launch_sink_attn(const P& p, const KvcacheSink& sink, int dtype, unsigned grid, hipStream_t s) {
    const KvcSinkBlock<P> sp{as_window(p), sink};
    kvc_dispatch<64, 128>(kvc_kp(p), dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
#if FA_KVC_SINK_PLAIN
        if (!kvc_kp(p).is_local) {
            if (kvc_kp(p).is_causal) kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_sink_plain_kernel<T, K::D, true, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_sink_plain_kernel<T, K::D, true, K::PAGED, K::ES>), grid, s, sp);
            else kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_sink_plain_kernel<T, K::D, false, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_sink_plain_kernel<T, K::D, false, K::PAGED, K::ES>), grid, s, sp);
            return;
        }
#endif
        kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_sink_kernel<T, K::D, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_sink_kernel<T, K::D, K::PAGED, K::ES>), grid, s, sp);
    });
    return hipGetLastError();
}

// behind the attention launch of a split call (n_split > 1, the partial planes of the call without sinks)
template <typename P>
hipError_t launch_sink_combine(const P& p, const KvcacheSink& sink, int dtype, hipStream_t s) {
    const KvcSinkBlock<P> sp{p, sink};
    kvc_dispatch_td<64, 128>(dtype, kvc_kp(p).d, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        kvc_launch_combine<K::D>(kvc_pick<P>(fa_kvcache_sink_combine_kernel<T, K::D>, fa_kvcache_sink_combine_ragged_kernel<T, K::D>), kvc_kp(p).rows_total, s, sp);
    });
    return hipGetLastError();
}

}  // namespace

// grid = b x h_k x row tiles (dense), slots x h_k (ragged)
hipError_t launch_kvcache_sink_attn(const KvcacheKernelParams& kp, const KvcacheSink& sink, int dtype, unsigned grid, hipStream_t s) { return launch_sink_attn(kp, sink, dtype, grid, s); }
hipError_t launch_kvcache_sink_attn(const KvcacheRaggedParams& rp, const KvcacheSink& sink, int dtype, unsigned grid, hipStream_t s) { return launch_sink_attn(rp, sink, dtype, grid, s); }
hipError_t launch_kvcache_sink_combine(const KvcacheKernelParams& kp, const KvcacheSink& sink, int dtype, hipStream_t s) { return launch_sink_combine(kp, sink, dtype, s); }
hipError_t launch_kvcache_sink_combine(const KvcacheRaggedParams& rp, const KvcacheSink& sink, int dtype, hipStream_t s) { return launch_sink_combine(rp, sink, dtype, s); }

}  // namespace fa
