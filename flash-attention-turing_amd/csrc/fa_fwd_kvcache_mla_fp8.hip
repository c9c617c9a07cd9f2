// fa_fwd_kvcache_mla_fp8.hip — MLA decode, dense and sparse, over an FP8 latent KV cache of 656-byte rows (kv_format = FA_MLA_KV_FP8_ROWS656): every
// kernel of fa_run_mla_fwd_kvcache / fa_run_mla_sparse_fwd_kvcache for that format.
//
//   The attention body is kvcache_mla_attn of fa_kvcache_mla_attn.hpp with the row format MlaRows8 (which describes the row, its loads and the
//   dequantisation), dense and SPARSE.  This file names its instantiations and holds the append and the launchers.
//   * The append (dense call only) quantises kv_new in place: one wave per new row, lane l holds columns 8 l .. 8 l + 7, the 16 lanes of a tile take
//     amax over their finite elements by cross-lane max, scale = max(amax, 2^-24) / 448 (the correctly rounded quotient), codes by quant8_e4m3
//     (fa_kvcache_quant.hpp), the rope part copied.  Drop and clamp rules of fa_kvcache_mla_append_kernel.
//   Kernels of this file: 8 dense attention ((fp16, bf16) x (causal, not) x (contiguous, paged)), 4 sparse attention ((fp16, bf16) x (contiguous, paged)),
//   4 append ((fp16, bf16) x (contiguous, paged)), 2 combine (fa_kvcache_combine_kernel at D = 512).
#include "fa_kvcache_mla_attn.hpp"
#include "fa_kvcache_quant.hpp"

namespace fa {

namespace {

// ONE workgroup per compute unit, as the 16-bit MLA kernels ship: O^T (128 registers), Q^T (72) and the staging set (24) next to the softmax; with the
// register class ahead of the range's length in the allocator (build.py EXTRA_FLAGS) Q^T and the staging set take the AGPRs.
template <typename T, bool CAUSAL, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_mla_fp8_kernel(const KvcacheMlaParams mp) {
    kvcache_mla_attn<T, MlaRows8, CAUSAL, PAGED, false>(mp.kp, nullptr, 0, 0, 0);
}

template <typename T, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_mla_sparse_fp8_kernel(const KvcacheMlaSparseParams sp) {
    kvcache_mla_attn<T, MlaRows8, false, PAGED, true>(sp.kp, sp.indices, sp.idx_batch, sp.idx_row, sp.topk);
}

// kv_new (b, seqlen_new, 1, 576) of T -> whole 656-byte cache rows cache_seqlens[i] .. + seqlen_new - 1: one wave per new row, four rows a workgroup.  Lane l
// holds columns 8 l .. 8 l + 7; lanes 16 g .. 16 g + 15 are tile g.  Rows at or past the capacity seqlen_cache are dropped; PAGED: row (.) % page_size of
// page min((uint32_t)block_table[i][(.) / page_size], num_blocks - 1) - the rules of fa_kvcache_mla_append_kernel.  kc in bytes, kn in elements.
template <typename T, bool PAGED>
__global__ __launch_bounds__(256) void fa_kvcache_mla_append_fp8_kernel(const KvcacheMlaParams mp) {
    const KvcacheKernelParams& p = mp.kp;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (int64_t)p.b * p.seqlen_new) return;
    const int t = (int)(r % p.seqlen_new);
    const int bidx = (int)(r / p.seqlen_new);
    const int cs = p.cache_seqlens[bidx];
    const int row = (cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return;
    int64_t blk = bidx, prow = row;
    if constexpr (PAGED) {
        const int col = row / p.page_size;
        prow = row - col * p.page_size;
        blk = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
    }
    const char* src = (const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row);
    char* dst = (char*)p.k_cache + (blk * p.kc.batch + prow * p.kc.row);
    const u32x4 x = *(const u32x4*)(src + 16 * lane);
    // amax over the finite elements (NaN and +-inf skipped: |bits| below the first non-finite pattern), exact in fp32
    float amax = 0.f;
    static_for<0, 8>([&](auto ee) {
        constexpr int e = decltype(ee)::value;
        const uint16_t bits = (uint16_t)((x[e >> 1] >> (16 * (e & 1))) & 0x7fffu);
        const bool finite = bits < (__is_same(T, _Float16) ? 0x7c00u : 0x7f80u);
        amax = fmaxf(amax, finite ? LP<T>::to_float(bits) : 0.f);
    });
    static_for<0, 4>([&](auto ss) { amax = fmaxf(amax, __shfl_xor(amax, 1 << decltype(ss)::value, 64)); });
    const float scale = fmaxf(amax, 0x1p-24f) / 448.f;
    *(u32x2*)(dst + 8 * lane) = quant8_e4m3<T>(x, scale);
    if ((lane & 15) == 0) *(float*)(dst + MlaRows8::kScales + 4 * (lane >> 4)) = scale;
    if (lane < 2 * kMlaDR / 16) *(u32x4*)(dst + MlaRows8::kRope + 16 * lane) = *(const u32x4*)(src + 2 * kMlaDV + 16 * lane);
}

}  // namespace

// append, attention, combine: launch_fwd_kvcache_mla for kv_format = FA_MLA_KV_FP8_ROWS656.  mp.kp as there, with kc in bytes and cache_fp8 = 1.
hipError_t launch_fwd_kvcache_mla_fp8(KvcacheMlaParams mp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = mp.kp;
    if (kp.d != kMlaDV || mp.d_qk != kMlaDK || kp.h_k != 1 || !kp.cache_fp8) return hipErrorInvalidValue;
    finish_params(kp, (int64_t)kp.b * kp.h * kp.seqlen_q, kMlaRows);
    const bool paged = kp.block_table != nullptr;
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        if (kp.k_new != nullptr && kp.seqlen_new > 0) {
            const int64_t n = (int64_t)kp.b * kp.seqlen_new;
            auto* append = paged ? fa_kvcache_mla_append_fp8_kernel<T, true> : fa_kvcache_mla_append_fp8_kernel<T, false>;
            hipLaunchKernelGGL(append, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, mp);
        }
        auto* kernel = kp.is_causal ? (paged ? fa_fwd_kvcache_mla_fp8_kernel<T, true, true> : fa_fwd_kvcache_mla_fp8_kernel<T, true, false>)
                                    : (paged ? fa_fwd_kvcache_mla_fp8_kernel<T, false, true> : fa_fwd_kvcache_mla_fp8_kernel<T, false, false>);
        kvc_launch_attn(kernel, grid, s, mp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) mla_launch_combine(kp, dtype, s);
    return hipGetLastError();
}

// attention, combine: launch_fwd_kvcache_mla_sparse for kv_format = FA_MLA_KV_FP8_ROWS656 (the split is sized as there).
hipError_t launch_fwd_kvcache_mla_sparse_fp8(KvcacheMlaSparseParams sp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = sp.kp;
    if (kp.d != kMlaDV || sp.d_qk != kMlaDK || kp.h_k != 1 || !kp.cache_fp8 || sp.indices == nullptr || sp.topk < kKvcStep || sp.topk % kKvcStep != 0)
        return hipErrorInvalidValue;
    mla_sparse_finish_params(kp, sp.topk);
    const bool paged = kp.block_table != nullptr;
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.seqlen_q * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        kvc_launch_attn(paged ? fa_fwd_kvcache_mla_sparse_fp8_kernel<T, true> : fa_fwd_kvcache_mla_sparse_fp8_kernel<T, false>, grid, s, sp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) mla_launch_combine(kp, dtype, s);
    return hipGetLastError();
}

}  // namespace fa
