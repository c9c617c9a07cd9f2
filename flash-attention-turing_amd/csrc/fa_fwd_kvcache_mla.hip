// fa_fwd_kvcache_mla.hip — multi-head latent attention (MLA) decode over a latent KV cache of 16-bit rows: every kernel of fa_run_mla_fwd_kvcache.
//
//   The attention body is kvcache_mla_attn of fa_kvcache_mla_attn.hpp (which describes it) with the row format MlaRows16, dense.  This file names its
//   instantiations and holds the append and the launcher.
//   * The append copies the 72 16-byte slots of a kv_new row, contiguous or through the table, with the drop and clamp rules of the other appends.
//   Kernels of this file: 8 attention ((fp16, bf16) x (causal, not) x (contiguous, paged)), 2 append, 2 combine.
#include "fa_kvcache_mla_attn.hpp"

namespace fa {

namespace {

// ONE workgroup per compute unit, as at head_dim 256: a lane holds O^T (128 registers), Q^T (72) and the staging set (36) next to the softmax, about
// 330 registers.  Built for two workgroups (256 registers) the kernels spill 400 bytes a lane; at one, with the register class ahead of the range's
// length in the allocator (build.py EXTRA_FLAGS, the flag of fa_fwd_kvcache_d256.hip), Q^T and the staging set take the AGPRs: no scratch and no
// v_accvgpr moves in the loop.  FA_MLA_WG_PER_CU = 2 builds the spilling variant (the A/B of DESIGN.md).
#ifndef FA_MLA_WG_PER_CU
#define FA_MLA_WG_PER_CU 1
#endif

template <typename T, bool CAUSAL, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, FA_MLA_WG_PER_CU) void fa_fwd_kvcache_mla_kernel(const KvcacheMlaParams mp) {
    kvcache_mla_attn<T, MlaRows16, CAUSAL, PAGED, false>(mp.kp, nullptr, 0, 0, 0);
}

// kv_new (b, seqlen_new, 1, 576) -> cache rows cache_seqlens[i] .. + seqlen_new - 1: one thread per 16-byte slot of a new row.  Rows at or past the
// capacity seqlen_cache are dropped; PAGED: row (.) % page_size of page min((uint32_t)block_table[i][(.) / page_size], num_blocks - 1), so the
// column read is always inside the table row, and whatever a needed entry holds, nothing is written outside the pool.
template <bool PAGED>
__global__ __launch_bounds__(256) void fa_kvcache_mla_append_kernel(const KvcacheMlaParams mp) {
    const KvcacheKernelParams& p = mp.kp;
    constexpr int SLOTS = kMlaDK / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)p.b * p.seqlen_new * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    const int64_t r = i / SLOTS;
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
    const u32x4 x = *(const u32x4*)((const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row + 8 * slot));
    *(u32x4*)((char*)p.k_cache + 2 * (blk * p.kc.batch + prow * p.kc.row + 8 * slot)) = x;
}

}  // namespace

// append, attention, combine.  mp.kp as the C ABI filled it: d = 512 (the width of V, of o and of the partial planes), h_k = 1, h_ratio = h, k_cache the
// latent cache, k_new the new rows, n_split chosen (kvcache_split over this grid: b x ceil(seqlen_q * h / 64) workgroups a split).
hipError_t launch_fwd_kvcache_mla(KvcacheMlaParams mp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = mp.kp;
    if (kp.d != kMlaDV || mp.d_qk != kMlaDK || kp.h_k != 1) return hipErrorInvalidValue;
    finish_params(kp, (int64_t)kp.b * kp.h * kp.seqlen_q, kMlaRows);
    const bool paged = kp.block_table != nullptr;
    if (kp.k_new != nullptr && kp.seqlen_new > 0) {
        const int64_t n = (int64_t)kp.b * kp.seqlen_new * (kMlaDK / 8);
        hipLaunchKernelGGL(paged ? fa_kvcache_mla_append_kernel<true> : fa_kvcache_mla_append_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mp);
    }
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        auto* kernel = kp.is_causal ? (paged ? fa_fwd_kvcache_mla_kernel<T, true, true> : fa_fwd_kvcache_mla_kernel<T, true, false>)
                                    : (paged ? fa_fwd_kvcache_mla_kernel<T, false, true> : fa_fwd_kvcache_mla_kernel<T, false, false>);
        kvc_launch_attn(kernel, grid, s, mp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) mla_launch_combine(kp, dtype, s);
    return hipGetLastError();
}

}  // namespace fa
