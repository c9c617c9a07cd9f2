// fa_fwd_kvcache_mla_sparse.hip — sparse MLA decode over a latent KV cache of 16-bit rows (DeepSeek Sparse Attention: top-k key indices per query
// token): every kernel of fa_run_mla_sparse_fwd_kvcache.
//
//   The attention body is kvcache_mla_attn of fa_kvcache_mla_attn.hpp (which describes the sparse tiling, split and staging) with the row format
//   MlaRows16, SPARSE.  This file names its instantiations and holds the launcher.
//   Kernels of this file: 4 attention ((fp16, bf16) x (contiguous, paged)), 2 combine.  There is no append.
#include "fa_kvcache_mla_attn.hpp"

namespace fa {

namespace {

// ONE workgroup per compute unit, as the dense MLA kernels ship (fa_fwd_kvcache_mla.hip): O^T (128 registers), Q^T (72) and the staging set (36) next
// to the softmax; with the register class ahead of the range's length in the allocator (build.py EXTRA_FLAGS) Q^T and the staging set take the AGPRs.
template <typename T, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_mla_sparse_kernel(const KvcacheMlaSparseParams sp) {
    kvcache_mla_attn<T, MlaRows16, false, PAGED, true>(sp.kp, sp.indices, sp.idx_batch, sp.idx_row, sp.topk);
}

}  // namespace

// attention, combine.  sp.kp as the C ABI filled it: d = 512, h_k = 1, h_ratio = h, k_cache the latent cache, n_split chosen (kvcache_split over topk and
// this grid: b x seqlen_q x ceil(h / 64) workgroups a split; mla_sparse_finish_params).
hipError_t launch_fwd_kvcache_mla_sparse(KvcacheMlaSparseParams sp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = sp.kp;
    if (kp.d != kMlaDV || sp.d_qk != kMlaDK || kp.h_k != 1 || sp.indices == nullptr || sp.topk < kKvcStep || sp.topk % kKvcStep != 0) return hipErrorInvalidValue;
    mla_sparse_finish_params(kp, sp.topk);
    const bool paged = kp.block_table != nullptr;
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.seqlen_q * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        kvc_launch_attn(paged ? fa_fwd_kvcache_mla_sparse_kernel<T, true> : fa_fwd_kvcache_mla_sparse_kernel<T, false>, grid, s, sp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) mla_launch_combine(kp, dtype, s);
    return hipGetLastError();
}

}  // namespace fa
