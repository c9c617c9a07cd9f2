// fa_kvcache_kernels.hpp — the combine and append kernels of a decode call over a KV cache, dense and ragged, as templates: instantiated by the files
// that launch them (launch_combine / launch_append of fa_kvcache_launch.hpp), and kvcache_steps, the steps a launch's splits must cover.
// The merge loop is written out in both combine kernels (and in kvcache_sink_combine of fa_fwd_kvcache_sink.hip) and the index decode in all four
// append kernels ON PURPOSE: folded into one helper they give the same bits but other instructions - fa_kvcache_combine_kernel went from 28 VGPRs /
// 583 instructions to 32 / 595 with the two loops in an always-inline helper and to 34 / 590 routed through the sink combine with a SINK flag -
// and tests/test_kvcache_fp8_cpu.py pins the registers of these kernels.
#pragma once
#include "fa_kvcache_attn.hpp"

namespace fa {

namespace {

// One pass per output row over the splits, in split order (deterministic): O = sum_s exp(lse_s - M) O_s / sum_s exp(lse_s - M),
// LSE = M + log(sum); splits with LSE = -inf saw no key of the row and are skipped (their O plane was never written); a row no split saw
// is a dead row: O = 0, LSE = 0.  A NaN partial (a NaN or +inf score in its split; its O plane is written) makes the row NaN, O and LSE,
// as one pass over all keys would: fmaxf drops NaN from M, so it is tracked on the side.
template <typename T, int D>
__global__ __launch_bounds__(kKvcCombineThreads) void fa_kvcache_combine_kernel(const KvcacheKernelParams p) {
    constexpr int TPR = D / 8;                              // threads per row, 8 columns each
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)blockIdx.x * (kKvcCombineThreads / TPR) + tid / TPR;
    if (R >= p.rows_total) return;
    const int col = (tid % TPR) * 8;
    const int ns = p.n_split;
    float M = -INFINITY;
    bool nan_part = false;
    for (int s = 0; s < ns; ++s) {
        const float ls = p.ws_lse[(int64_t)s * p.rows_total + R];
        nan_part |= __builtin_isnan(ls);
        M = fmaxf(M, ls);
    }
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
    if (nan_part) sum = __builtin_nanf("");
    const bool live = !(sum == 0.f);
    const float inv = live ? 1.0f / sum : 0.f;
    const int t = (int)(R % p.seqlen_q);
    const int64_t bhq = R / p.seqlen_q;
    const int hq = (int)(bhq % p.h), bidx = (int)(bhq / p.h);
    char* orow = (char*)p.o_ptr + 2 * ((int64_t)bidx * p.o.batch + (int64_t)t * p.o.row + (int64_t)hq * p.o.head + col);
    *(u32x4*)orow = u32x4{LP<T>::pack2(acc[0] * inv, acc[1] * inv), LP<T>::pack2(acc[2] * inv, acc[3] * inv),
                          LP<T>::pack2(acc[4] * inv, acc[5] * inv), LP<T>::pack2(acc[6] * inv, acc[7] * inv)};
    if (tid % TPR == 0) p.lse_ptr[R] = live ? M + logf(sum) : 0.f;
}

// k_new / v_new (b, seqlen_new, h_k, d) -> cache rows cache_seqlens[i] .. + seqlen_new - 1; rows at or past seqlen_cache are dropped
// (a caller that breaks the documented precondition loses the rows that do not fit, nothing is written outside the cache).
template <int D>
__global__ __launch_bounds__(256) void fa_kvcache_append_kernel(const KvcacheKernelParams p) {
    constexpr int SLOTS = D / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)p.b * p.seqlen_new * p.h_k * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    int64_t r = i / SLOTS;
    const int kvh = (int)(r % p.h_k);
    r /= p.h_k;
    const int t = (int)(r % p.seqlen_new);
    const int bidx = (int)(r / p.seqlen_new);
    const int cs = p.cache_seqlens[bidx];
    const int row = (cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return;
    const u32x4 kx = *(const u32x4*)((const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row + (int64_t)kvh * p.kn.head + 8 * slot));
    const u32x4 vx = *(const u32x4*)((const char*)p.v_new + 2 * ((int64_t)bidx * p.vn.batch + (int64_t)t * p.vn.row + (int64_t)kvh * p.vn.head + 8 * slot));
    *(u32x4*)((char*)p.k_cache + 2 * ((int64_t)bidx * p.kc.batch + (int64_t)row * p.kc.row + (int64_t)kvh * p.kc.head + 8 * slot)) = kx;
    *(u32x4*)((char*)p.v_cache + 2 * ((int64_t)bidx * p.vc.batch + (int64_t)row * p.vc.row + (int64_t)kvh * p.vc.head + 8 * slot)) = vx;
}

// The same through the block table of a paged cache: row cache_seqlens[i] + t is row (.) % page_size of page
// min((uint32_t)block_table[i][(.) / page_size], num_blocks - 1); rows at or past the capacity seqlen_cache are dropped, so the column
// read is always inside the table row, and whatever a needed entry holds, nothing is written outside the pool.
template <int D>
__global__ __launch_bounds__(256) void fa_kvcache_append_paged_kernel(const KvcacheKernelParams p) {
    constexpr int SLOTS = D / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)p.b * p.seqlen_new * p.h_k * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    int64_t r = i / SLOTS;
    const int kvh = (int)(r % p.h_k);
    r /= p.h_k;
    const int t = (int)(r % p.seqlen_new);
    const int bidx = (int)(r / p.seqlen_new);
    const int cs = p.cache_seqlens[bidx];
    const int row = (cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return;
    const int col = row / p.page_size, prow = row - col * p.page_size;
    const int64_t page = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
    const u32x4 kx = *(const u32x4*)((const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row + (int64_t)kvh * p.kn.head + 8 * slot));
    const u32x4 vx = *(const u32x4*)((const char*)p.v_new + 2 * ((int64_t)bidx * p.vn.batch + (int64_t)t * p.vn.row + (int64_t)kvh * p.vn.head + 8 * slot));
    *(u32x4*)((char*)p.k_cache + 2 * (page * p.kc.batch + (int64_t)prow * p.kc.row + (int64_t)kvh * p.kc.head + 8 * slot)) = kx;
    *(u32x4*)((char*)p.v_cache + 2 * (page * p.vc.batch + (int64_t)prow * p.vc.row + (int64_t)kvh * p.vc.head + 8 * slot)) = vx;
}

// The append into an 8-bit cache, both layouts: 8 elements per thread, quantised by quant8_e4m3 of fa_kvcache_quant.hpp (16 bytes read, 8 written).  Rows and pages are
// found exactly as in the 16-bit kernels above.
template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(256) void fa_kvcache_append_fp8_kernel(const KvcacheKernelParams p) {
    constexpr int SLOTS = D / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)p.b * p.seqlen_new * p.h_k * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    int64_t r = i / SLOTS;
    const int kvh = (int)(r % p.h_k);
    r /= p.h_k;
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
    const float kd = p.k_descale != nullptr ? p.k_descale[(int64_t)bidx * p.kds_batch + (int64_t)kvh * p.kds_head] : 1.f;
    const float vd = p.v_descale != nullptr ? p.v_descale[(int64_t)bidx * p.vds_batch + (int64_t)kvh * p.vds_head] : 1.f;
    const u32x4 kx = *(const u32x4*)((const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row + (int64_t)kvh * p.kn.head + 8 * slot));
    const u32x4 vx = *(const u32x4*)((const char*)p.v_new + 2 * ((int64_t)bidx * p.vn.batch + (int64_t)t * p.vn.row + (int64_t)kvh * p.vn.head + 8 * slot));
    *(u32x2*)((char*)p.k_cache + (blk * p.kc.batch + prow * p.kc.row + (int64_t)kvh * p.kc.head + 8 * slot)) = quant8_e4m3<T>(kx, kd);
    *(u32x2*)((char*)p.v_cache + (blk * p.vc.batch + prow * p.vc.row + (int64_t)kvh * p.vc.head + 8 * slot)) = quant8_e4m3<T>(vx, vd);
}

// fa_kvcache_combine_kernel over the h * total_q rows of a ragged call: row R = hq * total_q + (packed query row)
template <typename T, int D>
__global__ __launch_bounds__(kKvcCombineThreads) void fa_kvcache_combine_ragged_kernel(const KvcacheRaggedParams rp) {
    const KvcacheKernelParams& p = rp.kp;
    constexpr int TPR = D / 8;                              // threads per row, 8 columns each
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)blockIdx.x * (kKvcCombineThreads / TPR) + tid / TPR;
    if (R >= p.rows_total) return;
    const int hq = (int)(R / rp.total_q);
    const int64_t row = R - (int64_t)hq * rp.total_q;
    if (row >= rp.cu_q[p.b]) return;                        // a surplus row of q: no partial was written, o / lse stay the caller's
    const int col = (tid % TPR) * 8;
    const int ns = p.n_split;
    float M = -INFINITY;
    bool nan_part = false;
    for (int s = 0; s < ns; ++s) {
        const float ls = p.ws_lse[(int64_t)s * p.rows_total + R];
        nan_part |= __builtin_isnan(ls);
        M = fmaxf(M, ls);
    }
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
    if (nan_part) sum = __builtin_nanf("");
    const bool live = !(sum == 0.f);
    const float inv = live ? 1.0f / sum : 0.f;
    char* orow = (char*)p.o_ptr + 2 * (row * p.o.row + (int64_t)hq * p.o.head + col);
    *(u32x4*)orow = u32x4{LP<T>::pack2(acc[0] * inv, acc[1] * inv), LP<T>::pack2(acc[2] * inv, acc[3] * inv),
                          LP<T>::pack2(acc[4] * inv, acc[5] * inv), LP<T>::pack2(acc[6] * inv, acc[7] * inv)};
    if (tid % TPR == 0) p.lse_ptr[R] = live ? M + logf(sum) : 0.f;
}

// k_new / v_new (total_kn, h_k, d) -> the caches.  One thread per 8 elements of a packed new row r; its sequence is the i with cu_kn[i] <= r <
// cu_kn[i + 1] (bisection over the b + 1 entries; empty sequences share a value and are stepped over), rows at or past cu_kn[b] are not read.
// The row goes to cache row max(cache_seqlens[i], 0) + (r - cu_kn[i]); at or past the capacity seqlen_cache it is dropped, so nothing is written
// outside the sequence's capacity or, through a clamped table entry, outside the pool.  ES = 1: quantised as in fa_kvcache_append_fp8_kernel.
template <typename T, int D, bool PAGED, int ES>
__global__ __launch_bounds__(256) void fa_kvcache_append_ragged_kernel(const KvcacheRaggedParams rp) {
    const KvcacheKernelParams& p = rp.kp;
    constexpr int SLOTS = D / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = rp.total_kn * p.h_k * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    int64_t r = i / SLOTS;
    const int kvh = (int)(r % p.h_k);
    r /= p.h_k;
    int lo = 0, hi = p.b;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rp.cu_kn[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    if (lo >= p.b) return;                                  // a surplus row past cu_kn[b]
    const int bidx = lo;
    const int64_t t = r - rp.cu_kn[bidx];
    if (t < 0) return;                                      // (cu_kn[0] > 0: rows in front of the first sequence belong to nobody)
    const int cs = p.cache_seqlens[bidx];
    const int64_t row = (int64_t)(cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return;
    int64_t blk = bidx, prow = row;
    if constexpr (PAGED) {
        const int col = (int)(row / p.page_size);
        prow = row - (int64_t)col * p.page_size;
        blk = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
    }
    const u32x4 kx = *(const u32x4*)((const char*)p.k_new + 2 * (r * p.kn.row + (int64_t)kvh * p.kn.head + 8 * slot));
    const u32x4 vx = *(const u32x4*)((const char*)p.v_new + 2 * (r * p.vn.row + (int64_t)kvh * p.vn.head + 8 * slot));
    char* kdst = (char*)p.k_cache + ES * (blk * p.kc.batch + prow * p.kc.row + (int64_t)kvh * p.kc.head + 8 * slot);
    char* vdst = (char*)p.v_cache + ES * (blk * p.vc.batch + prow * p.vc.row + (int64_t)kvh * p.vc.head + 8 * slot);
    if constexpr (ES == 1) {
        const float kd = p.k_descale != nullptr ? p.k_descale[(int64_t)bidx * p.kds_batch + (int64_t)kvh * p.kds_head] : 1.f;
        const float vd = p.v_descale != nullptr ? p.v_descale[(int64_t)bidx * p.vds_batch + (int64_t)kvh * p.vds_head] : 1.f;
        *(u32x2*)kdst = quant8_e4m3<T>(kx, kd);
        *(u32x2*)vdst = quant8_e4m3<T>(vx, vd);
    } else {
        *(u32x4*)kdst = kx;
        *(u32x4*)vdst = vx;
    }
}

// 32-key steps the splits of a launch must cover.  A window with a left edge bounds what one workgroup reads from its base: the tile's
// largest lim minus its smallest lo is at most left + seqlen_q + max(right, 0), plus up to kKvcStep - 1 keys of the base's alignment.
inline int64_t kvcache_steps(const KvcacheKernelParams& kp) {
    int64_t keys = kp.seqlen_cache;
    if (kp.is_local && kp.window_left >= 0) {
        const int64_t span = (int64_t)kp.window_left + kp.seqlen_q + (kp.window_right > 0 ? kp.window_right : 0) + kKvcStep - 1;
        if (span < keys) keys = span;
    }
    return (keys + kKvcStep - 1) / kKvcStep;
}

}  // namespace

}  // namespace fa
