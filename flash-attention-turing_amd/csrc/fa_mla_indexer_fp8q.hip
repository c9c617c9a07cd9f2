// fa_mla_indexer_fp8q.hip — the index logits of fa_run_mla_indexer_logits for FP8 (e4m3) index queries over an FP8 index-key cache
// (fa_mla_indexer_params_v2, q_format = FA_IDX_Q_FP8_E4M3): DeepGEMM's fp8_paged_mqa_logits, e4m3 on both sides of the product.
//
//   logit[t, j] = k_scale[j] * sum_h weights[t, h] * relu(sum_d float(qcode[t, h, d]) * float(kcode[j, d]))   for the keys j < n_t that token t sees.  The scale of
//   the quantised queries is the caller's, folded into weights.
//
//   The body of fa_mla_indexer_logits_kernel<T, 1, PAGED> (fa_mla_indexer.hip) with the product replaced: a workgroup serves one token and a range of wg_keys
//   keys, its four waves take a quarter of the range each and share nothing (no LDS, no barrier).
//   * S = Q K^T on v_mfma_f32_16x16x128_f8f6f4 with e4m3 operands (idx_mfma_e4m3): ONE MFMA per (16 heads, 16 keys) where the 16-bit q_idx kernels issue four
//     16x16x32 ones behind eight conversions.  Q is the A operand; the result has the C / D layout of 16x16x32 - lane l holds key l & 15 and heads 4 (l >> 4) + r
//     of each head block - so the ReLU, the 16 fused multiply-adds in head-block / register order, sum_four_groups and * k_scale are those of that kernel.
//   * Operands.  A lane's 32 bytes of a row are bytes 16 g .. and 64 + 16 g .. (g = l >> 4): for a key these are the two 16-byte loads the FP8-cache path of
//     fa_mla_indexer.hip issues already, now used as they arrive; Q is loaded the same way.  Both sides permute the contraction index identically, so the sum
//     covers the 128 columns whatever order the instruction walks them in.  Every product of two e4m3 values is exact in fp32.
//   * Q of the token stays in registers: 4 head blocks x 8 = 32 (the 16-bit kernels: 64).  Head blocks past h hold zeros and their MFMAs are skipped by a
//     wave-uniform branch.
//   * The ReLU is idxp_relu (the IEEE 754-2019 maximum): a NaN code reaches its column as a NaN, exactly as in fa_mla_indexer_prefill_fp8q.hip, so the two
//     calls agree bit for bit on every input.
//   * Steps of 32 keys with the next step's loads in flight, the contiguous descriptor that ends at row n_t, the paged per-block descriptors over the visible
//     rows of a page with clamped table entries fetched one step ahead, k_scale loaded by the storing lanes under j < n_t, stores by lanes 0 .. 31 under
//     j < n_t with 64-bit row offsets: all as in fa_mla_indexer.hip.  The launcher's wg_keys / n_chunks rule is that file's too.
//   Kernels of this file: 2 (contiguous, paged).
#include "fa_device.hpp"
#include "fa_params.hpp"
#include "fa_mla_indexer.hpp"

namespace fa {

namespace {

template <bool PAGED>
__global__ __launch_bounds__(kIdxThreads, 3) void fa_mla_indexer_fp8q_logits_kernel(const MlaIndexerParams p) {
    constexpr int NHB = 4;                      // head blocks of 16 (h = 64)
    constexpr int ROWB = kIdxD;                 // bytes of a key and of a head of Q

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t id = blockIdx.x;
    const int chunk = (int)(id % (uint32_t)p.n_chunks);
    const int tok = (int)(id / (uint32_t)p.n_chunks);
    const int t = tok % p.seqlen_q, bidx = tok / p.seqlen_q;
    const int L = idx_len(p.cache_seqlens, bidx, p.seqlen_cache);
    const int n = idx_visible(L, p.seqlen_q, t, p.is_causal);
    // this wave's keys: a quarter of the workgroup's range, cut at n
    const int wave_keys = p.wg_keys / kIdxWaves;
    const int64_t kb64 = (int64_t)chunk * p.wg_keys + (int64_t)wave * wave_keys;
    if (kb64 >= n) return;                      // (no barrier in this kernel: a wave leaves on its own)
    const int k_begin = (int)kb64;
    const int k_end = min(k_begin + wave_keys, n);

    const uint32_t colb = (uint32_t)(16 * g);   // byte offset of this lane group's first 16 bytes in a row; the second 16: 64 further on

    // ---- Q of the token (codes; strides in bytes) and the weights of the heads this lane sums -------------------------------------------------
    const int h = p.h;
    u32x4 qf[NHB][2];
    float w[NHB][4];
    {
        const char* qtok = (const char*)p.q_ptr + ((int64_t)bidx * p.q_batch + (int64_t)t * p.q_row);
        const float* wtok = p.w_ptr + ((int64_t)bidx * p.w_batch + (int64_t)t * p.w_row);
        static_for<0, NHB>([&](auto hh) {
            constexpr int hb = decltype(hh)::value;
            const int head = 16 * hb + n16;
            static_for<0, 2>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                qf[hb][i] = head < h ? *(const u32x4*)(qtok + ((int64_t)head * p.q_head + colb + 64 * i)) : u32x4{0u, 0u, 0u, 0u};
            });
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int hd = 16 * hb + 4 * g + r;
                w[hb][r] = hd < h ? wtok[(int64_t)hd * p.w_head] : 0.f;
            });
        });
    }
    const bool hb1 = h > 16, hb2 = h > 32;      // (wave-uniform) head blocks 1 and 2 .. 3 exist

    // ---- key addressing -------------------------------------------------------------------------------------------------------------------
    const uint32_t row_b = (uint32_t)p.k_row;
    const char* kbase = uniform_ptr((const char*)p.k_cache + (PAGED ? (int64_t)0 : (int64_t)bidx * p.k_batch));
    const rsrc_t krs = make_rsrc(kbase, !PAGED && n > 0 ? (uint32_t)(n - 1) * row_b + ROWB : 0u);
    const int P = PAGED ? p.page_size : 1;
    const int32_t* tbl = PAGED ? p.block_table + (int64_t)bidx * p.bt_stride : nullptr;
    const int last_col = PAGED ? p.seqlen_cache / P - 1 : 0;
    // paged: column and row-in-page of the two 16-key blocks of the step whose table entries were fetched last, and those entries
    int pcol = 0, prip = 0;                     // of block 0; block 1 follows 16 rows on
    uint32_t pent[2] = {0u, 0u};
    auto fetch_entries = [&]() __attribute__((always_inline)) {
        if constexpr (PAGED) {
            int c1 = pcol, r1 = prip + 16;
            if (r1 >= P) { r1 = 0; c1 += 1; }
            pent[0] = (uint32_t)tbl[min(pcol, last_col)];
            pent[1] = (uint32_t)tbl[min(c1, last_col)];
        }
    };
    auto advance_entries = [&]() __attribute__((always_inline)) {      // one step (32 keys) on
        if constexpr (PAGED) {
            prip += kIdxStep;
            while (prip >= P) { prip -= P; pcol += 1; }
        }
    };
    const float* ksp = p.k_scale;

    // the loads of the step at key0: st[kb][i] and the scale of the key this lane stores (lanes 0 .. 31: key0 + lane)
    auto load_step = [&](int key0, u32x4 (&st)[2][2], float& scale) __attribute__((always_inline)) {
        const float* sp = nullptr;
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            rsrc_t r;
            uint32_t off;
            if constexpr (PAGED) {
                int rip = prip + 16 * kb;
                if (rip >= P) rip -= P;         // (block 1 starts the next page: its entry is pent[1])
                const int64_t page = (int64_t)min(pent[kb], (uint32_t)(p.num_blocks - 1));
                const int nvalid = min(max(n - (key0 + 16 * kb - rip), 0), P);          // visible rows of this page
                r = make_rsrc(kbase + page * p.k_batch, nvalid > 0 ? (uint32_t)(nvalid - 1) * row_b + ROWB : 0u);
                off = (uint32_t)(rip + n16) * row_b;
                if (g == kb && ksp != nullptr) sp = ksp + page * p.ks_batch + (int64_t)(rip + n16) * p.ks_row;
            } else {
                r = krs;
                off = (uint32_t)(key0 + 16 * kb + n16) * row_b;
                if (g == kb && ksp != nullptr) sp = ksp + (int64_t)bidx * p.ks_batch + (int64_t)(key0 + 16 * kb + n16) * p.ks_row;
            }
            st[kb][0] = buf_load16(r, off + colb);
            st[kb][1] = buf_load16(r, off + colb + 64u);
        });
        scale = 1.0f;
        if (sp != nullptr && key0 + lane < n) scale = *sp;         // (sp is null in lanes 32 .. 63 and without k_scale)
        if constexpr (PAGED) {
            advance_entries();
            fetch_entries();                    // the table entries of the step after this one
        }
    };

    float* lrow = p.logits + ((int64_t)bidx * p.lg_batch + (int64_t)t * p.lg_row);

    auto compute_step = [&](int key0, const u32x4 (&st)[2][2], float scale) __attribute__((always_inline)) {
        f32x4 acc[2][NHB];
        static_for<0, 2>([&](auto bb) {
            static_for<0, NHB>([&](auto hh) { acc[decltype(bb)::value][decltype(hh)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });
        });
        const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            acc[kb][0] = idx_mfma_e4m3(qf[0][0], qf[0][1], st[kb][0], st[kb][1], zero);
        });
        if (hb1) {
            static_for<0, 2>([&](auto bb) {
                constexpr int kb = decltype(bb)::value;
                acc[kb][1] = idx_mfma_e4m3(qf[1][0], qf[1][1], st[kb][0], st[kb][1], zero);
            });
        }
        if (hb2) {
            static_for<0, 2>([&](auto bb) {
                constexpr int kb = decltype(bb)::value;
                acc[kb][2] = idx_mfma_e4m3(qf[2][0], qf[2][1], st[kb][0], st[kb][1], zero);
                acc[kb][3] = idx_mfma_e4m3(qf[3][0], qf[3][1], st[kb][0], st[kb][1], zero);
            });
        }
        // ReLU, weights, head sum: inside the lane, then across the four lane groups
        float tot[2];
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            float s = 0.f;
            static_for<0, NHB>([&](auto hh) {
                constexpr int hb = decltype(hh)::value;
                static_for<0, 4>([&](auto rr) {
                    constexpr int r = decltype(rr)::value;
                    s = __builtin_fmaf(w[hb][r], idxp_relu(acc[kb][hb][r]), s);
                });
            });
            tot[kb] = sum_four_groups(s);
        });
        const int key = key0 + lane;            // lanes 0 .. 31: group g holds block g's keys
        if (lane < kIdxStep && key < n) lrow[key] = scale * (g == 0 ? tot[0] : tot[1]);
    };

    // ---- the wave's steps, the next one's loads in flight -------------------------------------------------------------------------------------
    if constexpr (PAGED) {
        pcol = k_begin / P;
        prip = k_begin - pcol * P;
        fetch_entries();
    }
    u32x4 sa[2][2], sb[2][2];
    float ca, cb;
    load_step(k_begin, sa, ca);
    for (int key = k_begin; key < k_end; key += 2 * kIdxStep) {
        load_step(key + kIdxStep, sb, cb);      // (past k_end: the descriptors end at n, the loads return zeros and nothing is stored)
        compute_step(key, sa, ca);
        if (key + kIdxStep >= k_end) break;
        load_step(key + 2 * kIdxStep, sa, ca);
        compute_step(key + kIdxStep, sb, cb);
    }
}

}  // namespace

hipError_t launch_mla_indexer_logits_fp8q(MlaIndexerParams p, hipStream_t s) {
    if (!p.cache_fp8) return hipErrorInvalidValue;
    const int64_t grid = mla_indexer_logits_shape(p);      // the rule of launch_mla_indexer_logits
    if (grid == 0) return hipErrorInvalidValue;
    void (*k)(const MlaIndexerParams) = p.block_table != nullptr ? fa_mla_indexer_fp8q_logits_kernel<true> : fa_mla_indexer_fp8q_logits_kernel<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kIdxThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fa
