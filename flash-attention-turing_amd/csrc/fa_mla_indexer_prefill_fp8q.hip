// fa_mla_indexer_prefill_fp8q.hip — the index logits of fa_run_mla_indexer_prefill_logits for FP8 (e4m3) index queries over an FP8 index-key cache
// (fa_mla_indexer_params_v2, q_format = FA_IDX_Q_FP8_E4M3): DeepGEMM's fp8_mqa_logits, e4m3 on both sides of the product.
//
//   The tile of fa_mla_indexer_prefill.hip - a workgroup of four waves serves kIdxpTQ consecutive tokens of one sequence and one range of wg_keys keys, all
//   four waves walk the same 32-key steps under the step protocol of fa_kvcache_stage.hpp - with the arithmetic of fa_mla_indexer_fp8q.hip:
//   * Staging.  The 32 key rows of a step are 4 KB of codes: one 16-byte load a lane (thread tid: row tid / 8, bytes 16 (tid % 8) ..), stored as they are -
//     nothing is widened - as 32 rows x 128 B.  Two stages, 8 KB.
//   * LDS layout.  The rule (ds_read_b128): the bank of byte address a is (a / 4) % 64 - a 256-byte bank row, sixteen 16-byte bank slots - and a wave's
//     read is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; only lanes of one group conflict.  A read is
//     conflict-free when the 16 lanes of every group fall into 16 different bank slots.  A fragment read of this kernel: lane l = 16 g + n16 reads slot
//     g (+ 4 for the second read) of row 16 kb + n16, so a group holds all 16 rows, eight of them at slot s (rows R) and eight at slot s ^ 1 (rows R'), where
//     {row >> 1 : R} = {0, 1, 6, 7} and {row >> 1 : R'} = {2, 3, 4, 5} or the other way round.  Two 128-byte rows share a bank row, so the bank slot of
//     (row, physical slot ps) is 8 (row & 1) + ps.  The layout: ps = slot ^ ((row >> 1) & 7), byte offset 128 row + 16 ps (idxq_tile_off).  Both row sets are
//     closed under x -> x ^ 1 in (row >> 1), so s ^ 1 ^ {2, 3, 4, 5} = s ^ {2, 3, 4, 5} and the eight (row >> 1) values of a group give eight different ps;
//     the row parity supplies the sixteenth part: 16 different bank slots, no conflict.  The staging store (ds_write_b128, banks (a / 4) % 32, groups of 8
//     consecutive lanes) writes the eight slots of one row from one group: 128 contiguous bytes in a permuted order, every bank once.
//   * Arithmetic per (token, key): that of fa_mla_indexer_fp8q.hip, operand for operand - Q the A operand of v_mfma_f32_16x16x128_f8f6f4 (32 registers a token),
//     the key fragment bytes 16 g .. and 64 + 16 g .. of key lane & 15, ONE MFMA per (token, 16 keys, 16 heads), idxp_relu, the 16 fused multiply-adds in
//     head-block / register order, sum_four_groups, * k_scale.  The same operands in the same lanes: the same bits as the decode call, NaN included.  A wave reads
//     two 16-byte fragments per 16-key block and feeds the MFMAs of its kIdxpNT tokens from them.
//   * Key range, inactive waves, tokens past sq, stores, k_scale, the grid and wg_keys (mla_indexer_prefill_shape): as in fa_mla_indexer_prefill.hip.
//   Kernels of this file: 2 (contiguous, paged).
#include "fa_kvcache_stage.hpp"
#include "fa_mla_indexer.hpp"

namespace fa {

namespace {

static_assert(kIdxpTQ == 4 || kIdxpTQ == 8, "a wave serves one or two tokens");
static_assert(kIdxStep == kKvcStep && kIdxMaxWgKeys % kKvcStep == 0 && kIdxpMinWgKeys % kKvcStep == 0, "the steps of kvc_stage_step");
constexpr int kIdxpNT = kIdxpTQ / kIdxWaves;        // tokens of a wave
constexpr int kIdxqImage = kKvcStep * kIdxD;        // 32 rows x 128 B

// byte offset of 16-byte slot `slot` (0 .. 7) of row `row` in a stage image: the layout derived in the file header
FA_DEV uint32_t idxq_tile_off(uint32_t row, uint32_t slot) { return row * (uint32_t)kIdxD + ((slot ^ ((row >> 1) & 7u)) << 4); }

template <bool PAGED>
__global__ __launch_bounds__(kIdxThreads, 2) void fa_mla_indexer_prefill_fp8q_logits_kernel(const MlaIndexerParams p) {
    constexpr int NT = kIdxpNT;
    constexpr int NHB = 4;                      // head blocks of 16 (h = 64)
    constexpr int ROWB = kIdxD;                 // bytes of a key and of a head of Q
    __shared__ __attribute__((aligned(16))) char smem[2 * kIdxqImage];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t id = blockIdx.x;
    const int n_tiles = (p.seqlen_q + kIdxpTQ - 1) / kIdxpTQ;
    const int chunk = (int)(id % (uint32_t)p.n_chunks);
    const int tix = (int)(id / (uint32_t)p.n_chunks);
    const int tile = tix % n_tiles, bidx = tix / n_tiles;
    const int L = idx_len(p.cache_seqlens, bidx, p.seqlen_cache);
    const int t0 = tile * kIdxpTQ;
    const int n_last = __builtin_amdgcn_readfirstlane(idx_visible(L, p.seqlen_q, min(t0 + kIdxpTQ, p.seqlen_q) - 1, p.is_causal));
    // the workgroup's keys, cut at n_last.  (Scalars, the same in every wave: the workgroup leaves here or not at all.)
    const int64_t kb64 = (int64_t)chunk * p.wg_keys;
    if (kb64 >= n_last) return;
    const int k_begin = (int)kb64;
    const int k_end = min(k_begin + p.wg_keys, n_last);

    // ---- this wave's tokens: Q (codes; strides in bytes), the weights of the heads this lane sums, the keys each sees ------------------------------
    const int h = p.h;
    const int tw0 = t0 + wave * NT;
    const bool active = tw0 < p.seqlen_q;       // (wave-uniform) false: staging and barriers only
    const uint32_t colb = (uint32_t)(16 * g);   // byte offset of this lane group's first 16 bytes in a row; the second 16: 64 further on
    u32x4 qf[NT][NHB][2];
    float w[NT][NHB][4];
    int n[NT];
    float* lrow[NT];
    static_for<0, NT>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        const int t = tw0 + i;
        const bool ok = t < p.seqlen_q;         // (wave-uniform)
        n[i] = ok ? idx_visible(L, p.seqlen_q, t, p.is_causal) : 0;
        lrow[i] = p.logits + ((int64_t)bidx * p.lg_batch + (int64_t)t * p.lg_row);
        const char* qtok = (const char*)p.q_ptr + ((int64_t)bidx * p.q_batch + (int64_t)t * p.q_row);
        const float* wtok = p.w_ptr + ((int64_t)bidx * p.w_batch + (int64_t)t * p.w_row);
        static_for<0, NHB>([&](auto hh) {
            constexpr int hb = decltype(hh)::value;
            const int head = 16 * hb + n16;
            static_for<0, 2>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                qf[i][hb][j] = ok && head < h ? *(const u32x4*)(qtok + ((int64_t)head * p.q_head + colb + 64 * j)) : u32x4{0u, 0u, 0u, 0u};
            });
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int hd = 16 * hb + 4 * g + r;
                w[i][hb][r] = ok && hd < h ? wtok[(int64_t)hd * p.w_head] : 0.f;
            });
        });
    });
    const int n_hi = n[NT - 1] > n[0] ? n[NT - 1] : n[0];         // the keys the wave's tokens see between them (n_t does not fall with t)
    const bool hb1 = h > 16, hb2 = h > 32;      // (wave-uniform) head blocks 1 and 2 .. 3 exist

    // ---- key addressing -------------------------------------------------------------------------------------------------------------------
    const uint32_t row_b = (uint32_t)p.k_row;
    const char* kbase = uniform_ptr((const char*)p.k_cache + (PAGED ? (int64_t)0 : (int64_t)bidx * p.k_batch));
    const rsrc_t krs = make_rsrc(kbase, !PAGED ? (uint32_t)(n_last - 1) * row_b + ROWB : 0u);       // (n_last > k_begin >= 0)
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
            prip += kKvcStep;
            while (prip >= P) { prip -= P; pcol += 1; }
        }
    };
    // staging: row tid / 8 of the step (block wave / 2, wave-uniform; row (tid / 8) % 16 within it), codes 16 (tid % 8) .. + 15 = slot tid % 8 of the image row
    const int srow = (tid >> 3) & 15;
    const int sblk = __builtin_amdgcn_readfirstlane(wave >> 1);
    const uint32_t sslot = (uint32_t)(tid & 7);
    const float* ksp = p.k_scale;

    // the loads of the step at key0: the lane's 16 bytes of the 32 rows, and the scale of the key this lane stores (lanes 0 .. 31: key0 + lane)
    auto load_step = [&](int key0, u32x4& st, float& scale) __attribute__((always_inline)) {
        const float* sp = nullptr;
        rsrc_t r[2];
        uint32_t off[2];
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            if constexpr (PAGED) {
                int rip = prip + 16 * kb;
                if (rip >= P) rip -= P;         // (block 1 starts the next page: its entry is pent[1])
                const int64_t page = (int64_t)min(pent[kb], (uint32_t)(p.num_blocks - 1));
                const int nvalid = min(max(n_last - (key0 + 16 * kb - rip), 0), P);     // visible rows of this page
                r[kb] = make_rsrc(kbase + page * p.k_batch, nvalid > 0 ? (uint32_t)(nvalid - 1) * row_b + ROWB : 0u);
                off[kb] = (uint32_t)(rip + srow) * row_b + 16u * sslot;
                if (g == kb && ksp != nullptr) sp = ksp + page * p.ks_batch + (int64_t)(rip + n16) * p.ks_row;
            } else {
                r[kb] = krs;
                off[kb] = (uint32_t)(key0 + 16 * kb + srow) * row_b + 16u * sslot;
                if (g == kb && ksp != nullptr) sp = ksp + (int64_t)bidx * p.ks_batch + (int64_t)(key0 + 16 * kb + n16) * p.ks_row;
            }
        });
        st = sblk == 0 ? buf_load16(r[0], off[0]) : buf_load16(r[1], off[1]);
        scale = 1.0f;
        if (sp != nullptr && key0 + lane < n_hi) scale = *sp;      // (sp is null in lanes 32 .. 63 and without k_scale)
        if constexpr (PAGED) {
            advance_entries();
            fetch_entries();                    // the table entries of the step after this one
        }
    };

    // the image of the step in stage BUF: the codes as they were loaded
    auto store_step = [&](auto bufc, const u32x4& st) __attribute__((always_inline)) {
        FA_LDS char* img = (FA_LDS char*)smem + decltype(bufc)::value * kIdxqImage;
        *(FA_LDS u32x4*)(img + idxq_tile_off((uint32_t)(16 * sblk + srow), sslot)) = st;
    };

    // one 32-key step of this wave's tokens over the image of stage BUF: every key fragment is read once and serves the wave's NT tokens
    auto compute_step = [&](auto bufc, int key0, float scale) __attribute__((always_inline)) {
        const FA_LDS char* img = (const FA_LDS char*)smem + decltype(bufc)::value * kIdxqImage;
        float tot[NT][2];
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            const u32x4 klo = *(const FA_LDS u32x4*)(img + idxq_tile_off((uint32_t)(16 * kb + n16), (uint32_t)g));
            const u32x4 khi = *(const FA_LDS u32x4*)(img + idxq_tile_off((uint32_t)(16 * kb + n16), (uint32_t)(4 + g)));
            f32x4 acc[NT][NHB];
            static_for<0, NT>([&](auto ii) {
                static_for<0, NHB>([&](auto hh) { acc[decltype(ii)::value][decltype(hh)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });
            });
            // the head blocks that exist, in one basic block for each head count (the form of fa_mla_indexer_prefill.hip)
            auto head_blocks = [&](auto nn) __attribute__((always_inline)) {
                static_for<0, decltype(nn)::value>([&](auto hh) {
                    constexpr int hb = decltype(hh)::value;
                    static_for<0, NT>([&](auto ii) {
                        constexpr int i = decltype(ii)::value;
                        acc[i][hb] = idx_mfma_e4m3(qf[i][hb][0], qf[i][hb][1], klo, khi, acc[i][hb]);
                    });
                });
            };
            if (hb2) head_blocks(std::integral_constant<int, 4>{});
            else if (hb1) head_blocks(std::integral_constant<int, 2>{});
            else head_blocks(std::integral_constant<int, 1>{});
            // ReLU, weights, head sum: inside the lane, then across the four lane groups
            static_for<0, NT>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                float s = 0.f;
                static_for<0, NHB>([&](auto hh) {
                    constexpr int hb = decltype(hh)::value;
                    static_for<0, 4>([&](auto rr) {
                        constexpr int r = decltype(rr)::value;
                        s = __builtin_fmaf(w[i][hb][r], idxp_relu(acc[i][hb][r]), s);
                    });
                });
                tot[i][kb] = sum_four_groups(s);
            });
        });
        const int key = key0 + lane;            // lanes 0 .. 31: group g holds block g's keys
        static_for<0, NT>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            if (lane < kKvcStep && key < n[i]) lrow[i][key] = scale * (g == 0 ? tot[i][0] : tot[i][1]);
        });
    };

    // ---- the 32-key steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp) ---------------------------------------
    // k_begin and k_end are the workgroup's: every wave meets the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the image is read by compute_step alone, as the B
    // operand of MFMAs: what comes out of it are logits, which reach a maximum, fused multiply-adds and stores of VALUES - every address (idxq_tile_off of
    // lane constants, the logits row of the wave's token, key0 + lane under key < n_t, table columns and pages from the block table), every index and every
    // loop bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st;
        float sc0 = 1.0f, sc1 = 1.0f;           // k_scale of the step in stage 0 / stage 1
        if constexpr (PAGED) {
            pcol = k_begin / P;
            prip = k_begin - pcol * P;
            fetch_entries();
        }
        int key = k_begin;                      // (k_begin < k_end)
        load_step(key, st, sc0);
        kvc_stage_slow_writer(-1, wave);
        store_step(std::integral_constant<int, 0>{}, st);
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(key + kKvcStep, st, sc1);
        auto load = [&](auto bufc, int key0) __attribute__((always_inline)) {
            if constexpr (decltype(bufc)::value == 0) load_step(key0, st, sc0);
            else load_step(key0, st, sc1);
        };
        auto store = [&](auto bufc) __attribute__((always_inline)) { store_step(bufc, st); };
        auto compute = [&](auto bufc, int key0) __attribute__((always_inline)) { compute_step(bufc, key0, decltype(bufc)::value == 0 ? sc0 : sc1); };
        for (; key < k_end; key += 2 * kKvcStep) {
            kvc_stage_step(std::integral_constant<int, 0>{}, key, k_begin, k_end, wave, active, load, store, compute);
            if (key + kKvcStep < k_end) kvc_stage_step(std::integral_constant<int, 1>{}, key + kKvcStep, k_begin, k_end, wave, active, load, store, compute);
        }
    }
}

}  // namespace

hipError_t launch_mla_indexer_prefill_logits_fp8q(MlaIndexerParams p, hipStream_t s) {
    if ((p.h != 16 && p.h != 32 && p.h != 64) || !p.cache_fp8) return hipErrorInvalidValue;
    mla_indexer_prefill_shape(p);               // the tile and ranges rule of launch_mla_indexer_prefill_logits
    const int64_t grid = (int64_t)p.b * ((p.seqlen_q + kIdxpTQ - 1) / kIdxpTQ) * p.n_chunks;
    if (grid <= 0 || grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    void (*k)(const MlaIndexerParams) = p.block_table != nullptr ? fa_mla_indexer_prefill_fp8q_logits_kernel<true> : fa_mla_indexer_prefill_fp8q_logits_kernel<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kIdxThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fa
