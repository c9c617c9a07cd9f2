// fa_mla_indexer_prefill.hip — the index logits of the DeepSeek-V3.2 indexer for a prompt chunk (fa_run_mla_indexer_prefill_logits): the arithmetic of
// fa_mla_indexer.hip with a step's keys staged once per workgroup and used by several tokens.
//
//   fa_mla_indexer.hip gives a workgroup one token; its waves read their keys straight from memory, which is right when every key is used once.  A chunk of
//   sq tokens loads and widens the visible cache sq times that way.  Here a workgroup of four waves serves a TILE of kIdxpTQ consecutive tokens of one
//   sequence (FA_IDXP_TQ: 4 = one token a wave, 8 = two) and one range of wg_keys keys, and all four waves walk the SAME 32-key steps:
//   * Staging.  The 32 key rows of a step are loaded once per workgroup through registers - 4 KB of e4m3 codes is one 16-byte load a lane (lane of thread
//     tid: row tid / 8, bytes 16 (tid % 8) ..), a 16-bit cache two (row 16 j + tid / 16, slot tid % 16) - widened where the image is written (idx_widen8, exact)
//     and stored as 32 rows x 256 B in the swizzled layout of lds_tile_off<128>.  Two stages (16 KB), the step protocol of fa_kvcache_stage.hpp: one barrier a
//     step, the loads of step n + 1 in flight while step n computes.
//   * Arithmetic per (token, key): that of fa_mla_indexer.hip, operand for operand.  Q is the A operand of v_mfma_f32_16x16x32 and stays in registers (64 a
//     token); a lane's key fragment of chunk c is the 8 elements at column 16 (g + 4 (c >> 1)) + 8 (c & 1) of key lane & 15 - slot 2 g + 8 (c >> 1) + (c & 1) of
//     the image row, read with ds_read_b128 (16 rows distinct mod 16 at one slot: no bank conflict) - the chunks are accumulated in order 0 .. 3 per head block,
//     then ReLU, the 16 fused multiply-adds in head-block / register order, sum_four_groups and * k_scale.  The same operands in the same lanes in the same
//     order: the same bits as the decode call - except that the ReLU here keeps a NaN (idxp_relu), so a NaN key reaches its column as a NaN.  With two tokens a wave every fragment read from LDS feeds two MFMAs.
//   * Key range.  A tile reads keys [chunk * wg_keys, min(.. + wg_keys, n_last)), n_last = the keys its last token sees (causal) or L.  The contiguous
//     descriptor ends at row n_last; a paged 16-key block lies in one page and gets a descriptor over the visible rows of its page, its table entry a scalar
//     fetched one step ahead and clamped to the pool.  A workgroup whose range starts at or past n_last returns before any barrier: the condition is made of
//     scalars (block index, lengths, parameters) and is the same in every wave; behind it no wave leaves before the last barrier.
//   * Tokens of the tile at or past sq: a wave whose first token is one is inactive - it stages and meets every barrier and computes nothing; the second
//     token of an active wave then holds zeros for Q, sees n_t = 0 keys and stores nothing.
//   * Stores.  Lanes 0 .. 31 of a wave store the step's 32 logits of each of its tokens (128 contiguous bytes) under j < n_t; k_scale is loaded by those
//     lanes, one step ahead, under j < the largest n_t of the wave's tokens.  Row offsets of `logits` are 64-bit.
//   * Grid: b x ceil(sq / kIdxpTQ) x n_chunks, the chunk fastest.  wg_keys (mla_indexer_prefill_shape) is a multiple of 32 sized so that a launch with few
//     tiles still brings two workgroups a compute unit, at least kIdxpMinWgKeys and at most kIdxMaxWgKeys.
//   Kernels of this file: 8 ((fp16, bf16) x (16-bit, e4m3 cache) x (contiguous, paged)).
#include "fa_kvcache_stage.hpp"
#include "fa_mla_indexer.hpp"

namespace fa {

namespace {

static_assert(kIdxpTQ == 4 || kIdxpTQ == 8, "a wave serves one or two tokens");
static_assert(kIdxStep == kKvcStep && kIdxMaxWgKeys % kKvcStep == 0 && kIdxpMinWgKeys % kKvcStep == 0, "the steps of kvc_stage_step");
constexpr int kIdxpNT = kIdxpTQ / kIdxWaves;        // tokens of a wave
constexpr int kIdxpImage = kKvcStep * kIdxD * 2;    // 32 rows x 256 B

// ES = bytes per cache element: 2 = T, 1 = e4m3 codes
template <typename T, int ES, bool PAGED>
__global__ __launch_bounds__(kIdxThreads, 2) void fa_mla_indexer_prefill_logits_kernel(const MlaIndexerParams p) {
    constexpr int NT = kIdxpNT;
    constexpr int NHB = 4;                      // head blocks of 16 (h = 64)
    constexpr int NC = kIdxD / 32;              // 16x16x32 MFMAs per tile
    constexpr int NL = ES == 1 ? 1 : 2;         // 16-byte loads per lane and step
    constexpr int ROWB = kIdxD * ES;            // bytes of a key
    __shared__ __attribute__((aligned(16))) char smem[2 * kIdxpImage];

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

    // ---- this wave's tokens: Q in the permuted column order, the weights of the heads this lane sums, the keys each sees ------------------------
    const int h = p.h;
    const int tw0 = t0 + wave * NT;
    const bool active = tw0 < p.seqlen_q;       // (wave-uniform) false: staging and barriers only
    u32x4 qf[NT][NHB][NC];
    float w[NT][NHB][4];
    int n[NT];
    float* lrow[NT];
    static_for<0, NT>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        const int t = tw0 + i;
        const bool ok = t < p.seqlen_q;         // (wave-uniform)
        n[i] = ok ? idx_visible(L, p.seqlen_q, t, p.is_causal) : 0;
        lrow[i] = p.logits + ((int64_t)bidx * p.lg_batch + (int64_t)t * p.lg_row);
        const char* qtok = (const char*)p.q_ptr + 2 * ((int64_t)bidx * p.q_batch + (int64_t)t * p.q_row);
        const float* wtok = p.w_ptr + ((int64_t)bidx * p.w_batch + (int64_t)t * p.w_row);
        static_for<0, NHB>([&](auto hh) {
            constexpr int hb = decltype(hh)::value;
            const int head = 16 * hb + n16;
            static_for<0, NC>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                const int col = 16 * (g + 4 * (c >> 1)) + 8 * (c & 1);
                qf[i][hb][c] = ok && head < h ? *(const u32x4*)(qtok + 2 * ((int64_t)head * p.q_head + col)) : u32x4{0u, 0u, 0u, 0u};
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
    // staging: the rows and bytes of a step this lane moves.  FP8: row tid / 8 (block wave / 2, wave-uniform), codes 16 (tid % 8) .. + 15 = slots 2 (tid % 8)
    // and + 1 of the image row.  16-bit: load j is row tid / 16 of block j, slot tid % 16.
    const int srow = ES == 1 ? (tid >> 3) & 15 : tid >> 4;      // row within the 16-key block
    const int sblk = __builtin_amdgcn_readfirstlane(wave >> 1); // FP8: the block of this wave's rows
    const int sslot = ES == 1 ? 2 * (tid & 7) : tid & 15;       // 16-byte slot of the image row (FP8: the first of two)
    const uint32_t scolb = ES == 1 ? 16u * (tid & 7) : 16u * (tid & 15);
    const float* ksp = p.k_scale;

    // the loads of the step at key0: the lane's part of the 32 rows, and the scale of the key this lane stores (lanes 0 .. 31: key0 + lane)
    auto load_step = [&](int key0, u32x4 (&st)[NL], float& scale) __attribute__((always_inline)) {
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
                off[kb] = (uint32_t)(rip + srow) * row_b + scolb;
                if (g == kb && ksp != nullptr) sp = ksp + page * p.ks_batch + (int64_t)(rip + n16) * p.ks_row;
            } else {
                r[kb] = krs;
                off[kb] = (uint32_t)(key0 + 16 * kb + srow) * row_b + scolb;
                if (g == kb && ksp != nullptr) sp = ksp + (int64_t)bidx * p.ks_batch + (int64_t)(key0 + 16 * kb + n16) * p.ks_row;
            }
        });
        if constexpr (ES == 1) {
            st[0] = sblk == 0 ? buf_load16(r[0], off[0]) : buf_load16(r[1], off[1]);
        } else {
            st[0] = buf_load16(r[0], off[0]);
            st[1] = buf_load16(r[1], off[1]);
        }
        scale = 1.0f;
        if (sp != nullptr && key0 + lane < n_hi) scale = *sp;      // (sp is null in lanes 32 .. 63 and without k_scale)
        if constexpr (PAGED) {
            advance_entries();
            fetch_entries();                    // the table entries of the step after this one
        }
    };

    // the image of the step in stage BUF, widened where it is written
    auto store_step = [&](auto bufc, const u32x4 (&st)[NL]) __attribute__((always_inline)) {
        FA_LDS char* img = (FA_LDS char*)smem + decltype(bufc)::value * kIdxpImage;
        if constexpr (ES == 1) {
            const uint32_t row = (uint32_t)(16 * sblk + srow);
            *(FA_LDS u32x4*)(img + lds_tile_off<kIdxD>(row, (uint32_t)sslot)) = idx_widen8<T>(st[0].x, st[0].y);
            *(FA_LDS u32x4*)(img + lds_tile_off<kIdxD>(row, (uint32_t)sslot + 1u)) = idx_widen8<T>(st[0].z, st[0].w);
        } else {
            *(FA_LDS u32x4*)(img + lds_tile_off<kIdxD>((uint32_t)srow, (uint32_t)sslot)) = st[0];
            *(FA_LDS u32x4*)(img + lds_tile_off<kIdxD>((uint32_t)(16 + srow), (uint32_t)sslot)) = st[1];
        }
    };

    // one 32-key step of this wave's tokens over the image of stage BUF: every key fragment is read once and serves the wave's NT tokens
    auto compute_step = [&](auto bufc, int key0, float scale) __attribute__((always_inline)) {
        const FA_LDS char* img = (const FA_LDS char*)smem + decltype(bufc)::value * kIdxpImage;
        float tot[NT][2];
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            u32x4 kf[NC];
            static_for<0, NC>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                kf[c] = *(const FA_LDS u32x4*)(img + lds_tile_off<kIdxD>((uint32_t)(16 * kb + n16), (uint32_t)(2 * g + 8 * (c >> 1) + (c & 1))));
            });
            f32x4 acc[NT][NHB];
            static_for<0, NT>([&](auto ii) {
                static_for<0, NHB>([&](auto hh) { acc[decltype(ii)::value][decltype(hh)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });
            });
            // the head blocks that exist, in ONE basic block for each head count: NT x head blocks independent accumulators between two MFMAs of the same
            // one, where a branch per head block (the form of fa_mla_indexer.hip) leaves NT.  Per accumulator the chunks still come in order 0 .. 3.  (Measured
            // level with the branch-per-block form, DESIGN.md 3.21: the step is bound by its MFMAs and the ReLU / weight epilogue together.)
            auto head_blocks = [&](auto nn) __attribute__((always_inline)) {
                static_for<0, NC>([&](auto cc) {
                    constexpr int c = decltype(cc)::value;
                    static_for<0, decltype(nn)::value>([&](auto hh) {
                        constexpr int hb = decltype(hh)::value;
                        static_for<0, NT>([&](auto ii) {
                            constexpr int i = decltype(ii)::value;
                            acc[i][hb] = LP<T>::mfma16(qf[i][hb][c], kf[c], acc[i][hb]);
                        });
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
    // operand of MFMAs: what comes out of it are logits, which reach a maximum, fused multiply-adds and stores of VALUES - every address (lds_tile_off of
    // lane constants, the logits row of the wave's token, key0 + lane under key < n_t, table columns and pages from the block table), every index and every
    // loop bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[NL];
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

// wg_keys: two workgroups per compute unit over b x tiles, in multiples of one step, between kIdxpMinWgKeys and kIdxMaxWgKeys
void mla_indexer_prefill_shape(MlaIndexerParams& p) {
    const int64_t tiles = (int64_t)p.b * ((p.seqlen_q + kIdxpTQ - 1) / kIdxpTQ), target = 2 * device_cu_count();
    int64_t wg = ((int64_t)p.seqlen_cache * (tiles > 0 ? tiles : 1) + target - 1) / target;
    wg = (wg + kKvcStep - 1) / kKvcStep * kKvcStep;
    wg = wg < kIdxpMinWgKeys ? kIdxpMinWgKeys : (wg > kIdxMaxWgKeys ? kIdxMaxWgKeys : wg);
    p.wg_keys = (int)wg;
    p.n_chunks = (int)((p.seqlen_cache + wg - 1) / wg);
    if (p.n_chunks < 1) p.n_chunks = 1;
}

hipError_t launch_mla_indexer_prefill_logits(MlaIndexerParams p, int dtype, hipStream_t s) {
    if (p.h != 16 && p.h != 32 && p.h != 64) return hipErrorInvalidValue;
    mla_indexer_prefill_shape(p);
    const int64_t grid = (int64_t)p.b * ((p.seqlen_q + kIdxpTQ - 1) / kIdxpTQ) * p.n_chunks;
    if (grid <= 0 || grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const bool paged = p.block_table != nullptr;
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        void (*k)(const MlaIndexerParams);
        if (p.cache_fp8) k = paged ? fa_mla_indexer_prefill_logits_kernel<T, 1, true> : fa_mla_indexer_prefill_logits_kernel<T, 1, false>;
        else k = paged ? fa_mla_indexer_prefill_logits_kernel<T, 2, true> : fa_mla_indexer_prefill_logits_kernel<T, 2, false>;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kIdxThreads), 0, s, p);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
