// fa_fwd_mla_prefill.hip — MLA prefill attention (fa_run_mla_prefill_fwd): 192-wide queries and keys, 128-wide values, dense and packed.
//
//   Before weight absorption an MLA layer (DeepSeek-V2 / V3 / R1, Kimi K2) is ordinary multi-head attention whose keys are 192 wide (128 no-rope
//   columns, then 64 rope columns) and whose values are 128 wide.  The body is the 64-row, LDS-staged body of fa_fwd_kvcache_prefill.hip
//   (kvcache_prefill_attn) with the following kept as they are: four waves, 16-row query column blocks (packed row r = t * (h / h_k) + j) in which a
//   lane owns one query row with private m / l; S^T = K Q^T on v_mfma_f32_16x16x32 with Q^T in registers; 32-key steps walked by all four waves together;
//   the K and V rows of a step loaded once per workgroup through registers into two LDS stages, one barrier per step; O^T += V^T P^T with V^T by
//   ds_read_b64_tr_b16; the causal k_hi per tile; a wave past the rows takes part in staging and barriers only.  What changes:
//   * K image: a 384-byte K row is no multiple of the 256-byte bank row lds_tile_off argues about (the case fa_device.hpp describes for the
//     1152-byte latent row), so a stage holds columns 0 .. 127 of K (32 rows x 256 B, lds_tile_off<128>), columns 128 .. 191 (32 rows x 128 B,
//     lds_tile_off<64>) and V (32 rows x 256 B, lds_tile_off<128>): 20 KB a stage, 40 KB for both.
//   * S^T takes six chunks per 16 keys (four from the wide K image, two from the narrow one), O^T has eight blocks of 16 columns.
//   * Staging: five 16-byte loads per lane and step.  A wave-wide load covers 4 rows x 16 slots of a wide image or 8 rows x 8 slots of the narrow
//     one; wave w takes rows 4 w .. 4 w + 3 and 16 + 4 w .. 16 + 4 w + 3 of the wide images and rows 8 w .. 8 w + 7 of the narrow one.
//   * Addressing: K / V are plain strided tensors; packed, sequence i starts at row cu_k[i] and is sk_i long.  No pages, no table, no append, no
//     key split (so no workspace and no combine).  The descriptors end at the sequence's last row: rows at or past it read as zeros and their
//     scores are masked.
//   * Packed grid: ceil(total_q * (h / h_k) / rows) + b tile slots per KV head, found through kvc_slot_lookup as in the ragged prefill kernels;
//     every sequence is tiled on its own from its first row.  Dense grid: b x h_k x tiles.
//   * A wave owns TWO query column blocks (FA_MLAP_WAVE_ROWS = 32), a workgroup 128 rows: every K / V^T fragment read from LDS feeds two MFMAs, which
//     halves the LDS reads per MFMA.  The body is light enough for it - by count 48 registers of Q^T, 64 of O^T and 20 of staging a lane.
//     FA_MLAP_WAVE_ROWS = 16 builds the 64-row workgroup of the sibling files (the A/B of DESIGN.md 3.17: the 128-row form measured faster).
//   Kernels of this file: 8 attention ((fp16, bf16) x (causal, not) x (dense, packed)).
#include "fa_mla_prefill_tile.hpp"

#ifndef FA_MLAP_WAVE_ROWS
#define FA_MLAP_WAVE_ROWS 32
#endif

namespace fa {

namespace {

static_assert(FA_MLAP_WAVE_ROWS == 16 || FA_MLAP_WAVE_ROWS == 32, "a wave owns one or two 16-row query column blocks");
constexpr int kMpQB = FA_MLAP_WAVE_ROWS / kKvcRows;         // query column blocks of a wave
constexpr int kMpRows = kKvcWaves * FA_MLAP_WAVE_ROWS;      // packed query rows of a workgroup

template <typename T, bool CAUSAL, bool PACKED>
FA_DEV void mla_prefill_attn(const MlaPrefillParams& p) {
    using Lds = MlapLds<>;              // K | K rope | V: 20 KB a stage, 40 KB
    constexpr int NC = kMlapNC;         // 16x16x32 MFMAs per 16 keys of S^T
    constexpr int NO = kMlapDV / 16;    // O^T blocks of 16 columns
    constexpr int QB = kMpQB;
    __shared__ __attribute__((aligned(16))) char smem[Lds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    MlapSeq<PACKED> seq;
    if (!seq.template find_tile<kMpRows, false>(p)) return;
    seq.read_bounds(p);
    if (PACKED && ((int)seq.q0 < 0 || seq.q0 + seq.sq > p.total_q)) return;     // rows outside q / o: not served
    seq.template cut<false>(p);
    const int tile = seq.tile, kvh = seq.kvh, sq = seq.sq, L = seq.L;
    const int rows_tile = sq * p.h_ratio;
    const int k_end = seq.template tile_key_end<kMpRows, CAUSAL>(p.h_ratio);
    const float c = p.scale_log2e;
    const float sc = p.scale;

    // ---- this lane's query rows (one per column block): Q^T fragments for the whole call, visible-key limit ---------------------------------
    const int wrow0 = tile * kMpRows + wave * FA_MLAP_WAVE_ROWS;
    const bool active = wrow0 < rows_tile;      // (wave-uniform) false: staging and barriers only
    bool row_ok[QB];
    int t[QB], hq[QB], lim[QB];
    u32x4 qf[QB][NC];
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        const int pr = wrow0 + kKvcRows * qb + n16;
        row_ok[qb] = pr < rows_tile;
        t[qb] = row_ok[qb] ? pr / p.h_ratio : 0;
        hq[qb] = kvh * p.h_ratio + (row_ok[qb] ? pr - t[qb] * p.h_ratio : 0);
        lim[qb] = row_ok[qb] ? L : 0;
        if (CAUSAL && row_ok[qb]) lim[qb] = min(L, L - sq + t[qb] + 1);
        const char* qrow = (const char*)p.q_ptr + 2 * seq.row_off(p.q, hq[qb], t[qb]);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            qf[qb][ci] = row_ok[qb] ? *(const u32x4*)(qrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    });

    // ---- staging: the K and V rows of a step (fa_mla_prefill_tile.hpp) ----------------------------------------------------------------------------
    const MlapLane ln(wave, lane);
    const MlapKvRows kv(p, seq);
    auto load_step = [&](int key0, u32x4 (&st)[kMlapNL]) __attribute__((always_inline)) { kv.load_step(ln, key0, st); };
    auto store_step = [&](auto bufc, const u32x4 (&st)[kMlapNL]) __attribute__((always_inline)) {
        mlap_store_step(mlap_images<Lds, decltype(bufc)::value>(smem), ln, st, [](auto) {});
    };

    // transposed-read addresses of this lane (fa_device.hpp lds_tile_off image): block c, half hh -> rows hh * 16 + 4 g + q, columns 16 c + 4 p
    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 oacc[QB][NO];
    float m_run[QB], l_run[QB];
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        static_for<0, NO>([&](auto cc) {
            oacc[qb][decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+v"(oacc[qb][decltype(cc)::value]));
        });
        m_run[qb] = kNegBig;
        l_run[qb] = 0.f;
    });

    // one 32-key step of this wave's rows over the images of stage BUF: every K and V^T fragment is read once and serves the wave's QB column blocks
    auto compute_step = [&](auto bufc, int key0) __attribute__((always_inline)) {
        const MlapImages im = mlap_images<Lds, decltype(bufc)::value>(smem);
        f32x4 s[QB][2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, QB>([&](auto qq) { s[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f}; });
            mlap_scores<T, b>(im, n16, g, qf, s);
        });
        u32x4 pf[QB];
        static_for<0, QB>([&](auto qq) {
            constexpr int qb = decltype(qq)::value;
            float mx = -INFINITY;
            static_for<0, 2>([&](auto kb) {
                constexpr int b = decltype(kb)::value;
                static_for<0, 4>([&](auto rr) {
                    constexpr int r = decltype(rr)::value;
                    const int key = key0 + 16 * b + 4 * g + r;
                    s[qb][b][r] = key < lim[qb] ? s[qb][b][r] : -INFINITY;
                    mx = fmaxf(mx, s[qb][b][r]);
                });
            });
            mx = max_four_groups(mx);
            const float m_new = fmaxf(m_run[qb], mx);
            const float alpha = fast_exp2((m_run[qb] - m_new) * c);
            m_run[qb] = m_new;
            const float mc = m_new * c;
            float pe[8];
            float ps = 0.f;
            static_for<0, 8>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                pe[j] = fast_exp2(__builtin_fmaf(s[qb][j >> 2][j & 3], c, -mc));
                ps += pe[j];
            });
            l_run[qb] = l_run[qb] * alpha + ps;
            pf[qb] = pack8<T>(pe);
            static_for<0, NO>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                oacc[qb][ci] *= alpha;
            });
        });
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const u32x4 vt = tr_frag<kMlapDV>(im.vimg, ci, g, q4, p4);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                oacc[qb][ci] = LP<T>::mfma16(vt, pf[qb], oacc[qb][ci]);
            });
        });
    };

    // ---- the 32-key steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp) ---------------------------------------
    // k_end is the workgroup's: every wave meets the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the three images are read by compute_step alone,
    // as MFMA operands (mlap_scores, tr_frag): what comes out of them are scores and O, which reach compares, exponentials and stores of VALUES - every
    // address (lds_tile_off of lane constants, row_off / row_index of the lane's row, the sequence's base rows from cu_seqlens), every index and every loop
    // bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[kMlapNL];
        int key = 0;
        if (key < k_end) {
            load_step(key, st);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st);
        }
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(key + kKvcStep, st);
        auto load = [&](auto, int key0) __attribute__((always_inline)) { load_step(key0, st); };
        auto store = [&](auto bufc) __attribute__((always_inline)) { store_step(bufc, st); };
        auto compute = [&](auto bufc, int key0) __attribute__((always_inline)) { compute_step(bufc, key0); };
        for (; key < k_end; key += 2 * kKvcStep) {
            kvc_stage_step(std::integral_constant<int, 0>{}, key, 0, k_end, wave, active, load, store, compute);
            if (key + kKvcStep < k_end) kvc_stage_step(std::integral_constant<int, 1>{}, key + kKvcStep, 0, k_end, wave, active, load, store, compute);
        }
    }

    // ---- epilogue: the lane's rows, columns 16 c + 4 g .. + 3 of every block c -------------------------------------------------------------------
    if (!active) return;
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        const float lsum = sum_four_groups(l_run[qb]);
        if (!row_ok[qb]) return;
        // dead = saw no key (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math
        const bool live = !(lsum == 0.f);
        const float inv = live ? 1.0f / lsum : 0.f;
        const float lse = live ? m_run[qb] * sc + logf(lsum) : 0.f;
        char* orow = (char*)p.o_ptr + 2 * (seq.row_off(p.o, hq[qb], t[qb]) + 4 * g);
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            mlap_store_block<T>(orow, ci, oacc[qb][ci], inv);
        });
        if (g == 0) p.lse_ptr[seq.row_index(p, hq[qb], t[qb])] = lse;
    });
}

// Two workgroups per compute unit: by count a lane holds 24 registers of Q^T and 32 of O^T per column block and 20 of staging next to the softmax
// (243 VGPRs with two column blocks, 122 - 146 with one; no AGPRs, no scratch), and 40 KB of LDS a workgroup leaves room for more than two.
template <typename T, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_mla_prefill_kernel(const MlaPrefillParams p) {
    mla_prefill_attn<T, CAUSAL, PACKED>(p);
}

}  // namespace

// p as the C ABI filled it; the tiles (dense) or tile slots (packed) are counted here.  grid = b x h_k x tiles (dense), slots x h_k (packed)
hipError_t launch_fwd_mla_prefill(MlaPrefillParams p, int dtype, hipStream_t s) {
    const bool packed = p.cu_q != nullptr;
    const int64_t rows = packed ? p.total_q : p.seqlen_q;
    if (p.b <= 0 || rows <= 0) return hipSuccess;
    const int64_t tiles = (rows * p.h_ratio + kMpRows - 1) / kMpRows;
    const int64_t per_head = packed ? tiles + p.b : tiles * p.b;
    const int64_t grid = per_head * p.h_k;
    if (grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (packed) p.slots = (int32_t)per_head;
    else p.n_row_tiles = (int32_t)tiles;
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        auto* kernel = mlap_select(p.is_causal, packed, [](auto c, auto k) { return fa_fwd_mla_prefill_kernel<T, decltype(c)::value, decltype(k)::value>; });
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kKvcThreads), 0, s, p);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
