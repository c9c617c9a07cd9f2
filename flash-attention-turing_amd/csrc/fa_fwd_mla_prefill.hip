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
#include "fa_kvcache_attn.hpp"
#include "fa_kvcache_stage_debug.hpp"

#ifndef FA_MLAP_WAVE_ROWS
#define FA_MLAP_WAVE_ROWS 32
#endif

namespace fa {

namespace {

static_assert(FA_MLAP_WAVE_ROWS == 16 || FA_MLAP_WAVE_ROWS == 32, "a wave owns one or two 16-row query column blocks");
constexpr int kMpQB = FA_MLAP_WAVE_ROWS / kKvcRows;         // query column blocks of a wave
constexpr int kMpRows = kKvcWaves * FA_MLAP_WAVE_ROWS;      // packed query rows of a workgroup
constexpr int kMpDN = 128;                  // the no-rope columns of K
constexpr int kMpDR = 64;                   // the rope columns of K
constexpr int kMpDK = kMpDN + kMpDR;
constexpr int kMpDV = 128;

struct MlapLds {
    static constexpr int kImageN = kKvcStep * kMpDN * 2;        // 32 rows x 256 B
    static constexpr int kImageR = kKvcStep * kMpDR * 2;        // 32 rows x 128 B
    static constexpr int kImageV = kKvcStep * kMpDV * 2;        // 32 rows x 256 B
    static constexpr int kStage = kImageN + kImageR + kImageV;  // 20 KB
    static constexpr int kBytes = 2 * kStage;                   // 40 KB
};

template <typename T, bool CAUSAL, bool PACKED>
FA_DEV void mla_prefill_attn(const MlaPrefillParams& p) {
    constexpr int NCN = kMpDN / 32;     // 16x16x32 MFMAs per 16 keys of S^T over the wide K image
    constexpr int NCR = kMpDR / 32;     // ... and over the narrow one
    constexpr int NC = NCN + NCR;
    constexpr int NO = kMpDV / 16;      // O^T blocks of 16 columns
    constexpr int QB = kMpQB;
    constexpr int NL = 5;               // loads per lane and step: two of the wide K image, one of the narrow one, two of V
    __shared__ __attribute__((aligned(16))) char smem[MlapLds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int n_tiles = PACKED ? p.slots : p.n_row_tiles;       // PACKED: the tile slots of a KV head, and `bh` below is the KV head
    int tile = id % n_tiles;
    const int bh = id / n_tiles;
    int bidx = bh / p.h_k, kvh = bh - bidx * p.h_k;
    int sq = p.seqlen_q, L = p.seqlen_k;        // query rows and keys of this sequence
    int64_t q0 = 0, k0 = 0;                     // PACKED: its first packed row of q / o and of k / v
    if constexpr (PACKED) {
        kvh = bh;
        const int slot = tile;
        if (!kvc_slot_lookup<kMpRows>(p.cu_q, p.b, p.h_ratio, (uint32_t)slot, bidx, tile)) return;     // a slack slot: nothing to write
        const int c0 = __builtin_amdgcn_readfirstlane(p.cu_q[bidx]);
        sq = __builtin_amdgcn_readfirstlane(p.cu_q[bidx + 1]) - c0;
        const int d0 = __builtin_amdgcn_readfirstlane(p.cu_k[bidx]);
        L = __builtin_amdgcn_readfirstlane(p.cu_k[bidx + 1]) - d0;
        q0 = c0;
        k0 = d0;
        // cu_seqlens that point outside the tensors (a broken precondition) never become an address: the sequence's rows are not served, and keys
        // are cut at the last row of k / v.  Every value here is the workgroup's, so all four waves leave together.
        if (c0 < 0 || q0 + sq > p.total_q) return;
        const int64_t k_left = p.total_k - k0;
        L = d0 < 0 || k_left < 0 ? 0 : (L > k_left ? (int)k_left : max(L, 0));
    }
    const int rows_tile = sq * p.h_ratio;
    // row (hq_, t_) of the LSE; element offset of its row in q / o (st = p.q or p.o)
    auto row_index = [&](int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (PACKED) return (int64_t)hq_ * p.total_q + q0 + t_;
        else return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t_;
    };
    auto row_off = [&](const TStride& st, int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (PACKED) return (q0 + t_) * st.row + (int64_t)hq_ * st.head;
        else return (int64_t)bidx * st.batch + (int64_t)t_ * st.row + (int64_t)hq_ * st.head;
    };
    // CAUSAL: the tile's keys end where its last row's do (t_last <= sq - 1, so k_end <= L; it may be <= 0: the tile sees nothing)
    int k_end = L;
    if constexpr (CAUSAL) {
        const int t_last = (min((tile + 1) * kMpRows, rows_tile) - 1) / p.h_ratio;
        k_end = __builtin_amdgcn_readfirstlane(min(L, L - sq + t_last + 1));
    }
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
        const char* qrow = (const char*)p.q_ptr + 2 * row_off(p.q, hq[qb], t[qb]);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            qf[qb][ci] = row_ok[qb] ? *(const u32x4*)(qrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    });

    // ---- staging: what this lane loads in a step -----------------------------------------------------------------------------------------------
    // loads 0, 1: K row 16 j + 4 w + lane / 16, 16-byte slot lane % 16 of its no-rope columns; load 2: K row 8 w + lane / 8, slot 16 + lane % 8 (the
    // rope columns); loads 3, 4: the V rows of loads 0, 1, slot lane % 16.
    const int wrow = 4 * wave + (lane >> 4), wslot = lane & 15;
    const int rrow = 8 * wave + (lane >> 3), rslot = lane & 7;
    const uint32_t krow_b = (uint32_t)(p.k.row * 2), vrow_b = (uint32_t)(p.v.row * 2);
    const char* kbase = uniform_ptr((const char*)p.k_ptr + 2 * ((PACKED ? k0 * p.k.row : (int64_t)bidx * p.k.batch) + (int64_t)kvh * p.k.head));
    const char* vbase = uniform_ptr((const char*)p.v_ptr + 2 * ((PACKED ? k0 * p.v.row : (int64_t)bidx * p.v.batch) + (int64_t)kvh * p.v.head));
    // one descriptor per tensor, ending at row L of the sequence (rows at or past L read as zeros: row indices are clamped to L, the row strides
    // are at least the row widths, and L x row stride < 2^31 bytes by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * krow_b + 2 * kMpDK : 0u);
    const rsrc_t vrs = make_rsrc(vbase, L > 0 ? (uint32_t)(L - 1) * vrow_b + 2 * kMpDV : 0u);
    auto load_step = [&](int key0, u32x4 (&st)[NL]) __attribute__((always_inline)) {
        static_for<0, 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t row = (uint32_t)min(key0 + 16 * j + wrow, L);
            st[j] = buf_load16(krs, row * krow_b + 16 * wslot);
            st[3 + j] = buf_load16(vrs, row * vrow_b + 16 * wslot);
        });
        st[2] = buf_load16(krs, (uint32_t)min(key0 + rrow, L) * krow_b + 2 * kMpDN + 16 * rslot);
    };
    // registers -> the three images of stage BUF
    auto store_step = [&](auto bufc, const u32x4 (&st)[NL]) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        FA_LDS char* nimg = (FA_LDS char*)smem + BUF * MlapLds::kStage;
        FA_LDS char* rimg = nimg + MlapLds::kImageN;
        FA_LDS char* vimg = rimg + MlapLds::kImageR;
        static_for<0, 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            *(FA_LDS u32x4*)(nimg + lds_tile_off<kMpDN>((uint32_t)(16 * j + wrow), (uint32_t)wslot)) = st[j];
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMpDV>((uint32_t)(16 * j + wrow), (uint32_t)wslot)) = st[3 + j];
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMpDR>((uint32_t)rrow, (uint32_t)rslot)) = st[2];
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
        constexpr int BUF = decltype(bufc)::value;
        const FA_LDS char* nimg = (const FA_LDS char*)smem + BUF * MlapLds::kStage;
        const FA_LDS char* rimg = nimg + MlapLds::kImageN;
        const FA_LDS char* vimg = rimg + MlapLds::kImageR;
        f32x4 s[QB][2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, QB>([&](auto qq) { s[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f}; });
            static_for<0, NCN>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(nimg + lds_tile_off<kMpDN>(16 * b + n16, 4 * ci + g));
                static_for<0, QB>([&](auto qq) {
                    constexpr int qb = decltype(qq)::value;
                    s[qb][b] = LP<T>::mfma16(kf, qf[qb][ci], s[qb][b]);
                });
            });
            static_for<0, NCR>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(rimg + lds_tile_off<kMpDR>(16 * b + n16, 4 * ci + g));
                static_for<0, QB>([&](auto qq) {
                    constexpr int qb = decltype(qq)::value;
                    s[qb][b] = LP<T>::mfma16(kf, qf[qb][NCN + ci], s[qb][b]);
                });
            });
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
            pf[qb] = u32x4{LP<T>::pack2(pe[0], pe[1]), LP<T>::pack2(pe[2], pe[3]), LP<T>::pack2(pe[4], pe[5]), LP<T>::pack2(pe[6], pe[7])};
            static_for<0, NO>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                oacc[qb][ci] *= alpha;
            });
        });
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMpDV>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMpDV>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(vimg, a0), v1 = lds_read_tr8(vimg, a1);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                oacc[qb][ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, pf[qb], oacc[qb][ci]);
            });
        });
    };

    // ---- the 32-key steps, all four waves together; two LDS stages in turn ---------------------------------------------------------------------
    // Stage n & 1 holds step n.  While step n computes, the loads of step n + 1 are in flight; they are written to the other stage behind the
    // compute - every wave left that stage's reads (step n - 1) in front of the last barrier - and one barrier publishes them.  The loads of
    // step n + 2 are issued behind that barrier, so nothing is outstanding when it is reached.  k_end is the workgroup's: every wave meets
    // the same barriers.
    // Test builds (FA_KVC_STAGE_DEBUG, fa_kvcache_stage_debug.hpp): the two helpers hold one wave back; FA_KVC_STAGE_RACY moves the step's barrier in front of store_step.
    // Why the racy form can neither hang nor fault here: (1) the barrier only changes places inside the same `if (key0 + kKvcStep < k_end)`, whose
    // condition is the workgroup's (k_end and key0 are the same in every wave, `active` is not part of it), so every wave still meets the same number
    // of barriers on every path; (2) the three images are read by compute_step alone, as MFMA operands (kf, v0 / v1): what comes out of them are scores
    // and O, which reach compares, exponentials and stores of VALUES - every address (lds_tile_off of lane constants, row_off / row_index of the lane's
    // row, the sequence's base rows from cu_seqlens), every index and every loop bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[NL];
        int key = 0;
        if (key < k_end) {
            load_step(key, st);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st);
        }
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(key + kKvcStep, st);
        auto step = [&](auto bufc, int key0) __attribute__((always_inline)) {
            constexpr int BUF = decltype(bufc)::value;
            kvc_stage_slow_reader(key0 / kKvcStep, wave);
            if (active) compute_step(bufc, key0);
            if (key0 + kKvcStep < k_end) {
#if FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                kvc_stage_slow_writer(key0 / kKvcStep, wave);
                store_step(std::integral_constant<int, BUF ^ 1>{}, st);
#if !FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                if (key0 + 2 * kKvcStep < k_end) load_step(key0 + 2 * kKvcStep, st);
            }
        };
        for (; key < k_end; key += 2 * kKvcStep) {
            step(std::integral_constant<int, 0>{}, key);
            if (key + kKvcStep < k_end) step(std::integral_constant<int, 1>{}, key + kKvcStep);
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
        char* orow = (char*)p.o_ptr + 2 * (row_off(p.o, hq[qb], t[qb]) + 4 * g);
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            *(u32x2*)(orow + 32 * ci) = u32x2{LP<T>::pack2(oacc[qb][ci][0] * inv, oacc[qb][ci][1] * inv), LP<T>::pack2(oacc[qb][ci][2] * inv, oacc[qb][ci][3] * inv)};
        });
        if (g == 0) p.lse_ptr[row_index(hq[qb], t[qb])] = lse;
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
        auto* kernel = p.is_causal ? (packed ? fa_fwd_mla_prefill_kernel<T, true, true> : fa_fwd_mla_prefill_kernel<T, true, false>)
                                   : (packed ? fa_fwd_mla_prefill_kernel<T, false, true> : fa_fwd_mla_prefill_kernel<T, false, false>);
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kKvcThreads), 0, s, p);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
