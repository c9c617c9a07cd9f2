// fa_bwd_mla_prefill.hip — the backward of MLA prefill attention (fa_run_mla_prefill_bwd): dQ, dK (192 wide) and dV (128 wide), dense and packed.
//
//   The 7-GEMM, two-launch, atomics-free form of fa_bwd.hip on the register-staged two-stage LDS body of fa_fwd_mla_prefill.hip (four waves, 32-row or
//   32-key steps walked by all four waves together, five 16-byte loads per lane and step through registers into the three images of a stage - 32 x 256 B,
//   32 x 128 B, 32 x 256 B - one barrier per step, compiler-scheduled).  With g = h / h_k, packed row r = t * g + j of a KV head is query t, head kvh * g + j.
//   * dQ kernel (first launch): the forward's tile and loop.  A workgroup owns 64 packed rows, a wave 16, a lane one row: Q^T (24 registers), dO^T (16),
//     lse_t, D_t and the 12 x 4 accumulators of dQ^T.  Per 32-key step S^T = K Q^T (K rows from the two K images), dP^T = V dO^T (V read as ROWS, the way K
//     is), P = exp(S * scale - lse) on visible pairs and exactly 0 elsewhere, dS = P (dP - D), and the lane's eight dS^T values, rounded to the dtype, are
//     the B operand of dQ^T += K^T dS^T with K^T by ds_read_b64_tr_b16 from both K images (the 64-wide one through lds_tile_off<64>).  The prologue forms
//     D_t = sum_c dO_tc O_tc from the lane's fragments of the two rows and a sum over the four lane groups, and writes it to dsoftmax_sum (layout of lse)
//     for the second launch.  One column block a wave ships (FA_MLAPB_WAVE_ROWS = 16).  FA_MLAPB_WAVE_ROWS = 32 builds two blocks a wave (128-row
//     workgroups, every K / V / K^T fragment read once for both): 48 + 32 + 96 registers of operands and accumulators before staging and scores, and this
//     compiler gives it 256 VGPRs with 32 - 88 of them spilled to 116 - 212 bytes of scratch in all eight kernels - not a form that may ship.
//   * dK/dV kernel (second launch, same stream): the mirror image.  A workgroup owns 64 keys of one (sequence, KV head), a wave 16, a lane one key: K
//     (24 registers) and V (16) stay in registers as B operands.  It walks the packed rows of the head's WHOLE group in 32-row steps - under `causal` from
//     the first row that sees the tile's first key - with Q (128 + 64 columns) in K's images, dO in V's and the step's 32 lse / D values next to them; a lane
//     builds each row's address from (t, head).  S = Q K^T and dP = dO V^T read Q / dO rows from LDS; the lane's P and dS values of the two 16-row blocks are
//     the B operands of dV^T += dO^T P and dK^T += Q^T dS with dO^T / Q^T by transposed reads.  48 + 32 accumulator registers.  The group loop inside the
//     workgroup is what makes GQA deterministic without a workspace or atomics.
//   One workgroup owns an output row from start to end; rows past a sequence are never written; a wave past the rows (keys) takes part in staging and
//   barriers only; a dead row gets dQ = 0 and a key no row sees dK = dV = 0, both written.  Rounding points: P and dS are rounded to the dtype in front of
//   their second matmuls, D comes from the rounded O, every output is rounded once.
//   Kernels of this file: 16 = (dQ, dK/dV) x (fp16, bf16) x (causal, not) x (dense, packed).
#include "fa_kvcache_attn.hpp"
#include "fa_kvcache_stage_debug.hpp"

#ifndef FA_MLAPB_WAVE_ROWS
#define FA_MLAPB_WAVE_ROWS 16
#endif

namespace fa {

namespace {

static_assert(FA_MLAPB_WAVE_ROWS == 16 || FA_MLAPB_WAVE_ROWS == 32, "a wave of the dQ kernel owns one or two 16-row query column blocks");
constexpr int kMbQB = FA_MLAPB_WAVE_ROWS / kKvcRows;        // query column blocks of a wave of the dQ kernel
constexpr int kMbRowsDq = kKvcWaves * FA_MLAPB_WAVE_ROWS;   // packed query rows of a dQ workgroup
constexpr int kMbRows = kKvcWaves * kKvcRows;       // keys of a dK/dV workgroup
constexpr int kMbDN = 128;                  // the no-rope columns of q / k
constexpr int kMbDR = 64;                   // the rope columns
constexpr int kMbDK = kMbDN + kMbDR;
constexpr int kMbDV = 128;

struct MlabLds {
    static constexpr int kImageN = kKvcStep * kMbDN * 2;        // 32 rows x 256 B
    static constexpr int kImageR = kKvcStep * kMbDR * 2;        // 32 rows x 128 B
    static constexpr int kImageV = kKvcStep * kMbDV * 2;        // 32 rows x 256 B
    static constexpr int kImages = kImageN + kImageR + kImageV; // 20 KB
    static constexpr int kRowF = kKvcStep * 4;                  // dK/dV: the step's 32 lse values, then its 32 D values
    static constexpr int kStageDq = kImages;
    static constexpr int kStageKv = kImages + 2 * kRowF;
};

// sum of the eight products of two fragments of 16-bit values
template <typename T>
FA_DEV float dot8(const u32x4& a, const u32x4& b) {
    float s = 0.f;
    static_for<0, 4>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        s = __builtin_fmaf(LP<T>::to_float((uint16_t)(a[i] & 0xffffu)), LP<T>::to_float((uint16_t)(b[i] & 0xffffu)), s);
        s = __builtin_fmaf(LP<T>::to_float((uint16_t)(a[i] >> 16)), LP<T>::to_float((uint16_t)(b[i] >> 16)), s);
    });
    return s;
}

// =============================================================================================================================================
// dQ (and D)
// =============================================================================================================================================
template <typename T, bool CAUSAL, bool PACKED>
FA_DEV void mla_prefill_dq(const MlaPrefillBwdParams& p) {
    constexpr int NCN = kMbDN / 32;     // 16x16x32 MFMAs per 16 keys of S^T over the wide K image
    constexpr int NCR = kMbDR / 32;     // ... and over the narrow one
    constexpr int NC = NCN + NCR;
    constexpr int NV = kMbDV / 32;      // ... of dP^T
    constexpr int NQN = kMbDN / 16;     // dQ^T blocks of 16 columns fed from the wide K image
    constexpr int NQR = kMbDR / 16;     // ... from the narrow one
    constexpr int QB = kMbQB;
    constexpr int NL = 5;               // loads per lane and step: two of the wide K image, one of the narrow one, two of V
    __shared__ __attribute__((aligned(16))) char smem[2 * MlabLds::kStageDq];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int n_tiles = PACKED ? p.slots : p.n_row_tiles;       // PACKED: the tile slots of a KV head, and `bh` below is the KV head
    int tile = id % n_tiles;
    const int bh = id / n_tiles;
    int bidx = bh / p.h_k, kvh = bh - bidx * p.h_k;
    int sq = p.seqlen_q, L = p.seqlen_k;
    int64_t q0 = 0, k0 = 0;
    if constexpr (PACKED) {
        kvh = bh;
        const int slot = tile;
        if (!kvc_slot_lookup<kMbRowsDq>(p.cu_q, p.b, p.h_ratio, (uint32_t)slot, bidx, tile)) return;     // a slack slot: nothing to write
        const int c0 = __builtin_amdgcn_readfirstlane(p.cu_q[bidx]);
        sq = __builtin_amdgcn_readfirstlane(p.cu_q[bidx + 1]) - c0;
        const int d0 = __builtin_amdgcn_readfirstlane(p.cu_k[bidx]);
        L = __builtin_amdgcn_readfirstlane(p.cu_k[bidx + 1]) - d0;
        q0 = c0;
        k0 = d0;
        // the forward's early-outs: cu_seqlens that point outside the tensors never become an address.  Every value here is the workgroup's.
        if (c0 < 0 || q0 + sq > p.total_q) return;
        const int64_t k_left = p.total_k - k0;
        L = d0 < 0 || k_left < 0 ? 0 : (L > k_left ? (int)k_left : max(L, 0));
    }
    const int rows_tile = sq * p.h_ratio;
    auto row_index = [&](int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (PACKED) return (int64_t)hq_ * p.total_q + q0 + t_;
        else return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t_;
    };
    auto row_off = [&](const TStride& st, int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (PACKED) return (q0 + t_) * st.row + (int64_t)hq_ * st.head;
        else return (int64_t)bidx * st.batch + (int64_t)t_ * st.row + (int64_t)hq_ * st.head;
    };
    int k_end = L;
    if constexpr (CAUSAL) {
        const int t_last = (min((tile + 1) * kMbRowsDq, rows_tile) - 1) / p.h_ratio;
        k_end = __builtin_amdgcn_readfirstlane(min(L, L - sq + t_last + 1));
    }
    const float c = p.scale_log2e;

    // ---- this lane's query row: Q^T and dO^T fragments for the whole call, lse, D, visible-key limit ------------------------------------------
    const int wrow0 = tile * kMbRowsDq + wave * FA_MLAPB_WAVE_ROWS;
    const bool active = wrow0 < rows_tile;      // (wave-uniform) false: staging and barriers only
    bool row_ok[QB];
    int t[QB], hq[QB], lim[QB];
    u32x4 qf[QB][NC], dof[QB][NV];
    float dsum[QB], lse2[QB];
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        const int pr = wrow0 + kKvcRows * qb + n16;
        row_ok[qb] = pr < rows_tile;
        t[qb] = row_ok[qb] ? pr / p.h_ratio : 0;
        hq[qb] = kvh * p.h_ratio + (row_ok[qb] ? pr - t[qb] * p.h_ratio : 0);
        lim[qb] = row_ok[qb] ? L : 0;
        if (CAUSAL && row_ok[qb]) lim[qb] = min(L, L - sq + t[qb] + 1);
        dsum[qb] = 0.f;
        lse2[qb] = 0.f;
        const char* qrow = (const char*)p.q_ptr + 2 * row_off(p.q, hq[qb], t[qb]);
        const char* orow = (const char*)p.o_ptr + 2 * row_off(p.o, hq[qb], t[qb]);
        const char* dorow = (const char*)p.do_ptr + 2 * row_off(p.dout, hq[qb], t[qb]);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            qf[qb][ci] = row_ok[qb] ? *(const u32x4*)(qrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
        static_for<0, NV>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            dof[qb][ci] = row_ok[qb] ? *(const u32x4*)(dorow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
            const u32x4 of = row_ok[qb] ? *(const u32x4*)(orow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
            dsum[qb] += dot8<T>(of, dof[qb][ci]);
        });
        // D_t: the lane's 32 columns, then the other three lane groups' (every lane of the wave takes part)
        dsum[qb] = sum_four_groups(dsum[qb]);
        if (row_ok[qb]) {
            lse2[qb] = p.lse_ptr[row_index(hq[qb], t[qb])] * kLog2e;
            if (g == 0) p.dsum_ptr[row_index(hq[qb], t[qb])] = dsum[qb];
        }
    });

    // ---- staging: what this lane loads in a step (the forward's) --------------------------------------------------------------------------------
    const int wrow = 4 * wave + (lane >> 4), wslot = lane & 15;
    const int rrow = 8 * wave + (lane >> 3), rslot = lane & 7;
    const uint32_t krow_b = (uint32_t)(p.k.row * 2), vrow_b = (uint32_t)(p.v.row * 2);
    const char* kbase = uniform_ptr((const char*)p.k_ptr + 2 * ((PACKED ? k0 * p.k.row : (int64_t)bidx * p.k.batch) + (int64_t)kvh * p.k.head));
    const char* vbase = uniform_ptr((const char*)p.v_ptr + 2 * ((PACKED ? k0 * p.v.row : (int64_t)bidx * p.v.batch) + (int64_t)kvh * p.v.head));
    // one descriptor per tensor, ending at row L of the sequence (rows at or past L read as zeros: row indices are clamped to L, the row strides
    // are at least the row widths, and L x row stride < 2^31 bytes by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * krow_b + 2 * kMbDK : 0u);
    const rsrc_t vrs = make_rsrc(vbase, L > 0 ? (uint32_t)(L - 1) * vrow_b + 2 * kMbDV : 0u);
    auto load_step = [&](int key0, u32x4 (&st)[NL]) __attribute__((always_inline)) {
        static_for<0, 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t row = (uint32_t)min(key0 + 16 * j + wrow, L);
            st[j] = buf_load16(krs, row * krow_b + 16 * wslot);
            st[3 + j] = buf_load16(vrs, row * vrow_b + 16 * wslot);
        });
        st[2] = buf_load16(krs, (uint32_t)min(key0 + rrow, L) * krow_b + 2 * kMbDN + 16 * rslot);
    };
    auto store_step = [&](auto bufc, const u32x4 (&st)[NL]) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        FA_LDS char* nimg = (FA_LDS char*)smem + BUF * MlabLds::kStageDq;
        FA_LDS char* rimg = nimg + MlabLds::kImageN;
        FA_LDS char* vimg = rimg + MlabLds::kImageR;
        static_for<0, 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            *(FA_LDS u32x4*)(nimg + lds_tile_off<kMbDN>((uint32_t)(16 * j + wrow), (uint32_t)wslot)) = st[j];
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMbDV>((uint32_t)(16 * j + wrow), (uint32_t)wslot)) = st[3 + j];
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMbDR>((uint32_t)rrow, (uint32_t)rslot)) = st[2];
    };

    // transposed-read addresses of this lane (fa_device.hpp lds_tile_off image): block c, half hh -> rows hh * 16 + 4 g + q, columns 16 c + 4 p
    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 dq[QB][NQN + NQR];
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        static_for<0, NQN + NQR>([&](auto cc) {
            dq[qb][decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+v"(dq[qb][decltype(cc)::value]));
        });
    });

    // one 32-key step of this wave's rows over the images of stage BUF: every K, V and K^T fragment is read once and serves the wave's QB column blocks
    auto compute_step = [&](auto bufc, int key0) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        const FA_LDS char* nimg = (const FA_LDS char*)smem + BUF * MlabLds::kStageDq;
        const FA_LDS char* rimg = nimg + MlabLds::kImageN;
        const FA_LDS char* vimg = rimg + MlabLds::kImageR;
        f32x4 s[QB][2], dp[QB][2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, QB>([&](auto qq) {
                s[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f};
                dp[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            });
            static_for<0, NCN>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(nimg + lds_tile_off<kMbDN>(16 * b + n16, 4 * ci + g));
                static_for<0, QB>([&](auto qq) {
                    constexpr int qb = decltype(qq)::value;
                    s[qb][b] = LP<T>::mfma16(kf, qf[qb][ci], s[qb][b]);
                });
            });
            static_for<0, NCR>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(rimg + lds_tile_off<kMbDR>(16 * b + n16, 4 * ci + g));
                static_for<0, QB>([&](auto qq) {
                    constexpr int qb = decltype(qq)::value;
                    s[qb][b] = LP<T>::mfma16(kf, qf[qb][NCN + ci], s[qb][b]);
                });
            });
            static_for<0, NV>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 vf = *(const FA_LDS u32x4*)(vimg + lds_tile_off<kMbDV>(16 * b + n16, 4 * ci + g));
                static_for<0, QB>([&](auto qq) {
                    constexpr int qb = decltype(qq)::value;
                    dp[qb][b] = LP<T>::mfma16(vf, dof[qb][ci], dp[qb][b]);
                });
            });
        });
        // hidden pairs: P = 0 and dS = 0 by selection, whatever exp gives there
        u32x4 dsf[QB];
        static_for<0, QB>([&](auto qq) {
            constexpr int qb = decltype(qq)::value;
            float ds[8];
            static_for<0, 8>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                const bool vis = key0 + 16 * (j >> 2) + 4 * g + (j & 3) < lim[qb];
                const float pe = fast_exp2(__builtin_fmaf(s[qb][j >> 2][j & 3], c, -lse2[qb]));
                ds[j] = vis ? pe * (dp[qb][j >> 2][j & 3] - dsum[qb]) : 0.f;
            });
            dsf[qb] = u32x4{LP<T>::pack2(ds[0], ds[1]), LP<T>::pack2(ds[2], ds[3]), LP<T>::pack2(ds[4], ds[5]), LP<T>::pack2(ds[6], ds[7])};
        });
        static_for<0, NQN>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMbDN>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMbDN>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(nimg, a0), v1 = lds_read_tr8(nimg, a1);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                dq[qb][ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, dsf[qb], dq[qb][ci]);
            });
        });
        // the 64-wide image, read transposed: the same 4-row x 16-column blocks, eight 16-byte slots a row
        static_for<0, NQR>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMbDR>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMbDR>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(rimg, a0), v1 = lds_read_tr8(rimg, a1);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                dq[qb][NQN + ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, dsf[qb], dq[qb][NQN + ci]);
            });
        });
    };

    // ---- the 32-key steps, all four waves together; two LDS stages in turn (the forward's schedule) ------------------------------------------------
    // Stage n & 1 holds step n.  While step n computes, the loads of step n + 1 are in flight; they are written to the other stage behind the
    // compute - every wave left that stage's reads (step n - 1) in front of the last barrier - and one barrier publishes them.  k_end is the
    // workgroup's: every wave meets the same barriers.
    // Test builds (FA_KVC_STAGE_DEBUG, fa_kvcache_stage_debug.hpp): the two helpers hold one wave back; FA_KVC_STAGE_RACY moves the step's barrier in front of store_step.
    // Why the racy form can neither hang nor fault here: (1) the barrier only changes places inside the same `if (key0 + kKvcStep < k_end)`, whose
    // condition is the workgroup's (k_end and key0 are the same in every wave, `active` is not part of it), so every wave still meets the same number
    // of barriers on every path; (2) the three images are read by compute_step alone, as MFMA operands (kf, vf, v0 / v1): what comes out of them are
    // scores, dP and dQ, which reach compares of VALUES, exponentials and the stores of dQ - every address (lds_tile_off of lane constants, row_off /
    // row_index of the lane's row, the sequence's base rows from cu_seqlens), every index and every loop bound comes from the parameters.  A stale image
    // gives wrong numbers.
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

    // ---- epilogue: the lane's row, columns 16 c + 4 g .. + 3 of every block c; a dead row (or no keys at all) writes zeros -------------------------
    if (!active) return;
    const float sc = p.scale;
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        if (!row_ok[qb]) return;
        char* dqrow = (char*)p.dq_ptr + 2 * (row_off(p.dq, hq[qb], t[qb]) + 4 * g);
        static_for<0, NQN + NQR>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            *(u32x2*)(dqrow + 32 * ci) =
                u32x2{LP<T>::pack2(dq[qb][ci][0] * sc, dq[qb][ci][1] * sc), LP<T>::pack2(dq[qb][ci][2] * sc, dq[qb][ci][3] * sc)};
        });
    });
}

// =============================================================================================================================================
// dK / dV
// =============================================================================================================================================
template <typename T, bool CAUSAL, bool PACKED>
FA_DEV void mla_prefill_dkdv(const MlaPrefillBwdParams& p) {
    constexpr int NCN = kMbDN / 32, NCR = kMbDR / 32, NC = NCN + NCR, NV = kMbDV / 32;
    constexpr int NKN = kMbDN / 16, NKR = kMbDR / 16, NO = kMbDV / 16;     // dK^T blocks from the wide / narrow Q image, dV^T blocks
    constexpr int NL = 5;               // loads per lane and step: two of the wide Q image, one of the narrow one, two of dO
    __shared__ __attribute__((aligned(16))) char smem[2 * MlabLds::kStageKv];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int n_tiles = PACKED ? p.slots : p.n_row_tiles;       // key tiles of a (batch, KV head) / PACKED: key-tile slots of a KV head
    int tile = id % n_tiles;
    const int bh = id / n_tiles;
    int bidx = bh / p.h_k, kvh = bh - bidx * p.h_k;
    int sq = p.seqlen_q, L = p.seqlen_k;
    int64_t q0 = 0, k0 = 0;
    if constexpr (PACKED) {
        kvh = bh;
        const int slot = tile;
        if (!kvc_slot_lookup<kMbRows>(p.cu_k, p.b, 1, (uint32_t)slot, bidx, tile)) return;     // a slack slot: nothing to write
        const int c0 = __builtin_amdgcn_readfirstlane(p.cu_q[bidx]);
        sq = __builtin_amdgcn_readfirstlane(p.cu_q[bidx + 1]) - c0;
        const int d0 = __builtin_amdgcn_readfirstlane(p.cu_k[bidx]);
        L = __builtin_amdgcn_readfirstlane(p.cu_k[bidx + 1]) - d0;
        q0 = c0;
        k0 = d0;
        // the forward's early-outs with the roles swapped: the keys are what this kernel writes, so a key range outside k / v is not served, and the
        // query rows are cut at the last row of q.  Every value here is the workgroup's, so all four waves leave together.
        if (d0 < 0 || k0 + L > p.total_k) return;
        const int64_t q_left = p.total_q - q0;
        sq = c0 < 0 || q_left < 0 ? 0 : (sq > q_left ? (int)q_left : max(sq, 0));
    }
    const int G = p.h_ratio;
    const int rows_total = sq * G;              // packed rows r = t * G + j of this KV head's group
    const int key0t = tile * kMbRows;
    const bool active = key0t + wave * kKvcRows < L;        // (wave-uniform) false: staging and barriers only
    const int mykey = key0t + wave * kKvcRows + n16;
    const bool key_ok = mykey < L;
    // the rows that see this lane's key are rmin <= r < rows_total: query t sees key j iff j <= L - sq + t, and r >= tmin * G iff t >= tmin
    int rmin = key_ok ? 0 : rows_total;
    int r_begin = 0;
    if constexpr (CAUSAL) {
        const int64_t shift = (int64_t)L - sq;
        const int64_t tmin = min(max((int64_t)mykey - shift, (int64_t)0), (int64_t)sq);
        rmin = key_ok ? (int)tmin * G : rows_total;
        const int64_t tmin0 = min(max((int64_t)key0t - shift, (int64_t)0), (int64_t)sq);
        r_begin = __builtin_amdgcn_readfirstlane(((int)tmin0 * G) & ~(kKvcStep - 1));      // the first row that sees the tile's first key, down to a step
    }
    const int r_end = rows_total;
    const float c = p.scale_log2e;

    auto key_off = [&](const TStride& st) __attribute__((always_inline)) -> int64_t {
        return (PACKED ? (k0 + mykey) * st.row : (int64_t)bidx * st.batch + (int64_t)mykey * st.row) + (int64_t)kvh * st.head;
    };
    // ---- this lane's key: K^T and V^T fragments for the whole call ----------------------------------------------------------------------------
    u32x4 kf[NC], vf[NV];
    {
        const char* krow = (const char*)p.k_ptr + 2 * key_off(p.k);
        const char* vrow = (const char*)p.v_ptr + 2 * key_off(p.v);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            kf[ci] = key_ok ? *(const u32x4*)(krow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
        static_for<0, NV>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            vf[ci] = key_ok ? *(const u32x4*)(vrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    }

    // ---- staging: what this lane loads in a step ------------------------------------------------------------------------------------------------
    // loads 0, 1: packed row 16 j + 4 w + lane / 16 of the step, 16-byte slot lane % 16 of Q's no-rope columns; load 2: row 8 w + lane / 8, slot 16 + lane % 8
    // (the rope columns); loads 3, 4: the dO rows of loads 0, 1.  The lanes of slot 0 also load the lse and D values of their two rows.  A row past the
    // group's last one is not loaded: zeros go to the images.  (t, j) of the lane's three rows are kept and advanced by a step at a time.
    const int wrow = 4 * wave + (lane >> 4), wslot = lane & 15;
    const int rrow = 8 * wave + (lane >> 3), rslot = lane & 7;
    const int q32 = kKvcStep / G, r32 = kKvcStep - q32 * G;     // a step of 32 packed rows is q32 query rows and r32 heads on
    int st_t[3], st_j[3];
    static_for<0, 3>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        const int r = r_begin + (i < 2 ? 16 * i + wrow : rrow);
        st_t[i] = r / G;
        st_j[i] = r - st_t[i] * G;
    });
    const char* qbase = (const char*)p.q_ptr + 2 * (PACKED ? q0 * p.q.row : (int64_t)bidx * p.q.batch);
    const char* dobase = (const char*)p.do_ptr + 2 * (PACKED ? q0 * p.dout.row : (int64_t)bidx * p.dout.batch);
    auto load_step = [&](u32x4 (&st)[NL], float (&sf)[4]) __attribute__((always_inline)) {
        static_for<0, 3>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            const bool ok = st_t[i] < sq;
            const int hq = kvh * G + st_j[i];
            const char* qrow = qbase + 2 * ((int64_t)st_t[i] * p.q.row + (int64_t)hq * p.q.head);
            if constexpr (i < 2) {
                const char* dorow = dobase + 2 * ((int64_t)st_t[i] * p.dout.row + (int64_t)hq * p.dout.head);
                st[i] = ok ? *(const u32x4*)(qrow + 16 * wslot) : u32x4{0u, 0u, 0u, 0u};
                st[3 + i] = ok ? *(const u32x4*)(dorow + 16 * wslot) : u32x4{0u, 0u, 0u, 0u};
                const bool okf = ok && wslot == 0;
                const int64_t ri = PACKED ? (int64_t)hq * p.total_q + q0 + st_t[i] : ((int64_t)bidx * p.h + hq) * p.seqlen_q + st_t[i];
                sf[2 * i] = okf ? p.lse_ptr[ri] : 0.f;
                sf[2 * i + 1] = okf ? p.dsum_ptr[ri] : 0.f;
            } else {
                st[2] = ok ? *(const u32x4*)(qrow + 2 * kMbDN + 16 * rslot) : u32x4{0u, 0u, 0u, 0u};
            }
            // the next step's row
            st_j[i] += r32;
            st_t[i] += q32;
            if (st_j[i] >= G) {
                st_j[i] -= G;
                st_t[i] += 1;
            }
        });
    };
    auto store_step = [&](auto bufc, const u32x4 (&st)[NL], const float (&sf)[4]) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        FA_LDS char* nimg = (FA_LDS char*)smem + BUF * MlabLds::kStageKv;
        FA_LDS char* rimg = nimg + MlabLds::kImageN;
        FA_LDS char* vimg = rimg + MlabLds::kImageR;
        FA_LDS float* frow = (FA_LDS float*)(vimg + MlabLds::kImageV);
        static_for<0, 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            *(FA_LDS u32x4*)(nimg + lds_tile_off<kMbDN>((uint32_t)(16 * j + wrow), (uint32_t)wslot)) = st[j];
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMbDV>((uint32_t)(16 * j + wrow), (uint32_t)wslot)) = st[3 + j];
            if (wslot == 0) {
                frow[16 * j + wrow] = sf[2 * j];
                frow[kKvcStep + 16 * j + wrow] = sf[2 * j + 1];
            }
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMbDR>((uint32_t)rrow, (uint32_t)rslot)) = st[2];
    };

    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 dk[NKN + NKR], dv[NO];
    static_for<0, NKN + NKR>([&](auto cc) {
        dk[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(dk[decltype(cc)::value]));
    });
    static_for<0, NO>([&](auto cc) {
        dv[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(dv[decltype(cc)::value]));
    });

    // one 32-row step over the images of stage BUF: rows 16 b + 4 g + r of the step are this lane's C rows, its key the C column
    auto compute_step = [&](auto bufc, int row0) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        const FA_LDS char* nimg = (const FA_LDS char*)smem + BUF * MlabLds::kStageKv;
        const FA_LDS char* rimg = nimg + MlabLds::kImageN;
        const FA_LDS char* vimg = rimg + MlabLds::kImageR;
        const FA_LDS char* frow = vimg + MlabLds::kImageV;
        f32x4 s[2], dp[2], lse4[2], d4[2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            static_for<0, NCN>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 a = *(const FA_LDS u32x4*)(nimg + lds_tile_off<kMbDN>(16 * b + n16, 4 * ci + g));
                s[b] = LP<T>::mfma16(a, kf[ci], s[b]);
            });
            static_for<0, NCR>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 a = *(const FA_LDS u32x4*)(rimg + lds_tile_off<kMbDR>(16 * b + n16, 4 * ci + g));
                s[b] = LP<T>::mfma16(a, kf[NCN + ci], s[b]);
            });
            static_for<0, NV>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 a = *(const FA_LDS u32x4*)(vimg + lds_tile_off<kMbDV>(16 * b + n16, 4 * ci + g));
                dp[b] = LP<T>::mfma16(a, vf[ci], dp[b]);
            });
            lse4[b] = *(const FA_LDS f32x4*)(frow + 4 * (16 * b + 4 * g));
            d4[b] = *(const FA_LDS f32x4*)(frow + 4 * (kKvcStep + 16 * b + 4 * g));
        });
        // hidden pairs (and rows past the group): P = 0 and dS = 0 by selection, whatever exp gives there
        float pe[8], ds[8];
        static_for<0, 8>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const int r = row0 + 16 * (j >> 2) + 4 * g + (j & 3);
            const bool vis = r >= rmin && r < rows_total;
            const float e = fast_exp2(__builtin_fmaf(s[j >> 2][j & 3], c, -lse4[j >> 2][j & 3] * kLog2e));
            pe[j] = vis ? e : 0.f;
            ds[j] = vis ? e * (dp[j >> 2][j & 3] - d4[j >> 2][j & 3]) : 0.f;
        });
        const u32x4 pf = u32x4{LP<T>::pack2(pe[0], pe[1]), LP<T>::pack2(pe[2], pe[3]), LP<T>::pack2(pe[4], pe[5]), LP<T>::pack2(pe[6], pe[7])};
        const u32x4 dsf = u32x4{LP<T>::pack2(ds[0], ds[1]), LP<T>::pack2(ds[2], ds[3]), LP<T>::pack2(ds[4], ds[5]), LP<T>::pack2(ds[6], ds[7])};
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMbDV>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMbDV>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(vimg, a0), v1 = lds_read_tr8(vimg, a1);
            dv[ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, pf, dv[ci]);
        });
        static_for<0, NKN>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMbDN>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMbDN>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(nimg, a0), v1 = lds_read_tr8(nimg, a1);
            dk[ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, dsf, dk[ci]);
        });
        static_for<0, NKR>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMbDR>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMbDR>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(rimg, a0), v1 = lds_read_tr8(rimg, a1);
            dk[NKN + ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, dsf, dk[NKN + ci]);
        });
    };

    // ---- the 32-row steps, all four waves together; two LDS stages in turn (the forward's schedule with rows in the place of keys) ----------------
    // Stage n & 1 holds step n.  load_step is called once per step, in order, so the rows it keeps advance with the loop.  r_begin and r_end are
    // the workgroup's: every wave meets the same barriers.
    // Test builds (FA_KVC_STAGE_DEBUG, fa_kvcache_stage_debug.hpp): the two helpers hold one wave back; FA_KVC_STAGE_RACY moves the step's barrier in front of store_step.
    // Why the racy form can neither hang nor fault here: (1) the barrier only changes places inside the same `if (row0 + kKvcStep < r_end)`, whose
    // condition is the workgroup's (r_end and row0 are the same in every wave, `active` is not part of it), so every wave still meets the same number
    // of barriers on every path; (2) the three images and the lse / D rows are read by compute_step alone, as MFMA operands (a, v0 / v1) and as the
    // operands of an exponential and a subtraction: what comes out of them are scores, P, dS, dK and dV, which reach the stores of VALUES - every
    // address (lds_tile_off of lane constants, the (t, head) rows of load_step, key_off of the lane's key, the base rows from cu_seqlens), every index,
    // every visibility compare (rmin, rows_total) and every loop bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[NL];
        float sf[4];
        int row = r_begin;
        if (row < r_end) {
            load_step(st, sf);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st, sf);
        }
        __syncthreads();
        if (row + kKvcStep < r_end) load_step(st, sf);
        auto step = [&](auto bufc, int row0) __attribute__((always_inline)) {
            constexpr int BUF = decltype(bufc)::value;
            kvc_stage_slow_reader((row0 - r_begin) / kKvcStep, wave);
            if (active) compute_step(bufc, row0);
            if (row0 + kKvcStep < r_end) {
#if FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                kvc_stage_slow_writer((row0 - r_begin) / kKvcStep, wave);
                store_step(std::integral_constant<int, BUF ^ 1>{}, st, sf);
#if !FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                if (row0 + 2 * kKvcStep < r_end) load_step(st, sf);
            }
        };
        for (; row < r_end; row += 2 * kKvcStep) {
            step(std::integral_constant<int, 0>{}, row);
            if (row + kKvcStep < r_end) step(std::integral_constant<int, 1>{}, row + kKvcStep);
        }
    }

    // ---- epilogue: the lane's key, columns 16 c + 4 g .. + 3 of every block c; a key no row sees writes zeros -------------------------------------
    if (!active || !key_ok) return;
    const float sc = p.scale;
    char* dkrow = (char*)p.dk_ptr + 2 * (key_off(p.dk) + 4 * g);
    char* dvrow = (char*)p.dv_ptr + 2 * (key_off(p.dv) + 4 * g);
    static_for<0, NKN + NKR>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        *(u32x2*)(dkrow + 32 * ci) = u32x2{LP<T>::pack2(dk[ci][0] * sc, dk[ci][1] * sc), LP<T>::pack2(dk[ci][2] * sc, dk[ci][3] * sc)};
    });
    static_for<0, NO>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        *(u32x2*)(dvrow + 32 * ci) = u32x2{LP<T>::pack2(dv[ci][0], dv[ci][1]), LP<T>::pack2(dv[ci][2], dv[ci][3])};
    });
}

// Two workgroups per compute unit for both kernels (256 registers a lane): the register and LDS counts the compiler reports are in DESIGN.md 3.18.
template <typename T, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_bwd_mla_prefill_dq_kernel(const MlaPrefillBwdParams p) {
    mla_prefill_dq<T, CAUSAL, PACKED>(p);
}

template <typename T, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_bwd_mla_prefill_dkdv_kernel(const MlaPrefillBwdParams p) {
    mla_prefill_dkdv<T, CAUSAL, PACKED>(p);
}

}  // namespace

// p as the C ABI filled it; the tiles (dense) or tile slots (packed) of each launch are counted here.  phases: 1 = dQ (and D), 2 = dK / dV, 3 = both, in
// that order on stream s.  dQ grid = b x h_k x row tiles (dense), slots x h_k (packed); dK/dV grid = b x h_k x key tiles (dense), key slots x h_k (packed).
hipError_t launch_bwd_mla_prefill(MlaPrefillBwdParams p, int dtype, int phases, hipStream_t s) {
    const bool packed = p.cu_q != nullptr;
    const int64_t rows = packed ? p.total_q : p.seqlen_q, keys = packed ? p.total_k : p.seqlen_k;
    if (p.b <= 0 || rows <= 0) return hipSuccess;
    const int64_t tiles = (rows * p.h_ratio + kMbRowsDq - 1) / kMbRowsDq, ktiles = (keys + kMbRows - 1) / kMbRows;
    const int64_t per_head = packed ? tiles + p.b : tiles * p.b, kper_head = packed ? ktiles + p.b : ktiles * p.b;
    if (per_head * p.h_k >= ((int64_t)1 << 31) || kper_head * p.h_k >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        if (phases & 1) {
            if (packed) p.slots = (int32_t)per_head;
            else p.n_row_tiles = (int32_t)tiles;
            auto* kernel = p.is_causal ? (packed ? fa_bwd_mla_prefill_dq_kernel<T, true, true> : fa_bwd_mla_prefill_dq_kernel<T, true, false>)
                                       : (packed ? fa_bwd_mla_prefill_dq_kernel<T, false, true> : fa_bwd_mla_prefill_dq_kernel<T, false, false>);
            hipLaunchKernelGGL(kernel, dim3((unsigned)(per_head * p.h_k)), dim3(kKvcThreads), 0, s, p);
        }
        if ((phases & 2) && keys > 0) {
            if (packed) p.slots = (int32_t)kper_head;
            else p.n_row_tiles = (int32_t)ktiles;
            auto* kernel = p.is_causal ? (packed ? fa_bwd_mla_prefill_dkdv_kernel<T, true, true> : fa_bwd_mla_prefill_dkdv_kernel<T, true, false>)
                                       : (packed ? fa_bwd_mla_prefill_dkdv_kernel<T, false, true> : fa_bwd_mla_prefill_dkdv_kernel<T, false, false>);
            hipLaunchKernelGGL(kernel, dim3((unsigned)(kper_head * p.h_k)), dim3(kKvcThreads), 0, s, p);
        }
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
