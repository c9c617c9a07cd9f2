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
#include "fa_mla_prefill_tile.hpp"

#ifndef FA_MLAPB_WAVE_ROWS
#define FA_MLAPB_WAVE_ROWS 16
#endif

namespace fa {

namespace {

static_assert(FA_MLAPB_WAVE_ROWS == 16 || FA_MLAPB_WAVE_ROWS == 32, "a wave of the dQ kernel owns one or two 16-row query column blocks");
constexpr int kMbQB = FA_MLAPB_WAVE_ROWS / kKvcRows;        // query column blocks of a wave of the dQ kernel
constexpr int kMbRowsDq = kKvcWaves * FA_MLAPB_WAVE_ROWS;   // packed query rows of a dQ workgroup
constexpr int kMbRows = kKvcWaves * kKvcRows;       // keys of a dK/dV workgroup
constexpr int kMbRowF = kKvcStep * 4;               // dK/dV: behind the images of a stage, the step's 32 lse values, then its 32 D values

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
    using Lds = MlapLds<>;              // K | K rope | V
    constexpr int NC = kMlapNC;         // 16x16x32 MFMAs per 16 keys of S^T
    constexpr int NV = kMlapDV / 32;    // ... of dP^T
    constexpr int NQN = kMlapDN / 16;   // dQ^T blocks of 16 columns fed from the wide K image
    constexpr int NQR = kMlapDR / 16;   // ... from the narrow one
    constexpr int QB = kMbQB;
    __shared__ __attribute__((aligned(16))) char smem[Lds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    MlapSeq<PACKED> seq;
    if (!seq.template find_tile<kMbRowsDq, false>(p)) return;
    seq.read_bounds(p);
    if (PACKED && ((int)seq.q0 < 0 || seq.q0 + seq.sq > p.total_q)) return;     // rows outside q / o / dout / dq: not served
    seq.template cut<false>(p);
    const int tile = seq.tile, kvh = seq.kvh, sq = seq.sq, L = seq.L;
    const int rows_tile = sq * p.h_ratio;
    const int k_end = seq.template tile_key_end<kMbRowsDq, CAUSAL>(p.h_ratio);
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
        const char* qrow = (const char*)p.q_ptr + 2 * seq.row_off(p.q, hq[qb], t[qb]);
        const char* orow = (const char*)p.o_ptr + 2 * seq.row_off(p.o, hq[qb], t[qb]);
        const char* dorow = (const char*)p.do_ptr + 2 * seq.row_off(p.dout, hq[qb], t[qb]);
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
            lse2[qb] = p.lse_ptr[seq.row_index(p, hq[qb], t[qb])] * kLog2e;
            if (g == 0) p.dsum_ptr[seq.row_index(p, hq[qb], t[qb])] = dsum[qb];
        }
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
        const MlapImages im = mlap_images<Lds, decltype(bufc)::value>(smem);
        f32x4 s[QB][2], dp[QB][2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, QB>([&](auto qq) {
                s[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f};
                dp[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            });
            mlap_scores<T, b>(im, n16, g, qf, s);
            mlap_rows_mfma<T, kMlapDV, 0, b>(im.vimg, n16, g, dof, dp);
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
            dsf[qb] = pack8<T>(ds);
        });
        static_for<0, NQN>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const u32x4 kt = tr_frag<kMlapDN>(im.nimg, ci, g, q4, p4);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                dq[qb][ci] = LP<T>::mfma16(kt, dsf[qb], dq[qb][ci]);
            });
        });
        // the 64-wide image, read transposed: the same 4-row x 16-column blocks, eight 16-byte slots a row
        static_for<0, NQR>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const u32x4 kt = tr_frag<kMlapDR>(im.rimg, ci, g, q4, p4);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                dq[qb][NQN + ci] = LP<T>::mfma16(kt, dsf[qb], dq[qb][NQN + ci]);
            });
        });
    };

    // ---- the 32-key steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp) ---------------------------------------
    // k_end is the workgroup's: every wave meets the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the three images are read by compute_step alone,
    // as MFMA operands (mlap_scores, mlap_rows_mfma, tr_frag): what comes out of them are scores, dP and dQ, which reach compares of VALUES, exponentials
    // and the stores of dQ - every address (lds_tile_off of lane constants, row_off / row_index of the lane's row, the sequence's base rows from
    // cu_seqlens), every index and every loop bound comes from the parameters.  A stale image gives wrong numbers.
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

    // ---- epilogue: the lane's row, columns 16 c + 4 g .. + 3 of every block c; a dead row (or no keys at all) writes zeros -------------------------
    if (!active) return;
    const float sc = p.scale;
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        if (!row_ok[qb]) return;
        char* dqrow = (char*)p.dq_ptr + 2 * (seq.row_off(p.dq, hq[qb], t[qb]) + 4 * g);
        static_for<0, NQN + NQR>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            mlap_store_block<T>(dqrow, ci, dq[qb][ci], sc);
        });
    });
}

// =============================================================================================================================================
// dK / dV
// =============================================================================================================================================
template <typename T, bool CAUSAL, bool PACKED>
FA_DEV void mla_prefill_dkdv(const MlaPrefillBwdParams& p) {
    using Lds = MlapLds<2 * kMbRowF>;   // Q | Q rope | dO | lse, D
    constexpr int NC = kMlapNC, NV = kMlapDV / 32;
    constexpr int NKN = kMlapDN / 16, NKR = kMlapDR / 16, NO = kMlapDV / 16;       // dK^T blocks from the wide / narrow Q image, dV^T blocks
    __shared__ __attribute__((aligned(16))) char smem[Lds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the tiles are key tiles: the keys are what this kernel writes, so a key range outside k / v is not served, and the query rows are cut at the last row of q
    MlapSeq<PACKED> seq;
    if (!seq.template find_tile<kMbRows, true>(p)) return;
    seq.read_bounds(p);
    if (PACKED && ((int)seq.k0 < 0 || seq.k0 + seq.L > p.total_k)) return;
    seq.template cut<true>(p);
    const int tile = seq.tile, bidx = seq.bidx, kvh = seq.kvh, sq = seq.sq, L = seq.L;
    const int64_t q0 = seq.q0, k0 = seq.k0;
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
    u32x4 kf[1][NC], vf[1][NV];       // ([1]: one B operand for mlap_rows_mfma)
    {
        const char* krow = (const char*)p.k_ptr + 2 * key_off(p.k);
        const char* vrow = (const char*)p.v_ptr + 2 * key_off(p.v);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            kf[0][ci] = key_ok ? *(const u32x4*)(krow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
        static_for<0, NV>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            vf[0][ci] = key_ok ? *(const u32x4*)(vrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    }

    // ---- staging: what this lane loads in a step ------------------------------------------------------------------------------------------------
    // loads 0, 1: packed row 16 j + 4 w + lane / 16 of the step, 16-byte slot lane % 16 of Q's no-rope columns; load 2: row 8 w + lane / 8, slot 16 + lane % 8
    // (the rope columns); loads 3, 4: the dO rows of loads 0, 1.  The lanes of slot 0 also load the lse and D values of their two rows.  A row past the
    // group's last one is not loaded: zeros go to the images.  (t, j) of the lane's three rows are kept and advanced by a step at a time.
    const MlapLane ln(wave, lane);
    const int wrow = ln.wrow, wslot = ln.wslot, rrow = ln.rrow, rslot = ln.rslot;
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
    auto load_step = [&](u32x4 (&st)[kMlapNL], float (&sf)[4]) __attribute__((always_inline)) {
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
                const int64_t ri = seq.row_index(p, hq, st_t[i]);
                sf[2 * i] = okf ? p.lse_ptr[ri] : 0.f;
                sf[2 * i + 1] = okf ? p.dsum_ptr[ri] : 0.f;
            } else {
                st[2] = ok ? *(const u32x4*)(qrow + 2 * kMlapDN + 16 * rslot) : u32x4{0u, 0u, 0u, 0u};
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
    auto store_step = [&](auto bufc, const u32x4 (&st)[kMlapNL], const float (&sf)[4]) __attribute__((always_inline)) {
        const MlapImages im = mlap_images<Lds, decltype(bufc)::value>(smem);
        FA_LDS float* frow = (FA_LDS float*)im.tail;
        mlap_store_step(im, ln, st, [&](auto jj) {
            constexpr int j = decltype(jj)::value;
            if (wslot == 0) {
                frow[16 * j + wrow] = sf[2 * j];
                frow[kKvcStep + 16 * j + wrow] = sf[2 * j + 1];
            }
        });
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
        const MlapImages im = mlap_images<Lds, decltype(bufc)::value>(smem);
        const FA_LDS char* frow = im.tail;
        f32x4 s[1][2], dp[1][2], lse4[2], d4[2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            s[0][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[0][b] = f32x4{0.f, 0.f, 0.f, 0.f};
            mlap_scores<T, b>(im, n16, g, kf, s);
            mlap_rows_mfma<T, kMlapDV, 0, b>(im.vimg, n16, g, vf, dp);
            lse4[b] = *(const FA_LDS f32x4*)(frow + 4 * (16 * b + 4 * g));
            d4[b] = *(const FA_LDS f32x4*)(frow + 4 * (kKvcStep + 16 * b + 4 * g));
        });
        // hidden pairs (and rows past the group): P = 0 and dS = 0 by selection, whatever exp gives there
        float pe[8], ds[8];
        static_for<0, 8>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const int r = row0 + 16 * (j >> 2) + 4 * g + (j & 3);
            const bool vis = r >= rmin && r < rows_total;
            const float e = fast_exp2(__builtin_fmaf(s[0][j >> 2][j & 3], c, -lse4[j >> 2][j & 3] * kLog2e));
            pe[j] = vis ? e : 0.f;
            ds[j] = vis ? e * (dp[0][j >> 2][j & 3] - d4[j >> 2][j & 3]) : 0.f;
        });
        const u32x4 pf = pack8<T>(pe), dsf = pack8<T>(ds);
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            dv[ci] = LP<T>::mfma16(tr_frag<kMlapDV>(im.vimg, ci, g, q4, p4), pf, dv[ci]);
        });
        static_for<0, NKN>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            dk[ci] = LP<T>::mfma16(tr_frag<kMlapDN>(im.nimg, ci, g, q4, p4), dsf, dk[ci]);
        });
        static_for<0, NKR>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            dk[NKN + ci] = LP<T>::mfma16(tr_frag<kMlapDR>(im.rimg, ci, g, q4, p4), dsf, dk[NKN + ci]);
        });
    };

    // ---- the 32-row steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp with rows in the place of keys) --------
    // load_step is called once per step, in order, so the rows it keeps advance with the loop.  r_begin and r_end are the workgroup's: every wave meets
    // the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the three images and the lse / D rows are read
    // by compute_step alone, as MFMA operands (mlap_scores, mlap_rows_mfma, tr_frag) and as the operands of an exponential and a subtraction: what comes
    // out of them are scores, P, dS, dK and dV, which reach the stores of VALUES - every address (lds_tile_off of lane constants, the (t, head) rows of
    // load_step, key_off of the lane's key, the base rows from cu_seqlens), every index, every visibility compare (rmin, rows_total) and every loop bound
    // comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[kMlapNL];
        float sf[4];
        int row = r_begin;
        if (row < r_end) {
            load_step(st, sf);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st, sf);
        }
        __syncthreads();
        if (row + kKvcStep < r_end) load_step(st, sf);
        auto load = [&](auto, int) __attribute__((always_inline)) { load_step(st, sf); };
        auto store = [&](auto bufc) __attribute__((always_inline)) { store_step(bufc, st, sf); };
        auto compute = [&](auto bufc, int row0) __attribute__((always_inline)) { compute_step(bufc, row0); };
        for (; row < r_end; row += 2 * kKvcStep) {
            kvc_stage_step(std::integral_constant<int, 0>{}, row, r_begin, r_end, wave, active, load, store, compute);
            if (row + kKvcStep < r_end) kvc_stage_step(std::integral_constant<int, 1>{}, row + kKvcStep, r_begin, r_end, wave, active, load, store, compute);
        }
    }

    // ---- epilogue: the lane's key, columns 16 c + 4 g .. + 3 of every block c; a key no row sees writes zeros -------------------------------------
    if (!active || !key_ok) return;
    const float sc = p.scale;
    char* dkrow = (char*)p.dk_ptr + 2 * (key_off(p.dk) + 4 * g);
    char* dvrow = (char*)p.dv_ptr + 2 * (key_off(p.dv) + 4 * g);
    static_for<0, NKN + NKR>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        mlap_store_block<T>(dkrow, ci, dk[ci], sc);
    });
    static_for<0, NO>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        mlap_store_block<T>(dvrow, ci, dv[ci], 1.f);
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
            auto* kernel = mlap_select(p.is_causal, packed, [](auto c, auto k) { return fa_bwd_mla_prefill_dq_kernel<T, decltype(c)::value, decltype(k)::value>; });
            hipLaunchKernelGGL(kernel, dim3((unsigned)(per_head * p.h_k)), dim3(kKvcThreads), 0, s, p);
        }
        if ((phases & 2) && keys > 0) {
            if (packed) p.slots = (int32_t)kper_head;
            else p.n_row_tiles = (int32_t)ktiles;
            auto* kernel = mlap_select(p.is_causal, packed, [](auto c, auto k) { return fa_bwd_mla_prefill_dkdv_kernel<T, decltype(c)::value, decltype(k)::value>; });
            hipLaunchKernelGGL(kernel, dim3((unsigned)(kper_head * p.h_k)), dim3(kKvcThreads), 0, s, p);
        }
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
