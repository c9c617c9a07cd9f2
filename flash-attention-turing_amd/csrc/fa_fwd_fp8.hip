// fa_fwd_fp8.hip — dense attention forward over FP8 (OCP e4m3) q, k and v (fa_run_fp8_fwd): head_dim 128, dense and packed, both matrix products on
// v_mfma_f32_16x16x128_f8f6f4.
//
//   The operand of that MFMA, as fa_mla_indexer.hpp states it (idx_mfma_e4m3): lane l = 16 g + n16 holds 32 codes of row n16, registers 0 .. 3 the 16 bytes
//   "lo", registers 4 .. 7 the 16 bytes "hi"; byte position i of a lane group's 32 is the same contraction index in A and in B.  C / D: lane = column n16,
//   register r = row 4 g + r.
//   * Work split.  A workgroup of four waves serves 64 packed query rows (row r = t * (h / h_k) + j, the packing of fa_fwd_mla_prefill.hip: the GQA heads of a
//     KV head share the staged keys) of one (sequence, KV head); a wave owns one 16-row column block, a lane one query row with private m / l.  All four
//     waves walk the same 128-key steps under the step protocol of fa_kvcache_stage.hpp (positions are counted in units of 4 keys, so that a step is
//     kKvcStep of them).  234 - 239 VGPRs, no scratch.  (A 128-row workgroup, two column blocks a wave, was tried and is not kept: DESIGN.md 3.25.)
//   * S^T = K Q^T.  A = 16 keys x 128 codes from the K image (lo = bytes 16 g .. of the key's row, hi = bytes 64 + 16 g ..), B = Q^T in registers for the whole
//     call (8 registers, the same bytes of the query's row).  One MFMA covers the whole head_dim: 8 per wave and step.  The lane then holds the
//     scores of keys 16 t + 4 g + r (t = 0 .. 7 the MFMA, r = 0 .. 3 the register) for its query.
//   * Softmax on those registers: masking by key index (skipped on steps that lie below every row's limit), the maximum and sum over the lane's 32 scores and
//     the four lane groups (two permlane steps, the sum only in the epilogue), p = exp2((s - m) * c) in fp32 with c = softmax_scale * q_descale * k_descale * log2 e
//     (s - m first: a row with one visible key has p = 1 exactly), l += p in fp32, the O^T rescale skipped when no maximum of the wave moved.
//   * P never goes through LDS: v_cvt_pk_fp8_f32 packs the four 256 p of MFMA t into dword t (byte r = key 16 t + 4 g + r); dwords 0 .. 3 are lo, 4 .. 7 hi of
//     the B operand of O^T += V^T P^T.  256 p: e4m3 then rounds to nearest down to p = 2^-18 (its smallest subnormal is 2^-9) where p itself is flushed below
//     2^-10, and 256 is exact to undo.
//   * V^T.  The A operand of that product is, for value column d and lane group g, the bytes V[16 t + 4 g + r][d] in the order (t, r): bytes along the KEY
//     axis.  The transpose is done once per workgroup while staging: thread (dq = tid % 32, G = (tid / 32) % 4, T = tid / 128) loads the dwords V[16 (4 T + tt) +
//     4 G + r][4 dq .. 4 dq + 3] (tt, r = 0 .. 3: 16 four-byte loads, a wave-wide load covers two whole 128-byte rows), transposes each 4 x 4 byte block with
//     eight v_perm_b32, and writes for each of its four columns d = 4 dq + jj ONE 16-byte slot: row d, slot G + 4 T of the V^T image = keys (tt, r) in order.
//     The consumer's operand is slot g (lo: t = 0 .. 3) and slot 4 + g (hi: t = 4 .. 7) of row 16 c + n16: the read pattern of the K image.
//   * LDS.  A stage is the K image (128 key rows x 128 B) and the V^T image (128 column rows x 128 B): 32 KB, two stages 64 KB, two workgroups a compute unit.
//     Both images use f8_tile_off: physical slot ps = slot ^ ((row >> 1) & 7) ^ ((row >> 4) & 1), byte offset 128 row + 16 ps.  Bank arithmetic
//     (ds_read_b128: bank slot of byte address a is (a / 16) % 16 within a 256-byte bank row, a read is served in four groups of 16 lanes {0-3, 12-15, 20-27},
//     {4-11, 16-19, 28-31} and the same + 32; two 128-byte rows share a bank row, so the bank slot of (row, ps) is 8 (row & 1) + ps): a fragment read takes slot
//     g (or 4 + g) of rows 16 c + n16.  (row >> 4) & 1 = c & 1 is one constant of the instruction, a bijection of ps.  A group holds all 16 rows, eight of
//     them at slot s with row >> 1 in {0, 1, 6, 7} and eight at slot s ^ 1 with row >> 1 in {2, 3, 4, 5} (or the other way round); both sets are closed under
//     x -> x ^ 1, so the eight values of row >> 1 give eight different ps and the row parity the sixteenth part: 16 different bank slots.  Writes (ds_write_b128:
//     groups of 8 consecutive lanes, 128 bytes a pass): K - the 8 lanes write the 8 slots of one row; V^T - the 8 lanes dq = 8 a + i write one slot of rows
//     d = 32 a + 4 i + jj: (d >> 1) & 7 = (2 i + (jj >> 1)) & 7 separates i mod 4 in bits 1 .. 2 and (d >> 4) & 1 = i >> 2 separates i from
//     i + 4 in bit 0: eight different ps.  By this arithmetic no access of the key loop conflicts; the service groups are the
//     ones fa_mla_indexer_prefill_fp8q.hip states: the arithmetic is derived, and the one counter run made (SQ_LDS_BANK_CONFLICT = 0 over a 16k
//     non-causal call, profiles/fp8_fwd_pmc.log) agrees with it.
//   * Epilogue: l over the four lane groups, out = (O^T / (256 l)) * v_descale in fp32, rounded once; a lane's four columns 16 c + 4 g .. of two neighbouring
//     blocks are exchanged with the neighbouring lane group (v_permlane16_swap) so that every lane stores 16 bytes.  LSE = m * scale + ln l, one fp32 a row.
//   Kernels of this file: 8 ((fp16, bf16) output x (causal, not) x (dense, packed)).
#include "fa_fwd_fp8.hpp"
#include "fa_mla_indexer.hpp"
#include "fa_mla_prefill_tile.hpp"

namespace fa {

namespace {

constexpr int kF8D = 128;                                   // head_dim = bytes of a row
constexpr int kF8Step = 128;                                // keys of a step
constexpr int kF8Unit = kF8Step / kKvcStep;                 // keys per position unit of kvc_stage_step
constexpr int kF8Rows = kKvcWaves * kKvcRows;               // packed query rows of a workgroup: one 16-row column block a wave
constexpr int kF8Image = kF8Step * kF8D;                    // 16 KB: the K image, and the V^T image
constexpr int kF8Stage = 2 * kF8Image;
constexpr float kF8PScale = 256.f;

// byte offset of 16-byte slot `slot` (0 .. 7) of row `row` (0 .. 127) in an image: the layout derived in the file header
FA_DEV uint32_t f8_tile_off(uint32_t row, uint32_t slot) { return row * (uint32_t)kF8D + ((slot ^ ((row >> 1) & 7u) ^ ((row >> 4) & 1u)) << 4); }

// 4 x 4 bytes: in[r] byte j -> out[j] byte r
FA_DEV void f8_transpose4(const uint32_t* in, uint32_t* out) {
    const uint32_t t0 = __builtin_amdgcn_perm(in[1], in[0], 0x05010400u), t1 = __builtin_amdgcn_perm(in[1], in[0], 0x07030602u);
    const uint32_t u0 = __builtin_amdgcn_perm(in[3], in[2], 0x05010400u), u1 = __builtin_amdgcn_perm(in[3], in[2], 0x07030602u);
    out[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

// four weights -> four e4m3 codes of 256 p, byte r = p[r]
FA_DEV uint32_t f8_pack4(float p0, float p1, float p2, float p3) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(p0 * kF8PScale, p1 * kF8PScale, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(p2 * kF8PScale, p3 * kF8PScale, lo, true);
}

template <typename T, bool CAUSAL, bool PACKED>
FA_DEV void fp8_fwd_attn(const Fp8FwdParams& p) {
    constexpr int NT = kF8Step / 16;        // MFMAs of S^T per step
    constexpr int NO = kF8D / 16;           // O^T blocks of 16 columns
    __shared__ __attribute__((aligned(16))) char smem[2 * kF8Stage];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    MlapSeq<PACKED> seq;
    if (!seq.template find_tile<kF8Rows, false>(p)) return;
    seq.read_bounds(p);
    if (PACKED && ((int)seq.q0 < 0 || seq.q0 + seq.sq > p.total_q)) return;     // rows outside q / o: not served
    seq.template cut<false>(p);
    const int tile = seq.tile, kvh = seq.kvh, sq = seq.sq, L = seq.L;
    const int rows_tile = sq * p.h_ratio;
    const int k_end = seq.template tile_key_end<kF8Rows, CAUSAL>(p.h_ratio);
    const float kd = p.kd_ptr != nullptr ? p.kd_ptr[(int64_t)seq.bidx * p.kd_batch + (int64_t)kvh * p.kd_head] : 1.0f;
    const float vd = p.vd_ptr != nullptr ? p.vd_ptr[(int64_t)seq.bidx * p.vd_batch + (int64_t)kvh * p.vd_head] : 1.0f;

    // ---- this lane's query row: Q^T for the whole call, the scale of its head, its visible-key limit ----------------------------------------------------
    const int wrow0 = tile * kF8Rows + wave * kKvcRows;
    const bool active = wrow0 < rows_tile;      // (wave-uniform) false: staging and barriers only
    const int pr = wrow0 + n16;
    const bool row_ok = pr < rows_tile;
    const int t = row_ok ? pr / p.h_ratio : 0;
    const int hq = kvh * p.h_ratio + (row_ok ? pr - t * p.h_ratio : 0);
    int lim = row_ok ? L : 0;
    if (CAUSAL && row_ok) lim = min(L, L - sq + t + 1);
    const float qd = p.qd_ptr != nullptr ? p.qd_ptr[(int64_t)seq.bidx * p.qd_batch + (int64_t)hq * p.qd_head] : 1.0f;
    const float sc = p.scale * qd * kd;
    const float c = sc * kLog2e;
    const char* qrow = (const char*)p.q_ptr + seq.row_off(p.q, hq, t);
    u32x4 qf[2];
    static_for<0, 2>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        qf[j] = row_ok ? *(const u32x4*)(qrow + 16 * g + 64 * j) : u32x4{0u, 0u, 0u, 0u};
    });
    // the smallest limit of the wave's rows (its first row's; wave-uniform): a step that ends at or below it needs no mask
    int lim_lo = L;
    if (CAUSAL) lim_lo = min(L, L - sq + wrow0 / p.h_ratio + 1);
    lim_lo = __builtin_amdgcn_readfirstlane(lim_lo);

    // ---- staging: descriptors that end at the sequence's last row (rows at or past it read as zeros, their scores are masked) -----------------------------
    const uint32_t krow_b = (uint32_t)p.k.row, vrow_b = (uint32_t)p.v.row;
    const char* kbase = uniform_ptr((const char*)p.k_ptr + ((PACKED ? seq.k0 * p.k.row : (int64_t)seq.bidx * p.k.batch) + (int64_t)kvh * p.k.head));
    const char* vbase = uniform_ptr((const char*)p.v_ptr + ((PACKED ? seq.k0 * p.v.row : (int64_t)seq.bidx * p.v.batch) + (int64_t)kvh * p.v.head));
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * krow_b + kF8D : 0u);
    const rsrc_t vrs = make_rsrc(vbase, L > 0 ? (uint32_t)(L - 1) * vrow_b + kF8D : 0u);
    const int krow = tid >> 3, kslot = tid & 7;                     // K: rows 32 i + krow, slot kslot
    const int vdq = tid & 31, vG = (tid >> 5) & 3, vT = tid >> 7;   // V: keys 16 (4 vT + tt) + 4 vG + r, bytes 4 vdq ..

    auto load_step = [&](int key0, u32x4 (&kst)[4], uint32_t (&vst)[16]) __attribute__((always_inline)) {
        static_for<0, 4>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            kst[i] = buf_load16(krs, (uint32_t)min(key0 + 32 * i + krow, L) * krow_b + 16u * kslot);
        });
        static_for<0, 16>([&](auto ii) {
            constexpr int i = decltype(ii)::value;      // i = 4 tt + r
            vst[i] = __builtin_amdgcn_raw_buffer_load_b32(vrs, (uint32_t)min(key0 + 16 * (4 * vT + (i >> 2)) + 4 * vG + (i & 3), L) * vrow_b + 4u * vdq, 0, 0);
        });
    };
    auto store_step = [&](auto bufc, const u32x4 (&kst)[4], const uint32_t (&vst)[16]) __attribute__((always_inline)) {
        FA_LDS char* kimg = (FA_LDS char*)smem + decltype(bufc)::value * kF8Stage;
        FA_LDS char* vimg = kimg + kF8Image;
        static_for<0, 4>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            *(FA_LDS u32x4*)(kimg + f8_tile_off((uint32_t)(32 * i + krow), (uint32_t)kslot)) = kst[i];
        });
        uint32_t vt[4][4];
        static_for<0, 4>([&](auto tt) { f8_transpose4(&vst[4 * decltype(tt)::value], vt[decltype(tt)::value]); });
        static_for<0, 4>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            *(FA_LDS u32x4*)(vimg + f8_tile_off((uint32_t)(4 * vdq + j), (uint32_t)(vG + 4 * vT))) = u32x4{vt[0][j], vt[1][j], vt[2][j], vt[3][j]};
        });
    };

    // fragment reads: block c of an image is rows 16 c + n16, slot g (lo) and 4 + g (hi).  Blocks c and c + 2 lie 4096 bytes apart with the same swizzle, so
    // four offsets (block parity x lo / hi) and immediates address every fragment of both images and both stages
    uint32_t foff[2][2];
    static_for<0, 4>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        foff[i >> 1][i & 1] = f8_tile_off((uint32_t)(16 * (i >> 1) + n16), (uint32_t)(4 * (i & 1) + g));
    });

    f32x4 oacc[NO];
    static_for<0, NO>([&](auto cc) { oacc[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });
    float m_run = kNegBig, l_run = 0.f;

    // one 128-key step of this wave's rows over the images of stage BUF; MASK: some key of the step lies at or past a row's limit
    auto compute_masked = [&](auto bufc, int key0, auto maskc) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(maskc)::value;
        const FA_LDS char* kimg = (const FA_LDS char*)smem + decltype(bufc)::value * kF8Stage;
        const FA_LDS char* vimg = kimg + kF8Image;
        f32x4 s[NT];
        static_for<0, NT>([&](auto tt) {
            constexpr int ti = decltype(tt)::value;
            const u32x4 klo = *(const FA_LDS u32x4*)(kimg + foff[ti & 1][0] + 2048 * (ti & ~1));
            const u32x4 khi = *(const FA_LDS u32x4*)(kimg + foff[ti & 1][1] + 2048 * (ti & ~1));
            s[ti] = idx_mfma_e4m3(klo, khi, qf[0], qf[1], f32x4{0.f, 0.f, 0.f, 0.f});
        });
        float mx = -INFINITY;
        static_for<0, NT>([&](auto tt) {
            constexpr int ti = decltype(tt)::value;
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                if constexpr (MASK) s[ti][r] = key0 + 16 * ti + 4 * g + r < lim ? s[ti][r] : -INFINITY;
                mx = fmaxf(mx, s[ti][r]);
            });
        });
        mx = max_four_groups(mx);
        const float m_new = fmaxf(m_run, mx);
        const float alpha = fast_exp2((m_run - m_new) * c);
        const bool moved = m_new > m_run;
        m_run = m_new;
        float ps = 0.f;
        uint32_t pw[NT];
        static_for<0, NT>([&](auto tt) {
            constexpr int ti = decltype(tt)::value;
            float pe[4];
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                pe[r] = fast_exp2((s[ti][r] - m_new) * c);
                ps += pe[r];
            });
            pw[ti] = f8_pack4(pe[0], pe[1], pe[2], pe[3]);
        });
        l_run = l_run * alpha + ps;
        const u32x4 plo = u32x4{pw[0], pw[1], pw[2], pw[3]}, phi = u32x4{pw[4], pw[5], pw[6], pw[7]};
        // alpha = 1 in every lane whose maximum stayed: skipping the multiplication changes no bit
        if (__builtin_amdgcn_ballot_w64(moved) != 0) {
            static_for<0, NO>([&](auto cc) { oacc[decltype(cc)::value] *= alpha; });
        }
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const u32x4 vlo = *(const FA_LDS u32x4*)(vimg + foff[ci & 1][0] + 2048 * (ci & ~1));
            const u32x4 vhi = *(const FA_LDS u32x4*)(vimg + foff[ci & 1][1] + 2048 * (ci & ~1));
            oacc[ci] = idx_mfma_e4m3(vlo, vhi, plo, phi, oacc[ci]);
        });
    };
    auto compute_step = [&](auto bufc, int key0) __attribute__((always_inline)) {
        if (key0 + kF8Step <= lim_lo) compute_masked(bufc, key0, std::false_type{});
        else compute_masked(bufc, key0, std::true_type{});
    };

    // ---- the 128-key steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp, positions in units of kF8Unit keys) -------
    // n_end is the workgroup's: every wave meets the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the two images are read by compute_step alone, as
    // MFMA operands: what comes out of them are scores and O, which reach compares, exponentials, conversions and stores of VALUES - every address
    // (f8_tile_off of lane constants, row_off / row_index of the lane's row, the sequence's base rows from cu_seqlens), every index and every loop bound comes
    // from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 kst[4];
        uint32_t vst[16];
        const int n_end = k_end > 0 ? (k_end + kF8Step - 1) / kF8Step * kKvcStep : 0;
        int pos = 0;
        if (pos < n_end) {
            load_step(0, kst, vst);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, kst, vst);
        }
        __syncthreads();
        if (pos + kKvcStep < n_end) load_step(kF8Step, kst, vst);
        auto load = [&](auto, int pos0) __attribute__((always_inline)) { load_step(pos0 * kF8Unit, kst, vst); };
        auto store = [&](auto bufc) __attribute__((always_inline)) { store_step(bufc, kst, vst); };
        auto compute = [&](auto bufc, int pos0) __attribute__((always_inline)) { compute_step(bufc, pos0 * kF8Unit); };
        for (; pos < n_end; pos += 2 * kKvcStep) {
            kvc_stage_step(std::integral_constant<int, 0>{}, pos, 0, n_end, wave, active, load, store, compute);
            if (pos + kKvcStep < n_end) kvc_stage_step(std::integral_constant<int, 1>{}, pos + kKvcStep, 0, n_end, wave, active, load, store, compute);
        }
    }

    // ---- epilogue: the lane's row.  Block pair (2 k, 2 k + 1): the lane holds columns 32 k + 4 g .. + 3 and 32 k + 16 + 4 g .. + 3; after the exchange with
    // lane group g ^ 1 an even group holds columns 32 k + 4 g .. + 7 and an odd one 32 k + 16 + 4 (g - 1) .. + 7: 16 bytes a store ----------------------------
    if (!active) return;
    const float lsum = sum_four_groups(l_run);
    // dead = saw no key (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math
    const bool live = !(lsum == 0.f);
    const float inv = live ? 1.0f / (kF8PScale * lsum) : 0.f;
    const float lse = live ? m_run * sc + logf(lsum) : 0.f;
    char* orow = (char*)p.o_ptr + 2 * (seq.row_off(p.o, hq, t) + ((g & 1) ? 16 + 4 * (g - 1) : 4 * g));
    static_for<0, NO / 2>([&](auto kk) {
        constexpr int k2 = decltype(kk)::value;
        const f32x4 &a = oacc[2 * k2], &b = oacc[2 * k2 + 1];
        // (v_permlane16_swap: the odd 16-lane rows of the first operand change places with the even rows of the second)
        const auto r0 = __builtin_amdgcn_permlane16_swap(LP<T>::pack2(a[0] * inv * vd, a[1] * inv * vd), LP<T>::pack2(b[0] * inv * vd, b[1] * inv * vd), false, false);
        const auto r1 = __builtin_amdgcn_permlane16_swap(LP<T>::pack2(a[2] * inv * vd, a[3] * inv * vd), LP<T>::pack2(b[2] * inv * vd, b[3] * inv * vd), false, false);
        if (row_ok) *(u32x4*)(orow + 64 * k2) = u32x4{(uint32_t)r0[0], (uint32_t)r1[0], (uint32_t)r0[1], (uint32_t)r1[1]};
    });
    if (row_ok && g == 0) p.lse_ptr[seq.row_index(p, hq, t)] = lse;
}

// Two workgroups per compute unit: 64 KB of LDS a workgroup, and by count a lane holds 8 registers of Q^T, 32 of O^T, 32 of scores and 8 of P next to 32 of
// staging.
template <typename T, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_fp8_kernel(const Fp8FwdParams p) {
    fp8_fwd_attn<T, CAUSAL, PACKED>(p);
}

}  // namespace

// p as the C ABI filled it; the tiles (dense) or tile slots (packed) are counted here.  grid = b x h_k x tiles (dense), slots x h_k (packed)
hipError_t launch_fwd_fp8(Fp8FwdParams p, int dtype, hipStream_t s) {
    const bool packed = p.cu_q != nullptr;
    const int64_t rows = packed ? p.total_q : p.seqlen_q;
    if (p.b <= 0 || rows <= 0) return hipSuccess;
    const int64_t tiles = (rows * p.h_ratio + kF8Rows - 1) / kF8Rows;
    const int64_t per_head = packed ? tiles + p.b : tiles * p.b;
    const int64_t grid = per_head * p.h_k;
    if (grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (packed) p.slots = (int32_t)per_head;
    else p.n_row_tiles = (int32_t)tiles;
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        auto* kernel = mlap_select(p.is_causal, packed, [](auto c, auto k) { return fa_fwd_fp8_kernel<T, decltype(c)::value, decltype(k)::value>; });
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kKvcThreads), 0, s, p);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
