// fa_fwd_prefill.hip — the prompt forward with a sliding window and attention sinks (fa_run_prefill_fwd): head_dim 64 / 128, dense and packed.
//
//   Key j is visible to row t of a sequence with sq rows and L keys iff 0 <= j < L and L - sq + t - left <= j <= L - sq + t + right (a side below 0 is
//   unbounded; a causal call arrives as right = 0).  Query head hq may carry one sink logit: it joins the running maximum and the denominator of every row
//   of the head, brings no value, and the LSE includes it (the rules of fa_fwd_kvcache_sink.hip).
//   * Work split.  One workgroup of four waves per (sequence, KV head, tile of 128 packed rows r = t * (h / h_k) + j), found with MlapSeq
//     (fa_mla_prefill_tile.hpp): the query heads of a KV head share the staged keys, and a tile holds 128 / (h / h_k) tokens.  A wave owns two 16-row column
//     blocks in which a lane owns one query row per block with private m / l; every K and V^T fragment read from LDS feeds two MFMAs.  A wave past the
//     rows takes part in staging and barriers only.
//   * Matrix products.  S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_16x16x32, Q^T resident in registers (d / 32 fragments per block), V^T by
//     ds_read_b64_tr_b16 from an lds_tile_off<d> image.
//   * Staging.  The K and V rows of a 32-key step are loaded once per workgroup through registers into one of two LDS stages under kvc_stage_step
//     (fa_kvcache_stage.hpp), one barrier per step.  A stage is K | V, 32 rows x 2 d bytes each: 16 KB at d 128 (32 KB for both), 8 KB at d 64 (16 KB).
//     At d 128 a lane moves two 16-byte pieces of K and two of V per step (rows 16 j + 4 w + lane / 16, slot lane % 16), at d 64 one of each (row 8 w +
//     lane / 8, slot lane % 8).  d 64 keeps the 32-key step: the step protocol, its adversarial-timing builds and the transposed read (two 16-row halves
//     of one image) are written for 32 keys, a 64-key step would need a second protocol, and one ds_read per MFMA stays one ds_read per MFMA either way.
//   * Window and key range.  Per tile: w0 = the first key its first token sees, k_end = the end of the keys its last token sees.  The loop walks
//     [k_lo, k_end) with k_lo = w0 floored to a step boundary counted from key 0, so a window that hides nothing walks the steps of the unwindowed call.
//     The descriptors start at row w0 and end at row k_end: keys below the tile's window, past its window or causal end, or past the sequence are never
//     read - they come back as zeros, and their scores are masked.  The work of a row scales with its window and the tile's tokens, not with L.
//     The per-row compare runs only on steps that an edge of one of the wave's rows crosses (a wave-uniform choice from the bounds of the wave's first
//     and last token); interior steps skip it.
//   * Sinks.  Once per row in the epilogue, in front of inv and lse; the loop does not know them.  No sinks = a sink of -inf, which adds + 0.0f: the
//     same code and the same bits.
//   * No key split, no workspace, no combine.  Dense grid: b x h_k x tiles.  Packed grid: ceil(total_q * (h / h_k) / 128) + b tile slots per KV head.
//   Kernels of this file: 8 ((fp16, bf16) x (d 64, 128) x (dense, packed)).  The windowed body serves plain and causal calls as (-1, -1) and (-1, 0): the
//   interior path is the unwindowed step plus two scalar compares, so a causal or plain instantiation would differ in nothing that is timed.
#include "fa_fwd_prefill.hpp"
#include "fa_mla_prefill_tile.hpp"

namespace fa {

namespace {

constexpr int kPfQB = 2;                                // query column blocks of a wave
constexpr int kPfWaveRows = kPfQB * kKvcRows;           // 32
constexpr int kPfRows = kKvcWaves * kPfWaveRows;        // packed query rows of a workgroup: 128

template <typename T, int D, bool PACKED>
FA_DEV void prefill_attn(const PrefillFwdParams& p) {
    constexpr int NC = D / 32;          // 16x16x32 MFMAs per 16 keys of S^T
    constexpr int NO = D / 16;          // O^T blocks of 16 columns
    constexpr int NL = D / 64;          // 16-byte pieces of K (and of V) a lane moves per step
    constexpr int QB = kPfQB;
    constexpr int kImage = kKvcStep * D * 2;        // 32 rows x 2 D bytes
    constexpr int kStage = 2 * kImage;              // K | V
    __shared__ __attribute__((aligned(16))) char smem[2 * kStage];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    MlapSeq<PACKED> seq;
    if (!seq.template find_tile<kPfRows, false>(p)) return;
    seq.read_bounds(p);
    if (PACKED && ((int)seq.q0 < 0 || seq.q0 + seq.sq > p.total_q)) return;     // rows outside q / o: not served
    seq.template cut<false>(p);
    const int tile = seq.tile, kvh = seq.kvh, sq = seq.sq, L = seq.L;
    const int rows_tile = sq * p.h_ratio;
    const float c = p.scale_log2e;
    const float sc = p.scale;

    // window bounds of token tq: lo <= key < lim (any negative lo = no lower bound), written so that nothing overflows for any window
    auto win_lo = [&](int tq) { return p.window_left >= 0 ? max(L - p.window_left, 0) - (sq - tq) : 0; };
    auto win_lim = [&](int tq) { return p.window_right >= 0 ? L - max(sq - 1 - tq - p.window_right, 0) : L; };
    const int t_first = tile * kPfRows / p.h_ratio, t_last = (min((tile + 1) * kPfRows, rows_tile) - 1) / p.h_ratio;
    const int w0 = __builtin_amdgcn_readfirstlane(max(win_lo(t_first), 0));        // <= L - 1 where L > 0, 0 otherwise
    const int k_lo = w0 & ~(kKvcStep - 1);
    const int k_hi = __builtin_amdgcn_readfirstlane(win_lim(t_last));              // <= L; may be <= w0: the tile sees nothing
    const int n_keys = max(k_hi - w0, 0);                                           // rows behind the descriptors
    const int k_end = n_keys > 0 ? k_hi : k_lo;

    // ---- this lane's query rows (one per column block): Q^T fragments for the whole call, visible-key range -----------------------------------
    const int wrow0 = tile * kPfRows + wave * kPfWaveRows;
    const bool active = wrow0 < rows_tile;      // (wave-uniform) false: staging and barriers only
    // the wave's edges: a step at key0 is interior iff every row of the wave sees all of its 32 keys
    const int lo_max = __builtin_amdgcn_readfirstlane(active ? win_lo((min(wrow0 + kPfWaveRows, rows_tile) - 1) / p.h_ratio) : 0);
    const int lim_min = __builtin_amdgcn_readfirstlane(active ? win_lim(wrow0 / p.h_ratio) : 0);
    bool row_ok[QB];
    int t[QB], hq[QB], lim[QB], lo[QB];
    u32x4 qf[QB][NC];
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        const int pr = wrow0 + kKvcRows * qb + n16;
        row_ok[qb] = pr < rows_tile;
        t[qb] = row_ok[qb] ? pr / p.h_ratio : 0;
        hq[qb] = kvh * p.h_ratio + (row_ok[qb] ? pr - t[qb] * p.h_ratio : 0);
        lim[qb] = row_ok[qb] ? win_lim(t[qb]) : 0;
        lo[qb] = win_lo(t[qb]);
        const char* qrow = (const char*)p.q_ptr + 2 * seq.row_off(p.q, hq[qb], t[qb]);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            qf[qb][ci] = row_ok[qb] ? *(const u32x4*)(qrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    });

    // ---- staging: the K and V rows of a step.  One descriptor per tensor, rows w0 .. k_hi - 1 of the sequence's KV head: a key outside them is addressed
    // as row n_keys (key - w0 wraps to a large unsigned number below w0), which lies past the descriptor's end and reads as zeros.  n_keys <= L, the row
    // strides are at least the row widths, and L x row stride < 2^31 bytes by the host checks. ------------------------------------------------------
    const int srow = D == 128 ? 4 * wave + (lane >> 4) : 8 * wave + (lane >> 3), sslot = D == 128 ? lane & 15 : lane & 7;
    const uint32_t krow_b = (uint32_t)(p.k.row * 2), vrow_b = (uint32_t)(p.v.row * 2);
    const char* kbase = uniform_ptr((const char*)p.k_ptr + 2 * ((PACKED ? (seq.k0 + w0) * p.k.row : (int64_t)seq.bidx * p.k.batch + (int64_t)w0 * p.k.row) + (int64_t)kvh * p.k.head));
    const char* vbase = uniform_ptr((const char*)p.v_ptr + 2 * ((PACKED ? (seq.k0 + w0) * p.v.row : (int64_t)seq.bidx * p.v.batch + (int64_t)w0 * p.v.row) + (int64_t)kvh * p.v.head));
    const rsrc_t krs = make_rsrc(kbase, n_keys > 0 ? (uint32_t)(n_keys - 1) * krow_b + 2 * D : 0u);
    const rsrc_t vrs = make_rsrc(vbase, n_keys > 0 ? (uint32_t)(n_keys - 1) * vrow_b + 2 * D : 0u);
    auto load_step = [&](int key0, u32x4 (&st)[2 * NL]) __attribute__((always_inline)) {
        static_for<0, NL>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t row = min((uint32_t)(key0 + 16 * j + srow - w0), (uint32_t)n_keys);
            st[j] = buf_load16(krs, row * krow_b + 16 * sslot);
            st[NL + j] = buf_load16(vrs, row * vrow_b + 16 * sslot);
        });
    };
    auto store_step = [&](auto bufc, const u32x4 (&st)[2 * NL]) __attribute__((always_inline)) {
        FA_LDS char* kimg = (FA_LDS char*)smem + decltype(bufc)::value * kStage;
        static_for<0, NL>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            *(FA_LDS u32x4*)(kimg + lds_tile_off<D>((uint32_t)(16 * j + srow), (uint32_t)sslot)) = st[j];
            *(FA_LDS u32x4*)(kimg + kImage + lds_tile_off<D>((uint32_t)(16 * j + srow), (uint32_t)sslot)) = st[NL + j];
        });
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

    // one 32-key step of this wave's rows over the images of stage BUF: every K and V^T fragment is read once and serves the wave's two column blocks
    auto compute_step = [&](auto bufc, int key0) __attribute__((always_inline)) {
        const FA_LDS char* kimg = (const FA_LDS char*)smem + decltype(bufc)::value * kStage;
        const FA_LDS char* vimg = kimg + kImage;
        f32x4 s[QB][2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, QB>([&](auto qq) { s[decltype(qq)::value][b] = f32x4{0.f, 0.f, 0.f, 0.f}; });
            mlap_rows_mfma<T, D, 0, b>(kimg, n16, g, qf, s);
        });
        // an edge of one of the wave's rows crosses the step (wave-uniform): the per-row compare; an interior step keeps its scores as they are
        if (key0 < lo_max || key0 + kKvcStep > lim_min) {
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                static_for<0, 2>([&](auto kb) {
                    constexpr int b = decltype(kb)::value;
                    static_for<0, 4>([&](auto rr) {
                        constexpr int r = decltype(rr)::value;
                        const int key = key0 + 16 * b + 4 * g + r;
                        s[qb][b][r] = (key < lim[qb] && key >= lo[qb]) ? s[qb][b][r] : -INFINITY;
                    });
                });
            });
        }
        u32x4 pf[QB];
        static_for<0, QB>([&](auto qq) {
            constexpr int qb = decltype(qq)::value;
            float mx = -INFINITY;
            static_for<0, 8>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                mx = fmaxf(mx, s[qb][j >> 2][j & 3]);
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
            const u32x4 vt = tr_frag<D>(vimg, ci, g, q4, p4);
            static_for<0, QB>([&](auto qq) {
                constexpr int qb = decltype(qq)::value;
                oacc[qb][ci] = LP<T>::mfma16(vt, pf[qb], oacc[qb][ci]);
            });
        });
    };

    // ---- the 32-key steps from k_lo, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp) -----------------------------
    // k_lo and k_end are the workgroup's: every wave meets the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the two images are read by compute_step alone,
    // as MFMA operands (mlap_rows_mfma, tr_frag): what comes out of them are scores and O, which reach compares, exponentials and stores of VALUES - every
    // address (lds_tile_off of lane constants, row_off / row_index of the lane's row, the sequence's base rows from cu_seqlens), every index and every loop
    // bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[2 * NL];
        int key = k_lo;
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
        // `active` is the wave's for the whole loop: one loop per value, so that neither carries the test (with the test and the edge branch of
        // compute_step in one loop hipcc builds a loop with two entries, which its own loop annotations - and tests/_kernel_isa.py - do not see)
        auto steps = [&](auto act) __attribute__((always_inline)) {
            for (; key < k_end; key += 2 * kKvcStep) {
                kvc_stage_step(std::integral_constant<int, 0>{}, key, k_lo, k_end, wave, decltype(act)::value, load, store, compute);
                if (key + kKvcStep < k_end) kvc_stage_step(std::integral_constant<int, 1>{}, key + kKvcStep, k_lo, k_end, wave, decltype(act)::value, load, store, compute);
            }
        };
        if (active) steps(std::true_type{});
        else steps(std::false_type{});
    }

    // ---- epilogue: the sink, then the lane's rows, columns 16 c + 4 g .. + 3 of every block c ----------------------------------------------------
    if (!active) return;
    static_for<0, QB>([&](auto qq) {
        constexpr int qb = decltype(qq)::value;
        float lsum = sum_four_groups(l_run[qb]);
        if (!row_ok[qb]) return;
        // M = max(row max, sink) in natural-log units.  The sink on top: the row's sums move down onto it and it counts 1; a row that saw no key (lsum = 0,
        // m = kNegBig) goes this way under a finite sink: lsum = 1, O = 0, LSE = the sink exactly.  Otherwise it adds exp(sink - max), which is + 0.0f for a
        // sink of -inf (= no sinks; the guard keeps -inf - -inf out of the exponential).  A NaN sink fails the comparison and makes the sum NaN.
        float sk = -INFINITY;
        if (p.sinks != nullptr) {
            if (p.sinks_16bit) sk = LP<T>::to_float(((const uint16_t*)p.sinks)[(int64_t)hq[qb] * p.sinks_stride]);
            else sk = ((const float*)p.sinks)[(int64_t)hq[qb] * p.sinks_stride];
        }
        const float ms = m_run[qb] * sc;
        float a = 1.f;
        const bool on_sink = sk > ms;
        if (on_sink) {
            a = fast_exp2((ms - sk) * kLog2e);
            lsum = __builtin_fmaf(lsum, a, 1.f);
        } else {
            lsum += sk == -INFINITY ? 0.f : fast_exp2((sk - ms) * kLog2e);
        }
        // dead = saw no key and no sink (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math
        const bool live = !(lsum == 0.f);
        const float inv = live ? a / lsum : 0.f;
        const float lse = live ? (on_sink ? sk : ms) + logf(lsum) : 0.f;
        char* orow = (char*)p.o_ptr + 2 * (seq.row_off(p.o, hq[qb], t[qb]) + 4 * g);
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            mlap_store_block<T>(orow, ci, oacc[qb][ci], inv);
        });
        if (g == 0) p.lse_ptr[seq.row_index(p, hq[qb], t[qb])] = lse;
    });
}

// Two workgroups per compute unit at either width (registers and LDS as compiled: DESIGN.md 3.26).
template <typename T, int D, bool PACKED>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_prefill_kernel(const PrefillFwdParams p) {
    prefill_attn<T, D, PACKED>(p);
}

}  // namespace

// p as the C ABI filled it; the tiles (dense) or tile slots (packed) are counted here.  grid = b x h_k x tiles (dense), slots x h_k (packed)
hipError_t launch_fwd_prefill(PrefillFwdParams p, int dtype, int d, hipStream_t s) {
    const bool packed = p.cu_q != nullptr;
    const int64_t rows = packed ? p.total_q : p.seqlen_q;
    if (p.b <= 0 || rows <= 0) return hipSuccess;
    const int64_t tiles = (rows * p.h_ratio + kPfRows - 1) / kPfRows;
    const int64_t per_head = packed ? tiles + p.b : tiles * p.b;
    const int64_t grid = per_head * p.h_k;
    if (grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (packed) p.slots = (int32_t)per_head;
    else p.n_row_tiles = (int32_t)tiles;
    auto launch = [&](auto* tt, auto dd) {
        using T = std::remove_pointer_t<decltype(tt)>;
        constexpr int D = decltype(dd)::value;
        auto* kernel = packed ? fa_fwd_prefill_kernel<T, D, true> : fa_fwd_prefill_kernel<T, D, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kKvcThreads), 0, s, p);
    };
    auto by_width = [&](auto* tt) {
        if (d == 64) launch(tt, std::integral_constant<int, 64>{});
        else launch(tt, std::integral_constant<int, 128>{});
    };
    if (dtype == 0) by_width((_Float16*)nullptr);
    else by_width((__bf16*)nullptr);
    return hipGetLastError();
}

}  // namespace fa
