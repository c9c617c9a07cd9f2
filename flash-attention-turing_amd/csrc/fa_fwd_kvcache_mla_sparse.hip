// fa_fwd_kvcache_mla_sparse.hip — sparse MLA decode over a latent KV cache (DeepSeek Sparse Attention: top-k key indices per query token): every kernel of
// fa_run_mla_sparse_fwd_kvcache.
//
//   The body is kvcache_mla_attn of fa_fwd_kvcache_mla.hip with a gathered staging step.  Kept as they are: 64 rows a workgroup, four waves of 16 rows, a
//   lane owns one query row with private m / l; 32-slot steps walked by all four waves together; the two images per stage (lds_tile_off<512>,
//   lds_tile_off<64>), 72 KB; one barrier per step with the next step's loads issued behind it; S^T = K Q^T with qf[18] held for the whole split; V^T by
//   transposed reads from the 512 image of the same stage; the per-step arithmetic, the epilogue, the empty-split partials (LSE = -inf) and the plane layout
//   of the partials; the combine is fa_kvcache_combine_kernel at D = 512.  What changes:
//   * Tiling.  The lists of two query tokens differ, so a tile never spans two tokens: the grid is b x seqlen_q x ceil(h / 64) x n_split and a row within a
//     tile is the head index.  rows_total and the row index of o / lse / planes are the dense call's.
//   * Split.  Over the slots [0, topk) of the token's list, in multiples of 32 from slot 0 (kvcache_split / finish_params with topk in the place of
//     seqlen_cache and this grid's workgroup count).
//   * Staging.  Key key0 + r of a step is slot key0 + r of the list.  Lane l of every wave holds the index word of slot l & 31 of a step, loaded one step
//     before it is used (the paged kernels: two, so that the table entry is fetched one step ahead).  Slot s is valid iff (uint32_t)idx < L_i: the ballot of
//     that test is the step's 32-bit mask.  Wave w stages slots 8 w .. 8 w + 7; every 16-byte load stays inside one cache row.
//     Contiguous: the dense kernel's one descriptor per sequence, ending at row L_i; the row offset is min((uint32_t)idx, L_i) x row bytes, read from the
//     owning lane (v_readlane; the rope load, whose eight lane groups read eight rows, by ds_bpermute).  An invalid entry lands at the descriptor's end
//     and loads zeros.
//     Paged: lane l computes column and row-in-page of its slot (an invalid slot: column 0), gathers the table entry (column clamped to the table row,
//     entry to the pool) and forms the 64-bit address of the cache row.  A row of the 512 part gets a descriptor of its own over exactly that row - of
//     length 0 for an invalid slot, which loads zeros and reads nothing; the rope part is one per-lane load that the lanes of an invalid slot do not issue
//     (their zeros come from a load over an empty range).
//     The image row of an invalid slot is therefore written with zeros every step (LDS holds whatever the last workgroup left, and 0 x NaN is NaN),
//     and its score is -inf before the max, where the dense kernel applies key < lim.
//   Kernels of this file: 4 attention ((fp16, bf16) x (contiguous, paged)), 2 combine.  There is no append.
#include "fa_kvcache_launch.hpp"
#include "fa_kvcache_stage_debug.hpp"

namespace fa {

namespace {

constexpr int kMlaRows = kKvcPrefillRows;   // query rows (heads of one token) of a workgroup: 16 per wave
constexpr int kMlaDV = 512;                 // the compressed part: V, and columns 0 .. 511 of K
constexpr int kMlaDR = 64;                  // the rope part: columns 512 .. 575 of K
constexpr int kMlaDK = kMlaDV + kMlaDR;
constexpr int kMlaRowBytes = kMlaDK * 2;    // 1152: 72 16-byte slots

struct MlaLds {
    static constexpr int kImageV = kKvcStep * kMlaDV * 2;       // 32 rows x 1024 B
    static constexpr int kImageR = kKvcStep * kMlaDR * 2;       // 32 rows x 128 B
    static constexpr int kStage = kImageV + kImageR;            // 36 KB
    static constexpr int kBytes = 2 * kStage;                   // 72 KB
};

template <typename T, bool PAGED>
FA_DEV void kvcache_mla_sparse_attn(const KvcacheMlaSparseParams& sp) {
    const KvcacheKernelParams& p = sp.kp;
    constexpr int NCV = kMlaDV / 32;    // 16x16x32 MFMAs per 16 keys of S^T over the 512 image
    constexpr int NCR = kMlaDR / 32;    // ... and over the 64 image
    constexpr int NC = NCV + NCR;
    constexpr int NO = kMlaDV / 16;     // O^T blocks of 16 columns
    constexpr int RW = kKvcStep / kKvcWaves;    // slots of a step a wave stages: 8
    constexpr int NL = RW + 1;          // loads per lane and step
    __shared__ __attribute__((aligned(16))) char smem[MlaLds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int split = id % p.n_split;
    int rest = id / p.n_split;
    const int tile = rest % p.n_row_tiles;      // 64 heads of one token
    rest /= p.n_row_tiles;
    const int t = rest % p.seqlen_q;
    const int bidx = rest / p.seqlen_q;         // (one KV head)
    const int L = kvc_len(p, bidx);
    auto row_index = [&](int hq_) __attribute__((always_inline)) -> int64_t { return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t; };
    auto row_off = [&](const TStride& st, int hq_) __attribute__((always_inline)) -> int64_t {
        return (int64_t)bidx * st.batch + (int64_t)t * st.row + (int64_t)hq_ * st.head;
    };
    // the split's slots of the token's list (topk and split_keys are multiples of the step: every step has its 32 index words)
    const int k_begin = split * p.split_keys;
    const int k_end = min(k_begin + p.split_keys, sp.topk);
    const float c = p.scale_log2e;
    const float sc = p.scale;

    if (p.n_split > 1 && k_begin >= k_end) {        // no slot in this split: an empty partial (LSE = -inf), O is never looked at
        if (tid < kMlaRows) {
            const int hq_ = tile * kMlaRows + tid;
            if (hq_ < p.h) p.ws_lse[(int64_t)split * p.rows_total + row_index(hq_)] = -INFINITY;
        }
        return;
    }

    // ---- this lane's query row (a head of token t): Q^T fragments for the whole split ---------------------------------------------------
    const bool active = tile * kMlaRows + wave * kKvcRows < p.h;            // (wave-uniform) false: staging and barriers only
    const int hrow = tile * kMlaRows + wave * kKvcRows + n16;
    const bool row_ok = hrow < p.h;
    const int hq = row_ok ? hrow : 0;
    u32x4 qf[NC];
    {
        const char* qrow = (const char*)p.q_ptr + 2 * row_off(p.q, hq);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            qf[ci] = row_ok ? *(const u32x4*)(qrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    }

    // ---- staging: wave w loads slots 8 w .. 8 w + 7 of a step ----------------------------------------------------------------------------
    // load i < 8: slot 8 w + i, 16-byte slot `lane` of the 64 of its row's 512 part; load 8: slot 8 w + lane / 8, 16-byte slot 64 + lane % 8 (the rope part)
    const int row0 = wave * RW;
    const int rrow = lane >> 3, rslot = lane & 7;
    const int islot = lane & 31;                // the slot of a step whose index word this lane holds
    const uint32_t row_b = (uint32_t)(p.kc.row * 2);
    const char* kbase = uniform_ptr((const char*)p.k_cache + 2 * ((int64_t)(PAGED ? 0 : bidx) * p.kc.batch));
    // contiguous: one descriptor, ending at row L (row indices are clamped to L, where it reads zeros; L x row stride < 2^31 by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * row_b + kMlaRowBytes : 0u);
    const int32_t* ip = sp.indices + ((int64_t)bidx * sp.idx_batch + (int64_t)t * sp.idx_row);
    const int last_key0 = k_end - kKvcStep;     // the split's last step: index loads past it are clamped to it
    const int P = p.page_size;
    const int32_t* tbl = PAGED ? p.block_table + (int64_t)bidx * p.bt_stride : nullptr;
    const uint32_t last_col = PAGED ? (uint32_t)(p.seqlen_cache / P - 1) : 0u;
    uint32_t idxv = 0u;                         // index words of the step after the one whose rows (PAGED: whose table entries) were requested last
    uint32_t pg_v = 0u;                         // PAGED: the table entry (unclamped) of the lane's slot of the next step to load ...
    int prow_v = -1;                            // ... and the slot's row in its page, -1 = an invalid slot
    uint32_t mask0 = 0u, mask1 = 0u;            // valid slots of the step held by stage 0 / 1
    auto load_idx = [&](int key0) __attribute__((always_inline)) { idxv = (uint32_t)ip[min(key0, last_key0) + islot]; };
    auto prep_pages = [&]() __attribute__((always_inline)) {
        const bool ok = idxv < (uint32_t)L;
        const uint32_t j = ok ? idxv : 0u;
        const uint32_t col = j / (uint32_t)P;
        prow_v = ok ? (int)(j - col * (uint32_t)P) : -1;
        pg_v = (uint32_t)tbl[min(col, last_col)];
    };
    // the loads of one step into st, from the index words fetched ahead; the step's mask; the words (PAGED: and table entries) of later steps
    auto load_step = [&](auto bufc, int key0, u32x4 (&st)[NL]) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        uint32_t mask;
        if constexpr (PAGED) {
            mask = (uint32_t)__builtin_amdgcn_ballot_w64(prow_v >= 0);
            const int64_t page = min(pg_v, (uint32_t)(p.num_blocks - 1));
            const uint64_t a = (uint64_t)kbase + 2 * (uint64_t)(page * p.kc.batch + (int64_t)max(prow_v, 0) * p.kc.row);
            const uint32_t alo = (uint32_t)a, ahi = (uint32_t)(a >> 32);
            static_for<0, RW>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                // (readlane returns an int: the low word goes through uint32_t, or its sign would fill the high word)
                const uint64_t base = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(ahi, row0 + i) << 32) | (uint32_t)__builtin_amdgcn_readlane(alo, row0 + i);
                const rsrc_t r = make_rsrc((const char*)base, (mask >> (row0 + i)) & 1u ? (uint32_t)kMlaRowBytes : 0u);
                st[i] = buf_load16(r, 16 * lane);
            });
            const uint32_t rlo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), alo), rhi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), ahi);
            const char* rp = (const char*)(((uint64_t)rhi << 32) | rlo) + 2 * kMlaDV + 16 * rslot;
            // (the zeros of the lanes that do not load come from a load over an empty range: a constant would be kept in registers and copied every step)
            st[RW] = buf_load16(make_rsrc(kbase, 0u), 0u);
            if ((mask >> (row0 + rrow)) & 1u) st[RW] = *(const __attribute__((address_space(1))) u32x4*)rp;
            prep_pages();                       // the table entries of the step after this one
            load_idx(key0 + 2 * kKvcStep);      // the index words of the step after that
        } else {
            mask = (uint32_t)__builtin_amdgcn_ballot_w64(idxv < (uint32_t)L);
            const uint32_t offv = min(idxv, (uint32_t)L) * row_b;
            static_for<0, RW>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                st[i] = buf_load16(krs, (uint32_t)__builtin_amdgcn_readlane(offv, row0 + i) + 16 * lane);
            });
            st[RW] = buf_load16(krs, (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), offv) + 2 * kMlaDV + 16 * rslot);
            load_idx(key0 + kKvcStep);          // the index words of the step after this one
        }
        if constexpr (BUF == 0) mask0 = mask;
        else mask1 = mask;
    };
    // registers -> the two images of stage BUF
    auto store_step = [&](auto bufc, const u32x4 (&st)[NL]) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        FA_LDS char* vimg = (FA_LDS char*)smem + BUF * MlaLds::kStage;
        FA_LDS char* rimg = vimg + MlaLds::kImageV;
        static_for<0, RW>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>((uint32_t)(row0 + i), (uint32_t)lane)) = st[i];
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMlaDR>((uint32_t)(row0 + rrow), (uint32_t)rslot)) = st[RW];
    };

    // transposed-read addresses of this lane (fa_device.hpp lds_tile_off image): block c, half hh -> rows hh * 16 + 4 g + q, columns 16 c + 4 p
    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 oacc[NO];
    static_for<0, NO>([&](auto cc) {
        oacc[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(oacc[decltype(cc)::value]));
    });
    float m_run = kNegBig, l_run = 0.f;

    // one 32-slot step of this wave's 16 rows over the images of stage BUF: the arithmetic of kvcache_mla_attn, the step's mask in the place of key < lim
    auto compute_step = [&](auto bufc) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        const FA_LDS char* vimg = (const FA_LDS char*)smem + BUF * MlaLds::kStage;
        const FA_LDS char* rimg = vimg + MlaLds::kImageV;
        const uint32_t vm = (BUF == 0 ? mask0 : mask1) >> (4 * g);      // bit 16 b + r: slot 16 b + 4 g + r
        f32x4 s[2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            static_for<0, NCV>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>(16 * b + n16, 4 * ci + g));
                s[b] = LP<T>::mfma16(kf, qf[ci], s[b]);
            });
            static_for<0, NCR>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(rimg + lds_tile_off<kMlaDR>(16 * b + n16, 4 * ci + g));
                s[b] = LP<T>::mfma16(kf, qf[NCV + ci], s[b]);
            });
        });
        float mx = -INFINITY;
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                s[b][r] = (vm >> (16 * b + r)) & 1u ? s[b][r] : -INFINITY;
                mx = fmaxf(mx, s[b][r]);
            });
        });
        mx = max_four_groups(mx);
        const float m_new = fmaxf(m_run, mx);
        const float alpha = fast_exp2((m_run - m_new) * c);
        m_run = m_new;
        const float mc = m_new * c;
        float pe[8];
        float ps = 0.f;
        static_for<0, 8>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            pe[j] = fast_exp2(__builtin_fmaf(s[j >> 2][j & 3], c, -mc));
            ps += pe[j];
        });
        l_run = l_run * alpha + ps;
        const u32x4 pf = u32x4{LP<T>::pack2(pe[0], pe[1]), LP<T>::pack2(pe[2], pe[3]), LP<T>::pack2(pe[4], pe[5]), LP<T>::pack2(pe[6], pe[7])};
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            oacc[ci] *= alpha;
        });
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            const uint32_t a0 = lds_tile_off<kMlaDV>(4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const uint32_t a1 = lds_tile_off<kMlaDV>(16 + 4 * g + q4, 2 * ci + (p4 >> 1)) + 8 * (p4 & 1);
            const u32x2 v0 = lds_read_tr8(vimg, a0), v1 = lds_read_tr8(vimg, a1);
            oacc[ci] = LP<T>::mfma16(u32x4{v0.x, v0.y, v1.x, v1.y}, pf, oacc[ci]);
        });
    };

    // ---- the split's 32-slot steps, all four waves together; two LDS stages in turn (the schedule of kvcache_mla_attn) -------------------------
    // Stage n & 1 holds step n.  While step n computes, the loads of step n + 1 are in flight; they are written to the other stage behind the
    // compute and one barrier publishes them; the loads of step n + 2 are issued behind that barrier.  k_end is the workgroup's.
    // Test builds (FA_KVC_STAGE_DEBUG, fa_kvcache_stage_debug.hpp): the two helpers hold one wave back; FA_KVC_STAGE_RACY moves the step's barrier in front of store_step.
    // Why the racy form can neither hang nor fault here: (1) the barrier only changes places inside the same `if (key0 + kKvcStep < k_end)`, whose
    // condition is the workgroup's (k_begin, k_end and key0 are the same in every wave, `active` is not part of it), so every wave still meets the same
    // number of barriers on every path; (2) the two images are read by compute_step alone, as MFMA operands (kf, v0 / v1): what comes out of them are
    // scores and O, which reach compares, exponentials and stores of VALUES.  The gather does NOT go through them: the index words come from global memory
    // into registers (load_idx), cross lanes by v_readlane / ds_bpermute (the crossbar; no LDS byte is read or written), and masks, row offsets, table
    // columns and page addresses are computed from those registers.  Every address, index and loop bound comes from the parameters, the list and the
    // block table.  A stale image gives wrong numbers.
    {
        u32x4 st[NL];
        int key = k_begin;
        load_idx(key);
        if constexpr (PAGED) {
            prep_pages();
            load_idx(key + kKvcStep);
        }
        load_step(std::integral_constant<int, 0>{}, key, st);
        kvc_stage_slow_writer(-1, wave);
        store_step(std::integral_constant<int, 0>{}, st);
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(std::integral_constant<int, 1>{}, key + kKvcStep, st);
        auto step = [&](auto bufc, int key0) __attribute__((always_inline)) {
            constexpr int BUF = decltype(bufc)::value;
            kvc_stage_slow_reader((key0 - k_begin) / kKvcStep, wave);
            if (active) compute_step(bufc);
            if (key0 + kKvcStep < k_end) {
#if FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                kvc_stage_slow_writer((key0 - k_begin) / kKvcStep, wave);
                store_step(std::integral_constant<int, BUF ^ 1>{}, st);
#if !FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                if (key0 + 2 * kKvcStep < k_end) load_step(bufc, key0 + 2 * kKvcStep, st);
            }
        };
        for (; key < k_end; key += 2 * kKvcStep) {
            step(std::integral_constant<int, 0>{}, key);
            if (key + kKvcStep < k_end) step(std::integral_constant<int, 1>{}, key + kKvcStep);
        }
    }

    // ---- epilogue: the lane's row, columns 16 c + 4 g .. + 3 of every block c ---------------------------------------------------------
    if (!active) return;
    const float lsum = sum_four_groups(l_run);
    if (!row_ok) return;
    // dead = no valid slot (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math, and a
    // split partial is written so that the combine propagates it
    const bool live = !(lsum == 0.f);
    const float inv = live ? 1.0f / lsum : 0.f;
    const float lse = live ? m_run * sc + logf(lsum) : (p.n_split > 1 ? -INFINITY : 0.f);
    const int64_t R = row_index(hq);
    if (p.n_split == 1) {
        char* orow = (char*)p.o_ptr + 2 * (row_off(p.o, hq) + 4 * g);
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            *(u32x2*)(orow + 32 * ci) = u32x2{LP<T>::pack2(oacc[ci][0] * inv, oacc[ci][1] * inv), LP<T>::pack2(oacc[ci][2] * inv, oacc[ci][3] * inv)};
        });
        if (g == 0) p.lse_ptr[R] = lse;
    } else {
        float* prow = p.ws_o + ((int64_t)split * p.rows_total + R) * kMlaDV + 4 * g;
        if (live) {
            static_for<0, NO>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                *(f32x4*)(prow + 16 * ci) = f32x4{oacc[ci][0] * inv, oacc[ci][1] * inv, oacc[ci][2] * inv, oacc[ci][3] * inv};
            });
        }
        if (g == 0) p.ws_lse[(int64_t)split * p.rows_total + R] = lse;
    }
}

// ONE workgroup per compute unit, as the dense MLA kernels ship (fa_fwd_kvcache_mla.hip): O^T (128 registers), Q^T (72) and the staging set (36) next
// to the softmax; with the register class ahead of the range's length in the allocator (build.py EXTRA_FLAGS) Q^T and the staging set take the AGPRs.
template <typename T, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_mla_sparse_kernel(const KvcacheMlaSparseParams sp) {
    kvcache_mla_sparse_attn<T, PAGED>(sp);
}

}  // namespace

// attention, combine.  sp.kp as the C ABI filled it: d = 512, h_k = 1, h_ratio = h, k_cache the latent cache, n_split chosen (kvcache_split over topk and
// this grid: b x seqlen_q x ceil(h / 64) workgroups a split).  The split is sized on a copy that states the grid the way finish_params reads it:
// seqlen_q = 1 (a tile holds heads of one token) and seqlen_cache = topk.
hipError_t launch_fwd_kvcache_mla_sparse(KvcacheMlaSparseParams sp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = sp.kp;
    if (kp.d != kMlaDV || sp.d_qk != kMlaDK || kp.h_k != 1 || sp.indices == nullptr || sp.topk < kKvcStep || sp.topk % kKvcStep != 0) return hipErrorInvalidValue;
    {
        KvcacheKernelParams t = kp;
        t.seqlen_q = 1; t.seqlen_cache = sp.topk; t.is_local = 0;
        finish_params(t, (int64_t)kp.b * kp.h * kp.seqlen_q, kMlaRows);
        kp.n_row_tiles = t.n_row_tiles; kp.rows_total = t.rows_total; kp.n_split = t.n_split; kp.split_keys = t.split_keys; kp.ws_lse = t.ws_lse;
    }
    const bool paged = kp.block_table != nullptr;
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.seqlen_q * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        kvc_launch_attn(paged ? fa_fwd_kvcache_mla_sparse_kernel<T, true> : fa_fwd_kvcache_mla_sparse_kernel<T, false>, grid, s, sp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) {
        if (dtype == 0) kvc_launch_combine<kMlaDV>(fa_kvcache_combine_kernel<_Float16, kMlaDV>, kp.rows_total, s, kp);
        else kvc_launch_combine<kMlaDV>(fa_kvcache_combine_kernel<__bf16, kMlaDV>, kp.rows_total, s, kp);
    }
    return hipGetLastError();
}

}  // namespace fa
