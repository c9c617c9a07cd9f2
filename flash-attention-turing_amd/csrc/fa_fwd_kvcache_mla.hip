// fa_fwd_kvcache_mla.hip — multi-head latent attention (MLA) decode over a latent KV cache: every kernel of fa_run_mla_fwd_kvcache.
//
//   After weight absorption an MLA decode step is MQA over ONE "KV head" whose key is the 576-element latent row (512 compressed-KV elements,
//   then 64 rope elements) and whose value is the first 512 elements of the SAME row.  The body is the 64-row, LDS-staged body of
//   fa_fwd_kvcache_prefill.hip (kvcache_prefill_attn) with the following kept as they are: four waves of 16 packed rows (packed row r = t * h + j),
//   a lane owns one query row with private m / l; 32-key steps walked by all four waves together; two LDS stages and one barrier per step; the
//   causal k_hi per tile; empty-split partials with LSE = -inf; a wave past the rows takes part in staging and barriers only; the plane layout of
//   the split partials; the paged descriptor-per-16-key-block rule with the table entries fetched one step ahead.  What changes:
//   * Two images per stage in place of K + V: the 512 compressed columns (32 rows x 1024 B, lds_tile_off<512>) and the 64 rope columns (32 rows
//     x 128 B, lds_tile_off<64>).  36 KB a stage, 72 KB for both.  One image with a 1152-byte pitch would break the bank argument of
//     lds_tile_off (the pitch must be a multiple of the 256-byte bank row), hence the split.
//   * Staging: every wave-wide 16-byte load stays inside one 16-key block.  Wave w takes rows 8 w .. 8 w + 7 of the step: eight loads of the 64
//     slots of one row's 512 part each, and one load of the 8 slots of the rope part of all eight rows.  Nine loads per lane and step; the
//     latent row comes from memory once and serves both matmuls.
//   * S^T = K Q^T: 16 chunks of v_mfma_f32_16x16x32 with K fragments from the 512 image and 2 from the 64 image; qf[18] is held for the split.
//   * O^T += V^T P^T: 32 accumulator blocks (128 fp32 registers a lane); V^T comes by transposed reads (ds_read_b64_tr_b16) from the 512 image
//     of the same stage.  There is no V load and no V image.
//   * The epilogue writes 512-wide rows; the combine is fa_kvcache_combine_kernel at D = 512 (workspace and planes sized by d_v = kp.d = 512).
//   * The append copies the 72 16-byte slots of a kv_new row, contiguous or through the table, with the drop and clamp rules of the other appends.
//   Kernels of this file: 8 attention ((fp16, bf16) x (causal, not) x (contiguous, paged)), 2 append, 2 combine.
#include "fa_kvcache_launch.hpp"
#include "fa_kvcache_stage_debug.hpp"

namespace fa {

namespace {

constexpr int kMlaRows = kKvcPrefillRows;   // packed query rows of a workgroup: 16 per wave
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

template <typename T, bool CAUSAL, bool PAGED>
FA_DEV void kvcache_mla_attn(const KvcacheKernelParams& p) {
    constexpr int NCV = kMlaDV / 32;    // 16x16x32 MFMAs per 16 keys of S^T over the 512 image
    constexpr int NCR = kMlaDR / 32;    // ... and over the 64 image
    constexpr int NC = NCV + NCR;
    constexpr int NO = kMlaDV / 16;     // O^T blocks of 16 columns
    constexpr int RW = kKvcStep / kKvcWaves;    // rows of a step a wave stages: 8, inside one 16-key block
    constexpr int NL = RW + 1;          // loads per lane and step
    __shared__ __attribute__((aligned(16))) char smem[MlaLds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int split = id % p.n_split, rest = id / p.n_split;
    const int tile = rest % p.n_row_tiles;
    const int bidx = rest / p.n_row_tiles;      // (one KV head)
    const int sq = p.seqlen_q;
    const int L = kvc_len(p, bidx);
    const int rows_tile = sq * p.h;
    auto row_index = [&](int hq_, int t_) __attribute__((always_inline)) -> int64_t { return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t_; };
    auto row_off = [&](const TStride& st, int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        return (int64_t)bidx * st.batch + (int64_t)t_ * st.row + (int64_t)hq_ * st.head;
    };
    // CAUSAL: the tile's keys end where its last row's do (t_last <= sq - 1, so k_hi <= L; it may be <= 0: the tile sees nothing)
    int k_hi = L;
    if constexpr (CAUSAL) {
        const int t_last = (min((tile + 1) * kMlaRows, rows_tile) - 1) / p.h;
        k_hi = __builtin_amdgcn_readfirstlane(min(L, L - sq + t_last + 1));
    }
    const int k_begin = split * p.split_keys;
    const int k_end = min(k_begin + p.split_keys, k_hi);
    const float c = p.scale_log2e;
    const float sc = p.scale;

    if (p.n_split > 1 && k_begin >= k_end) {        // nothing to read in this split: an empty partial (LSE = -inf), O is never looked at
        if (tid < kMlaRows) {
            const int pr = tile * kMlaRows + tid;
            if (pr < rows_tile) {
                const int t = pr / p.h, hq = pr - t * p.h;
                p.ws_lse[(int64_t)split * p.rows_total + row_index(hq, t)] = -INFINITY;
            }
        }
        return;
    }

    // ---- this lane's query row: Q^T fragments for the whole split, visible-key limit -------------------------------------------------
    const bool active = tile * kMlaRows + wave * kKvcRows < rows_tile;      // (wave-uniform) false: staging and barriers only
    const int pr = tile * kMlaRows + wave * kKvcRows + n16;
    const bool row_ok = pr < rows_tile;
    const int t = row_ok ? pr / p.h : 0;
    const int hq = row_ok ? pr - t * p.h : 0;
    int lim = row_ok ? L : 0;
    if (CAUSAL && row_ok) lim = min(L, L - sq + t + 1);
    u32x4 qf[NC];
    {
        const char* qrow = (const char*)p.q_ptr + 2 * row_off(p.q, hq, t);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            qf[ci] = row_ok ? *(const u32x4*)(qrow + 2 * (32 * ci + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    }

    // ---- staging: wave w loads rows 8 w .. 8 w + 7 of a step, all in the 16-key block w >> 1 -------------------------------------------
    // load i < 8: row 8 w + i, slot `lane` of its 64 slots of the 512 part; load 8: row 8 w + lane / 8, slot 64 + lane % 8 (the rope part)
    const int row0 = wave * RW;
    const int rrow = lane >> 3, rslot = lane & 7;
    const uint32_t row_b = (uint32_t)(p.kc.row * 2);
    const char* kbase = uniform_ptr((const char*)p.k_cache + 2 * ((int64_t)(PAGED ? 0 : bidx) * p.kc.batch));
    // contiguous: one descriptor, ending at row L (rows at or past L read as zeros; row indices are clamped to L, and L x row stride < 2^31
    // by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * row_b + kMlaRowBytes : 0u);
    // Paged cache: a wave's eight rows lie in one 16-key block and so in one page.  Each step the wave builds the descriptor of its block, based at
    // the block's first row in its page and ending at the sequence's last valid row in the block (a block wholly past L has an empty range:
    // whatever its table entry says is never read).  The table entries of the step after the one being loaded are fetched (scalar loads)
    // together with that load; the cursor (column, row in page) moves by one step without a division.  Columns are clamped to the table row,
    // entries to the pool.
    const int P = p.page_size;
    typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
    const const_i32_ptr tbl = PAGED ? (const_i32_ptr)(p.block_table + (int64_t)bidx * p.bt_stride) : nullptr;
    const int last_col = PAGED ? p.seqlen_cache / P - 1 : 0;
    uint32_t pg0 = 0u, pg1 = 0u;                // table entries (unclamped) of the next step's blocks
    int rw0 = 0, rw1 = 0;                       // ... and the blocks' first rows in their pages
    int f_col = 0, f_row = 0, st_col = 0, st_row = 0;
    auto fetch_pages = [&]() __attribute__((always_inline)) {
        int c1 = f_col, r1 = f_row + 16;
        if (r1 >= P) { r1 -= P; c1 += 1; }
        pg0 = (uint32_t)tbl[min(f_col, last_col)]; rw0 = f_row;
        pg1 = (uint32_t)tbl[min(c1, last_col)]; rw1 = r1;
        f_col += st_col; f_row += st_row;
        if (f_row >= P) { f_row -= P; f_col += 1; }
    };
    if constexpr (PAGED) {
        f_col = __builtin_amdgcn_readfirstlane(k_begin / P);
        f_row = k_begin - f_col * P;
        st_col = __builtin_amdgcn_readfirstlane(kKvcStep / P);
        st_row = kKvcStep - st_col * P;
        fetch_pages();
    }
    auto load_step = [&](int key0, u32x4 (&st)[NL]) __attribute__((always_inline)) {
        if constexpr (PAGED) {
            const int blk = row0 >> 4;                                      // (wave-uniform)
            const int valid = min(max(L - (key0 + 16 * blk), 0), 16);
            const int64_t page = min(blk ? pg1 : pg0, (uint32_t)(p.num_blocks - 1));
            const int prow = blk ? rw1 : rw0;
            const char* base = uniform_ptr(kbase + 2 * (page * p.kc.batch + (int64_t)prow * p.kc.row));
            const rsrc_t r = make_rsrc(base, valid > 0 ? (uint32_t)(valid - 1) * row_b + kMlaRowBytes : 0u);
            static_for<0, RW>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                st[i] = buf_load16(r, (uint32_t)((row0 & 15) + i) * row_b + 16 * lane);
            });
            st[RW] = buf_load16(r, (uint32_t)((row0 & 15) + rrow) * row_b + 2 * kMlaDV + 16 * rslot);
            fetch_pages();                      // the table entries of the step after this one
        } else {
            static_for<0, RW>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                st[i] = buf_load16(krs, (uint32_t)min(key0 + row0 + i, L) * row_b + 16 * lane);
            });
            st[RW] = buf_load16(krs, (uint32_t)min(key0 + row0 + rrow, L) * row_b + 2 * kMlaDV + 16 * rslot);
        }
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

    // one 32-key step of this wave's 16 rows over the images of stage BUF
    auto compute_step = [&](auto bufc, int key0) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        const FA_LDS char* vimg = (const FA_LDS char*)smem + BUF * MlaLds::kStage;
        const FA_LDS char* rimg = vimg + MlaLds::kImageV;
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
                const int key = key0 + 16 * b + 4 * g + r;
                s[b][r] = key < lim ? s[b][r] : -INFINITY;
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

    // ---- the split's 32-key steps, all four waves together; two LDS stages in turn ---------------------------------------------------
    // Stage n & 1 holds step n.  While step n computes, the loads of step n + 1 are in flight; they are written to the other stage behind the
    // compute - every wave left that stage's reads (step n - 1) in front of the last barrier - and one barrier publishes them.  The loads of
    // step n + 2 are issued behind that barrier, so nothing is outstanding when it is reached.  k_end is the workgroup's: every wave meets
    // the same barriers.
    // Test builds (FA_KVC_STAGE_DEBUG, fa_kvcache_stage_debug.hpp): the two helpers hold one wave back; FA_KVC_STAGE_RACY moves the step's barrier in front of store_step.
    // Why the racy form can neither hang nor fault here: (1) the barrier only changes places inside the same `if (key0 + kKvcStep < k_end)`, whose
    // condition is the workgroup's (k_begin, k_end and key0 are the same in every wave, `active` is not part of it), so every wave still meets the same
    // number of barriers on every path; (2) the two images are read by compute_step alone, as MFMA operands (kf, v0 / v1): what comes out of them are
    // scores and O, which reach compares, exponentials and stores of VALUES - every address (lds_tile_off of lane constants, row_off / row_index of the
    // lane's row, the page cursor from block_table), every index and every loop bound comes from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[NL];
        int key = k_begin;
        if (key < k_end) {
            load_step(key, st);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st);
        }
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(key + kKvcStep, st);
        auto step = [&](auto bufc, int key0) __attribute__((always_inline)) {
            constexpr int BUF = decltype(bufc)::value;
            kvc_stage_slow_reader((key0 - k_begin) / kKvcStep, wave);
            if (active) compute_step(bufc, key0);
            if (key0 + kKvcStep < k_end) {
#if FA_KVC_STAGE_RACY
                __syncthreads();
#endif
                kvc_stage_slow_writer((key0 - k_begin) / kKvcStep, wave);
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

    // ---- epilogue: the lane's row, columns 16 c + 4 g .. + 3 of every block c ---------------------------------------------------------
    if (!active) return;
    const float lsum = sum_four_groups(l_run);
    if (!row_ok) return;
    // dead = saw no key (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math, and a
    // split partial is written so that the combine propagates it
    const bool live = !(lsum == 0.f);
    const float inv = live ? 1.0f / lsum : 0.f;
    const float lse = live ? m_run * sc + logf(lsum) : (p.n_split > 1 ? -INFINITY : 0.f);
    const int64_t R = row_index(hq, t);
    if (p.n_split == 1) {
        char* orow = (char*)p.o_ptr + 2 * (row_off(p.o, hq, t) + 4 * g);
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

// ONE workgroup per compute unit, as at head_dim 256: a lane holds O^T (128 registers), Q^T (72) and the staging set (36) next to the softmax, about
// 330 registers.  Built for two workgroups (256 registers) the kernels spill 400 bytes a lane; at one, with the register class ahead of the range's
// length in the allocator (build.py EXTRA_FLAGS, the flag of fa_fwd_kvcache_d256.hip), Q^T and the staging set take the AGPRs: no scratch and no
// v_accvgpr moves in the loop.  FA_MLA_WG_PER_CU = 2 builds the spilling variant (the A/B of DESIGN.md).
#ifndef FA_MLA_WG_PER_CU
#define FA_MLA_WG_PER_CU 1
#endif

template <typename T, bool CAUSAL, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, FA_MLA_WG_PER_CU) void fa_fwd_kvcache_mla_kernel(const KvcacheMlaParams mp) {
    kvcache_mla_attn<T, CAUSAL, PAGED>(mp.kp);
}

// kv_new (b, seqlen_new, 1, 576) -> cache rows cache_seqlens[i] .. + seqlen_new - 1: one thread per 16-byte slot of a new row.  Rows at or past the
// capacity seqlen_cache are dropped; PAGED: row (.) % page_size of page min((uint32_t)block_table[i][(.) / page_size], num_blocks - 1), so the
// column read is always inside the table row, and whatever a needed entry holds, nothing is written outside the pool.
template <bool PAGED>
__global__ __launch_bounds__(256) void fa_kvcache_mla_append_kernel(const KvcacheMlaParams mp) {
    const KvcacheKernelParams& p = mp.kp;
    constexpr int SLOTS = kMlaDK / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)p.b * p.seqlen_new * SLOTS;
    if (i >= n) return;
    const int slot = (int)(i % SLOTS);
    const int64_t r = i / SLOTS;
    const int t = (int)(r % p.seqlen_new);
    const int bidx = (int)(r / p.seqlen_new);
    const int cs = p.cache_seqlens[bidx];
    const int row = (cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return;
    int64_t blk = bidx, prow = row;
    if constexpr (PAGED) {
        const int col = row / p.page_size;
        prow = row - col * p.page_size;
        blk = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
    }
    const u32x4 x = *(const u32x4*)((const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row + 8 * slot));
    *(u32x4*)((char*)p.k_cache + 2 * (blk * p.kc.batch + prow * p.kc.row + 8 * slot)) = x;
}

}  // namespace

// append, attention, combine.  mp.kp as the C ABI filled it: d = 512 (the width of V, of o and of the partial planes), h_k = 1, h_ratio = h, k_cache the
// latent cache, k_new the new rows, n_split chosen (kvcache_split over this grid: b x ceil(seqlen_q * h / 64) workgroups a split).
hipError_t launch_fwd_kvcache_mla(KvcacheMlaParams mp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = mp.kp;
    if (kp.d != kMlaDV || mp.d_qk != kMlaDK || kp.h_k != 1) return hipErrorInvalidValue;
    finish_params(kp, (int64_t)kp.b * kp.h * kp.seqlen_q, kMlaRows);
    const bool paged = kp.block_table != nullptr;
    if (kp.k_new != nullptr && kp.seqlen_new > 0) {
        const int64_t n = (int64_t)kp.b * kp.seqlen_new * (kMlaDK / 8);
        hipLaunchKernelGGL(paged ? fa_kvcache_mla_append_kernel<true> : fa_kvcache_mla_append_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mp);
    }
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        auto* kernel = kp.is_causal ? (paged ? fa_fwd_kvcache_mla_kernel<T, true, true> : fa_fwd_kvcache_mla_kernel<T, true, false>)
                                    : (paged ? fa_fwd_kvcache_mla_kernel<T, false, true> : fa_fwd_kvcache_mla_kernel<T, false, false>);
        kvc_launch_attn(kernel, grid, s, mp);
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
