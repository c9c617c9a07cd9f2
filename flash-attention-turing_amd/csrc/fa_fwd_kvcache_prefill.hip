// fa_fwd_kvcache_prefill.hip — attention over a KV cache for prompt chunks: 64-row workgroups (fa_kvcache_options_v8: row_tile = 64).
//
//   The decode kernels (kvcache_attn of fa_kvcache_attn.hpp) cut the seqlen_q x (h / h_k) packed query rows of a KV head into tiles of 16, and every tile streams
//   the whole visible K / V of its head from memory on its own.  A chunk of a prompt - hundreds or thousands of rows over a paged or 8-bit cache,
//   which fwd / varlen_fwd cannot read - brings hundreds of such tiles per KV head.  Here a workgroup serves 64 packed rows:
//   * four waves, wave w owns rows 16 w .. 16 w + 15 of the tile with the per-row mapping of the decode kernel: S^T = K Q^T on
//     v_mfma_f32_16x16x32, a lane owns ONE query row (lane & 15) with private m / l, Q^T stays in registers for the whole split, and
//     O^T += V^T P^T takes P^T straight from the score accumulator.
//   * all four waves walk the SAME 32-key steps of the split in order.  The 32 K rows and 32 V rows of a step are loaded from the cache once per
//     workgroup - 64 rows of SLOTS 16-byte slots, a quarter per wave - through registers into LDS images every wave reads: K as the A operand
//     (16-byte row reads), V^T through ds_read_b64_tr_b16, both in the swizzled layout of lds_tile_off.  The images are double-buffered: the
//     loads of step n + 1 are in flight while step n computes, then written to the other buffer, one barrier per step.
//   * no merge at the end: each wave owns its rows, so the epilogue writes o / lse (unsplit) or the fp32 partials in the plane layout of the
//     decode kernels (split) straight from the accumulators.  Append, partial planes and combine are the unchanged kernels.
//   * 8-bit cache: the codes are widened (widen8, exact) when the images are written, so images, MFMAs and softmax are those of the 16-bit
//     kernels; k_descale folds into the scale and v_descale into the final normalisation.
//   * paged cache: the rule of the decode kernels - the 16 keys of an MFMA block share a page, entries are clamped min(uint32(entry), num_blocks -
//     1), the descriptors end at L so that rows at or past L read as zeros, and the table entries of a step are fetched one step ahead.
//   * causal: a tile's key range ends at the last key its last row sees, min(L, L - sq + t_last + 1) (the 16-row causal kernel walks to L);
//     a split that lies wholly past it writes an empty partial (LSE = -inf).
//   * a wave whose 16 rows all lie past the sequence's rows takes part in staging and barriers only.
//   One instantiation per (dtype, head_dim, causal, layout, cache element, dense / ragged): 64 attention kernels.  A window, a soft cap, sinks, a
//   tree mask, rotary and head_dim 256 are refused by the C ABI with row_tile = 64: nothing here serves them.
#include "fa_kvcache_launch.hpp"
#include "fa_kvcache_stage.hpp"

namespace fa {

namespace {

constexpr int kKvpRows = kKvcPrefillRows;    // packed query rows of a workgroup: 16 per wave

template <int D>
struct KvpLds {
    static constexpr int kImage = kKvcStep * D * 2;     // one image: 32 rows x D 16-bit
    static constexpr int kStage = 2 * kImage;           // K image, then V image
    static constexpr int kBytes = 2 * kStage;           // two stages
};

template <typename T, int D, bool CAUSAL, bool PAGED, int ES, bool RAGGED>
FA_DEV void kvcache_prefill_attn(const KvcacheKernelParams& p, const KvcacheRaggedParams* rg) {
    static_assert(ES == 1 || ES == 2, "cache elements are 16-bit (the dtype of q) or 8-bit (e4m3)");
    constexpr int NC = D / 32;          // 16x16x32 MFMAs per 16 keys of S^T (d chunks)
    constexpr int NO = D / 16;          // O^T blocks of 16 columns
    constexpr int SLOTS = D * ES / 16;  // 16-byte slots per cache row: 16, 8, 8, 4
    constexpr int RPW = 64 / SLOTS;     // cache rows per wave-wide 16-byte load: 4, 8, 8, 16 (a divisor of 16: they share a 16-key block)
    constexpr int RPP = kKvcWaves * RPW;        // rows per pass of the workgroup over the 64 rows of a step (32 of K, then 32 of V)
    constexpr int NP = 64 / RPP;        // passes = loads per lane and step: 4, 2, 2, 1
    __shared__ __attribute__((aligned(16))) char smem[KvpLds<D>::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    int n_tiles = p.n_row_tiles;                // RAGGED: the tile slots of a KV head, and `bh` below is the KV head
    if constexpr (RAGGED) n_tiles = rg->slots;
    const int split = id % p.n_split, rest = id / p.n_split;
    int tile = rest % n_tiles;
    const int bh = rest / n_tiles;
    int bidx = bh / p.h_k, kvh = bh - bidx * p.h_k;
    int sq = p.seqlen_q;                        // query rows of this sequence
    int64_t q0 = 0;                             // RAGGED: its first packed row
    if constexpr (RAGGED) {
        kvh = bh;
        if (rg->compact) {
            const int slot = tile;
            if (!kvc_slot_lookup<kKvpRows>(rg->cu_q, p.b, p.h_ratio, (uint32_t)slot, bidx, tile)) return;      // a slack slot: nothing to write
        } else {
            bidx = tile / p.n_row_tiles;        // (n_row_tiles = tiles of max_seqlen_q here)
            tile -= bidx * p.n_row_tiles;
        }
        const int c0 = rg->cu_q[bidx];
        sq = __builtin_amdgcn_readfirstlane(rg->cu_q[bidx + 1] - c0);
        q0 = __builtin_amdgcn_readfirstlane(c0);
        if (tile * kKvpRows >= sq * p.h_ratio) return;      // (plain slots of a sequence shorter than max_seqlen_q)
    }
    const int L = RAGGED ? kvc_len_ragged(*rg, bidx) : kvc_len(p, bidx);
    const int rows_tile = sq * p.h_ratio;
    // row (hq_, t_) of the LSE and of the partial planes; element offset of its row in q / o (st = p.q or p.o)
    auto row_index = [&](int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (RAGGED) return (int64_t)hq_ * rg->total_q + q0 + t_;
        else return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t_;
    };
    auto row_off = [&](const TStride& st, int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (RAGGED) return (q0 + t_) * st.row + (int64_t)hq_ * st.head;
        else return (int64_t)bidx * st.batch + (int64_t)t_ * st.row + (int64_t)hq_ * st.head;
    };
    // CAUSAL: the tile's keys end where its last row's do (t_last <= sq - 1, so k_hi <= L; it may be <= 0: the tile sees nothing)
    int k_hi = L;
    if constexpr (CAUSAL) {
        const int t_last = (min((tile + 1) * kKvpRows, rows_tile) - 1) / p.h_ratio;
        k_hi = __builtin_amdgcn_readfirstlane(min(L, L - sq + t_last + 1));
    }
    const int k_begin = split * p.split_keys;
    const int k_end = min(k_begin + p.split_keys, k_hi);
    // 8-bit cache: S = (Q . K codes) x k_descale, so the descale rides on the softmax scale; O = (P . V codes) x v_descale / l
    float kd = 1.f, vd = 1.f;
    if constexpr (ES == 1) {
        if (p.k_descale != nullptr) kd = p.k_descale[(int64_t)bidx * p.kds_batch + (int64_t)kvh * p.kds_head];
        if (p.v_descale != nullptr) vd = p.v_descale[(int64_t)bidx * p.vds_batch + (int64_t)kvh * p.vds_head];
    }
    const float c = ES == 1 ? p.scale_log2e * kd : p.scale_log2e;
    const float sc = ES == 1 ? p.scale * kd : p.scale;

    if (p.n_split > 1 && k_begin >= k_end) {        // nothing to read in this split: an empty partial (LSE = -inf), O is never looked at
        if (tid < kKvpRows) {
            const int pr = tile * kKvpRows + tid;
            if (pr < rows_tile) {
                const int t = pr / p.h_ratio, hq = kvh * p.h_ratio + (pr - t * p.h_ratio);
                p.ws_lse[(int64_t)split * p.rows_total + row_index(hq, t)] = -INFINITY;
            }
        }
        return;
    }

    // ---- this lane's query row: Q^T fragments for the whole split, visible-key limit -------------------------------------------------
    const bool active = tile * kKvpRows + wave * kKvcRows < rows_tile;      // (wave-uniform) false: staging and barriers only
    const int pr = tile * kKvpRows + wave * kKvcRows + n16;
    const bool row_ok = pr < rows_tile;
    const int t = row_ok ? pr / p.h_ratio : 0;
    const int hq = kvh * p.h_ratio + (row_ok ? pr - t * p.h_ratio : 0);
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

    // ---- staging: what this wave loads in pass j of a step ---------------------------------------------------------------------------
    // row R = j * RPP + wave * RPW + lane / SLOTS of the step's 64 rows (R < 32: K row R, else V row R - 32), 16-byte slot lane % SLOTS of it.
    // The RPW rows of a wave lie in one 16-key block, and whether they are K or V is a constant of the pass (NP > 1) or of the wave (NP = 1).
    const int lrow = lane / SLOTS, lslot = lane % SLOTS;
    auto pass_is_v = [&](int j) __attribute__((always_inline)) { return NP == 1 ? wave >= 2 : j * RPP >= 32; };
    auto pass_row0 = [&](int j) __attribute__((always_inline)) { return (j * RPP + wave * RPW) & 31; };     // first row of the wave's, 0 .. 31
    const uint32_t krow_b = (uint32_t)(p.kc.row * ES), vrow_b = (uint32_t)(p.vc.row * ES);
    const char* kbase = uniform_ptr((const char*)p.k_cache + ES * ((int64_t)(PAGED ? 0 : bidx) * p.kc.batch + (int64_t)kvh * p.kc.head));
    const char* vbase = uniform_ptr((const char*)p.v_cache + ES * ((int64_t)(PAGED ? 0 : bidx) * p.vc.batch + (int64_t)kvh * p.vc.head));
    // contiguous: one descriptor per tensor, ending at row L (rows at or past L read as zeros; row indices are clamped to L, and L x row
    // stride < 2^31 by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * krow_b + ES * D : 0u);
    const rsrc_t vrs = make_rsrc(vbase, L > 0 ? (uint32_t)(L - 1) * vrow_b + ES * D : 0u);
    // Paged cache: a step's two 16-key blocks each lie in one page.  A pass builds the descriptor of its block, based at the block's first row
    // in its page and ending at the sequence's last valid row in the block (a block wholly past L has an empty range: whatever its table entry
    // says is never read).  The table entries of the step after the one being loaded are fetched (scalar loads) together with that load; the
    // cursor (column, row in page) moves by one step without a division.  Columns are clamped to the table row, entries to the pool.
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
    auto load_step = [&](int key0, u32x4 (&st)[NP]) __attribute__((always_inline)) {
        static_for<0, NP>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const bool is_v = pass_is_v(j);
            const int r0 = pass_row0(j);
            const uint32_t row_b = is_v ? vrow_b : krow_b;
            if constexpr (PAGED) {
                const int blk = r0 >> 4;                                    // (wave-uniform)
                const int valid = min(max(L - (key0 + 16 * blk), 0), 16);
                const int64_t page = min(blk ? pg1 : pg0, (uint32_t)(p.num_blocks - 1));
                const int prow = blk ? rw1 : rw0;
                const TStride& cs = is_v ? p.vc : p.kc;
                const char* base = uniform_ptr((is_v ? vbase : kbase) + ES * (page * cs.batch + (int64_t)prow * cs.row));
                const rsrc_t r = make_rsrc(base, valid > 0 ? (uint32_t)(valid - 1) * row_b + ES * D : 0u);
                st[j] = buf_load16(r, (uint32_t)((r0 & 15) + lrow) * row_b + 16 * lslot);
            } else {
                const uint32_t off = (uint32_t)min(key0 + r0 + lrow, L) * row_b + 16 * lslot;
                if constexpr (NP == 1) st[j] = is_v ? buf_load16(vrs, off) : buf_load16(krs, off);
                else st[j] = buf_load16(j * RPP >= 32 ? vrs : krs, off);
            }
        });
        if constexpr (PAGED) fetch_pages();     // the table entries of the step after this one
    };
    // registers -> the images of stage BUF (ES = 1: widened to T first, so the images and their reads are those of the 16-bit cache)
    auto store_step = [&](auto bufc, const u32x4 (&st)[NP]) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        static_for<0, NP>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            FA_LDS char* img = (FA_LDS char*)smem + BUF * KvpLds<D>::kStage + (pass_is_v(j) ? KvpLds<D>::kImage : 0);
            const uint32_t row = (uint32_t)(pass_row0(j) + lrow);
            if constexpr (ES == 2) {
                *(FA_LDS u32x4*)(img + lds_tile_off<D>(row, lslot)) = st[j];
            } else {
                *(FA_LDS u32x4*)(img + lds_tile_off<D>(row, 2 * lslot)) = widen8<T>(st[j].x, st[j].y);
                *(FA_LDS u32x4*)(img + lds_tile_off<D>(row, 2 * lslot + 1)) = widen8<T>(st[j].z, st[j].w);
            }
        });
    };

    // transposed-read addresses of this lane (fa_device.hpp lds_tile_off image): block c, half hh -> rows hh * 16 + 4 g + q, columns 16 c + 4 p
    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 oacc[NO];
    static_for<0, NO>([&](auto cc) {
        oacc[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(oacc[decltype(cc)::value]));
    });
    float m_run = kNegBig, l_run = 0.f;

    // one 32-key step of this wave's 16 rows over the images of stage BUF: the step of the decode kernel with both operands from LDS
    auto compute_step = [&](auto bufc, int key0) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        const FA_LDS char* kimg = (const FA_LDS char*)smem + BUF * KvpLds<D>::kStage;
        const FA_LDS char* vimg = kimg + KvpLds<D>::kImage;
        f32x4 s[2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            static_for<0, NC>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                const u32x4 kf = *(const FA_LDS u32x4*)(kimg + lds_tile_off<D>(16 * b + n16, 4 * ci + g));
                s[b] = LP<T>::mfma16(kf, qf[ci], s[b]);
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
        const u32x4 pf = pack8<T>(pe);
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            oacc[ci] *= alpha;
        });
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            oacc[ci] = LP<T>::mfma16(tr_frag<D>(vimg, ci, g, q4, p4), pf, oacc[ci]);
        });
    };

    // ---- the split's 32-key steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp) ---------------------------
    // k_begin and k_end are the workgroup's: every wave meets the same barriers.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, part (2) (part (1) stands at kvc_stage_step): the images are read by compute_step alone, as
    // MFMA operands (kf, tr_frag): what comes out of them are scores and O, which reach compares, exponentials and stores of VALUES - every address
    // (lds_tile_off of lane constants, row_off / row_index of the lane's row, the page cursor from block_table), every index and every loop bound comes
    // from the parameters.  A stale image gives wrong numbers.
    {
        u32x4 st[NP];
        int key = k_begin;
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
            kvc_stage_step(std::integral_constant<int, 0>{}, key, k_begin, k_end, wave, active, load, store, compute);
            if (key + kKvcStep < k_end) kvc_stage_step(std::integral_constant<int, 1>{}, key + kKvcStep, k_begin, k_end, wave, active, load, store, compute);
        }
    }

    // ---- epilogue: the lane's row, columns 16 c + 4 g .. + 3 of every block c ---------------------------------------------------------
    if (!active) return;
    const float lsum = sum_four_groups(l_run);
    if (!row_ok) return;
    // dead = saw no key (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math, and a
    // split partial is written so that the combine propagates it
    const bool live = !(lsum == 0.f);
    const float inv = live ? (ES == 1 ? vd / lsum : 1.0f / lsum) : 0.f;
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
        float* prow = p.ws_o + ((int64_t)split * p.rows_total + R) * D + 4 * g;
        if (live) {
            static_for<0, NO>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                *(f32x4*)(prow + 16 * ci) = f32x4{oacc[ci][0] * inv, oacc[ci][1] * inv, oacc[ci][2] * inv, oacc[ci][3] * inv};
            });
        }
        if (g == 0) p.ws_lse[(int64_t)split * p.rows_total + R] = lse;
    }
}

template <typename T, int D, bool CAUSAL, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_prefill_kernel(const KvcacheKernelParams p) {
    kvcache_prefill_attn<T, D, CAUSAL, PAGED, ES, false>(p, nullptr);
}

template <typename T, int D, bool CAUSAL, bool PAGED, int ES>
__global__ __launch_bounds__(kKvcThreads, 2) void fa_fwd_kvcache_ragged_prefill_kernel(const KvcacheRaggedParams rp) {
    kvcache_prefill_attn<T, D, CAUSAL, PAGED, ES, true>(rp.kp, &rp);
}

// p as the dense / ragged launcher finished it for 64-row tiles (row tiles or slots, split, partial planes)
template <typename P>
hipError_t launch_prefill_attn(const P& p, int dtype, unsigned grid, hipStream_t s) {
    kvc_dispatch<64, 128>(kvc_kp(p), dtype, [&](auto leaf) {
        using K = decltype(leaf);
        using T = typename K::T;
        if (kvc_kp(p).is_causal) kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_prefill_kernel<T, K::D, true, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_prefill_kernel<T, K::D, true, K::PAGED, K::ES>), grid, s, p);
        else kvc_launch_attn(kvc_pick<P>(fa_fwd_kvcache_prefill_kernel<T, K::D, false, K::PAGED, K::ES>, fa_fwd_kvcache_ragged_prefill_kernel<T, K::D, false, K::PAGED, K::ES>), grid, s, p);
    });
    return hipGetLastError();
}

}  // namespace

// grid = b x h_k x row tiles x n_split (dense), slots x h_k x n_split (ragged)
hipError_t launch_kvcache_prefill_attn(const KvcacheKernelParams& kp, int dtype, unsigned grid, hipStream_t s) { return launch_prefill_attn(kp, dtype, grid, s); }
hipError_t launch_kvcache_prefill_attn(const KvcacheRaggedParams& rp, int dtype, unsigned grid, hipStream_t s) { return launch_prefill_attn(rp, dtype, grid, s); }

}  // namespace fa
