// fa_mla_indexer.hip — the DeepSeek-V3.2 "lightning indexer" in front of sparse MLA decode: every kernel of fa_run_mla_indexer_logits and
// fa_run_mla_indexer_topk.
//
//   logit[t, j] = k_scale[j] * sum_h weights[t, h] * relu(q_idx[t, h, :] . k[j, :])   for the keys j < n_t that token t sees; the topk largest are the
//   `indices` of fa_run_mla_sparse_fwd_kvcache.
//
//   Logits kernel (8: (fp16, bf16) x (16-bit, e4m3 cache) x (contiguous, paged)).  A workgroup serves one token and a range of wg_keys keys; its four
//   waves take a quarter of the range each and share nothing: no LDS, no barrier.  Every key is used once per token, so an LDS image would only be
//   a copy between the load and the MFMA.
//   * S = Q K^T on v_mfma_f32_16x16x32 with Q as the A operand: a tile is 16 heads x 16 keys, lane l holds key l & 15 and heads 4 (l >> 4) + r of
//     each of the h / 16 head blocks.  The head sum is therefore 16 fused multiply-adds inside the lane and one sum over the four 16-lane groups
//     (v_permlane16_swap, v_permlane32_swap); with K as the A operand it would be a 16-lane row reduction per key, four times the cross-lane work.
//   * Q of the token stays in registers for the whole range: 4 head blocks x 4 chunks of 32 columns x 4 registers = 64.  Head blocks past h hold
//     zeros and their MFMAs are skipped by a wave-uniform branch.
//   * The contraction index is permuted so that an FP8 key row is read with 16-byte loads: lane group g reads bytes 16 g .. 16 g + 15 and
//     64 + 16 g .. of the 128-byte row, i.e. chunk c covers columns 16 (g + 4 (c >> 1)) + 8 (c & 1) + 0 .. 7; Q is loaded with the same permutation
//     and a 16-bit cache uses it too (four loads per key).  The codes are widened exactly (v_cvt_scalef32_pk_*_fp8, scale 1) in front of the MFMA.
//   * A step is 32 keys (two column blocks); the loads of the next step are in flight while this one computes.  Contiguous: one descriptor per
//     sequence that ends at row n_t, so a key at or past n_t loads zeros and reads nothing.  Paged: a 16-key block lies in one page (page sizes
//     are multiples of 16), so the table entry is a scalar, fetched one step before its loads, clamped to the pool, and the block gets a descriptor
//     over the visible rows of its page (empty past n_t).  k_scale is loaded by the lanes that store, under j < n_t.
//   * Lanes 0 .. 31 store the step's 32 logits (128 contiguous bytes) under j < n_t: an entry at or past n_t is never written.  Row offsets of
//     `logits` are 64-bit.
//   Selection kernel (1).  One workgroup of 1024 threads per (sequence, token) row; n_t <= topk is the identity list padded with -1.  Otherwise a
//   radix select on u(x) = bits ^ (sign ? ~0 : 1 << 31), most significant digit first: three passes over digits of 12, 10 and 10 bits, each an
//   LDS histogram (ds_add_u32) of the entries that match the prefix so far, a suffix scan of the bins and the choice of the bin in which the
//   topk-th largest key lies.  That leaves the threshold key T and r, the number of entries equal to T that belong to the result.  The ordered
//   compaction gives each of the 16 waves a contiguous range of positions: a counting pass (entries above T, entries equal to T), one barrier,
//   and an emitting pass in which ballots and population counts give every selected position its slot: (entries above T before it) +
//   min(entries equal to T before it, r).  Every pass loads eight entries a thread before it uses the first: one workgroup reads the row five
//   times, and what bounds it is the latency of those reads.  Integer work throughout: the result does not depend on timing.  Entries at or
//   past n_t are never read.
#include "fa_device.hpp"
#include "fa_params.hpp"
#include "fa_mla_indexer.hpp"

namespace fa {

namespace {

// ES = bytes per cache element: 2 = T, 1 = e4m3 codes
template <typename T, int ES, bool PAGED>
__global__ __launch_bounds__(kIdxThreads, 2) void fa_mla_indexer_logits_kernel(const MlaIndexerParams p) {
    constexpr int NHB = 4;                      // head blocks of 16 (h = 64)
    constexpr int NC = kIdxD / 32;              // 16x16x32 MFMAs per tile
    constexpr int NL = ES == 1 ? 2 : 4;         // 16-byte loads per key and lane
    constexpr int ROWB = kIdxD * ES;            // bytes of a key

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t id = blockIdx.x;
    const int chunk = (int)(id % (uint32_t)p.n_chunks);
    const int tok = (int)(id / (uint32_t)p.n_chunks);
    const int t = tok % p.seqlen_q, bidx = tok / p.seqlen_q;
    const int L = idx_len(p.cache_seqlens, bidx, p.seqlen_cache);
    const int n = idx_visible(L, p.seqlen_q, t, p.is_causal);
    // this wave's keys: a quarter of the workgroup's range, cut at n
    const int wave_keys = p.wg_keys / kIdxWaves;
    const int64_t kb64 = (int64_t)chunk * p.wg_keys + (int64_t)wave * wave_keys;
    if (kb64 >= n) return;                      // (no barrier in this kernel: a wave leaves on its own)
    const int k_begin = (int)kb64;
    const int k_end = min(k_begin + wave_keys, n);

    // ---- Q of the token, in the permuted column order, and the weights of the heads this lane sums ------------------------------------------
    const int h = p.h;
    u32x4 qf[NHB][NC];
    float w[NHB][4];
    {
        const char* qtok = (const char*)p.q_ptr + 2 * ((int64_t)bidx * p.q_batch + (int64_t)t * p.q_row);
        const float* wtok = p.w_ptr + ((int64_t)bidx * p.w_batch + (int64_t)t * p.w_row);
        static_for<0, NHB>([&](auto hh) {
            constexpr int hb = decltype(hh)::value;
            const int head = 16 * hb + n16;
            static_for<0, NC>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                const int col = 16 * (g + 4 * (c >> 1)) + 8 * (c & 1);
                qf[hb][c] = head < h ? *(const u32x4*)(qtok + 2 * ((int64_t)head * p.q_head + col)) : u32x4{0u, 0u, 0u, 0u};
            });
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int hd = 16 * hb + 4 * g + r;
                w[hb][r] = hd < h ? wtok[(int64_t)hd * p.w_head] : 0.f;
            });
        });
    }
    const bool hb1 = h > 16, hb2 = h > 32;      // (wave-uniform) head blocks 1 and 2 .. 3 exist

    // ---- key addressing -------------------------------------------------------------------------------------------------------------------
    const uint32_t row_b = (uint32_t)p.k_row;
    const char* kbase = uniform_ptr((const char*)p.k_cache + (PAGED ? (int64_t)0 : (int64_t)bidx * p.k_batch));
    const rsrc_t krs = make_rsrc(kbase, !PAGED && n > 0 ? (uint32_t)(n - 1) * row_b + ROWB : 0u);
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
            prip += kIdxStep;
            while (prip >= P) { prip -= P; pcol += 1; }
        }
    };
    const uint32_t colb = (uint32_t)(16 * g);   // byte offset of this lane group's first load in an FP8 row; a 16-bit row: twice that
    const float* ksp = p.k_scale;

    // the loads of the step at key0: st[kb][i] and the scale of the key this lane stores (lanes 0 .. 31: key0 + lane)
    auto load_step = [&](int key0, u32x4 (&st)[2][NL], float& scale) __attribute__((always_inline)) {
        const float* sp = nullptr;
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            rsrc_t r;
            uint32_t off;
            if constexpr (PAGED) {
                int rip = prip + 16 * kb;
                if (rip >= P) rip -= P;         // (block 1 starts the next page: its entry is pent[1])
                const int64_t page = (int64_t)min(pent[kb], (uint32_t)(p.num_blocks - 1));
                const int nvalid = min(max(n - (key0 + 16 * kb - rip), 0), P);          // visible rows of this page
                r = make_rsrc(kbase + page * p.k_batch, nvalid > 0 ? (uint32_t)(nvalid - 1) * row_b + ROWB : 0u);
                off = (uint32_t)(rip + n16) * row_b;
                if (g == kb && ksp != nullptr) sp = ksp + page * p.ks_batch + (int64_t)(rip + n16) * p.ks_row;
            } else {
                r = krs;
                off = (uint32_t)(key0 + 16 * kb + n16) * row_b;
                if (g == kb && ksp != nullptr) sp = ksp + (int64_t)bidx * p.ks_batch + (int64_t)(key0 + 16 * kb + n16) * p.ks_row;
            }
            static_for<0, NL>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                // FP8: bytes 16 g and 64 + 16 g; 16-bit: chunk i at element 16 (g + 4 (i >> 1)) + 8 (i & 1)
                const uint32_t cb = ES == 1 ? colb + 64u * i : 2u * (colb + 64u * (i >> 1) + 8u * (i & 1));
                st[kb][i] = buf_load16(r, off + cb);
            });
        });
        scale = 1.0f;
        if (sp != nullptr && key0 + lane < n) scale = *sp;         // (sp is null in lanes 32 .. 63 and without k_scale)
        if constexpr (PAGED) {
            advance_entries();
            fetch_entries();                    // the table entries of the step after this one
        }
    };

    float* lrow = p.logits + ((int64_t)bidx * p.lg_batch + (int64_t)t * p.lg_row);

    auto compute_step = [&](int key0, const u32x4 (&st)[2][NL], float scale) __attribute__((always_inline)) {
        f32x4 acc[2][NHB];
        static_for<0, 2>([&](auto bb) {
            static_for<0, NHB>([&](auto hh) { acc[decltype(bb)::value][decltype(hh)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });
        });
        u32x4 kf[2][NC];
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            static_for<0, NC>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                if constexpr (ES == 1) kf[kb][c] = (c & 1) ? idx_widen8<T>(st[kb][c >> 1].z, st[kb][c >> 1].w) : idx_widen8<T>(st[kb][c >> 1].x, st[kb][c >> 1].y);
                else kf[kb][c] = st[kb][c];
            });
        });
        static_for<0, NC>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            static_for<0, 2>([&](auto bb) {
                constexpr int kb = decltype(bb)::value;
                acc[kb][0] = LP<T>::mfma16(qf[0][c], kf[kb][c], acc[kb][0]);
            });
        });
        if (hb1) {
            static_for<0, NC>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                static_for<0, 2>([&](auto bb) {
                    constexpr int kb = decltype(bb)::value;
                    acc[kb][1] = LP<T>::mfma16(qf[1][c], kf[kb][c], acc[kb][1]);
                });
            });
        }
        if (hb2) {
            static_for<0, NC>([&](auto cc) {
                constexpr int c = decltype(cc)::value;
                static_for<0, 2>([&](auto bb) {
                    constexpr int kb = decltype(bb)::value;
                    acc[kb][2] = LP<T>::mfma16(qf[2][c], kf[kb][c], acc[kb][2]);
                    acc[kb][3] = LP<T>::mfma16(qf[3][c], kf[kb][c], acc[kb][3]);
                });
            });
        }
        // ReLU, weights, head sum: inside the lane, then across the four lane groups
        float tot[2];
        static_for<0, 2>([&](auto bb) {
            constexpr int kb = decltype(bb)::value;
            float s = 0.f;
            static_for<0, NHB>([&](auto hh) {
                constexpr int hb = decltype(hh)::value;
                static_for<0, 4>([&](auto rr) {
                    constexpr int r = decltype(rr)::value;
                    s = __builtin_fmaf(w[hb][r], fmaxf(acc[kb][hb][r], 0.f), s);
                });
            });
            tot[kb] = sum_four_groups(s);
        });
        const int key = key0 + lane;            // lanes 0 .. 31: group g holds block g's keys
        if (lane < kIdxStep && key < n) lrow[key] = scale * (g == 0 ? tot[0] : tot[1]);
    };

    // ---- the wave's steps, the next one's loads in flight -------------------------------------------------------------------------------------
    if constexpr (PAGED) {
        pcol = k_begin / P;
        prip = k_begin - pcol * P;
        fetch_entries();
    }
    u32x4 sa[2][NL], sb[2][NL];
    float ca, cb;
    load_step(k_begin, sa, ca);
    for (int key = k_begin; key < k_end; key += 2 * kIdxStep) {
        load_step(key + kIdxStep, sb, cb);      // (past k_end: the descriptors end at n, the loads return zeros and nothing is stored)
        compute_step(key, sa, ca);
        if (key + kIdxStep >= k_end) break;
        load_step(key + 2 * kIdxStep, sa, ca);
        compute_step(key + kIdxStep, sb, cb);
    }
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------------
FA_DEV uint32_t topk_key(float x) {
    const uint32_t b = __builtin_bit_cast(uint32_t, x);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ __launch_bounds__(kTopkThreads) void fa_mla_indexer_topk_kernel(const MlaTopkParams p) {
    constexpr int NW = kTopkThreads / 64;
    constexpr int U = 8;                        // entries a thread loads before it uses the first: eight row reads in flight per thread
    constexpr int kBins = 4096;                 // bins of the widest pass: four per thread
    __shared__ uint32_t hist[kBins];
    __shared__ uint32_t scan_w[NW];
    __shared__ uint32_t sel[2];
    __shared__ uint32_t cnt_gt[NW], cnt_eq[NW];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = blockIdx.x;
    const int t = row % p.seqlen_q, bidx = row / p.seqlen_q;
    const int L = idx_len(p.cache_seqlens, bidx, p.seqlen_cache);
    const int n = idx_visible(L, p.seqlen_q, t, p.is_causal);
    const float* x = p.logits + ((int64_t)bidx * p.lg_batch + (int64_t)t * p.lg_row);
    int32_t* out = p.indices + (int64_t)row * p.topk;
    const int topk = p.topk;

    if (n <= topk) {                            // (the workgroup's condition: every thread takes this branch or none)
        for (int j = tid; j < topk; j += kTopkThreads) out[j] = j < n ? j : -1;
        return;
    }

    // ---- radix select: the key T of the topk-th largest entry, and r = how many entries equal to T are in the result ------------------------------
    // Three passes over digits of 12, 10 and 10 bits, the most significant first.  The first digit is sign, exponent and three mantissa bits: logits of
    // one row share a few exponents, and with the exponent alone as the digit most lanes of a wave would add to the same LDS word.
    uint32_t prefix = 0u, krem = (uint32_t)topk;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
        const int nbins = pass == 0 ? kBins : 1024, per = nbins / kTopkThreads;       // bins a thread scans: 4, then 1
        const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (pass == 1 ? 20 : 10);
        static_for<0, kBins / kTopkThreads>([&](auto kk) { hist[tid + decltype(kk)::value * kTopkThreads] = 0u; });
        __syncthreads();
        for (int base = tid; base < n; base += U * kTopkThreads) {
            float v[U];
            static_for<0, U>([&](auto ee) {
                constexpr int e = decltype(ee)::value;
                const int j = base + e * kTopkThreads;
                v[e] = j < n ? x[j] : 0.f;
            });
            static_for<0, U>([&](auto ee) {
                constexpr int e = decltype(ee)::value;
                const uint32_t u = topk_key(v[e]);
                if (base + e * kTopkThreads < n && (u & himask) == prefix) atomicAdd(&hist[(u >> shift) & (uint32_t)(nbins - 1)], 1u);
            });
        }
        __syncthreads();
        // bins in DESCENDING digit order, `per` consecutive ones a thread: reversed bin rb holds digit nbins - 1 - rb.  An inclusive prefix sum over the
        // reversed bins is the number of matching entries with this digit or a higher one.
        uint32_t c[kBins / kTopkThreads], csum = 0u;
        static_for<0, kBins / kTopkThreads>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            c[k] = k < per ? hist[nbins - 1 - (tid * per + k)] : 0u;
            csum += c[k];
        });
        uint32_t incl = csum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= off) incl += y;
        }
        if (lane == 63) scan_w[wave] = incl;
        __syncthreads();
        for (int v = 0; v < wave; ++v) incl += scan_w[v];
        uint32_t run = incl - csum;
        if (incl >= krem && run < krem) {       // exactly one thread: the matching entries number at least krem
            bool done = false;
            static_for<0, kBins / kTopkThreads>([&](auto kk) {
                constexpr int k = decltype(kk)::value;
                if (!done && k < per) {
                    if (run + c[k] >= krem) {
                        sel[0] = prefix | ((uint32_t)(nbins - 1 - (tid * per + k)) << shift);
                        sel[1] = krem - run;
                        done = true;
                    }
                    run += c[k];
                }
            });
        }
        __syncthreads();
        prefix = sel[0];
        krem = sel[1];
    }
    const uint32_t T = prefix, r = krem;

    // ---- ordered compaction: wave v owns positions [v * seg, (v + 1) * seg) -------------------------------------------------------------------------
    const int seg = ((n + NW * 64 - 1) / (NW * 64)) * 64;
    const int s0 = wave * seg, s1 = min(s0 + seg, n);
    uint32_t gt = 0u, eq = 0u;
    for (int base = s0; base < s1; base += 64 * U) {
        float v[U];
        static_for<0, U>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + 64 * e + lane;
            v[e] = j < s1 ? x[j] : 0.f;
        });
        static_for<0, U>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const bool in = base + 64 * e + lane < s1;
            const uint32_t u = topk_key(v[e]);
            gt += (uint32_t)__popcll(__ballot(in && u > T));
            eq += (uint32_t)__popcll(__ballot(in && u == T));
        });
    }
    if (lane == 0) { cnt_gt[wave] = gt; cnt_eq[wave] = eq; }
    __syncthreads();
    gt = 0u; eq = 0u;
    for (int v = 0; v < wave; ++v) { gt += cnt_gt[v]; eq += cnt_eq[v]; }
    const uint64_t below = (1ull << lane) - 1ull;
    for (int base = s0; base < s1; base += 64 * U) {
        float v[U];
        static_for<0, U>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + 64 * e + lane;
            v[e] = j < s1 ? x[j] : 0.f;
        });
        static_for<0, U>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + 64 * e + lane;
            const uint32_t u = topk_key(v[e]);
            const bool is_gt = j < s1 && u > T, is_eq = j < s1 && u == T;
            const uint64_t bg = __ballot(is_gt), be = __ballot(is_eq);
            const uint32_t g_before = gt + (uint32_t)__popcll(bg & below), e_before = eq + (uint32_t)__popcll(be & below);
            const uint32_t slot = g_before + min(e_before, r);
            // (slot < topk follows from the counts; the test keeps a row that another stream rewrites under the kernel from storing outside the list)
            if ((is_gt || (is_eq && e_before < r)) && slot < (uint32_t)topk) out[slot] = j;
            gt += (uint32_t)__popcll(bg);
            eq += (uint32_t)__popcll(be);
        });
    }
}

}  // namespace

// wg_keys, n_chunks and the grid of a decode logits launch (0: nothing the kernels can run)
int64_t mla_indexer_logits_shape(MlaIndexerParams& p) {
    if (p.h != 16 && p.h != 32 && p.h != 64) return 0;
    // the key range of a workgroup: two workgroups per compute unit over b x seqlen_q tokens, in multiples of one step per wave
    const int64_t tokens = (int64_t)p.b * p.seqlen_q, target = 2 * device_cu_count();
    constexpr int64_t unit = kIdxStep * kIdxWaves;
    int64_t wg = ((int64_t)p.seqlen_cache * tokens + target - 1) / target;
    wg = (wg + unit - 1) / unit * unit;
    wg = wg < unit ? unit : (wg > kIdxMaxWgKeys ? kIdxMaxWgKeys : wg);
    p.wg_keys = (int)wg;
    p.n_chunks = (int)((p.seqlen_cache + wg - 1) / wg);
    const int64_t grid = tokens * p.n_chunks;
    return grid <= 0 || grid >= ((int64_t)1 << 31) ? 0 : grid;
}

hipError_t launch_mla_indexer_logits(MlaIndexerParams p, int dtype, hipStream_t s) {
    const int64_t grid = mla_indexer_logits_shape(p);
    if (grid == 0) return hipErrorInvalidValue;
    const bool paged = p.block_table != nullptr;
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        void (*k)(const MlaIndexerParams);
        if (p.cache_fp8) k = paged ? fa_mla_indexer_logits_kernel<T, 1, true> : fa_mla_indexer_logits_kernel<T, 1, false>;
        else k = paged ? fa_mla_indexer_logits_kernel<T, 2, true> : fa_mla_indexer_logits_kernel<T, 2, false>;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kIdxThreads), 0, s, p);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    return hipGetLastError();
}

hipError_t launch_mla_indexer_topk(const MlaTopkParams& p, hipStream_t s) {
    const int64_t rows = (int64_t)p.b * p.seqlen_q;
    if (rows <= 0 || rows >= ((int64_t)1 << 31) || p.topk < 32 || p.topk % 32 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fa_mla_indexer_topk_kernel, dim3((unsigned)rows), dim3(kTopkThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace fa
