// fa_mla_indexer_topk_split.hip — the top-k selection of fa_mla_indexer.hip with one logits row spread over several workgroups (fa_run_mla_indexer_topk_v2 with
// num_splits > 1).  The contract is that kernel's, word for word, and the work is integer throughout: for every input and every split count the `indices`
// buffer equals that of the one-workgroup kernel in every word.
//
//   A row's positions [0, n_t) are cut on the device into S contiguous chunks of ceil(n_t / 64 S) * 64 positions (the last ones shorter or empty), so a short
//   sequence in a large cache still spreads.  Five launches on the stream, grid rows x S (the first: rows x 6), 1024 threads each; a workgroup never reads what
//   another workgroup of its own launch writes, so the only ordering is stream order: no spin loop, no grid barrier, no cooperative launch.
//     zero     clears the row histograms in the workspace (a kernel, not a memset node: the call stays capturable whatever the runtime does with those).
//     hist<0>  histograms the 12-bit first digit of its chunk in LDS (ds_add_u32, eight loads in flight per thread, as in the one-workgroup kernel) and adds
//              its non-zero bins to the row's 4096-bin histogram in the workspace with global_atomic_add_u32 (no return value: nothing waits).  Integer adds
//              commute, so the sum does not depend on the order of the workgroups.
//     hist<1>  every chunk redoes the suffix scan of that row histogram (16 KB out of L2) and so derives the same 12-bit prefix and remaining count; then the
//              second digit (10 bits) of the entries that match the prefix, in the same way.
//     hist<2>  scans both, histograms the last digit (10 bits) of the entries that match the 22-bit prefix, adds it to the row, and also leaves a record of its
//              own: that private 1024-bin histogram and the count of its entries ABOVE the 22-bit prefix.
//     emit     scans all three row histograms: the threshold key T and r, the number of entries equal to T that belong to the result.  The entries above T and
//              equal to T in all EARLIER chunks come from their records - thread d sums bin d of the earlier chunks (coalesced 4 KB rows), bins above T's last
//              digit and the above-prefix counts go through one block reduction - so no chunk re-reads another chunk's logits.  Then the counting pass and the
//              ballot / population-count emitting pass of the one-workgroup kernel over its own chunk, with slot = (entries above T before it) + min(entries
//              equal to T before it, r): chunk c thereby gets min(eq_c, max(r - eq_before, 0)) of the threshold ties.
//   A row with n_t <= topk is left alone by zero-cost early returns in the hist launches and chunk 0 of the emit launch writes its identity list; an empty chunk
//   returns at once in every launch, and since chunks are contiguous no non-empty chunk ever reads the record of an empty one.
//   Workspace, per row: 4096 + 1024 + 1024 histogram words, then S records of kTopkRecWords words (1024 bins, the above-prefix count, padding to 64 bytes).
//   Only the histograms are accumulated into, and the zero launch clears them in every call: a caller's workspace may hold anything.
#include "fa_device.hpp"
#include "fa_params.hpp"
#include "fa_mla_indexer.hpp"

namespace fa {

namespace {

constexpr int kNW = kTopkThreads / 64;
constexpr int kU = 8;                           // entries a thread loads before it uses the first

struct Chunk {
    int n, c0, c1;                              // the row's visible length; this workgroup's positions [c0, c1) (c0 >= c1: nothing to do)
    const float* x;
    uint32_t* ws;                               // the row's workspace
    int row, c;
};

FA_DEV Chunk topk_chunk(const MlaTopkSplitParams& p) {
    Chunk k;
    const uint32_t S = (uint32_t)p.n_split;
    k.row = (int)(blockIdx.x / S);
    k.c = (int)(blockIdx.x % S);
    const int t = k.row % p.seqlen_q, bidx = k.row / p.seqlen_q;
    const int L = idx_len(p.cache_seqlens, bidx, p.seqlen_cache);
    k.n = idx_visible(L, p.seqlen_q, t, p.is_causal);
    k.x = p.logits + ((int64_t)bidx * p.lg_batch + (int64_t)t * p.lg_row);
    k.ws = p.ws + (int64_t)k.row * mla_topk_row_words(p.n_split);
    const int64_t unit = 64 * (int64_t)S;
    const int64_t len = ((int64_t)k.n + unit - 1) / unit * 64, b0 = (int64_t)k.c * len;
    k.c0 = (int)(b0 < k.n ? b0 : k.n);
    k.c1 = (int)(b0 + len < k.n ? b0 + len : k.n);
    return k;
}

// One step of the radix select over a finished row histogram `bins` (global memory, written by an earlier launch): bins in DESCENDING digit order, `per`
// consecutive ones a thread; an inclusive prefix sum over the reversed bins is the number of matching entries with this digit or a higher one.  The thread in
// whose bins the krem-th largest lies publishes the longer prefix and what remains.  Every thread of the workgroup calls this.
template <int NBINS, int SHIFT>
FA_DEV void topk_scan_row(const uint32_t* bins, uint32_t& prefix, uint32_t& krem, uint32_t* scan_w, uint32_t* sel) {
    constexpr int per = NBINS / kTopkThreads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t c[per], csum = 0u;
    static_for<0, per>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        c[k] = bins[NBINS - 1 - (tid * per + k)];
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
    if (incl >= krem && run < krem) {           // exactly one thread: the matching entries number at least krem
        bool done = false;
        static_for<0, per>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            if (!done) {
                if (run + c[k] >= krem) {
                    sel[0] = prefix | ((uint32_t)(NBINS - 1 - (tid * per + k)) << SHIFT);
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
    __syncthreads();                            // (sel and scan_w are written again by the next step)
}

// sum of v over the workgroup, in every thread
FA_DEV uint32_t block_sum(uint32_t v, uint32_t* part) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < kNW; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(kTopkThreads) void fa_mla_topk_split_zero_kernel(const MlaTopkSplitParams p) {
    constexpr uint32_t blocks = kTopkHistWords / kTopkThreads;
    const uint32_t row = blockIdx.x / blocks, blk = blockIdx.x % blocks;
    p.ws[(int64_t)row * mla_topk_row_words(p.n_split) + blk * kTopkThreads + threadIdx.x] = 0u;
}

// PASS 0, 1, 2: the digit of 12, 10, 10 bits
template <int PASS>
__global__ __launch_bounds__(kTopkThreads) void fa_mla_topk_split_hist_kernel(const MlaTopkSplitParams p) {
    constexpr int NBINS = PASS == 0 ? 4096 : 1024, per = NBINS / kTopkThreads;
    constexpr int shift = PASS == 0 ? 20 : (PASS == 1 ? 10 : 0);
    constexpr uint32_t himask = PASS == 0 ? 0u : 0xffffffffu << (PASS == 1 ? 20 : 10);
    constexpr int off = PASS == 0 ? 0 : (PASS == 1 ? 4096 : 5120);      // this digit's row histogram in the workspace
    __shared__ uint32_t hist[NBINS];
    __shared__ uint32_t scan_w[kNW];
    __shared__ uint32_t sel[2];

    const int tid = threadIdx.x;
    const Chunk k = topk_chunk(p);
    if (k.n <= p.topk || k.c0 >= k.c1) return;  // (the workgroup's condition: every thread leaves or none)
    uint32_t prefix = 0u, krem = (uint32_t)p.topk;
    if constexpr (PASS >= 1) topk_scan_row<4096, 20>(k.ws, prefix, krem, scan_w, sel);
    if constexpr (PASS >= 2) topk_scan_row<1024, 10>(k.ws + 4096, prefix, krem, scan_w, sel);

    static_for<0, per>([&](auto kk) { hist[tid + decltype(kk)::value * kTopkThreads] = 0u; });
    __syncthreads();
    uint32_t above = 0u;                        // PASS 2: this thread's entries above the 22-bit prefix
    for (int base = k.c0 + tid; base < k.c1; base += kU * kTopkThreads) {
        float v[kU];
        static_for<0, kU>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + e * kTopkThreads;
            v[e] = j < k.c1 ? k.x[j] : 0.f;
        });
        static_for<0, kU>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const uint32_t u = topk_key(v[e]);
            if (base + e * kTopkThreads < k.c1) {
                if ((u & himask) == prefix) atomicAdd(&hist[(u >> shift) & (uint32_t)(NBINS - 1)], 1u);
                if constexpr (PASS == 2) above += (u & himask) > prefix ? 1u : 0u;
            }
        });
    }
    __syncthreads();
    uint32_t* rec = k.ws + kTopkHistWords + (int64_t)k.c * kTopkRecWords;
    static_for<0, per>([&](auto kk) {
        const int bin = tid + decltype(kk)::value * kTopkThreads;
        const uint32_t cnt = hist[bin];
        if (cnt != 0u) atomicAdd(k.ws + off + bin, cnt);
        if constexpr (PASS == 2) rec[bin] = cnt;
    });
    if constexpr (PASS == 2) {
        const uint32_t tot = block_sum(above, scan_w);
        if (tid == 0) rec[1024] = tot;
    }
}

__global__ __launch_bounds__(kTopkThreads) void fa_mla_topk_split_emit_kernel(const MlaTopkSplitParams p) {
    __shared__ uint32_t scan_w[kNW];
    __shared__ uint32_t sel[2];
    __shared__ uint32_t cnt_gt[kNW], cnt_eq[kNW];
    __shared__ uint32_t eq_rec;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Chunk k = topk_chunk(p);
    const int topk = p.topk;
    int32_t* out = p.indices + (int64_t)k.row * topk;
    if (k.n <= topk) {
        if (k.c == 0)
            for (int j = tid; j < topk; j += kTopkThreads) out[j] = j < k.n ? j : -1;
        return;
    }
    if (k.c0 >= k.c1) return;

    uint32_t T = 0u, r = (uint32_t)topk;
    topk_scan_row<4096, 20>(k.ws, T, r, scan_w, sel);
    topk_scan_row<1024, 10>(k.ws + 4096, T, r, scan_w, sel);
    topk_scan_row<1024, 0>(k.ws + 5120, T, r, scan_w, sel);

    // ---- entries above T and equal to T in the chunks before this one, from their records: thread d holds bin d ------------------------------------------
    const uint32_t* recs = k.ws + kTopkHistWords;
    const uint32_t dT = T & 1023u;
    uint32_t mine = 0u;
    for (int cc = 0; cc < k.c; ++cc) mine += recs[(int64_t)cc * kTopkRecWords + tid];
    if ((uint32_t)tid == dT) eq_rec = mine;
    uint32_t part = (uint32_t)tid > dT ? mine : 0u;
    if (tid < k.c) part += recs[(int64_t)tid * kTopkRecWords + 1024];   // (at most kTopkMaxSplits = 64 chunks)
    const uint32_t gt0 = block_sum(part, scan_w), eq0 = eq_rec;          // (block_sum's barrier orders eq_rec)

    // ---- ordered compaction of the chunk: wave v owns positions [c0 + v * seg, c0 + (v + 1) * seg) -----------------------------------------------------------
    const int seg = ((k.c1 - k.c0 + kNW * 64 - 1) / (kNW * 64)) * 64;
    const int s0 = min(k.c0 + wave * seg, k.c1), s1 = min(s0 + seg, k.c1);
    const float* x = k.x;
    uint32_t gt = 0u, eq = 0u;
    for (int base = s0; base < s1; base += 64 * kU) {
        float v[kU];
        static_for<0, kU>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + 64 * e + lane;
            v[e] = j < s1 ? x[j] : 0.f;
        });
        static_for<0, kU>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const bool in = base + 64 * e + lane < s1;
            const uint32_t u = topk_key(v[e]);
            gt += (uint32_t)__popcll(__ballot(in && u > T));
            eq += (uint32_t)__popcll(__ballot(in && u == T));
        });
    }
    if (lane == 0) { cnt_gt[wave] = gt; cnt_eq[wave] = eq; }
    __syncthreads();
    gt = gt0; eq = eq0;
    for (int v = 0; v < wave; ++v) { gt += cnt_gt[v]; eq += cnt_eq[v]; }
    const uint64_t below = (1ull << lane) - 1ull;
    for (int base = s0; base < s1; base += 64 * kU) {
        float v[kU];
        static_for<0, kU>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + 64 * e + lane;
            v[e] = j < s1 ? x[j] : 0.f;
        });
        static_for<0, kU>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            const int j = base + 64 * e + lane;
            const uint32_t u = topk_key(v[e]);
            const bool is_gt = j < s1 && u > T, is_eq = j < s1 && u == T;
            const uint64_t bg = __ballot(is_gt), be = __ballot(is_eq);
            const uint32_t g_before = gt + (uint32_t)__popcll(bg & below), e_before = eq + (uint32_t)__popcll(be & below);
            const uint32_t slot = g_before + min(e_before, r);
            // (slot < topk follows from the counts; the test keeps a row that another stream rewrites between the launches from storing outside the list)
            if ((is_gt || (is_eq && e_before < r)) && slot < (uint32_t)topk) out[slot] = j;
            gt += (uint32_t)__popcll(bg);
            eq += (uint32_t)__popcll(be);
        });
    }
}

}  // namespace

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------------------
int64_t mla_topk_workspace_bytes(int64_t rows, int n_split) { return n_split > 1 ? rows * mla_topk_row_words(n_split) * 4 : 0; }

// the most chunks a row of this capacity is ever cut into: chunk bounds are multiples of 64.  (A capacity within two passes of 2^31 stays with the one-workgroup
// kernel: the loops here step past the end of a chunk in 32-bit positions.)
int mla_topk_max_splits(int seqlen_cache) {
    if (seqlen_cache > INT32_MAX - 2 * kU * kTopkThreads) return 1;
    const int64_t blocks = ((int64_t)seqlen_cache + 63) / 64;
    return (int)(blocks < kTopkMaxSplits ? (blocks < 1 ? 1 : blocks) : kTopkMaxSplits);
}

// The automatic rule: see DESIGN.md ("Top-k selection over several workgroups") for the table it was read from.
int mla_topk_auto_splits(int64_t rows, int seqlen_cache, int topk) {
    if (rows <= 0 || seqlen_cache <= topk || seqlen_cache < kTopkAutoMinLen) return 1;
    const int64_t by_rows = device_cu_count() / rows;                  // chunks until every compute unit has a workgroup
    const int64_t by_len = seqlen_cache / kTopkAutoMinChunk;            // no chunk shorter than this
    int64_t s = by_rows < by_len ? by_rows : by_len;
    const int cap = mla_topk_max_splits(seqlen_cache);
    if (s > cap) s = cap;
    return s < kTopkAutoMinSplits ? 1 : (int)s;
}

hipError_t launch_mla_indexer_topk_split(const MlaTopkSplitParams& p, hipStream_t s) {
    const int64_t rows = (int64_t)p.b * p.seqlen_q;
    if (rows <= 0 || p.n_split < 2 || p.n_split > mla_topk_max_splits(p.seqlen_cache) || rows * p.n_split >= ((int64_t)1 << 31) ||
        rows * (kTopkHistWords / kTopkThreads) >= ((int64_t)1 << 31) || p.topk < 32 || p.topk % 32 != 0 || p.ws == nullptr)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(rows * p.n_split)), block(kTopkThreads);
    hipLaunchKernelGGL(fa_mla_topk_split_zero_kernel, dim3((unsigned)(rows * (kTopkHistWords / kTopkThreads))), block, 0, s, p);
    hipLaunchKernelGGL(fa_mla_topk_split_hist_kernel<0>, grid, block, 0, s, p);
    hipLaunchKernelGGL(fa_mla_topk_split_hist_kernel<1>, grid, block, 0, s, p);
    hipLaunchKernelGGL(fa_mla_topk_split_hist_kernel<2>, grid, block, 0, s, p);
    hipLaunchKernelGGL(fa_mla_topk_split_emit_kernel, grid, block, 0, s, p);
    return hipGetLastError();
}

}  // namespace fa
