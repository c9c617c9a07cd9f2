// fa_kvcache_attn.hpp — the attention body of decode attention over a KV cache: kvcache_attn and what it needs.  Included by every fa_fwd_kvcache*.hip;
// each of them wraps the instantiations it owns in __global__ kernels of its own (the templates below sit in an anonymous namespace).
//
// Decode reads every K/V byte of the valid cache prefix once per step: the work is HBM-bound, and the prefill kernels are the wrong shape
// for it (256 query rows per workgroup, one workgroup per query head).  Here:
//   * the seqlen_q x (h / h_k) query rows of one KV head are PACKED into row tiles of 16 (packed row r = t * h_ratio + j: query position t,
//     query head kv_head * h_ratio + j), so K/V are read once per KV head and row tile, not once per query head;
//   * the key range is split over workgroups (fixed multiples of kKvcStep over seqlen_cache, sized by the host from the capacity) so that
//     batch 1 fills the chip; the splits leave fp32 partial O / LSE in a workspace and a combine kernel merges them by their LSE in fixed order;
//   * one workgroup = 4 waves; wave w takes the 32-key steps w, w + 4, ... of its split with a private online softmax and the waves are
//     merged through LDS at the end.
// Per 32-key step a wave computes S^T = K Q^T with v_mfma_f32_16x16x32 (A = K rows straight from HBM: 16-byte loads per lane, B = Q^T held in
// registers for the whole split) and O^T += V^T P^T (B = P^T straight from the S^T accumulator, A = V^T through a per-wave LDS image read with
// ds_read_b64_tr_b16 - the one place the operand layout needs LDS).  With the scores transposed, a lane owns ONE query row (lane & 15) and
// four keys per 16-key block, so the row statistics stay per lane and O^T comes out with the row on the lane as well.
//   S^T (16 keys x 16 rows), block kb:  lane l holds key 16 kb + 4 (l >> 4) + r, row l & 15   (r = 0..3)
//   P^T k-slots of a step:              slot 8 g + j  <->  key 4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4)       (g = l >> 4)
//   O^T block c:                        lane l holds column 16 c + 4 g + r of row l & 15
// Next step's K and V are loaded into a second register set before the current step is computed (two sets, no copies).  K/V rows are
// addressed through buffer descriptors whose range ends at the sequence's valid length L: rows at or past L read as zeros (V zeros matter:
// 0 x NaN from an uninitialised cache row would poison O), and the scores of keys past L or behind the causal limit are masked to -inf.
// Sliding window (the _local kernels, KvcacheKernelParams::is_local): each lane's row sees keys lo_t <= key < lim_t, and a workgroup's key range
// starts at the 32-aligned base below the first row w0 its tile sees; its descriptors start at w0, so rows below w0 read as zeros like rows
// at or past L.  The plain kernels are the same template with LOCAL = false: their code does not change.
// 8-bit cache (the _fp8 kernels, KvcacheKernelParams::cache_fp8; template parameter ES = 1): K / V hold e4m3 codes, one byte per element.  The
// loads stay 16 bytes per lane (so a K load carries two chunks' worth of a key and the d-elements of a k-slot are permuted, in Q alike; a V
// load covers 16 elements of a row), the codes are widened to T in registers - exactly - in front of the same MFMAs and the same LDS image,
// and the (batch, KV head) descales fold into the softmax scale (K) and the final normalisation (V).  The append quantises k_new / v_new.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "fa_device.hpp"
#include "fa_kvcache_quant.hpp"
#include "fa_params.hpp"

namespace fa {

namespace {

constexpr int kKvcWaves = 4;
constexpr int kKvcThreads = 64 * kKvcWaves;
constexpr int kKvcMaxSplits = 128;
constexpr int kKvcMinStepsPerSplit = 8;      // 256 keys: two steps per wave before a split pays its prologue and merge
constexpr int kKvcCombineThreads = 256;
// How the 8-bit kernels load K (DESIGN.md "FP8 KV cache"): 0 = 16 bytes per lane, the d-elements of a k-slot permuted (Q is loaded with the
// same permutation); 1 = 8 bytes per lane and chunk in the 16-bit kernels' mapping.  The experiment switch of the measurement; 0 ships.
#ifndef FA_KVC_FP8_KLOAD8
#define FA_KVC_FP8_KLOAD8 0
#endif
// How the tree-mask kernels (TREE, fa_fwd_kvcache_tree.hip) select: 0 = every step tests the row's bits; 1 = a step that lies wholly in the
// prefix (a wave-uniform comparison) takes the plain select and only the steps that overlap the draft tokens test bits.  Same values either
// way.  The experiment switch of DESIGN.md 3.11; 0 ships.
#ifndef FA_KVC_TREE_UNIFORM
#define FA_KVC_TREE_UNIFORM 0
#endif

template <int D>
struct KvcLds {
    static constexpr int kVStage = 32 * D * 2;                                  // one wave's V image: 32 rows x D 16-bit
    static constexpr int kOPitch = D + 4;                                       // fp32 merge rows, padded by 16 bytes
    static constexpr int kMerge = kKvcWaves * kKvcRows * kOPitch * 4 + 2 * kKvcWaves * kKvcRows * 4;
    static constexpr int kBytes = kKvcWaves * kVStage > kMerge ? kKvcWaves * kVStage : kMerge;
};

FA_DEV int kvc_len(const KvcacheKernelParams& p, int bidx) {
    int L = p.seqlen_cache;
    if (p.cache_seqlens != nullptr) {
        const int cs = p.cache_seqlens[bidx];
        L = min((cs > 0 ? cs : 0) + p.seqlen_new, p.seqlen_cache);
    }
    return __builtin_amdgcn_readfirstlane(L);
}

// Ragged query batches (KvcacheRaggedParams): the length of sequence `seq` with its own appended rows sn = cu_kn[seq + 1] - cu_kn[seq] in
// place of seqlen_new.
FA_DEV int kvc_len_ragged(const KvcacheRaggedParams& rg, int seq) {
    const KvcacheKernelParams& p = rg.kp;
    int L = p.seqlen_cache;
    if (p.cache_seqlens != nullptr) {
        const int cs = p.cache_seqlens[seq];
        const int sn = rg.cu_kn != nullptr ? max(rg.cu_kn[seq + 1] - rg.cu_kn[seq], 0) : 0;
        L = min((cs > 0 ? cs : 0) + sn, p.seqlen_cache);
    }
    return __builtin_amdgcn_readfirstlane(L);
}

// Tile slot of the compact ragged grid -> (sequence, row tile inside it); false = a slack slot past the last tile (the workgroup exits).
// varlen_slot_lookup (fa_device.hpp) with tiles of ROWS packed rows, ceil(sq_i * h_ratio / ROWS) - kKvcRows for kvcache_attn, kKvcPrefillRows for the
// 64-row body of fa_fwd_kvcache_prefill.hip - and without its batch limit: the sequences
// are taken kVarlenMaxBatch at a time (one round of independent loads and a wave prefix sum each), so a batch of up to 512 costs what the
// prefill lookup costs and a larger one a further round per 512 sequences.  Every wave computes the same answer from the same data.
template <int ROWS>
FA_DEV bool kvc_slot_lookup(const int32_t* cu, int b, int h_ratio, uint32_t slot, int& seq, int& tile) {
    const int lane = threadIdx.x & 63;
    for (int b0 = 0; b0 < b; b0 += kVarlenMaxBatch) {
        const int b1 = min(b0 + kVarlenMaxBatch, b);
        const int per = (b1 - b0 + 63) >> 6;                         // sequences per lane, <= kVarlenSeqPerLane
        const int i0 = b0 + lane * per;
        int c[kVarlenSeqPerLane + 1];
#pragma unroll
        for (int j = 0; j <= kVarlenSeqPerLane; ++j) c[j] = cu[min(i0 + min(j, per), b1)];
        uint32_t t[kVarlenSeqPerLane], mine = 0;
#pragma unroll
        for (int j = 0; j < kVarlenSeqPerLane; ++j) {
            t[j] = (j < per) ? (uint32_t)((max(c[j + 1] - c[j], 0) * h_ratio + ROWS - 1) / ROWS) : 0u;
            mine += t[j];
        }
        uint32_t incl = mine;                                        // inclusive prefix over the 64 lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, off);
            if (lane >= off) incl += y;
        }
        uint32_t run = incl - mine;
        int f_seq = -1, f_tile = 0;
#pragma unroll
        for (int j = 0; j < kVarlenSeqPerLane; ++j) {
            if (slot >= run && slot < run + t[j]) { f_seq = i0 + j; f_tile = (int)(slot - run); }
            run += t[j];
        }
        const uint64_t m = __ballot(f_seq >= 0);
        if (m != 0) {
            const int src = __ffsll((long long)m) - 1;
            seq = __builtin_amdgcn_readlane(f_seq, src);
            tile = __builtin_amdgcn_readlane(f_tile, src);
            return true;
        }
        slot -= (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);  // the tiles of this round of sequences
    }
    return false;
}

// Eight e4m3 codes (two words, bytes in element order) -> eight T: exact, every finite e4m3 value is a T value; the NaN codes become NaN.
template <typename T>
FA_DEV u32x4 widen8(uint32_t w0, uint32_t w1) {
    if constexpr (sizeof(T) == 2 && __is_same(T, _Float16)) {
        return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true))};
    } else {
        return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true))};
    }
}

// tanh(x) from y = 2 log2(e) x with the exponential and reciprocal instructions (gfx950 has no tanh): 1 - 2 / (2^y + 1).  +-1 at +-inf (2^y
// overflows to inf, whose reciprocal is 0, or underflows to 0), NaN passes through, absolute error about 1e-7.
FA_DEV float kvc_tanh2(float y) { return __builtin_fmaf(-2.f, fast_rcp(fast_exp2(y) + 1.f), 1.f); }

// The attention body of both cache layouts; PAGED changes how K / V rows are addressed (load_step), nothing else.
// ES = bytes per cache element: 2 = the dtype of q (T), 1 = FP8 e4m3 codes, widened to T in registers (widen8: exact) in front of the same
// MFMAs; the descales of the (batch, KV head) fold into the softmax scale (K) and the final normalisation (V).  ES is a template
// parameter: the ES = 2 instantiations are the code they were before the 8-bit cache existed.
// RAGGED (fa_fwd_kvcache_ragged.hip; `rg` is read only then): the workgroup's (sequence, row tile) comes from a tile slot of a grid sized by the
// tokens present, the sequence brings its own sq rows at packed rows q0 .. q0 + sq - 1 of q / o and its own appended length, and rows of the
// LSE and of the partial planes are (head, packed row).  Everything behind those few values is the code below as it is: a tile never spans two
// sequences, so a sequence of a ragged call goes through exactly the steps of the dense call on it alone.  RAGGED is a template parameter:
// the dense instantiations are the code they were.
// SOFTCAP (fa_fwd_kvcache_softcap.hip; `cap_pre` is read only then): every score becomes softcap * tanh(s * softmax_scale / softcap) in front of
// the mask.  The step keeps t = tanh(s * pre) with pre = cap_pre * k_descale, cap_pre = 2 log2(e) * softmax_scale / softcap from the host, and
// the host puts the cap where the scale was: p.scale = softcap, p.scale_log2e = softcap * log2(e).  The running max then lives in tanh units
// and nothing behind the mask knows the difference; the descale of an 8-bit K rides on pre, inside the tanh, not on c.  SOFTCAP is a template
// parameter: the instantiations without it are the code they were.
// SINK (fa_fwd_kvcache_sink.hip; `sinks` / `sinks_stride` are read only then, and only by an unsplit launch): query head hq has a learned logit
// sinks[hq * sinks_stride] that joins the softmax denominator and brings no value.  It enters once per row in the epilogue, behind the merge
// of the four waves and in front of inv and lse, as one more key whose score, in natural-log units, is the sink and whose V row is zero: the
// 32-key loop does not know it.  A split launch (n_split > 1) writes the partials of the call without sinks - the sink combine of
// fa_fwd_kvcache_sink.hip adds the term there.  SINK is a template parameter: the instantiations without it are the code they were.
// TREE (fa_fwd_kvcache_tree.hip; `tree` is read only then): the last sq keys of a sequence are the draft tokens of a speculation tree, and query
// row t sees key j < L iff j < base = L - sq or bit j - base of its 64-bit word (tree->ptr[batch * batch_stride + t * row_stride]; ragged:
// ptr[(q0 + t) * row_stride]) is set.  The lane owns one query row for the whole split, so it loads the word once in the prologue, next to lim,
// and the select of the step tests a bit where the plain kernels compare with lim.  Steps, splits, loads, softmax and epilogue are the code of
// the plain kernels over [0, L): the lower-triangle mask gives the causal call's bits and the full mask the non-causal call's.  TREE is a
// template parameter (with CAUSAL = LOCAL = SOFTCAP = SINK = false): the instantiations without it are the code they were.
template <typename T, int D, bool CAUSAL, bool PAGED, bool LOCAL = false, int ES = 2, bool RAGGED = false, bool SOFTCAP = false, bool SINK = false,
          bool TREE = false>
FA_DEV void kvcache_attn(const KvcacheKernelParams& p, const KvcacheRaggedParams* rg = nullptr, float cap_pre = 0.f, const float* sinks = nullptr,
                         int64_t sinks_stride = 0, const KvcacheTree* tree = nullptr) {
    static_assert(ES == 1 || ES == 2, "cache elements are 16-bit (the dtype of q) or 8-bit (e4m3)");
    static_assert(!TREE || (!CAUSAL && !LOCAL && !SOFTCAP && !SINK), "a tree mask stands alone: no causal limit, window, soft cap or sinks");
    constexpr int NC = D / 32;          // 16x16x32 MFMAs per 16 keys of S^T (d chunks)
    constexpr int NO = D / 16;          // O^T blocks of 16 columns
    constexpr int SLOTS = D * ES / 16;  // 16-byte slots per cache row
    constexpr int VRPL = 64 / SLOTS;    // V rows per wave-wide 16-byte load
    constexpr int NV = kKvcStep / VRPL; // V loads per lane and step
    constexpr bool K8 = ES == 1 && FA_KVC_FP8_KLOAD8;
    constexpr int NK = K8 ? NC : NC * ES / 2;     // K loads per lane and 16-key block (16 bytes each; K8: 8 bytes)
    using kfrag_t = std::conditional_t<K8, u32x2, u32x4>;
    __shared__ __attribute__((aligned(16))) char smem[KvcLds<D>::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    int n_tiles = p.n_row_tiles;                // RAGGED: the tile slots of a KV head, and `bh` below is the KV head
    if constexpr (RAGGED) n_tiles = rg->slots;
    int split = id % p.n_split, rest = id / p.n_split;
    int tile = rest % n_tiles, bh = rest / n_tiles;
    // 8-bit head_dim 64: a (key, head) row is 64 bytes, half a 128-byte line whose other half belongs to the neighbouring KV head.  That
    // head's workgroup is n_split x n_row_tiles launch slots away - for an unsplit launch on the next XCD (workgroup i runs on XCD i % 8),
    // behind another L2, so every line comes from memory twice.  With an even h_k the two heads of a pair are therefore made neighbours in
    // time on ONE XCD: workgroups i and i + 8 of every 16 take the two heads of a pair, and the pairs run through (split, tile, pair) in the
    // usual order.  Only the order of the workgroups changes, not what any of them computes; the last gridDim.x % 16 keep their places
    // among themselves.
    if constexpr (ES * D < 128) {
        if ((p.h_k & 1) == 0) {
            const int l = id < (int)(gridDim.x & ~15u) ? ((id & ~15) | ((id & 7) << 1) | ((id >> 3) & 1)) : id;
            int r = l >> 1;
            split = r % p.n_split; r /= p.n_split;
            tile = r % n_tiles;
            bh = 2 * (r / n_tiles) + (l & 1);
        }
    }
    int bidx = bh / p.h_k, kvh = bh - bidx * p.h_k;
    int sq = p.seqlen_q;                        // query rows of this sequence
    int64_t q0 = 0;                             // RAGGED: its first packed row
    if constexpr (RAGGED) {
        kvh = bh;
        if (rg->compact) {
            const int slot = tile;
            if (!kvc_slot_lookup<kKvcRows>(rg->cu_q, p.b, p.h_ratio, (uint32_t)slot, bidx, tile)) return;     // a slack slot: nothing to write
        } else {
            bidx = tile / p.n_row_tiles;        // (n_row_tiles = tiles of max_seqlen_q here)
            tile -= bidx * p.n_row_tiles;
        }
        const int c0 = rg->cu_q[bidx];
        sq = __builtin_amdgcn_readfirstlane(rg->cu_q[bidx + 1] - c0);
        q0 = __builtin_amdgcn_readfirstlane(c0);
        if (tile * kKvcRows >= sq * p.h_ratio) return;      // (plain slots of a sequence shorter than max_seqlen_q)
    }
    const int L = RAGGED ? kvc_len_ragged(*rg, bidx) : kvc_len(p, bidx);
    const int rows_tile = sq * p.h_ratio;
    // window bounds of query position tq (LOCAL): lo_t = L - seqlen_q + t - left (any negative value = no lower bound), lim_t = min(L, L -
    // seqlen_q + t + right + 1); written so that nothing overflows for any L and left < seqlen_cache, right < seqlen_q - 1 (host-normalised)
    auto win_lo = [&](int tq) { return p.window_left >= 0 ? max(L - p.window_left, 0) - (sq - tq) : 0; };
    auto win_lim = [&](int tq) { return p.window_right >= 0 ? L - max(sq - 1 - tq - p.window_right, 0) : L; };
    // row (hq_, t_) of the LSE and of the partial planes; element offset of its row in q / o (st = p.q or p.o)
    auto row_index = [&](int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (RAGGED) return (int64_t)hq_ * rg->total_q + q0 + t_;
        else return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t_;
    };
    auto row_off = [&](const TStride& st, int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        if constexpr (RAGGED) return (q0 + t_) * st.row + (int64_t)hq_ * st.head;
        else return (int64_t)bidx * st.batch + (int64_t)t_ * st.row + (int64_t)hq_ * st.head;
    };
    // LOCAL: w0 = the first key the tile's first row (the smallest lo) sees; the splits start at w0 rounded down to a step and end at the
    // largest lim of the tile (its last row's).  Plain: w0 = 0, the splits cover [0, L).
    const int w0 = LOCAL ? __builtin_amdgcn_readfirstlane(max(win_lo(tile * kKvcRows / p.h_ratio), 0)) : 0;
    const int k_hi = LOCAL ? __builtin_amdgcn_readfirstlane(win_lim((min((tile + 1) * kKvcRows, rows_tile) - 1) / p.h_ratio)) : L;
    const int k_begin = (w0 & ~(kKvcStep - 1)) + split * p.split_keys;
    const int k_end = min(k_begin + p.split_keys, k_hi);
    // 8-bit cache: S = (Q . K codes) x k_descale, so the descale rides on the softmax scale; O = (P . V codes) x v_descale / l
    float kd = 1.f, vd = 1.f;
    if constexpr (ES == 1) {
        if (p.k_descale != nullptr) kd = p.k_descale[(int64_t)bidx * p.kds_batch + (int64_t)kvh * p.kds_head];
        if (p.v_descale != nullptr) vd = p.v_descale[(int64_t)bidx * p.vds_batch + (int64_t)kvh * p.vds_head];
    }
    const float c = (ES == 1 && !SOFTCAP) ? p.scale_log2e * kd : p.scale_log2e;
    const float sc = (ES == 1 && !SOFTCAP) ? p.scale * kd : p.scale;
    const float pre = ES == 1 ? cap_pre * kd : cap_pre;        // (SOFTCAP only)

    if (p.n_split > 1 && k_begin >= k_end) {        // nothing to read in this split: an empty partial (LSE = -inf), O is never looked at
        if (tid < kKvcRows) {
            const int pr = tile * kKvcRows + tid;
            if (pr < rows_tile) {
                const int t = pr / p.h_ratio, hq = kvh * p.h_ratio + (pr - t * p.h_ratio);
                p.ws_lse[(int64_t)split * p.rows_total + row_index(hq, t)] = -INFINITY;
            }
        }
        return;
    }

    // ---- this lane's query row: Q^T fragments for the whole split, visible-key limit -------------------------------------------------
    const int pr = tile * kKvcRows + n16;
    const bool row_ok = pr < rows_tile;
    const int t = row_ok ? pr / p.h_ratio : 0;
    const int hq = kvh * p.h_ratio + (row_ok ? pr - t * p.h_ratio : 0);
    int lim = row_ok ? L : 0;
    if (CAUSAL && row_ok) lim = min(L, L - sq + t + 1);
    if (LOCAL && row_ok) lim = win_lim(t);
    const int lo = LOCAL ? win_lo(t) : 0;
    // TREE: the row's mask word (a row past the tile sees nothing: lim = 0) and the first draft key; base < 0 where L < sq - the bits of keys
    // below 0 are never asked for, since key >= 0
    [[maybe_unused]] uint64_t tbits = 0;
    [[maybe_unused]] const int tbase = L - sq;
    if constexpr (TREE) {
        if (row_ok) tbits = (uint64_t)(RAGGED ? tree->ptr[(q0 + t) * tree->row_stride] : tree->ptr[(int64_t)bidx * tree->batch_stride + (int64_t)t * tree->row_stride]);
    }
    u32x4 qf[NC];
    {
        const char* qrow = (const char*)p.q_ptr + 2 * row_off(p.q, hq, t);
        static_for<0, NC>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            // ES = 1: a 16-byte K load brings d-elements 64 li + 16 g .. + 15, which feed chunks 2 li and 2 li + 1 eight by eight; the dot
            // product over d does not care which d-elements a k-slot carries as long as Q carries the same ones
            constexpr int d0 = (ES == 2 || K8) ? 32 * ci : 64 * (ci / 2) + 8 * (ci & 1);
            constexpr int dg = (ES == 2 || K8) ? 8 : 16;
            qf[ci] = row_ok ? *(const u32x4*)(qrow + 2 * (d0 + dg * g)) : u32x4{0u, 0u, 0u, 0u};
        });
    }

    // ---- K / V of this (batch, KV head): descriptors end at row L ------------------------------------------------------------------
    // (contiguous LOCAL: they start at row w0 <= L, and a row is addressed as min((uint32_t)(key - w0), L - w0): rows below w0 and at or
    // past L both fall outside the range)
    const uint32_t krow_b = (uint32_t)(p.kc.row * ES), vrow_b = (uint32_t)(p.vc.row * ES);
    const int wb = PAGED ? 0 : w0;
    const char* kbase = uniform_ptr((const char*)p.k_cache + ES * ((int64_t)(PAGED ? 0 : bidx) * p.kc.batch + (int64_t)kvh * p.kc.head + (int64_t)wb * p.kc.row));
    const char* vbase = uniform_ptr((const char*)p.v_cache + ES * ((int64_t)(PAGED ? 0 : bidx) * p.vc.batch + (int64_t)kvh * p.vc.head + (int64_t)wb * p.vc.row));
    const rsrc_t krs = make_rsrc(kbase, L > wb ? (uint32_t)(L - wb - 1) * krow_b + ES * D : 0u);
    const rsrc_t vrs = make_rsrc(vbase, L > wb ? (uint32_t)(L - wb - 1) * vrow_b + ES * D : 0u);
    // Paged cache: a step's two 16-key blocks each lie in one page (page_size is a multiple of 16).  Every block gets its own descriptors,
    // based at the block's first row in its page and ending at the sequence's last valid row in the block (rows at or past L read as
    // zeros, as above; a block wholly past L has an empty range, so whatever its table entry says is never read).  The table entries of
    // the step after the one being loaded are fetched (scalar loads) together with that load, one compute step before they are needed;
    // the fetch cursor (column, row in page) moves by the wave stride without a division.  Columns are clamped to the table row,
    // entries to the pool: min((uint32_t)entry, num_blocks - 1).  Page offsets are 64-bit; in-page offsets < 2^31 by the host checks.
    // LOCAL: a block's descriptors start at its first row at or past w0 (skip rows in) and the rows are addressed like the contiguous case,
    // min((uint32_t)(row - skip), valid - skip): rows below w0 read as zeros, and a block wholly below w0 reads nothing.
    const int P = p.page_size;
    // (read through the constant address space: the table is not written while the kernel runs, and so the compiler issues scalar loads
    // that only a later lgkmcnt wait depends on; as a plain global pointer it gets vector loads that wait behind the K / V loads in flight)
    typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
    const const_i32_ptr tbl = PAGED ? (const_i32_ptr)(p.block_table + (int64_t)bidx * p.bt_stride) : nullptr;
    const int last_col = PAGED ? p.seqlen_cache / P - 1 : 0;
    uint32_t pg[2] = {0u, 0u};                  // table entries (unclamped: consumed by the next load_step) of the next step's blocks
    int rw[2] = {0, 0};                         // ... and the blocks' first rows in their pages
    int f_col = 0, f_row = 0, st_col = 0, st_row = 0;
    auto fetch_pages = [&]() __attribute__((always_inline)) {
        int c1 = f_col, r1 = f_row + 16;
        if (r1 >= P) { r1 -= P; c1 += 1; }
        pg[0] = (uint32_t)tbl[min(f_col, last_col)]; rw[0] = f_row;
        pg[1] = (uint32_t)tbl[min(c1, last_col)]; rw[1] = r1;
        f_col += st_col; f_row += st_row;
        if (f_row >= P) { f_row -= P; f_col += 1; }
    };
    if constexpr (PAGED) {
        const int key_first = __builtin_amdgcn_readfirstlane(k_begin + wave * kKvcStep);
        f_col = __builtin_amdgcn_readfirstlane(key_first / P);
        f_row = key_first - f_col * P;
        st_col = __builtin_amdgcn_readfirstlane(kKvcWaves * kKvcStep / P);
        st_row = kKvcWaves * kKvcStep - st_col * P;
        fetch_pages();
    }
    // (row indices are clamped to L: a row at L is past the descriptor's range, and (L) x row stride < 2^31 by the host checks)
    auto crow = [&](int key) __attribute__((always_inline)) {
        return LOCAL ? min((uint32_t)(key - w0), (uint32_t)(L - w0)) : (uint32_t)min(key, L);
    };
    auto load_k = [&](rsrc_t r, uint32_t off, int ci) __attribute__((always_inline)) {
        if constexpr (K8) return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, off + 32 * ci, 0, 0));
        else return buf_load16(r, off + 64 * ci);
    };
    constexpr int kKG = K8 ? 8 : 16;    // bytes per lane group g within a K load
    auto load_step = [&](int key0, kfrag_t (&kf)[2][NK], u32x4 (&vf)[NV]) __attribute__((always_inline)) {
        if constexpr (PAGED) {
            rsrc_t kr[2], vr[2];
            int skip[2], nrow[2];
            static_for<0, 2>([&](auto kb) {
                constexpr int b = decltype(kb)::value;
                const int valid = min(max(L - (key0 + 16 * b), 0), 16);
                skip[b] = LOCAL ? min(max(w0 - (key0 + 16 * b), 0), 16) : 0;     // <= valid (w0 <= L)
                nrow[b] = valid - skip[b];
                const int64_t page = min(pg[b], (uint32_t)(p.num_blocks - 1));
                const int64_t pk = page * p.kc.batch + (int64_t)(rw[b] + skip[b]) * p.kc.row;
                const int64_t pv = page * p.vc.batch + (int64_t)(rw[b] + skip[b]) * p.vc.row;
                kr[b] = make_rsrc(uniform_ptr(kbase + ES * pk), nrow[b] > 0 ? (uint32_t)(nrow[b] - 1) * krow_b + ES * D : 0u);
                vr[b] = make_rsrc(uniform_ptr(vbase + ES * pv), nrow[b] > 0 ? (uint32_t)(nrow[b] - 1) * vrow_b + ES * D : 0u);
            });
            // row r of block b within its descriptor
            auto brow = [&](int b, int r) __attribute__((always_inline)) {
                return LOCAL ? min((uint32_t)(r - skip[b]), (uint32_t)nrow[b]) : (uint32_t)r;
            };
            static_for<0, 2>([&](auto kb) {
                constexpr int b = decltype(kb)::value;
                const uint32_t off = brow(b, n16) * krow_b + kKG * g;
                static_for<0, NK>([&](auto cc) {
                    constexpr int ci = decltype(cc)::value;
                    kf[b][ci] = load_k(kr[b], off, ci);
                });
            });
            static_for<0, NV>([&](auto iv) {
                constexpr int i = decltype(iv)::value;
                constexpr int b = (i * VRPL) / 16;
                const uint32_t off = brow(b, (i * VRPL) % 16 + lane / SLOTS) * vrow_b + 16 * (lane % SLOTS);
                vf[i] = buf_load16(vr[b], off);
            });
            fetch_pages();                          // the table entries of the step after this one
        } else {
            static_for<0, 2>([&](auto kb) {
                constexpr int b = decltype(kb)::value;
                const uint32_t off = crow(key0 + 16 * b + n16) * krow_b + kKG * g;
                static_for<0, NK>([&](auto cc) {
                    constexpr int ci = decltype(cc)::value;
                    kf[b][ci] = load_k(krs, off, ci);
                });
            });
            static_for<0, NV>([&](auto iv) {
                constexpr int i = decltype(iv)::value;
                const uint32_t off = crow(key0 + i * VRPL + lane / SLOTS) * vrow_b + 16 * (lane % SLOTS);
                vf[i] = buf_load16(vrs, off);
            });
        }
    };

    FA_LDS char* vstage = (FA_LDS char*)smem + wave * KvcLds<D>::kVStage;
    // transposed-read addresses of this lane (fa_device.hpp lds_tile_off image): block c, half hh -> rows hh * 16 + 4 g + q, columns 16 c + 4 p
    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 oacc[NO];
    // (the empty asm pins the zeros here: sunk into the path that skips the loop, they were laid out straight behind the loop's last MFMA,
    // which the conservative hazard scan of tests/_mfma_hazards.py reads as a write to a result still in flight)
    static_for<0, NO>([&](auto cc) {
        oacc[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(oacc[decltype(cc)::value]));
    });
    float m_run = kNegBig, l_run = 0.f;

    auto compute_step = [&](int key0, const kfrag_t (&kf)[2][NK], const u32x4 (&vf)[NV]) __attribute__((always_inline)) {
        f32x4 s[2];
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            static_for<0, NC>([&](auto cc) {
                constexpr int ci = decltype(cc)::value;
                if constexpr (ES == 2) {
                    s[b] = LP<T>::mfma16(kf[b][ci], qf[ci], s[b]);
                } else if constexpr (K8) {
                    s[b] = LP<T>::mfma16(widen8<T>(kf[b][ci].x, kf[b][ci].y), qf[ci], s[b]);
                } else {
                    const u32x4 k8 = kf[b][ci / 2];
                    s[b] = LP<T>::mfma16((ci & 1) ? widen8<T>(k8.z, k8.w) : widen8<T>(k8.x, k8.y), qf[ci], s[b]);
                }
            });
        });
        // V -> this wave's LDS image while the MFMAs run (ES = 1: widened to T first, so the image and its transposed reads stay as they are)
        static_for<0, NV>([&](auto iv) {
            constexpr int i = decltype(iv)::value;
            if constexpr (ES == 2) {
                *(FA_LDS u32x4*)(vstage + lds_tile_off<D>(i * VRPL + lane / SLOTS, lane % SLOTS)) = vf[i];
            } else {
                *(FA_LDS u32x4*)(vstage + lds_tile_off<D>(i * VRPL + lane / SLOTS, 2 * (lane % SLOTS))) = widen8<T>(vf[i].x, vf[i].y);
                *(FA_LDS u32x4*)(vstage + lds_tile_off<D>(i * VRPL + lane / SLOTS, 2 * (lane % SLOTS) + 1)) = widen8<T>(vf[i].z, vf[i].w);
            }
        });
        float mx = -INFINITY;
        [[maybe_unused]] const bool tree_step = !(TREE && FA_KVC_TREE_UNIFORM) || key0 + kKvcStep > tbase;     // (key0, tbase: wave-uniform)
        static_for<0, 2>([&](auto kb) {
            constexpr int b = decltype(kb)::value;
            static_for<0, 4>([&](auto rr) {
                constexpr int r = decltype(rr)::value;
                const int key = key0 + 16 * b + 4 * g + r;
                if constexpr (SOFTCAP) s[b][r] = kvc_tanh2(s[b][r] * pre);
                if constexpr (TREE) {
                    // u = key - tbase: the draft token this key is.  u < 0: the prefix; 0 <= u < sq <= 64: bit u; the count is masked to 0 .. 63 so
                    // that the shift is defined for every u, and u >= sq only where key >= L, which lim (= L, 0 for a row past the tile) cuts
                    const int u = key - tbase;
                    if (tree_step) s[b][r] = (key < lim && (u < 0 || ((tbits >> (u & 63)) & 1) != 0)) ? s[b][r] : -INFINITY;
                    else s[b][r] = key < lim ? s[b][r] : -INFINITY;
                } else {
                    s[b][r] = (key < lim && (!LOCAL || key >= lo)) ? s[b][r] : -INFINITY;
                }
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
        asm volatile("" ::: "memory");      // the image written above is read back below (same wave: LDS keeps the order)
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            oacc[ci] = LP<T>::mfma16(tr_frag<D>(vstage, ci, g, q4, p4), pf, oacc[ci]);
        });
        asm volatile("" ::: "memory");      // ... before the next step overwrites it
    };

    // ---- the split's 32-key steps, interleaved over the waves; two register sets in turn -----------------------------------------
    {
        kfrag_t ka[2][NK], kb2[2][NK];
        u32x4 va[NV], vb[NV];
        int key = k_begin + wave * kKvcStep;
        const int stride = kKvcWaves * kKvcStep;
        if (key < k_end) load_step(key, ka, va);
        for (; key < k_end; key += 2 * stride) {
            const int k1 = key + stride;
            if (k1 < k_end) load_step(k1, kb2, vb);
            compute_step(key, ka, va);
            if (k1 < k_end) {
                if (k1 + stride < k_end) load_step(k1 + stride, ka, va);
                compute_step(k1, kb2, vb);
            }
        }
    }

    // ---- merge the four waves through LDS --------------------------------------------------------------------------------------
    l_run = sum_four_groups(l_run);
    __syncthreads();                               // every wave is done with its V image (the merge planes overlay them)
    FA_LDS float* ow_l = (FA_LDS float*)smem;
    FA_LDS float* mw_l = ow_l + kKvcWaves * kKvcRows * KvcLds<D>::kOPitch;
    FA_LDS float* lw_l = mw_l + kKvcWaves * kKvcRows;
    static_for<0, NO>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        *(FA_LDS f32x4*)(ow_l + (wave * kKvcRows + n16) * KvcLds<D>::kOPitch + 16 * ci + 4 * g) = oacc[ci];
    });
    if (g == 0) {
        mw_l[wave * kKvcRows + n16] = m_run;
        lw_l[wave * kKvcRows + n16] = l_run;
    }
    __syncthreads();

    constexpr int CPT = D / 16;                    // output columns per thread: 16 threads per row
    const int row = tid >> 4, col = (tid & 15) * CPT;
    const int opr = tile * kKvcRows + row;
    if (opr >= rows_tile) return;
    float mrow = kNegBig;
    static_for<0, kKvcWaves>([&](auto ww) { mrow = fmaxf(mrow, mw_l[decltype(ww)::value * kKvcRows + row]); });
    float lsum = 0.f, acc[CPT];
    static_for<0, CPT>([&](auto jj) { acc[decltype(jj)::value] = 0.f; });
    static_for<0, kKvcWaves>([&](auto ww) {
        constexpr int w = decltype(ww)::value;
        const float a = fast_exp2((mw_l[w * kKvcRows + row] - mrow) * c);
        lsum += lw_l[w * kKvcRows + row] * a;
        static_for<0, CPT / 4>([&](auto qq) {
            constexpr int qi = decltype(qq)::value;
            const f32x4 x = *(const FA_LDS f32x4*)(ow_l + (w * kKvcRows + row) * KvcLds<D>::kOPitch + col + 4 * qi);
            static_for<0, 4>([&](auto ee) { acc[4 * qi + decltype(ee)::value] += a * x[decltype(ee)::value]; });
        });
    });
    const int ot = opr / p.h_ratio, ohq = kvh * p.h_ratio + (opr - ot * p.h_ratio);
    [[maybe_unused]] float sink_top = 0.f;      // SINK: the sink where it is the row's maximum (on_sink)
    [[maybe_unused]] bool on_sink = false;
    if constexpr (SINK) {
        // M = max(row max, sink), compared in natural-log units.  The sink on top: the row's sums move down onto it and it counts 1.  Otherwise
        // it adds exp(sink - max) to the sum, which is + 0.0f for a sink of -inf (the guard keeps -inf - -inf out of the exponential): the
        // bits of the call without sinks.  A row that saw no key (lsum = 0, mrow = kNegBig) goes the first way under a finite sink: lsum = 1,
        // O = 0, LSE = the sink exactly.  A NaN sink fails the comparison and makes the sum NaN: O and LSE of the head's rows are NaN.
        if (p.n_split == 1) {
            const float sk = sinks[(int64_t)ohq * sinks_stride];
            const float ms = mrow * sc;
            if (sk > ms) {
                const float a = fast_exp2((ms - sk) * 1.4426950408889634f);
                lsum = __builtin_fmaf(lsum, a, 1.f);
                static_for<0, CPT>([&](auto jj) { acc[decltype(jj)::value] *= a; });
                sink_top = sk;
                on_sink = true;
            } else {
                lsum += sk == -INFINITY ? 0.f : fast_exp2((sk - ms) * 1.4426950408889634f);
            }
        }
    }
    // dead = saw no key (lsum == 0); a NaN or +inf score leaves lsum = NaN, which is live: O and LSE come out NaN as in fp32 math, and a
    // split partial is written so that the combine propagates it
    const bool live = !(lsum == 0.f);
    const float inv = live ? (ES == 1 ? vd / lsum : 1.0f / lsum) : 0.f;
    float lse = live ? mrow * sc + logf(lsum) : (p.n_split > 1 ? -INFINITY : 0.f);
    if constexpr (SINK) {
        if (on_sink) lse = sink_top + logf(lsum);
    }
    const int64_t R = row_index(ohq, ot);
    if (p.n_split == 1) {
        char* orow = (char*)p.o_ptr + 2 * (row_off(p.o, ohq, ot) + col);
        uint32_t w[CPT / 2];
        static_for<0, CPT / 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            w[j] = LP<T>::pack2(acc[2 * j] * inv, acc[2 * j + 1] * inv);
        });
        if constexpr (CPT == 16) {         // (head_dim 256, fa_fwd_kvcache_d256.hip: 32 bytes of the row per thread)
            *(u32x4*)orow = u32x4{w[0], w[1], w[2], w[3]};
            *(u32x4*)(orow + 16) = u32x4{w[4], w[5], w[6], w[7]};
        } else if constexpr (CPT == 8) *(u32x4*)orow = u32x4{w[0], w[1], w[2], w[3]};
        else *(u32x2*)orow = u32x2{w[0], w[1]};
        if ((tid & 15) == 0) p.lse_ptr[R] = lse;
    } else {
        float* prow = p.ws_o + ((int64_t)split * p.rows_total + R) * D + col;
        if (live) {
            static_for<0, CPT / 4>([&](auto qq) {
                constexpr int qi = decltype(qq)::value;
                *(f32x4*)(prow + 4 * qi) = f32x4{acc[4 * qi] * inv, acc[4 * qi + 1] * inv, acc[4 * qi + 2] * inv, acc[4 * qi + 3] * inv};
            });
        }
        if ((tid & 15) == 0) p.ws_lse[(int64_t)split * p.rows_total + R] = lse;
    }
}

}  // namespace

}  // namespace fa
