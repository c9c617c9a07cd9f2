// fa_kvcache_mla_attn.hpp — the ONE body of MLA decode over a latent KV cache: dense and sparse (top-k lists), 16-bit rows and 656-byte FP8 rows.
// Templates only; fa_fwd_kvcache_mla.hip, fa_fwd_kvcache_mla_sparse.hip and fa_fwd_kvcache_mla_fp8.hip name the instantiations (their __global__ wrappers).
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
//   * S^T = K Q^T: 16 chunks of v_mfma_f32_16x16x32 with K fragments from the 512 image and 2 from the 64 image; qf[18] is held for the split.
//   * O^T += V^T P^T: 32 accumulator blocks (128 fp32 registers a lane); V^T comes by transposed reads (ds_read_b64_tr_b16) from the 512 image
//     of the same stage.  There is no V load and no V image.
//   * The epilogue writes 512-wide rows; the combine is fa_kvcache_combine_kernel at D = 512 (workspace and planes sized by d_v = kp.d = 512).
//   SPARSE (DeepSeek Sparse Attention: top-k key indices per query token) changes three things:
//   * Tiling.  The lists of two query tokens differ, so a tile never spans two tokens: the grid is b x seqlen_q x ceil(h / 64) x n_split and a row within a
//     tile is the head index.  rows_total and the row index of o / lse / planes are the dense call's.  The split is over the slots [0, topk) of the list.
//   * Staging.  Key key0 + r of a step is slot key0 + r of the list.  Lane l of every wave holds the index word of slot l & 31 of a step, loaded one step
//     before it is used (paged: two, so that the table entry is fetched one step ahead).  Slot s is valid iff (uint32_t)idx < L_i: the ballot of that test
//     is the step's 32-bit mask.  Contiguous: the dense kernel's one descriptor per sequence; the row offset is min((uint32_t)idx, L_i) x row bytes, read
//     from the owning lane, so an invalid entry lands at the descriptor's end and loads zeros.  Paged: lane l computes column and row-in-page of its slot
//     (an invalid slot: column 0), gathers the table entry (column clamped to the table row, entry to the pool) and forms the 64-bit address of the cache
//     row; the loads of an invalid slot are not issued or run over an empty range.  The image row of an invalid slot is therefore written with zeros
//     every step (LDS holds whatever the last workgroup left, and 0 x NaN is NaN).
//   * One select: an invalid slot's score is -inf before the max, where the dense kernel applies key < lim.
//   The row format (Fmt: MlaRows16, MlaRows8) supplies what a lane holds of a step between its loads and the LDS writes, the row loads of the four
//   addressing modes and the LDS writes.  The FP8 codes are dequantised where the 512 image is written, so everything behind the barrier reads the LDS
//   bytes the 16-bit kernels read for the dequantised cache, and the two calls agree to the bit.
#pragma once
#include "fa_kvcache_launch.hpp"
#include "fa_kvcache_stage.hpp"

namespace fa {

namespace {

constexpr int kMlaRows = kKvcPrefillRows;   // packed query rows of a workgroup: 16 per wave
constexpr int kMlaDV = 512;                 // the compressed part: V, and columns 0 .. 511 of K
constexpr int kMlaDR = 64;                  // the rope part: columns 512 .. 575 of K
constexpr int kMlaDK = kMlaDV + kMlaDR;
constexpr int kMlaWaveRows = kKvcStep / kKvcWaves;      // rows of a step a wave stages: 8, inside one 16-key block

struct MlaLds {
    static constexpr int kImageV = kKvcStep * kMlaDV * 2;       // 32 rows x 1024 B
    static constexpr int kImageR = kKvcStep * kMlaDR * 2;       // 32 rows x 128 B
    static constexpr int kStage = kImageV + kImageR;            // 36 KB
    static constexpr int kBytes = 2 * kStage;                   // 72 KB
};

// ---- the row formats ----------------------------------------------------------------------------------------------------------------------------------
// A format has Stage, what a lane holds of one step between its loads and the LDS writes; kRowBytes and kUnit (bytes per unit of the cache strides kc);
// an object with the lane's constants; and, for wave w staging rows row0 = 8 w .. 8 w + 7 of a step, the step's loads into st in the four addressing modes
//   load_rows(krs, row0, key0, L, row_b, st)         contiguous: rows min(key0 + row0 + ., L) of the sequence's descriptor
//   load_block(r, row0, row_b, st)                   paged dense: rows (row0 & 15) + . of the descriptor of the wave's 16-key block
//   load_listed(krs, row0, offv, st)                 sparse contiguous: lane s < 32 holds the byte offset offv of slot s's row in the sequence's descriptor
//   load_gathered(kbase, row0, mask, alo, ahi, st)   sparse paged: lane s < 32 holds the 64-bit address (ahi : alo) of slot s's row, bit s of mask = valid
// and store<T>(vimg, rimg, row0, st): registers -> the two images of a stage.
// The inputs are taken BY REFERENCE, as the lambdas of the body capture them: by value the same arithmetic comes out with two staging registers exchanged in
// the contiguous kernels (tools/isa_diff.py against the bodies these replaced).
// kSparseFromDense records two places where the sparse bodies this one replaced differed in appearance only, and where the other form changes their
// instructions.  true (the FP8 body, which held dense and sparse): the sparse prologue keeps the dense `if (key < k_end)` around step 0 - always true there
// (topk >= 32 and an empty split has returned), which hipcc cannot see - and the last table column is computed where the dense body computes it.  false (the
// 16-bit sparse body, which stood alone): no test around step 0, the last column is computed behind the sparse pointers.

// 1152-byte rows of 576 16-bit elements (72 16-byte slots).  Every wave-wide 16-byte load stays inside one row: eight loads of the 64 slots of one row's
// 512 part each, and one load of the 8 slots of the rope part of all eight rows (row row0 + lane / 8, slot 64 + lane % 8).  Nine loads and 36 staging
// registers per lane and step; the latent row comes from memory once and serves both matmuls.
struct MlaRows16 {
    static constexpr int kUnit = 2;                     // bytes per unit of the cache strides kc: they count elements
    static constexpr int kRowBytes = kMlaDK * 2;
    static constexpr bool kSparseFromDense = false;
    using Stage = u32x4[kMlaWaveRows + 1];
    const int lane, rrow, rslot;
    FA_DEV explicit MlaRows16(int lane_) : lane(lane_), rrow(lane_ >> 3), rslot(lane_ & 7) {}

    FA_DEV void load_rows(const rsrc_t& krs, const int& row0, const int& key0, const int& L, const uint32_t& row_b, Stage& st) const {
        static_for<0, kMlaWaveRows>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            st[i] = buf_load16(krs, (uint32_t)min(key0 + row0 + i, L) * row_b + 16 * lane);
        });
        st[kMlaWaveRows] = buf_load16(krs, (uint32_t)min(key0 + row0 + rrow, L) * row_b + 2 * kMlaDV + 16 * rslot);
    }
    FA_DEV void load_block(const rsrc_t& r, const int& row0, const uint32_t& row_b, Stage& st) const {
        static_for<0, kMlaWaveRows>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            st[i] = buf_load16(r, (uint32_t)((row0 & 15) + i) * row_b + 16 * lane);
        });
        st[kMlaWaveRows] = buf_load16(r, (uint32_t)((row0 & 15) + rrow) * row_b + 2 * kMlaDV + 16 * rslot);
    }
    // (a row of the 512 part is the wave's: its offset is read from the owning lane by v_readlane; the rope load, whose eight lane groups read eight rows, by ds_bpermute)
    FA_DEV void load_listed(const rsrc_t& krs, const int& row0, const uint32_t& offv, Stage& st) const {
        static_for<0, kMlaWaveRows>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            st[i] = buf_load16(krs, (uint32_t)__builtin_amdgcn_readlane(offv, row0 + i) + 16 * lane);
        });
        st[kMlaWaveRows] = buf_load16(krs, (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), offv) + 2 * kMlaDV + 16 * rslot);
    }
    // A row of the 512 part gets a descriptor of its own over exactly that row - of length 0 for an invalid slot, which loads zeros and reads nothing; the
    // rope part is one per-lane load that the lanes of an invalid slot do not issue.
    FA_DEV void load_gathered(const char* const& kbase, const int& row0, const uint32_t& mask, const uint32_t& alo, const uint32_t& ahi, Stage& st) const {
        static_for<0, kMlaWaveRows>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            // (readlane returns an int: the low word goes through uint32_t, or its sign would fill the high word)
            const uint64_t base = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(ahi, row0 + i) << 32) | (uint32_t)__builtin_amdgcn_readlane(alo, row0 + i);
            const rsrc_t r = make_rsrc((const char*)base, (mask >> (row0 + i)) & 1u ? (uint32_t)kRowBytes : 0u);
            st[i] = buf_load16(r, 16 * lane);
        });
        const uint32_t rlo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), alo), rhi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), ahi);
        const char* rp = (const char*)(((uint64_t)rhi << 32) | rlo) + 2 * kMlaDV + 16 * rslot;
        // (the zeros of the lanes that do not load come from a load over an empty range: a constant would be kept in registers and copied every step)
        st[kMlaWaveRows] = buf_load16(make_rsrc(kbase, 0u), 0u);
        if ((mask >> (row0 + rrow)) & 1u) st[kMlaWaveRows] = *(const __attribute__((address_space(1))) u32x4*)rp;
    }
    template <typename T>
    FA_DEV void store(FA_LDS char* const& vimg, FA_LDS char* const& rimg, const int& row0, const Stage& st) const {
        static_for<0, kMlaWaveRows>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>((uint32_t)(row0 + i), (uint32_t)lane)) = st[i];
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMlaDR>((uint32_t)(row0 + rrow), (uint32_t)rslot)) = st[kMlaWaveRows];
    }
};

FA_DEV uint32_t buf_load4(rsrc_t r, uint32_t byte_off) { return __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0); }

// eight codes (two dwords) x scale -> eight elements of T: one 16-byte slot of the 512 image
template <typename T>
FA_DEV u32x4 dequant8(uint32_t w0, uint32_t w1, float s) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
    return u32x4{LP<T>::pack2(a[0] * s, a[1] * s), LP<T>::pack2(b[0] * s, b[1] * s), LP<T>::pack2(c[0] * s, c[1] * s), LP<T>::pack2(d[0] * s, d[1] * s)};
}

// 656-byte FP8 rows (kv_format = FA_MLA_KV_FP8_ROWS656): bytes 0 .. 511 the e4m3 codes of columns 0 .. 511, bytes 512 .. 527 four fp32 scales (scale g
// serves columns 128 g .. 128 g + 127), bytes 528 .. 655 the 64 rope elements in q's dtype T.  The row stands for kv[c] = round_to_T(fp32(code[c]) *
// scale[c / 128]) (c < 512; one fp32 product, rounded once to nearest-even) and kv[512 + r] = the stored rope element.
//   * Loads.  A 16-byte load of the code part covers 16 columns; a row is 32 of them, so one wave-wide load covers two rows: load j < 4 takes row
//     row0 + 2 j + lane / 32, chunk lane % 32, and with it the scale dword of the chunk's tile (chunk / 8).  The rope part is one 16-byte load per lane at
//     byte 528 of row row0 + lane / 8.  Nine loads and 24 staging registers per lane and step.  The lanes of one load read two rows, so no row is
//     wave-uniform (sparse contiguous: every offset comes from its owning lane by ds_bpermute).
//   * Rows past L, pages past L and whatever an invalid slot names are never read, and they load as code 0 under scale 0: a zero image row.
//   * Dequantisation (store): v_cvt_pk_f32_fp8 (exact), one v_mul_f32 by the tile's scale, LP<T>::pack2 (round to nearest-even: v_cvt_pk_bf16_f32 /
//     v_cvt_pk_f16_f32, never the truncating v_cvt_pkrtz).  A chunk fills the two 16-byte slots 2 chunk, 2 chunk + 1 of its image row.
struct MlaRows8 {
    static constexpr int kUnit = 1;                     // the cache strides kc are in BYTES
    static constexpr int kScales = kMlaDV;              // byte of a row where the four fp32 scales start
    static constexpr int kRope = kMlaDV + 16;           // ... and where the rope elements start
    static constexpr int kRowBytes = kRope + 2 * kMlaDR;        // 656: 41 16-byte slots
    static constexpr bool kSparseFromDense = true;
    static constexpr int NJ = kMlaWaveRows / 2;         // code loads per lane and step: two rows each
    struct Stage {
        u32x4 code[NJ];         // load j: 16 codes of row row0 + 2 j + lane / 32
        uint32_t scale[NJ];     // ... and the fp32 scale of their tile
        u32x4 rope;
    };
    const int hw, ch;
    const uint32_t coff, soff;
    const int rrow, rslot;
    const uint32_t roff;
    FA_DEV explicit MlaRows8(int lane_)
        : hw(lane_ >> 5), ch(lane_ & 31), coff(16 * ch), soff(kScales + 4 * (ch >> 3)), rrow(lane_ >> 3), rslot(lane_ & 7), roff(kRope + 16 * rslot) {}

    FA_DEV void load_rows(const rsrc_t& krs, const int& row0, const int& key0, const int& L, const uint32_t& row_b, Stage& st) const {
        static_for<0, NJ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t ro = (uint32_t)min(key0 + row0 + 2 * j + hw, L) * row_b;
            st.code[j] = buf_load16(krs, ro + coff);
            st.scale[j] = buf_load4(krs, ro + soff);
        });
        st.rope = buf_load16(krs, (uint32_t)min(key0 + row0 + rrow, L) * row_b + roff);
    }
    FA_DEV void load_block(const rsrc_t& r, const int& row0, const uint32_t& row_b, Stage& st) const {
        static_for<0, NJ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t ro = (uint32_t)((row0 & 15) + 2 * j + hw) * row_b;
            st.code[j] = buf_load16(r, ro + coff);
            st.scale[j] = buf_load4(r, ro + soff);
        });
        st.rope = buf_load16(r, (uint32_t)((row0 & 15) + rrow) * row_b + roff);
    }
    FA_DEV void load_listed(const rsrc_t& krs, const int& row0, const uint32_t& offv, Stage& st) const {
        static_for<0, NJ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t ro = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + 2 * j + hw), offv);
            st.code[j] = buf_load16(krs, ro + coff);
            st.scale[j] = buf_load4(krs, ro + soff);
        });
        st.rope = buf_load16(krs, (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), offv) + roff);
    }
    // per-lane loads from the 64-bit row address (ds_bpermute of both halves) that the lanes of an invalid slot do not issue
    FA_DEV void load_gathered(const char* const& kbase, const int& row0, const uint32_t& mask, const uint32_t& alo, const uint32_t& ahi, Stage& st) const {
        const rsrc_t none = make_rsrc(kbase, 0u);
        typedef const __attribute__((address_space(1))) u32x4* g16_ptr;
        typedef const __attribute__((address_space(1))) uint32_t* g4_ptr;
        // (the zeros of the lanes that do not load come from loads over an empty range, as in MlaRows16 - each at an offset of its own: identical loads
        // are merged into one whose zeros are then copied into every staging register, 16 v_accvgpr moves a step)
        static_for<0, NJ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const int slot = row0 + 2 * j + hw;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * slot, alo), hi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * slot, ahi);
            const char* rp = (const char*)(((uint64_t)hi << 32) | lo);
            st.code[j] = buf_load16(none, 16u * j);
            st.scale[j] = buf_load4(none, 64u + 4u * j);
            if ((mask >> slot) & 1u) {
                st.code[j] = *(g16_ptr)(rp + coff);
                st.scale[j] = *(g4_ptr)(rp + soff);
            }
        });
        const uint32_t rlo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), alo), rhi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), ahi);
        const char* rp = (const char*)(((uint64_t)rhi << 32) | rlo) + roff;
        st.rope = buf_load16(none, 80u);
        if ((mask >> (row0 + rrow)) & 1u) st.rope = *(g16_ptr)rp;
    }
    // the codes become elements of T here
    template <typename T>
    FA_DEV void store(FA_LDS char* const& vimg, FA_LDS char* const& rimg, const int& row0, const Stage& st) const {
        static_for<0, NJ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const float s = __builtin_bit_cast(float, st.scale[j]);
            const uint32_t row = (uint32_t)(row0 + 2 * j + hw);
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>(row, (uint32_t)(2 * ch))) = dequant8<T>(st.code[j].x, st.code[j].y, s);
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>(row, (uint32_t)(2 * ch + 1))) = dequant8<T>(st.code[j].z, st.code[j].w, s);
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMlaDR>((uint32_t)(row0 + rrow), (uint32_t)rslot)) = st.rope;
    }
};

// ---- the body -----------------------------------------------------------------------------------------------------------------------------------------
// SPARSE = false: the dense call (indices, idx_*, topk are not read).  SPARSE = true: CAUSAL is false; a tile is 64 heads of one token and the keys of a
// step are the slots of the token's list.
template <typename T, typename Fmt, bool CAUSAL, bool PAGED, bool SPARSE>
FA_DEV void kvcache_mla_attn(const KvcacheKernelParams& p, const int32_t* indices, int64_t idx_batch, int64_t idx_row, int topk) {
    static_assert(!(SPARSE && CAUSAL), "the list is the mask");
    constexpr int NCV = kMlaDV / 32;    // 16x16x32 MFMAs per 16 keys of S^T over the 512 image
    constexpr int NCR = kMlaDR / 32;    // ... and over the 64 image
    constexpr int NC = NCV + NCR;
    constexpr int NO = kMlaDV / 16;     // O^T blocks of 16 columns
    constexpr int RW = kMlaWaveRows;
    __shared__ __attribute__((aligned(16))) char smem[MlaLds::kBytes];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, n16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int id = blockIdx.x;
    const int split = id % p.n_split;
    int rest = id / p.n_split;
    const int tile = rest % p.n_row_tiles;
    rest /= p.n_row_tiles;
    const int tok = SPARSE ? rest % p.seqlen_q : 0;             // SPARSE: the tile's token
    const int bidx = SPARSE ? rest / p.seqlen_q : rest;         // (one KV head)
    const int sq = p.seqlen_q;
    const int L = kvc_len(p, bidx);
    const int rows_tile = SPARSE ? p.h : sq * p.h;
    auto row_index = [&](int hq_, int t_) __attribute__((always_inline)) -> int64_t { return ((int64_t)bidx * p.h + hq_) * p.seqlen_q + t_; };
    auto row_off = [&](const TStride& st, int hq_, int t_) __attribute__((always_inline)) -> int64_t {
        return (int64_t)bidx * st.batch + (int64_t)t_ * st.row + (int64_t)hq_ * st.head;
    };
    // dense: the keys [0, k_hi); CAUSAL: the tile's keys end where its last row's do (t_last <= sq - 1, so k_hi <= L; it may be <= 0: the tile sees
    // nothing).  SPARSE: the slots [0, topk) of the token's list (topk and split_keys are multiples of the step: every step has its 32 index words)
    int k_hi = SPARSE ? topk : L;
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
                const int t = SPARSE ? tok : pr / p.h, hq = SPARSE ? pr : pr - t * p.h;
                p.ws_lse[(int64_t)split * p.rows_total + row_index(hq, t)] = -INFINITY;
            }
        }
        return;
    }

    // ---- this lane's query row: Q^T fragments for the whole split, visible-key limit -------------------------------------------------
    const bool active = tile * kMlaRows + wave * kKvcRows < rows_tile;      // (wave-uniform) false: staging and barriers only
    const int pr = tile * kMlaRows + wave * kKvcRows + n16;
    const bool row_ok = pr < rows_tile;
    const int t = SPARSE ? tok : (row_ok ? pr / p.h : 0);
    const int hq = row_ok ? (SPARSE ? pr : pr - t * p.h) : 0;
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

    // ---- staging: wave w loads rows 8 w .. 8 w + 7 of a step (dense paged: all in the 16-key block w >> 1) -------------------------------
    const int row0 = wave * RW;
    const Fmt fmt(lane);
    const int islot = lane & 31;                // SPARSE: the slot of a step whose index word this lane holds
    const uint32_t row_b = (uint32_t)(p.kc.row * Fmt::kUnit);
    const char* kbase = uniform_ptr((const char*)p.k_cache + Fmt::kUnit * ((int64_t)(PAGED ? 0 : bidx) * p.kc.batch));
    // contiguous: one descriptor, ending at row L (rows at or past L read as zeros; row indices are clamped to L, and L x row stride < 2^31
    // by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * row_b + Fmt::kRowBytes : 0u);
    // Dense paged: a wave's eight rows lie in one 16-key block and so in one page.  Each step the wave builds the descriptor of its block, based at
    // the block's first row in its page and ending at the sequence's last valid row in the block (a block wholly past L has an empty range:
    // whatever its table entry says is never read).  The table entries of the step after the one being loaded are fetched (scalar loads)
    // together with that load; the cursor (column, row in page) moves by one step without a division.  Columns are clamped to the table row,
    // entries to the pool.
    const int P = p.page_size;
    typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
    const const_i32_ptr tbl = PAGED && !SPARSE ? (const_i32_ptr)(p.block_table + (int64_t)bidx * p.bt_stride) : nullptr;
    // (the last column of a table row: here, or - kSparseFromDense = false - as late_col behind the sparse pointers)
    constexpr bool kLateCol = SPARSE && !Fmt::kSparseFromDense;
    const int last_col = PAGED && !kLateCol ? p.seqlen_cache / P - 1 : 0;
    const int32_t* ip = SPARSE ? indices + ((int64_t)bidx * idx_batch + (int64_t)tok * idx_row) : nullptr;
    const int last_key0 = k_end - kKvcStep;     // SPARSE: the split's last step: index loads past it are clamped to it
    const int32_t* stbl = PAGED && SPARSE ? p.block_table + (int64_t)bidx * p.bt_stride : nullptr;
    const uint32_t late_col = PAGED && kLateCol ? (uint32_t)(p.seqlen_cache / P - 1) : 0u;
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
    if constexpr (PAGED && !SPARSE) {
        f_col = __builtin_amdgcn_readfirstlane(k_begin / P);
        f_row = k_begin - f_col * P;
        st_col = __builtin_amdgcn_readfirstlane(kKvcStep / P);
        st_row = kKvcStep - st_col * P;
        fetch_pages();
    }
    // SPARSE: lane l holds the index word of slot l & 31 of a step, fetched one step ahead (paged: two, so that the table entry is fetched one step ahead)
    uint32_t idxv = 0u;                         // index words of the step after the one whose rows (PAGED: whose table entries) were requested last
    uint32_t pg_v = 0u;                         // SPARSE paged: the table entry (unclamped) of the lane's slot of the next step to load ...
    int prow_v = -1;                            // ... and the slot's row in its page, -1 = an invalid slot
    uint32_t mask0 = 0u, mask1 = 0u;            // SPARSE: valid slots of the step held by stage 0 / 1
    auto load_idx = [&](int key0) __attribute__((always_inline)) { idxv = (uint32_t)ip[min(key0, last_key0) + islot]; };
    auto prep_pages = [&]() __attribute__((always_inline)) {
        const bool ok = idxv < (uint32_t)L;
        const uint32_t j = ok ? idxv : 0u;
        const uint32_t col = j / (uint32_t)P;
        prow_v = ok ? (int)(j - col * (uint32_t)P) : -1;
        pg_v = (uint32_t)stbl[min(col, kLateCol ? late_col : (uint32_t)last_col)];
    };
    // the loads of one step into st; SPARSE: from the index words fetched ahead, with the step's mask and the words (PAGED: and table entries) of later steps
    auto load_step = [&](auto bufc, int key0, typename Fmt::Stage& st) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        if constexpr (SPARSE) {
            uint32_t mask;
            if constexpr (PAGED) {
                mask = (uint32_t)__builtin_amdgcn_ballot_w64(prow_v >= 0);
                const int64_t page = min(pg_v, (uint32_t)(p.num_blocks - 1));
                const uint64_t a = (uint64_t)kbase + Fmt::kUnit * (uint64_t)(page * p.kc.batch + (int64_t)max(prow_v, 0) * p.kc.row);
                const uint32_t alo = (uint32_t)a, ahi = (uint32_t)(a >> 32);
                fmt.load_gathered(kbase, row0, mask, alo, ahi, st);
                prep_pages();                       // the table entries of the step after this one
                load_idx(key0 + 2 * kKvcStep);      // the index words of the step after that
            } else {
                mask = (uint32_t)__builtin_amdgcn_ballot_w64(idxv < (uint32_t)L);
                const uint32_t offv = min(idxv, (uint32_t)L) * row_b;
                fmt.load_listed(krs, row0, offv, st);
                load_idx(key0 + kKvcStep);          // the index words of the step after this one
            }
            if constexpr (BUF == 0) mask0 = mask;
            else mask1 = mask;
        } else if constexpr (PAGED) {
            const int blk = row0 >> 4;                                      // (wave-uniform)
            const int valid = min(max(L - (key0 + 16 * blk), 0), 16);
            const int64_t page = min(blk ? pg1 : pg0, (uint32_t)(p.num_blocks - 1));
            const int prow = blk ? rw1 : rw0;
            const char* base = uniform_ptr(kbase + Fmt::kUnit * (page * p.kc.batch + (int64_t)prow * p.kc.row));
            fmt.load_block(make_rsrc(base, valid > 0 ? (uint32_t)(valid - 1) * row_b + Fmt::kRowBytes : 0u), row0, row_b, st);
            fetch_pages();                      // the table entries of the step after this one
        } else {
            fmt.load_rows(krs, row0, key0, L, row_b, st);
        }
    };
    // registers -> the two images of stage BUF
    auto store_step = [&](auto bufc, const typename Fmt::Stage& st) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        FA_LDS char* vimg = (FA_LDS char*)smem + BUF * MlaLds::kStage;
        fmt.template store<T>(vimg, vimg + MlaLds::kImageV, row0, st);
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
        const uint32_t vm = (BUF == 0 ? mask0 : mask1) >> (4 * g);      // SPARSE: bit 16 b + r: slot 16 b + 4 g + r
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
                if constexpr (SPARSE) {
                    s[b][r] = (vm >> (16 * b + r)) & 1u ? s[b][r] : -INFINITY;
                } else {
                    const int key = key0 + 16 * b + 4 * g + r;
                    s[b][r] = key < lim ? s[b][r] : -INFINITY;
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
        static_for<0, NO>([&](auto cc) {
            constexpr int ci = decltype(cc)::value;
            oacc[ci] = LP<T>::mfma16(tr_frag<kMlaDV>(vimg, ci, g, q4, p4), pf, oacc[ci]);
        });
    };

    // ---- the split's 32-key steps, all four waves together; two LDS stages in turn (the schedule of fa_kvcache_stage.hpp) ---------------------------
    // k_begin and k_end are the workgroup's: every wave meets the same barriers.  (SPARSE: k_begin < k_end always - topk >= 32 and an empty split has
    // returned.)  load_step takes the stage its step will go to: step n + 2 goes where step n is.
    // Why FA_KVC_STAGE_RACY can neither hang nor fault here, in the dense and in the sparse body, with either row format, part (2) (part (1) stands at
    // kvc_stage_step): the two images are read by compute_step alone, as MFMA operands (kf, tr_frag): what comes out of them are scores and O, which reach compares, exponentials and stores of VALUES.  Rows, codes, tile scales
    // and rope words travel memory -> registers (-> dequant8) -> image, never back.  The gather does NOT go through the images: the sparse index words come
    // from global memory into registers (load_idx), cross lanes by v_readlane / ds_bpermute (the crossbar; no LDS byte is read or written), and masks, row
    // offsets, table columns and page addresses are computed from those registers.  Every address (lds_tile_off of lane constants, row_off / row_index of
    // the lane's row, the page cursor), every index and every loop bound comes from the parameters, the list and the block table.  A stale image gives
    // wrong numbers.
    {
        typename Fmt::Stage st;
        int key = k_begin;
        if constexpr (SPARSE) {
            load_idx(key);
            if constexpr (PAGED) {
                prep_pages();
                load_idx(key + kKvcStep);
            }
        }
        if ((SPARSE && !Fmt::kSparseFromDense) || key < k_end) {
            load_step(std::integral_constant<int, 0>{}, key, st);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st);
        }
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(std::integral_constant<int, 1>{}, key + kKvcStep, st);
        auto load = [&](auto bufc, int key0) __attribute__((always_inline)) { load_step(bufc, key0, st); };
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

// ---- what the launchers and the appends share -----------------------------------------------------------------------------------------------------------
// (The destination-row rule of the two append kernels - drop at the capacity, clamp the table entry to the pool - stays written out in each of them: folded
// into one helper it keeps its arithmetic, but the 16-bit paged append comes out with its instructions in another order.)
// The split of a sparse call is over topk and the grid b x seqlen_q x ceil(h / 64): sized on a copy that states the grid the way finish_params reads it,
// seqlen_q = 1 (a tile holds heads of one token) and seqlen_cache = topk.
inline void mla_sparse_finish_params(KvcacheKernelParams& kp, int32_t topk) {
    KvcacheKernelParams t = kp;
    t.seqlen_q = 1; t.seqlen_cache = topk; t.is_local = 0;
    finish_params(t, (int64_t)kp.b * kp.h * kp.seqlen_q, kMlaRows);
    kp.n_row_tiles = t.n_row_tiles; kp.rows_total = t.rows_total; kp.n_split = t.n_split; kp.split_keys = t.split_keys; kp.ws_lse = t.ws_lse;
}

// the combine of a split call: fa_kvcache_combine_kernel at D = 512
inline void mla_launch_combine(const KvcacheKernelParams& kp, int dtype, hipStream_t s) {
    if (dtype == 0) kvc_launch_combine<kMlaDV>(fa_kvcache_combine_kernel<_Float16, kMlaDV>, kp.rows_total, s, kp);
    else kvc_launch_combine<kMlaDV>(fa_kvcache_combine_kernel<__bf16, kMlaDV>, kp.rows_total, s, kp);
}

}  // namespace

}  // namespace fa
