// fa_fwd_kvcache_mla_fp8.hip — MLA decode, dense and sparse, over an FP8 latent KV cache of 656-byte rows (kv_format = FA_MLA_KV_FP8_ROWS656): every
// kernel of fa_run_mla_fwd_kvcache / fa_run_mla_sparse_fwd_kvcache for that format.
//
//   One latent row: bytes 0 .. 511 the e4m3 codes of columns 0 .. 511, bytes 512 .. 527 four fp32 scales (scale g serves columns 128 g .. 128 g + 127),
//   bytes 528 .. 655 the 64 rope elements in q's dtype T.  The row stands for kv[c] = round_to_T(fp32(code[c]) * scale[c / 128]) (c < 512; one fp32
//   product, rounded once to nearest-even) and kv[512 + r] = the stored rope element.
//   The body is kvcache_mla_attn of fa_fwd_kvcache_mla.hip and, with SPARSE, kvcache_mla_sparse_attn of fa_fwd_kvcache_mla_sparse.hip, restated: tiling,
//   split, the 32-key step, the two LDS images per stage (lds_tile_off<512>, lds_tile_off<64>, 72 KB), the barrier scheme, compute_step, the epilogue and
//   the partial planes are theirs word for word.  ONLY STAGING CHANGES: the codes are dequantised where the 512 image is written, so everything behind the
//   barrier reads the LDS bytes the 16-bit kernels read for the dequantised cache, and the two calls agree to the bit.
//   * Loads.  Wave w stages rows 8 w .. 8 w + 7 of a step.  A 16-byte load of the code part covers 16 columns; a row is 32 of them, so one wave-wide load
//     covers two rows: load j < 4 takes row 8 w + 2 j + lane / 32, chunk lane % 32, and with it the scale dword of the chunk's tile (chunk / 8).  The rope
//     part is one 16-byte load per lane at byte 528 of row 8 w + lane / 8.  Nine loads and 24 staging registers per lane and step.
//   * Descriptors.  Those of the 16-bit kernels with the 656-byte row: contiguous, one per sequence ending at row L (row indices clamped to L); paged dense,
//     one per wave and step over the wave's rows of its 16-key block, empty for a block past L.  SPARSE contiguous: the per-sequence descriptor with the
//     row offset of the list entry (min((uint32_t)idx, L) rows: an invalid entry lands at the descriptor's end); the lanes of one load read two rows, so the
//     offsets come from the owning lanes by ds_bpermute.  SPARSE paged: per-lane loads from the 64-bit row address (ds_bpermute of both halves) that the
//     lanes of an invalid slot do not issue; their zeros come from a load over an empty range.  Rows past L, pages past L and whatever an invalid slot names
//     are never read, and they load as code 0 under scale 0: a zero image row.
//   * Dequantisation (store_step): v_cvt_pk_f32_fp8 (exact), one v_mul_f32 by the tile's scale, LP<T>::pack2 (round to nearest-even: v_cvt_pk_bf16_f32 /
//     v_cvt_pk_f16_f32, never the truncating v_cvt_pkrtz).  A chunk fills the two 16-byte slots 2 chunk, 2 chunk + 1 of its image row.
//   * The append (dense call only) quantises kv_new in place: one wave per new row, lane l holds columns 8 l .. 8 l + 7, the 16 lanes of a tile take
//     amax over their finite elements by cross-lane max, scale = max(amax, 2^-24) / 448 (the correctly rounded quotient), codes by quant8_e4m3
//     (fa_kvcache_quant.hpp), the rope part copied.  Drop and clamp rules of fa_kvcache_mla_append_kernel.
//   Kernels of this file: 8 dense attention ((fp16, bf16) x (causal, not) x (contiguous, paged)), 4 sparse attention ((fp16, bf16) x (contiguous, paged)),
//   4 append ((fp16, bf16) x (contiguous, paged)), 2 combine (fa_kvcache_combine_kernel at D = 512).
#include "fa_kvcache_launch.hpp"
#include "fa_kvcache_quant.hpp"
#include "fa_kvcache_stage_debug.hpp"

namespace fa {

namespace {

constexpr int kMlaRows = kKvcPrefillRows;   // packed query rows of a workgroup: 16 per wave
constexpr int kMlaDV = 512;                 // the compressed part: V, and columns 0 .. 511 of K
constexpr int kMlaDR = 64;                  // the rope part: columns 512 .. 575 of K
constexpr int kMlaDK = kMlaDV + kMlaDR;
constexpr int kMla8Scales = kMlaDV;         // byte of a row where the four fp32 scales start
constexpr int kMla8Rope = kMlaDV + 16;      // ... and where the rope elements start
constexpr int kMla8RowBytes = kMla8Rope + 2 * kMlaDR;   // 656: 41 16-byte slots

struct MlaLds {
    static constexpr int kImageV = kKvcStep * kMlaDV * 2;       // 32 rows x 1024 B
    static constexpr int kImageR = kKvcStep * kMlaDR * 2;       // 32 rows x 128 B
    static constexpr int kStage = kImageV + kImageR;            // 36 KB
    static constexpr int kBytes = 2 * kStage;                   // 72 KB
};

// what a lane holds of one step between its loads and the LDS writes
struct Mla8Stage {
    u32x4 code[4];      // load j: 16 codes of row 8 w + 2 j + lane / 32
    uint32_t scale[4];  // ... and the fp32 scale of their tile
    u32x4 rope;
};

FA_DEV uint32_t buf_load4(rsrc_t r, uint32_t byte_off) { return __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0); }

// eight codes (two dwords) x scale -> eight elements of T: one 16-byte slot of the 512 image
template <typename T>
FA_DEV u32x4 dequant8(uint32_t w0, uint32_t w1, float s) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
    return u32x4{LP<T>::pack2(a[0] * s, a[1] * s), LP<T>::pack2(b[0] * s, b[1] * s), LP<T>::pack2(c[0] * s, c[1] * s), LP<T>::pack2(d[0] * s, d[1] * s)};
}

// SPARSE = false: the dense call (indices, idx_*, topk are not read).  SPARSE = true: CAUSAL is false; a tile is 64 heads of one token and the keys of a
// step are the slots of the token's list.
template <typename T, bool CAUSAL, bool PAGED, bool SPARSE>
FA_DEV void kvcache_mla8_attn(const KvcacheKernelParams& p, const int32_t* indices, int64_t idx_batch, int64_t idx_row, int topk) {
    static_assert(!(SPARSE && CAUSAL), "the list is the mask");
    constexpr int NCV = kMlaDV / 32;    // 16x16x32 MFMAs per 16 keys of S^T over the 512 image
    constexpr int NCR = kMlaDR / 32;    // ... and over the 64 image
    constexpr int NC = NCV + NCR;
    constexpr int NO = kMlaDV / 16;     // O^T blocks of 16 columns
    constexpr int RW = kKvcStep / kKvcWaves;    // rows of a step a wave stages: 8, inside one 16-key block
    constexpr int NJ = RW / 2;          // code loads per lane and step: two rows each
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
    // dense: the keys [0, k_hi); CAUSAL: the tile's keys end where its last row's do.  SPARSE: the slots [0, topk) of the token's list
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
    // load j < 4: row 8 w + 2 j + lane / 32, 16-byte chunk lane % 32 of its 512 codes, and scale (lane % 32) / 8; rope: row 8 w + lane / 8, 16-byte slot
    // lane % 8 of its 128 rope bytes.  The cache strides kc are in BYTES.
    const int row0 = wave * RW;
    const int hw = lane >> 5, ch = lane & 31;
    const uint32_t coff = 16 * ch, soff = kMla8Scales + 4 * (ch >> 3);
    const int rrow = lane >> 3, rslot = lane & 7;
    const uint32_t roff = kMla8Rope + 16 * rslot;
    const uint32_t row_b = (uint32_t)p.kc.row;
    const char* kbase = uniform_ptr((const char*)p.k_cache + (int64_t)(PAGED ? 0 : bidx) * p.kc.batch);
    // contiguous: one descriptor, ending at row L (rows at or past L read as zeros; row indices are clamped to L, and L x row stride < 2^31
    // by the host checks)
    const rsrc_t krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * row_b + kMla8RowBytes : 0u);
    const int P = p.page_size;
    // dense paged: the table cursor of kvcache_mla_attn - the entries of the step after the one being loaded are fetched with that load
    typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
    const const_i32_ptr tbl = PAGED && !SPARSE ? (const_i32_ptr)(p.block_table + (int64_t)bidx * p.bt_stride) : nullptr;
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
    if constexpr (PAGED && !SPARSE) {
        f_col = __builtin_amdgcn_readfirstlane(k_begin / P);
        f_row = k_begin - f_col * P;
        st_col = __builtin_amdgcn_readfirstlane(kKvcStep / P);
        st_row = kKvcStep - st_col * P;
        fetch_pages();
    }
    // SPARSE: the index words of kvcache_mla_sparse_attn - lane l holds the word of slot l & 31 of a step, fetched one step ahead (paged: two, so that the
    // table entry is fetched one step ahead)
    const int islot = lane & 31;
    const int32_t* ip = SPARSE ? indices + ((int64_t)bidx * idx_batch + (int64_t)tok * idx_row) : nullptr;
    const int last_key0 = k_end - kKvcStep;     // the split's last step: index loads past it are clamped to it
    const int32_t* stbl = PAGED && SPARSE ? p.block_table + (int64_t)bidx * p.bt_stride : nullptr;
    uint32_t idxv = 0u;
    uint32_t pg_v = 0u;                         // SPARSE paged: the table entry (unclamped) of the lane's slot of the next step to load ...
    int prow_v = -1;                            // ... and the slot's row in its page, -1 = an invalid slot
    uint32_t mask0 = 0u, mask1 = 0u;            // SPARSE: valid slots of the step held by stage 0 / 1
    auto load_idx = [&](int key0) __attribute__((always_inline)) { idxv = (uint32_t)ip[min(key0, last_key0) + islot]; };
    auto prep_pages = [&]() __attribute__((always_inline)) {
        const bool ok = idxv < (uint32_t)L;
        const uint32_t j = ok ? idxv : 0u;
        const uint32_t col = j / (uint32_t)P;
        prow_v = ok ? (int)(j - col * (uint32_t)P) : -1;
        pg_v = (uint32_t)stbl[min(col, (uint32_t)last_col)];
    };
    auto load_step = [&](auto bufc, int key0, Mla8Stage& st) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        if constexpr (SPARSE && PAGED) {
            const uint32_t mask = (uint32_t)__builtin_amdgcn_ballot_w64(prow_v >= 0);
            const int64_t page = min(pg_v, (uint32_t)(p.num_blocks - 1));
            const uint64_t a = (uint64_t)kbase + (uint64_t)(page * p.kc.batch + (int64_t)max(prow_v, 0) * p.kc.row);
            const uint32_t alo = (uint32_t)a, ahi = (uint32_t)(a >> 32);
            const rsrc_t none = make_rsrc(kbase, 0u);
            typedef const __attribute__((address_space(1))) u32x4* g16_ptr;
            typedef const __attribute__((address_space(1))) uint32_t* g4_ptr;
            // (the zeros of the lanes that do not load come from loads over an empty range, as in kvcache_mla_sparse_attn - each at an offset of its own:
            // identical loads are merged into one whose zeros are then copied into every staging register, 16 v_accvgpr moves a step)
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
            prep_pages();                       // the table entries of the step after this one
            load_idx(key0 + 2 * kKvcStep);      // the index words of the step after that
            if constexpr (BUF == 0) mask0 = mask;
            else mask1 = mask;
        } else if constexpr (SPARSE) {
            const uint32_t mask = (uint32_t)__builtin_amdgcn_ballot_w64(idxv < (uint32_t)L);
            const uint32_t offv = min(idxv, (uint32_t)L) * row_b;
            static_for<0, NJ>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                const uint32_t ro = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + 2 * j + hw), offv);
                st.code[j] = buf_load16(krs, ro + coff);
                st.scale[j] = buf_load4(krs, ro + soff);
            });
            st.rope = buf_load16(krs, (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (row0 + rrow), offv) + roff);
            load_idx(key0 + kKvcStep);          // the index words of the step after this one
            if constexpr (BUF == 0) mask0 = mask;
            else mask1 = mask;
        } else if constexpr (PAGED) {
            const int blk = row0 >> 4;                                      // (wave-uniform)
            const int valid = min(max(L - (key0 + 16 * blk), 0), 16);
            const int64_t page = min(blk ? pg1 : pg0, (uint32_t)(p.num_blocks - 1));
            const int prow = blk ? rw1 : rw0;
            const char* base = uniform_ptr(kbase + (page * p.kc.batch + (int64_t)prow * p.kc.row));
            const rsrc_t r = make_rsrc(base, valid > 0 ? (uint32_t)(valid - 1) * row_b + kMla8RowBytes : 0u);
            static_for<0, NJ>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                const uint32_t ro = (uint32_t)((row0 & 15) + 2 * j + hw) * row_b;
                st.code[j] = buf_load16(r, ro + coff);
                st.scale[j] = buf_load4(r, ro + soff);
            });
            st.rope = buf_load16(r, (uint32_t)((row0 & 15) + rrow) * row_b + roff);
            fetch_pages();                      // the table entries of the step after this one
        } else {
            static_for<0, NJ>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                const uint32_t ro = (uint32_t)min(key0 + row0 + 2 * j + hw, L) * row_b;
                st.code[j] = buf_load16(krs, ro + coff);
                st.scale[j] = buf_load4(krs, ro + soff);
            });
            st.rope = buf_load16(krs, (uint32_t)min(key0 + row0 + rrow, L) * row_b + roff);
        }
    };
    // registers -> the two images of stage BUF; the codes become elements of T here
    auto store_step = [&](auto bufc, const Mla8Stage& st) __attribute__((always_inline)) {
        constexpr int BUF = decltype(bufc)::value;
        FA_LDS char* vimg = (FA_LDS char*)smem + BUF * MlaLds::kStage;
        FA_LDS char* rimg = vimg + MlaLds::kImageV;
        static_for<0, NJ>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const float s = __builtin_bit_cast(float, st.scale[j]);
            const uint32_t row = (uint32_t)(row0 + 2 * j + hw);
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>(row, (uint32_t)(2 * ch))) = dequant8<T>(st.code[j].x, st.code[j].y, s);
            *(FA_LDS u32x4*)(vimg + lds_tile_off<kMlaDV>(row, (uint32_t)(2 * ch + 1))) = dequant8<T>(st.code[j].z, st.code[j].w, s);
        });
        *(FA_LDS u32x4*)(rimg + lds_tile_off<kMlaDR>((uint32_t)(row0 + rrow), (uint32_t)rslot)) = st.rope;
    };

    // transposed-read addresses of this lane (fa_device.hpp lds_tile_off image): block c, half hh -> rows hh * 16 + 4 g + q, columns 16 c + 4 p
    const int q4 = n16 >> 2, p4 = n16 & 3;

    f32x4 oacc[NO];
    static_for<0, NO>([&](auto cc) {
        oacc[decltype(cc)::value] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(oacc[decltype(cc)::value]));
    });
    float m_run = kNegBig, l_run = 0.f;

    // one 32-key step of this wave's 16 rows over the images of stage BUF: the arithmetic of kvcache_mla_attn (SPARSE: the step's mask in the place of
    // key < lim, as in kvcache_mla_sparse_attn)
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

    // ---- the split's 32-key steps, all four waves together; two LDS stages in turn (the schedule of kvcache_mla_attn) ----------------------
    // Stage n & 1 holds step n.  While step n computes, the loads of step n + 1 are in flight; they are written to the other stage behind the
    // compute - every wave left that stage's reads (step n - 1) in front of the last barrier - and one barrier publishes them.  The loads of
    // step n + 2 are issued behind that barrier, so nothing is outstanding when it is reached.  k_end is the workgroup's: every wave meets
    // the same barriers.  (SPARSE: k_begin < k_end always - topk >= 32 and an empty split has returned.)
    // Test builds (FA_KVC_STAGE_DEBUG, fa_kvcache_stage_debug.hpp): the two helpers hold one wave back; FA_KVC_STAGE_RACY moves the step's barrier in front of store_step.
    // Why the racy form can neither hang nor fault here, in the dense and in the sparse body: (1) the barrier only changes places inside the same
    // `if (key0 + kKvcStep < k_end)`, whose condition is the workgroup's (k_begin, k_end and key0 are the same in every wave, `active` is not part of it),
    // so every wave still meets the same number of barriers on every path; (2) the two images are read by compute_step alone, as MFMA operands (kf, v0 /
    // v1): what comes out of them are scores and O, which reach compares, exponentials and stores of VALUES.  Codes, tile scales and rope words travel
    // memory -> registers -> dequant8 -> image, never back; the sparse index words, masks, row offsets and page addresses live in registers and cross lanes
    // by ds_bpermute (the crossbar; no LDS byte is read or written).  Every address, index and loop bound comes from the parameters, the list and the block
    // table.  A stale image gives wrong numbers.
    {
        Mla8Stage st;
        int key = k_begin;
        if constexpr (SPARSE) {
            load_idx(key);
            if constexpr (PAGED) {
                prep_pages();
                load_idx(key + kKvcStep);
            }
        }
        if (key < k_end) {
            load_step(std::integral_constant<int, 0>{}, key, st);
            kvc_stage_slow_writer(-1, wave);
            store_step(std::integral_constant<int, 0>{}, st);
        }
        __syncthreads();
        if (key + kKvcStep < k_end) load_step(std::integral_constant<int, 1>{}, key + kKvcStep, st);
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

// ONE workgroup per compute unit, as the 16-bit MLA kernels ship: O^T (128 registers), Q^T (72) and the staging set (24) next to the softmax; with the
// register class ahead of the range's length in the allocator (build.py EXTRA_FLAGS) Q^T and the staging set take the AGPRs.
template <typename T, bool CAUSAL, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_mla_fp8_kernel(const KvcacheMlaParams mp) {
    kvcache_mla8_attn<T, CAUSAL, PAGED, false>(mp.kp, nullptr, 0, 0, 0);
}

template <typename T, bool PAGED>
__global__ __launch_bounds__(kKvcThreads, 1) void fa_fwd_kvcache_mla_sparse_fp8_kernel(const KvcacheMlaSparseParams sp) {
    kvcache_mla8_attn<T, false, PAGED, true>(sp.kp, sp.indices, sp.idx_batch, sp.idx_row, sp.topk);
}

// kv_new (b, seqlen_new, 1, 576) of T -> whole 656-byte cache rows cache_seqlens[i] .. + seqlen_new - 1: one wave per new row, four rows a workgroup.  Lane l
// holds columns 8 l .. 8 l + 7; lanes 16 g .. 16 g + 15 are tile g.  Rows at or past the capacity seqlen_cache are dropped; PAGED: row (.) % page_size of
// page min((uint32_t)block_table[i][(.) / page_size], num_blocks - 1) - the rules of fa_kvcache_mla_append_kernel.  kc in bytes, kn in elements.
template <typename T, bool PAGED>
__global__ __launch_bounds__(256) void fa_kvcache_mla_append_fp8_kernel(const KvcacheMlaParams mp) {
    const KvcacheKernelParams& p = mp.kp;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (int64_t)p.b * p.seqlen_new) return;
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
    const char* src = (const char*)p.k_new + 2 * ((int64_t)bidx * p.kn.batch + (int64_t)t * p.kn.row);
    char* dst = (char*)p.k_cache + (blk * p.kc.batch + prow * p.kc.row);
    const u32x4 x = *(const u32x4*)(src + 16 * lane);
    // amax over the finite elements (NaN and +-inf skipped: |bits| below the first non-finite pattern), exact in fp32
    float amax = 0.f;
    static_for<0, 8>([&](auto ee) {
        constexpr int e = decltype(ee)::value;
        const uint16_t bits = (uint16_t)((x[e >> 1] >> (16 * (e & 1))) & 0x7fffu);
        const bool finite = bits < (__is_same(T, _Float16) ? 0x7c00u : 0x7f80u);
        amax = fmaxf(amax, finite ? LP<T>::to_float(bits) : 0.f);
    });
    static_for<0, 4>([&](auto ss) { amax = fmaxf(amax, __shfl_xor(amax, 1 << decltype(ss)::value, 64)); });
    const float scale = fmaxf(amax, 0x1p-24f) / 448.f;
    *(u32x2*)(dst + 8 * lane) = quant8_e4m3<T>(x, scale);
    if ((lane & 15) == 0) *(float*)(dst + kMla8Scales + 4 * (lane >> 4)) = scale;
    if (lane < 2 * kMlaDR / 16) *(u32x4*)(dst + kMla8Rope + 16 * lane) = *(const u32x4*)(src + 2 * kMlaDV + 16 * lane);
}

template <typename T>
void mla8_combine(const KvcacheKernelParams& kp, hipStream_t s) {
    kvc_launch_combine<kMlaDV>(fa_kvcache_combine_kernel<T, kMlaDV>, kp.rows_total, s, kp);
}

}  // namespace

// append, attention, combine: launch_fwd_kvcache_mla for kv_format = FA_MLA_KV_FP8_ROWS656.  mp.kp as there, with kc in bytes and cache_fp8 = 1.
hipError_t launch_fwd_kvcache_mla_fp8(KvcacheMlaParams mp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = mp.kp;
    if (kp.d != kMlaDV || mp.d_qk != kMlaDK || kp.h_k != 1 || !kp.cache_fp8) return hipErrorInvalidValue;
    finish_params(kp, (int64_t)kp.b * kp.h * kp.seqlen_q, kMlaRows);
    const bool paged = kp.block_table != nullptr;
    const unsigned grid = (unsigned)((int64_t)kp.b * kp.n_row_tiles * kp.n_split);
    auto launch = [&](auto* tt) {
        using T = std::remove_pointer_t<decltype(tt)>;
        if (kp.k_new != nullptr && kp.seqlen_new > 0) {
            const int64_t n = (int64_t)kp.b * kp.seqlen_new;
            auto* append = paged ? fa_kvcache_mla_append_fp8_kernel<T, true> : fa_kvcache_mla_append_fp8_kernel<T, false>;
            hipLaunchKernelGGL(append, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, mp);
        }
        auto* kernel = kp.is_causal ? (paged ? fa_fwd_kvcache_mla_fp8_kernel<T, true, true> : fa_fwd_kvcache_mla_fp8_kernel<T, true, false>)
                                    : (paged ? fa_fwd_kvcache_mla_fp8_kernel<T, false, true> : fa_fwd_kvcache_mla_fp8_kernel<T, false, false>);
        kvc_launch_attn(kernel, grid, s, mp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) {
        if (dtype == 0) mla8_combine<_Float16>(kp, s);
        else mla8_combine<__bf16>(kp, s);
    }
    return hipGetLastError();
}

// attention, combine: launch_fwd_kvcache_mla_sparse for kv_format = FA_MLA_KV_FP8_ROWS656 (the split is sized as there).
hipError_t launch_fwd_kvcache_mla_sparse_fp8(KvcacheMlaSparseParams sp, int dtype, hipStream_t s) {
    KvcacheKernelParams& kp = sp.kp;
    if (kp.d != kMlaDV || sp.d_qk != kMlaDK || kp.h_k != 1 || !kp.cache_fp8 || sp.indices == nullptr || sp.topk < kKvcStep || sp.topk % kKvcStep != 0)
        return hipErrorInvalidValue;
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
        kvc_launch_attn(paged ? fa_fwd_kvcache_mla_sparse_fp8_kernel<T, true> : fa_fwd_kvcache_mla_sparse_fp8_kernel<T, false>, grid, s, sp);
    };
    if (dtype == 0) launch((_Float16*)nullptr);
    else launch((__bf16*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (kp.n_split > 1) {
        if (dtype == 0) mla8_combine<_Float16>(kp, s);
        else mla8_combine<__bf16>(kp, s);
    }
    return hipGetLastError();
}

}  // namespace fa
