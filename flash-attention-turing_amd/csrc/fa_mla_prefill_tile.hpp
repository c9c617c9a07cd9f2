// fa_mla_prefill_tile.hpp — the tile that the MLA prefill forward (fa_fwd_mla_prefill.hip) and the two kernels of its backward (fa_bwd_mla_prefill.hip) share.
//
//   192-wide q / k (128 no-rope columns, then 64 rope columns), 128-wide v / o.  A workgroup of four waves walks 32-row steps of one operand side through
//   registers into two LDS stages (the schedule of fa_kvcache_stage.hpp); a stage holds three images: the 128 no-rope columns (32 rows x 256 B,
//   lds_tile_off<128>), the 64 rope columns (32 rows x 128 B, lds_tile_off<64>) - a 384-byte row is no multiple of the 256-byte bank row lds_tile_off
//   argues about - and a 128-wide image (32 rows x 256 B).  The forward and dQ put K | K rope | V there, dK/dV puts Q | Q rope | dO.
//   Here: the constants and the LDS layout, the workgroup's sequence, the lane's staging slots with the K / V loads and the image writes, and the fragment
//   expressions.  What a body computes between them (softmax, dS, which rows are live) is the body's.
#pragma once
#include "fa_kvcache_attn.hpp"
#include "fa_kvcache_stage.hpp"

namespace fa {

constexpr int kMlapDN = 128;                // the no-rope columns of q / k
constexpr int kMlapDR = 64;                 // the rope columns
constexpr int kMlapDK = kMlapDN + kMlapDR;
constexpr int kMlapDV = 128;
constexpr int kMlapNC = kMlapDK / 32;       // 16x16x32 MFMAs per 16 rows of a product over the 192 columns: four over the wide image, two over the narrow one
constexpr int kMlapNL = 5;                  // 16-byte loads per lane and step: two of the wide image, one of the narrow one, two of the 128-wide one

// TAIL: bytes a body keeps behind the three images of a stage
template <int TAIL = 0>
struct MlapLds {
    static constexpr int kImageN = kKvcStep * kMlapDN * 2;      // 32 rows x 256 B
    static constexpr int kImageR = kKvcStep * kMlapDR * 2;      // 32 rows x 128 B
    static constexpr int kImageV = kKvcStep * kMlapDV * 2;      // 32 rows x 256 B
    static constexpr int kStage = kImageN + kImageR + kImageV + TAIL;       // 20 KB + TAIL
    static constexpr int kBytes = 2 * kStage;
};

// ---- the workgroup's sequence ---------------------------------------------------------------------------------------------------------------------------
// Dense grid: b x h_k x tiles.  Packed grid: tiles + b tile slots per KV head, found through kvc_slot_lookup; every sequence is tiled on its own from its
// first row, sequence i starts at row cu_q[i] of q / o and row cu_k[i] of k / v.
template <bool PACKED>
struct MlapSeq {
    int bidx, tile, kvh;        // the sequence, the tile inside it, the KV head
    int sq, L;                  // query rows and keys of the sequence
    int64_t q0 = 0, k0 = 0;     // PACKED: its first packed row of q / o and of k / v - cu_q[bidx] and cu_k[bidx], so (int)q0 < 0 asks for a negative entry

    // A body calls find_tile (false: a slack slot, nothing to write) and read_bounds, leaves if the range of the side it SERVES lies outside its tensor, and
    // calls cut for the other side.  The served side is the one the kernel writes: packed query rows (KEYS = false: the forward, dQ) or keys (KEYS = true:
    // dK/dV), ROWS of them a tile.  (Members in the order bidx, tile, and the range test as an `if (a || b) return` of the body: as a predicate here the two
    // branches come out as one, and in the other order two scalars of the slot lookup change places - tools/isa_diff.py.)
    template <int ROWS, bool KEYS, typename P>
    FA_DEV bool find_tile(const P& p) {
        const int id = blockIdx.x;
        const int n_tiles = PACKED ? p.slots : p.n_row_tiles;       // PACKED: the tile slots of a KV head, and `bh` below is the KV head
        tile = id % n_tiles;
        const int bh = id / n_tiles;
        bidx = bh / p.h_k, kvh = bh - bidx * p.h_k;
        sq = p.seqlen_q, L = p.seqlen_k;
        if constexpr (PACKED) {
            kvh = bh;
            const int slot = tile;
            return kvc_slot_lookup<ROWS>(KEYS ? p.cu_k : p.cu_q, p.b, KEYS ? 1 : p.h_ratio, (uint32_t)slot, bidx, tile);       // false: a slack slot
        } else {
            return true;
        }
    }
    // PACKED: the sequence's bounds.  cu_seqlens that point outside the tensors (a broken precondition) never become an address: a range of the served side
    // outside its tensor is not served, and the other side is cut at its tensor's last row.  Every value here is the workgroup's, so all four waves leave
    // together.
    template <typename P>
    FA_DEV void read_bounds(const P& p) {
        if constexpr (PACKED) {
            const int c0 = __builtin_amdgcn_readfirstlane(p.cu_q[bidx]);
            sq = __builtin_amdgcn_readfirstlane(p.cu_q[bidx + 1]) - c0;
            const int d0 = __builtin_amdgcn_readfirstlane(p.cu_k[bidx]);
            L = __builtin_amdgcn_readfirstlane(p.cu_k[bidx + 1]) - d0;
            q0 = c0;
            k0 = d0;
        }
    }
    template <bool KEYS, typename P>
    FA_DEV void cut(const P& p) {
        if constexpr (PACKED) {
            int& n = KEYS ? sq : L;
            const int64_t first = KEYS ? q0 : k0, left = (KEYS ? p.total_q : p.total_k) - first;
            n = (int)first < 0 || left < 0 ? 0 : (n > left ? (int)left : max(n, 0));
        }
    }
    // row (hq, t) of lse / dsoftmax_sum; element offset of its row in q / o / dout / dq (st = their strides)
    template <typename P>
    FA_DEV int64_t row_index(const P& p, int hq, int t) const {
        if constexpr (PACKED) return (int64_t)hq * p.total_q + q0 + t;
        else return ((int64_t)bidx * p.h + hq) * p.seqlen_q + t;
    }
    FA_DEV int64_t row_off(const TStride& st, int hq, int t) const {
        if constexpr (PACKED) return (q0 + t) * st.row + (int64_t)hq * st.head;
        else return (int64_t)bidx * st.batch + (int64_t)t * st.row + (int64_t)hq * st.head;
    }
    // CAUSAL: the keys of a tile of ROWS packed query rows end where its last row's do (t_last <= sq - 1, so the result is <= L; it may be <= 0: the tile
    // sees nothing)
    template <int ROWS, bool CAUSAL>
    FA_DEV int tile_key_end(int h_ratio) const {
        if constexpr (!CAUSAL) return L;
        const int t_last = (min((tile + 1) * ROWS, sq * h_ratio) - 1) / h_ratio;
        return __builtin_amdgcn_readfirstlane(min(L, L - sq + t_last + 1));
    }
};

// ---- staging ----------------------------------------------------------------------------------------------------------------------------------------------
// What a lane moves in a step.  A wave-wide 16-byte load covers 4 rows x 16 slots of a 128-wide image or 8 rows x 8 slots of the narrow one: loads 0, 1 are
// row 16 j + 4 w + lane / 16, slot lane % 16 of the wide image, load 2 is row 8 w + lane / 8, slot lane % 8 of the narrow one, loads 3, 4 are the rows of
// loads 0, 1 in the third image.
struct MlapLane {
    int wrow, wslot, rrow, rslot;
    FA_DEV MlapLane(int wave, int lane) : wrow(4 * wave + (lane >> 4)), wslot(lane & 15), rrow(8 * wave + (lane >> 3)), rslot(lane & 7) {}
};

struct MlapImages {
    FA_LDS char *nimg, *rimg, *vimg, *tail;
};
template <typename Lds, int BUF>
FA_DEV MlapImages mlap_images(char* smem) {
    FA_LDS char* nimg = (FA_LDS char*)smem + BUF * Lds::kStage;
    return MlapImages{nimg, nimg + Lds::kImageN, nimg + Lds::kImageN + Lds::kImageR, nimg + Lds::kImageN + Lds::kImageR + Lds::kImageV};
}

// registers -> the three images of a stage; with_rows(j) is the body's own write next to rows 16 j + wrow
template <typename WithRows>
FA_DEV void mlap_store_step(const MlapImages& im, const MlapLane& ln, const u32x4 (&st)[kMlapNL], WithRows&& with_rows) {
    static_for<0, 2>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        *(FA_LDS u32x4*)(im.nimg + lds_tile_off<kMlapDN>((uint32_t)(16 * j + ln.wrow), (uint32_t)ln.wslot)) = st[j];
        *(FA_LDS u32x4*)(im.vimg + lds_tile_off<kMlapDV>((uint32_t)(16 * j + ln.wrow), (uint32_t)ln.wslot)) = st[3 + j];
        with_rows(jj);
    });
    *(FA_LDS u32x4*)(im.rimg + lds_tile_off<kMlapDR>((uint32_t)ln.rrow, (uint32_t)ln.rslot)) = st[2];
}

// The K / V rows of a sequence's KV head (the forward, dQ).  K / V are plain strided tensors; one descriptor per tensor, ending at row L of the sequence:
// rows at or past L read as zeros (row indices are clamped to L, the row strides are at least the row widths, and L x row stride < 2^31 bytes by the host
// checks) and their scores are masked.
struct MlapKvRows {
    uint32_t krow_b, vrow_b;
    rsrc_t krs, vrs;
    int L;
    template <bool PACKED, typename P>
    FA_DEV MlapKvRows(const P& p, const MlapSeq<PACKED>& s) : krow_b((uint32_t)(p.k.row * 2)), vrow_b((uint32_t)(p.v.row * 2)), L(s.L) {
        const char* kbase = uniform_ptr((const char*)p.k_ptr + 2 * ((PACKED ? s.k0 * p.k.row : (int64_t)s.bidx * p.k.batch) + (int64_t)s.kvh * p.k.head));
        const char* vbase = uniform_ptr((const char*)p.v_ptr + 2 * ((PACKED ? s.k0 * p.v.row : (int64_t)s.bidx * p.v.batch) + (int64_t)s.kvh * p.v.head));
        krs = make_rsrc(kbase, L > 0 ? (uint32_t)(L - 1) * krow_b + 2 * kMlapDK : 0u);
        vrs = make_rsrc(vbase, L > 0 ? (uint32_t)(L - 1) * vrow_b + 2 * kMlapDV : 0u);
    }
    FA_DEV void load_step(const MlapLane& ln, int key0, u32x4 (&st)[kMlapNL]) const {
        static_for<0, 2>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            const uint32_t row = (uint32_t)min(key0 + 16 * j + ln.wrow, L);
            st[j] = buf_load16(krs, row * krow_b + 16 * ln.wslot);
            st[3 + j] = buf_load16(vrs, row * vrow_b + 16 * ln.wslot);
        });
        st[2] = buf_load16(krs, (uint32_t)min(key0 + ln.rrow, L) * krow_b + 2 * kMlapDN + 16 * ln.rslot);
    }
};

// ---- fragments --------------------------------------------------------------------------------------------------------------------------------------------
// acc[qb][B] += A x bf[qb][C0 + ci] over the W / 32 chunks ci of rows 16 B + n16 of a 32-row lds_tile_off<W> image (n16 = lane % 16, g = lane / 16): every A
// fragment is read once and serves the QB B operands
template <typename T, int W, int C0, int B, int QB, int NB>
FA_DEV void mlap_rows_mfma(const FA_LDS char* img, int n16, int g, const u32x4 (&bf)[QB][NB], f32x4 (&acc)[QB][2]) {
    static_for<0, W / 32>([&](auto cc) {
        constexpr int ci = decltype(cc)::value;
        const u32x4 a = *(const FA_LDS u32x4*)(img + lds_tile_off<W>(16 * B + n16, 4 * ci + g));
        static_for<0, QB>([&](auto qq) {
            constexpr int qb = decltype(qq)::value;
            acc[qb][B] = LP<T>::mfma16(a, bf[qb][C0 + ci], acc[qb][B]);
        });
    });
}
// the 192-column product over the wide and the narrow image: S^T = K Q^T (the forward, dQ), S = Q K^T (dK/dV)
template <typename T, int B, int QB>
FA_DEV void mlap_scores(const MlapImages& im, int n16, int g, const u32x4 (&bf)[QB][kMlapNC], f32x4 (&s)[QB][2]) {
    mlap_rows_mfma<T, kMlapDN, 0, B>(im.nimg, n16, g, bf, s);
    mlap_rows_mfma<T, kMlapDR, kMlapDN / 32, B>(im.rimg, n16, g, bf, s);
}

// columns 16 ci + 4 g .. + 3 of an output row from its accumulator block, times sc (row: the row's address + 4 g elements)
template <typename T>
FA_DEV void mlap_store_block(char* row, int ci, const f32x4& a, float sc) {
    *(u32x2*)(row + 32 * ci) = u32x2{LP<T>::pack2(a[0] * sc, a[1] * sc), LP<T>::pack2(a[2] * sc, a[3] * sc)};
}

// host: the (causal, packed) instantiation of a kernel template, of(causal, packed) with two std::bool_constant
template <typename F>
auto mlap_select(bool causal, bool packed, F of) {
    return causal ? (packed ? of(std::true_type{}, std::true_type{}) : of(std::true_type{}, std::false_type{}))
                  : (packed ? of(std::false_type{}, std::true_type{}) : of(std::false_type{}, std::false_type{}));
}

}  // namespace fa
