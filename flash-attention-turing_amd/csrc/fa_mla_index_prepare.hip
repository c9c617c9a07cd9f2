// fa_mla_index_prepare.hip — the front end of the DeepSeek-V3.2 indexer (fa_run_mla_index_prepare_queries / fa_run_mla_index_prepare_append): the 128-point
// Hadamard rotation the model applies to every index query head and every index key after RoPE (rotate_activation), the e4m3 row quantiser behind it, and for
// the keys the placement into the index-key cache.  One launch each; no LDS, no barrier, no scratch.
//
//   * Rows.  A workgroup is four waves and 64 rows, a wave owns 16.  Lane (g, n16) = (lane >> 4, lane & 15) belongs to row n16 of its wave throughout: it loads
//     from that row, reduces over it and stores to it.  Rows past the end (and key rows that are surplus or dropped) are loaded as +0 and not stored, so every
//     lane runs the cross-lane steps.
//   * Loads.  Lane (g, n16) loads 16 bytes at elements 32 c + 8 g of its row, c = 0 .. 3: the B operand of v_mfma_f32_16x16x32 for the contraction block c,
//     straight from global memory (the qf[] fragment of fa_fwd_kvcache_prefill.hip).
//   * The transform, Y^T (128 x 16) = H (128 x 128) . X^T (128 x 16), H[i][j] = (-1) ** popcount(i & j).  H is never loaded.  For output block ib (rows
//     16 ib + il) and contraction index j = 32 c + 8 g + e the bits of i & j split into il & (8 (g & 1) + e) and ib & (2 c + (g >> 1)), so
//         sign = parity(il & (8 (g & 1) + e))  ^  parity(ib & 2 c)  ^  ((ib & 1) & (g >> 1)).
//     The first term is one fragment of +-1.0 per lane, built once from the lane index; the second is a compile-time negation; the third negates the upper two
//     lane groups when ib is odd.  Four copies of the fragment (base, -base, mixed, -mixed: 16 registers) cover all 32 (ib, c) pairs, and the 32 MFMAs of a wave
//     take their A operand from one of them with no instruction in between.  Products with +-1 are exact, the sums are fp32.
//   * Epilogue, in registers.  Lane (g, n16) holds columns 16 ib + 4 g + r of its row.  Times fl32(128 ** -0.5), rounded to T (v_cvt_pk, RNE) - the model's
//     transform returns its input dtype - then the quantiser of fa_mla_cache_io.hip on those 16-bit words: amax over the finite elements (io_amax8), over the
//     row's four lanes (max_four_groups), scale = max(amax, 2^-24) / 448 by a true division, UE8M0 on its bits, codes by quant8_e4m3.  HAD = false skips the
//     MFMAs and runs the same epilogue on the words as loaded (lane (g, n16) then holds columns 32 c + 8 g + e).
//   * Stores.  A lane's codes are eight dwords, 16 (HAD) or two times 4 (plain) bytes apart.  Two 4 x 4 transposes over (register, lane group) - four
//     v_permlane32_swap and four v_permlane16_swap - leave lane (G, n16) with bytes 32 G .. 32 G + 31 of its row: two 16-byte stores a lane, 64 contiguous
//     bytes per row and instruction, against eight dword stores with 16 ("The indexer's front end").  Lane (0, n16) writes the row's scale (keys) or
//     weights * scale (queries).
//   Offsets are 64-bit.  Kernels of this file: 8 for queries ((fp16, bf16) x (rotated, plain) x (fp32 scale, UE8M0)), 16 for keys ((fp16, bf16) x (fp32 scale,
//   UE8M0) x (contiguous, paged) x (dense, packed)).
#include "fa_mla_index_prepare.hpp"

#include "fa_kvcache_quant.hpp"

namespace fa {

namespace {

constexpr float kRotScale = 0.08838834764831845f;      // fl32(128 ** -0.5)

// (register, lane group) transpose of four dwords over lanes l, l ^ 16, l ^ 32, l ^ 48: afterwards register j of group G holds what register G of group j held
FA_DEV void transpose_four_groups(uint32_t (&d)[4]) {
    static_for<0, 2>([&](auto jj) {        // bit 1 of the register index against bit 1 of the group: the upper half-wave of d[j] <-> the lower half-wave of d[j + 2]
        constexpr int j = decltype(jj)::value;
        auto r = __builtin_amdgcn_permlane32_swap(d[j], d[j + 2], false, false);
        d[j] = r[0];
        d[j + 2] = r[1];
    });
    static_for<0, 2>([&](auto jj) {        // bit 0 against bit 0: the odd 16-lane groups of d[j] <-> the even ones of d[j + 1]
        constexpr int j = 2 * decltype(jj)::value;
        auto r = __builtin_amdgcn_permlane16_swap(d[j], d[j + 1], false, false);
        d[j] = r[0];
        d[j + 1] = r[1];
    });
}

// The 16 rows of a wave.  src: the lane's row (read if ok).  Returns the row's scale and, for lane (G, n16), bytes 32 G .. 32 G + 15 (lo) and 32 G + 16 ..
// 32 G + 31 (hi) of the row's codes.  Every lane of the wave must call it.
template <typename T, bool HAD, bool UE8M0>
FA_DEV float prepare_rows(const char* src, bool ok, int lane, u32x4& lo, u32x4& hi) {
    const int g = lane >> 4;
    u32x4 x[4];
    static_for<0, 4>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        x[c] = ok ? *(const u32x4*)(src + 2 * (32 * c + 8 * g)) : u32x4{0u, 0u, 0u, 0u};
    });
    u32x4 u[4];     // HAD: u[k] = columns 32 k + 4 g + (0 .. 3) and 32 k + 16 + 4 g + (0 .. 3), rounded to T; plain: columns 32 k + 8 g + (0 .. 7)
    if constexpr (HAD) {
        const int il = lane & 15;
        u32x4 a[4];     // [0] base, [1] -base, [2] base with the upper two lane groups negated, [3] its negation
        static_for<0, 4>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            const uint32_t s0 = (uint32_t)__builtin_popcount(il & (8 * (g & 1) + 2 * k)) & 1u, s1 = (uint32_t)__builtin_popcount(il & (8 * (g & 1) + 2 * k + 1)) & 1u;
            a[0][k] = LP<T>::kOnes2 ^ (s0 << 15) ^ (s1 << 31);
            a[1][k] = a[0][k] ^ 0x80008000u;
            a[2][k] = a[0][k] ^ ((g >> 1) ? 0x80008000u : 0u);
            a[3][k] = a[2][k] ^ 0x80008000u;
        });
        f32x4 acc[8];
        static_for<0, 4>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            static_for<0, 8>([&](auto bb) {
                constexpr int ib = decltype(bb)::value;
                constexpr int which = 2 * (ib & 1) + (__builtin_popcount(ib & (2 * c)) & 1);
                acc[ib] = LP<T>::mfma16(a[which], x[c], c == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[ib]);
            });
        });
        static_for<0, 4>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            const f32x4 p = acc[2 * k] * kRotScale, q = acc[2 * k + 1] * kRotScale;
            u[k] = u32x4{LP<T>::pack2(p[0], p[1]), LP<T>::pack2(p[2], p[3]), LP<T>::pack2(q[0], q[1]), LP<T>::pack2(q[2], q[3])};
        });
    } else {
        static_for<0, 4>([&](auto kk) { u[decltype(kk)::value] = x[decltype(kk)::value]; });
    }
    float amax = fmaxf(fmaxf(io_amax8<T>(u[0]), io_amax8<T>(u[1])), fmaxf(io_amax8<T>(u[2]), io_amax8<T>(u[3])));
    float scale = fmaxf(max_four_groups(amax), 0x1p-24f) / 448.f;
    if constexpr (UE8M0) scale = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, scale) + 0x007fffffu) & 0x7f800000u);
    uint32_t cx[4], cy[4];
    static_for<0, 4>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        const u32x2 c8 = quant8_e4m3<T>(u[k], scale);
        cx[k] = c8.x;
        cy[k] = c8.y;
    });
    // before: group g, register k: cx = bytes 32 k + 4 g (HAD) / 32 k + 8 g (plain), cy = 16 (HAD) / 4 (plain) bytes behind.  After: group G, register j: k = G, g = j
    transpose_four_groups(cx);
    transpose_four_groups(cy);
    if constexpr (HAD) {
        lo = u32x4{cx[0], cx[1], cx[2], cx[3]};
        hi = u32x4{cy[0], cy[1], cy[2], cy[3]};
    } else {
        lo = u32x4{cx[0], cy[0], cx[1], cy[1]};
        hi = u32x4{cx[2], cy[2], cx[3], cy[3]};
    }
    return scale;
}

template <typename T, bool HAD, bool UE8M0>
__global__ __launch_bounds__(kIdxPrepThreads) void fa_mla_index_prepare_queries_kernel(const MlaIndexPrepareQParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kIdxPrepRows + 16 * (threadIdx.x >> 6) + (lane & 15);
    const bool ok = r < p.total;
    const uint32_t token = (uint32_t)(ok ? r : 0) / (uint32_t)p.heads, head = (uint32_t)(ok ? r : 0) - token * (uint32_t)p.heads;
    u32x4 lo, hi;
    const float scale = prepare_rows<T, HAD, UE8M0>((const char*)p.q + (int64_t)token * p.q_token + (int64_t)head * p.q_head, ok, lane, lo, hi);
    if (!ok) return;
    char* dst = (char*)p.codes + r * 128 + 32 * (lane >> 4);
    *(u32x4*)dst = lo;
    *(u32x4*)(dst + 16) = hi;
    if (lane < 16) p.w8[r] = p.weights[(int64_t)token * p.w_token + (int64_t)head * p.w_head] * scale;
}

template <typename T, bool UE8M0, bool PAGED, bool PACKED>
__global__ __launch_bounds__(kIdxPrepThreads) void fa_mla_index_prepare_append_kernel(const MlaCacheIoParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kIdxPrepRows + 16 * (threadIdx.x >> 6) + (lane & 15);
    int bidx = 0;
    int64_t t = 0, blk = 0, prow = 0;
    // (a surplus or dropped row is neither read nor written)
    const bool ok = r < p.total && io_locate<PACKED>(p, r, bidx, t) && io_append_place<PAGED>(p, bidx, t, blk, prow);
    u32x4 lo, hi;
    const float scale = prepare_rows<T, true, UE8M0>((const char*)p.src + (PACKED ? r * p.s_row : (int64_t)bidx * p.s_batch + t * p.s_row), ok, lane, lo, hi);
    if (!ok) return;
    char* dst = (char*)p.cache + blk * p.c_batch + prow * p.c_row + 32 * (lane >> 4);
    *(u32x4*)dst = lo;
    *(u32x4*)(dst + 16) = hi;
    if (lane < 16) p.k_scale[blk * p.ks_batch + prow * p.ks_row] = scale;
}

template <typename K, typename P>
hipError_t prep_launch(K* kernel, const P& p, hipStream_t s) {
    const int64_t grid = (p.total + kIdxPrepRows - 1) / kIdxPrepRows;
    if (grid <= 0 || grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kIdxPrepThreads), 0, s, p);
    return hipGetLastError();
}

// kernel<T, A, B> chosen by two run-time flags
#define FA_PREP_PICK2(KERNEL, T, a, b) ((a) ? ((b) ? KERNEL<T, true, true> : KERNEL<T, true, false>) : ((b) ? KERNEL<T, false, true> : KERNEL<T, false, false>))
// kernel<T, UE8M0, PAGED, PACKED> chosen by the two run-time layout flags
#define FA_PREP_PICK_IO(T, U) \
    (paged ? (packed ? fa_mla_index_prepare_append_kernel<T, U, true, true> : fa_mla_index_prepare_append_kernel<T, U, true, false>) \
           : (packed ? fa_mla_index_prepare_append_kernel<T, U, false, true> : fa_mla_index_prepare_append_kernel<T, U, false, false>))

}  // namespace

hipError_t launch_mla_index_prepare_queries(const MlaIndexPrepareQParams& p, int dtype, bool hadamard, bool ue8m0, hipStream_t s) {
    if (dtype == 0) return prep_launch(FA_PREP_PICK2(fa_mla_index_prepare_queries_kernel, _Float16, hadamard, ue8m0), p, s);
    return prep_launch(FA_PREP_PICK2(fa_mla_index_prepare_queries_kernel, __bf16, hadamard, ue8m0), p, s);
}

hipError_t launch_mla_index_prepare_append(const MlaCacheIoParams& p, int dtype, bool ue8m0, hipStream_t s) {
    const bool paged = p.block_table != nullptr, packed = p.cu != nullptr;
    if (dtype == 0) return ue8m0 ? prep_launch(FA_PREP_PICK_IO(_Float16, true), p, s) : prep_launch(FA_PREP_PICK_IO(_Float16, false), p, s);
    return ue8m0 ? prep_launch(FA_PREP_PICK_IO(__bf16, true), p, s) : prep_launch(FA_PREP_PICK_IO(__bf16, false), p, s);
}

}  // namespace fa
