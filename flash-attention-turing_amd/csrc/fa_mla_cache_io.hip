// fa_mla_cache_io.hip — stand-alone row movers of the MLA caches: append to the latent cache, gather from it, append to the index-key cache
// (fa_run_mla_cache_append / fa_run_mla_cache_gather / fa_run_mla_index_cache_append).  Memory-bound, bit-exact, no LDS, no MFMA.
//
//   * Rows.  A dense call has b x n rows, row r = (sequence r / n, row r % n); a packed call has p.total rows and finds the sequence of row r by bisection over
//     cu (as fa_kvcache_append_ragged_kernel does): the grid is sized from the packed tensor, rows at or past cu[b] or in front of cu[0] belong to nobody.
//   * Placement (both appends): new row t of sequence i goes to logical row max(cache_seqlens[i], 0) + t, dropped at or past the capacity; PAGED: row (.) %
//     page_size of page min((uint32_t)block_table[i][(.) / page_size], num_blocks - 1) - the rules of fa_kvcache_mla_append_kernel.  Whatever the table or the
//     lengths hold, a write lands inside the cache / the pool.
//   * Latent append: one wave per row.  16-bit cache: the 72 16-byte slots are copied (slots 64 .. 71 from src_pe, which is k_pe or the row's own rope part).
//     FP8 cache: the wave of fa_kvcache_mla_append_fp8_kernel - lane l holds columns 8 l .. 8 l + 7, the 16 lanes of a tile take amax over their finite
//     elements by cross-lane max, scale = max(amax, 2^-24) / 448, codes by quant8_e4m3 (fa_kvcache_quant.hpp), the rope part copied.
//   * Gather: one wave per output row.  Logical row max(seq_starts[i], 0) + t of sequence i; at or past L_i = min(max(cache_seqlens[i], 0), capacity) the
//     output row is +0 and neither the table nor the cache is read.  16-bit cache: 72 slots copied.  FP8 cache: lane l reads its eight codes and the scale of
//     their tile and writes slot l through dequant8 (fa_kvcache_mla_attn.hpp) - the bytes the attention kernels put into their LDS image; lanes 0 .. 7 copy
//     the rope slots.
//   * Index append: 16 lanes per 128-wide row, 16 rows a workgroup.  Copy, or the quantiser above with one tile per row; the scale goes to k_scale as it is
//     or rounded up to a power of two on its bits (UE8M0): (bits + 0x007fffff) & 0x7f800000.
//   Offsets are 64-bit throughout.  Kernels of this file: 12 latent append ((16-bit; FP8 fp16; FP8 bf16) x (contiguous, paged) x (dense, packed)), 12 gather
//   (likewise), 20 index append ((copy; fp32 scale and UE8M0 scale for fp16 and bf16) x (contiguous, paged) x (dense, packed)).
#include "fa_mla_cache_io.hpp"

#include "fa_kvcache_mla_attn.hpp"
#include "fa_kvcache_quant.hpp"

namespace fa {

namespace {

// row r of the grid -> (sequence, row within the sequence); false: the row belongs to nobody
template <bool PACKED>
FA_DEV bool io_locate(const MlaCacheIoParams& p, int64_t r, int& bidx, int64_t& t) {
    if constexpr (PACKED) {
        int lo = 0, hi = p.b;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.cu[mid] <= r) lo = mid;
            else hi = mid - 1;
        }
        if (lo >= p.b) return false;        // a surplus row past cu[b]
        bidx = lo;
        t = r - p.cu[lo];
        return t >= 0;                      // (cu[0] > 0: rows in front of the first sequence)
    } else {
        bidx = (int)(r / p.n);
        t = r % p.n;
        return true;
    }
}

// logical row `row` < seqlen_cache of sequence bidx -> (batch entry or page, row within it)
template <bool PAGED>
FA_DEV void io_place(const MlaCacheIoParams& p, int bidx, int64_t row, int64_t& blk, int64_t& prow) {
    blk = bidx;
    prow = row;
    if constexpr (PAGED) {
        const int64_t col = row / p.page_size;
        prow = row - col * p.page_size;
        blk = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
    }
}

// where new row t of sequence bidx goes; false: dropped
template <bool PAGED>
FA_DEV bool io_append_place(const MlaCacheIoParams& p, int bidx, int64_t t, int64_t& blk, int64_t& prow) {
    const int cs = p.cache_seqlens[bidx];
    const int64_t row = (int64_t)(cs > 0 ? cs : 0) + t;
    if (row >= p.seqlen_cache) return false;
    io_place<PAGED>(p, bidx, row, blk, prow);
    return true;
}

// amax over the finite elements of eight 16-bit values (NaN and +-inf skipped: |bits| below the first non-finite pattern), exact in fp32
template <typename T>
FA_DEV float io_amax8(u32x4 x) {
    float amax = 0.f;
    static_for<0, 8>([&](auto ee) {
        constexpr int e = decltype(ee)::value;
        const uint16_t bits = (uint16_t)((x[e >> 1] >> (16 * (e & 1))) & 0x7fffu);
        const bool finite = bits < (__is_same(T, _Float16) ? 0x7c00u : 0x7f80u);
        amax = fmaxf(amax, finite ? LP<T>::to_float(bits) : 0.f);
    });
    return amax;
}

// max over the 16 lanes of a tile
FA_DEV float io_max16(float v) {
    static_for<0, 4>([&](auto ss) { v = fmaxf(v, __shfl_xor(v, 1 << decltype(ss)::value, 64)); });
    return v;
}

template <typename T, bool FP8, bool PAGED, bool PACKED>
__global__ __launch_bounds__(kCacheIoThreads) void fa_mla_cache_append_kernel(const MlaCacheIoParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.total) return;
    int bidx;
    int64_t t, blk, prow;
    if (!io_locate<PACKED>(p, r, bidx, t)) return;
    if (!io_append_place<PAGED>(p, bidx, t, blk, prow)) return;
    const char* src = (const char*)p.src + (PACKED ? r * p.s_row : (int64_t)bidx * p.s_batch + t * p.s_row);
    const char* pe = (const char*)p.src_pe + (PACKED ? r * p.pe_row : (int64_t)bidx * p.pe_batch + t * p.pe_row);
    char* dst = (char*)p.cache + blk * p.c_batch + prow * p.c_row;
    const u32x4 x = *(const u32x4*)(src + 16 * lane);
    if constexpr (FP8) {
        const float scale = fmaxf(io_max16(io_amax8<T>(x)), 0x1p-24f) / 448.f;
        *(u32x2*)(dst + 8 * lane) = quant8_e4m3<T>(x, scale);
        if ((lane & 15) == 0) *(float*)(dst + MlaRows8::kScales + 4 * (lane >> 4)) = scale;
        if (lane < 2 * kMlaDR / 16) *(u32x4*)(dst + MlaRows8::kRope + 16 * lane) = *(const u32x4*)(pe + 16 * lane);
    } else {
        *(u32x4*)(dst + 16 * lane) = x;
        if (lane < 2 * kMlaDR / 16) *(u32x4*)(dst + 2 * kMlaDV + 16 * lane) = *(const u32x4*)(pe + 16 * lane);
    }
}

template <typename T, bool FP8, bool PAGED, bool PACKED>
__global__ __launch_bounds__(kCacheIoThreads) void fa_mla_cache_gather_kernel(const MlaCacheIoParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.total) return;
    int bidx;
    int64_t t;
    if (!io_locate<PACKED>(p, r, bidx, t)) return;
    char* dst = (char*)p.out + (PACKED ? r * p.o_row : (int64_t)bidx * p.o_batch + t * p.o_row);
    const int st = p.seq_starts != nullptr ? p.seq_starts[bidx] : 0;
    const int cs = p.cache_seqlens != nullptr ? p.cache_seqlens[bidx] : p.seqlen_cache;
    const int L = min(cs > 0 ? cs : 0, p.seqlen_cache);
    const int64_t pos = (int64_t)(st > 0 ? st : 0) + t;
    u32x4 v = u32x4{0u, 0u, 0u, 0u}, rope = v;
    if (pos < L) {
        int64_t blk, prow;
        io_place<PAGED>(p, bidx, pos, blk, prow);
        const char* src = (const char*)p.cache + blk * p.c_batch + prow * p.c_row;
        if constexpr (FP8) {
            const u32x2 c = *(const u32x2*)(src + 8 * lane);
            const float s = *(const float*)(src + MlaRows8::kScales + 4 * (lane >> 4));
            v = dequant8<T>(c.x, c.y, s);
            if (lane < 2 * kMlaDR / 16) rope = *(const u32x4*)(src + MlaRows8::kRope + 16 * lane);
        } else {
            v = *(const u32x4*)(src + 16 * lane);
            if (lane < 2 * kMlaDR / 16) rope = *(const u32x4*)(src + 2 * kMlaDV + 16 * lane);
        }
    }
    *(u32x4*)(dst + 16 * lane) = v;
    if (lane < 2 * kMlaDR / 16) *(u32x4*)(dst + 2 * kMlaDV + 16 * lane) = rope;
}

// MODE 0: copy; 1: quantise, fp32 scale; 2: quantise, the scale rounded up to a power of two
template <typename T, int MODE, bool PAGED, bool PACKED>
__global__ __launch_bounds__(kCacheIoThreads) void fa_mla_index_cache_append_kernel(const MlaCacheIoParams p) {
    const int l = threadIdx.x & 15;
    const int64_t r = (int64_t)blockIdx.x * (kCacheIoThreads / 16) + (threadIdx.x >> 4);
    if (r >= p.total) return;
    int bidx;
    int64_t t, blk, prow;
    if (!io_locate<PACKED>(p, r, bidx, t)) return;
    if (!io_append_place<PAGED>(p, bidx, t, blk, prow)) return;
    const char* src = (const char*)p.src + (PACKED ? r * p.s_row : (int64_t)bidx * p.s_batch + t * p.s_row);
    char* dst = (char*)p.cache + blk * p.c_batch + prow * p.c_row;
    const u32x4 x = *(const u32x4*)(src + 16 * l);
    if constexpr (MODE == 0) {
        *(u32x4*)(dst + 16 * l) = x;
    } else {
        // (the 16 lanes of a row took the same branches: the cross-lane max reads live lanes only)
        float scale = fmaxf(io_max16(io_amax8<T>(x)), 0x1p-24f) / 448.f;
        if constexpr (MODE == 2) scale = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, scale) + 0x007fffffu) & 0x7f800000u);
        *(u32x2*)(dst + 8 * l) = quant8_e4m3<T>(x, scale);
        if (l == 0) p.k_scale[blk * p.ks_batch + prow * p.ks_row] = scale;
    }
}

// kernel<T, A, PAGED, PACKED> chosen by the two run-time layout flags
#define FA_IO_PICK(KERNEL, T, A) \
    (paged ? (packed ? KERNEL<T, A, true, true> : KERNEL<T, A, true, false>) : (packed ? KERNEL<T, A, false, true> : KERNEL<T, A, false, false>))

template <typename K>
hipError_t io_launch(K* kernel, const MlaCacheIoParams& p, int rows_per_wg, hipStream_t s) {
    const int64_t grid = (p.total + rows_per_wg - 1) / rows_per_wg;
    if (grid <= 0 || grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kCacheIoThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mla_cache_append(const MlaCacheIoParams& p, int dtype, bool fp8, hipStream_t s) {
    const bool paged = p.block_table != nullptr, packed = p.cu != nullptr;
    if (!fp8) return io_launch(FA_IO_PICK(fa_mla_cache_append_kernel, _Float16, false), p, 4, s);      // (a copy: the element type does not matter)
    if (dtype == 0) return io_launch(FA_IO_PICK(fa_mla_cache_append_kernel, _Float16, true), p, 4, s);
    return io_launch(FA_IO_PICK(fa_mla_cache_append_kernel, __bf16, true), p, 4, s);
}

hipError_t launch_mla_cache_gather(const MlaCacheIoParams& p, int dtype, bool fp8, hipStream_t s) {
    const bool paged = p.block_table != nullptr, packed = p.cu != nullptr;
    if (!fp8) return io_launch(FA_IO_PICK(fa_mla_cache_gather_kernel, _Float16, false), p, 4, s);
    if (dtype == 0) return io_launch(FA_IO_PICK(fa_mla_cache_gather_kernel, _Float16, true), p, 4, s);
    return io_launch(FA_IO_PICK(fa_mla_cache_gather_kernel, __bf16, true), p, 4, s);
}

hipError_t launch_mla_index_cache_append(const MlaCacheIoParams& p, int dtype, int mode, hipStream_t s) {
    const bool paged = p.block_table != nullptr, packed = p.cu != nullptr;
    constexpr int R = kCacheIoThreads / 16;
    if (mode == 0) return io_launch(FA_IO_PICK(fa_mla_index_cache_append_kernel, _Float16, 0), p, R, s);
    if (mode == 1) return dtype == 0 ? io_launch(FA_IO_PICK(fa_mla_index_cache_append_kernel, _Float16, 1), p, R, s)
                                     : io_launch(FA_IO_PICK(fa_mla_index_cache_append_kernel, __bf16, 1), p, R, s);
    if (mode == 2) return dtype == 0 ? io_launch(FA_IO_PICK(fa_mla_index_cache_append_kernel, _Float16, 2), p, R, s)
                                     : io_launch(FA_IO_PICK(fa_mla_index_cache_append_kernel, __bf16, 2), p, R, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
