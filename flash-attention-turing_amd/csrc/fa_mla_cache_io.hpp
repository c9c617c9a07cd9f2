// fa_mla_cache_io.hpp — kernel parameters and launchers of the stand-alone row movers of the MLA caches (fa_mla_cache_io.hip): append to the latent cache,
// gather from it, append to the index-key cache.  Filled and validated by fa_capi.hip (fa_run_mla_cache_append / _gather / fa_run_mla_index_cache_append).
// A block of its own: no other kernel's kernarg segment changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.hpp"

namespace fa {

constexpr int kCacheIoThreads = 256;    // four waves; a wave owns one latent row, 16 lanes one index-key row

// One struct for the three calls; every stride is in BYTES (the C ABI's element strides are scaled where it is filled).
struct MlaCacheIoParams {
    void* cache;                    // the latent cache / the index-key cache (append: written; gather: read)
    const void* src;                // append: the new rows (latent: columns 0 .. 511 of a row are read from here)
    const void* src_pe;             // latent append: columns 512 .. 575 of new row (i, s), with strides of their own (k_pe, or kv_new + 512 elements)
    void* out;                      // gather: the caller's rows
    float* k_scale;                 // index append into an FP8 cache: one fp32 per cached token
    const int32_t* cache_seqlens;   // gather: NULL = the capacity
    const int32_t* block_table;     // NULL = contiguous
    const int32_t* cu;              // NULL = dense (b, n, ..) rows; else packed rows with cu[i] .. cu[i + 1] those of sequence i
    const int32_t* seq_starts;      // gather: NULL = 0
    int64_t c_batch, c_row;         // cache: batch / page and row
    int64_t s_batch, s_row;         // src (packed: s_batch unused)
    int64_t pe_batch, pe_row;       // src_pe
    int64_t o_batch, o_row;         // out (packed: o_batch unused)
    int64_t ks_batch, ks_row;       // k_scale, in ELEMENTS (any value)
    int64_t bt_stride;              // block_table rows, in elements
    int64_t total;                  // rows of the grid: b * n (dense) or the packed tensor's rows
    int b, n, seqlen_cache, page_size, num_blocks;
};

// ---- where a row of the grid lives: shared by fa_mla_cache_io.hip and fa_mla_index_prepare.hip (device code; one definition of placement, drop and clamp)
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

}  // namespace

// p.total > 0 and every field checked by the caller.  fp8: the 656-byte row format / e4m3 index keys.
hipError_t launch_mla_cache_append(const MlaCacheIoParams& p, int dtype, bool fp8, hipStream_t stream);
hipError_t launch_mla_cache_gather(const MlaCacheIoParams& p, int dtype, bool fp8, hipStream_t stream);
// mode: 0 = copy into a 16-bit cache, 1 = quantise with fp32 scales, 2 = quantise with scales rounded up to powers of two (UE8M0)
hipError_t launch_mla_index_cache_append(const MlaCacheIoParams& p, int dtype, int mode, hipStream_t stream);

}  // namespace fa
