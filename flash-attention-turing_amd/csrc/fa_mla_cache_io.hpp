// fa_mla_cache_io.hpp — kernel parameters and launchers of the stand-alone row movers of the MLA caches (fa_mla_cache_io.hip): append to the latent cache,
// gather from it, append to the index-key cache.  Filled and validated by fa_capi.hip (fa_run_mla_cache_append / _gather / fa_run_mla_index_cache_append).
// A block of its own: no other kernel's kernarg segment changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// p.total > 0 and every field checked by the caller.  fp8: the 656-byte row format / e4m3 index keys.
hipError_t launch_mla_cache_append(const MlaCacheIoParams& p, int dtype, bool fp8, hipStream_t stream);
hipError_t launch_mla_cache_gather(const MlaCacheIoParams& p, int dtype, bool fp8, hipStream_t stream);
// mode: 0 = copy into a 16-bit cache, 1 = quantise with fp32 scales, 2 = quantise with scales rounded up to powers of two (UE8M0)
hipError_t launch_mla_index_cache_append(const MlaCacheIoParams& p, int dtype, int mode, hipStream_t stream);

}  // namespace fa
