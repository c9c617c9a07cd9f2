// fa_mla_index_prepare.hpp — kernel parameters and launchers of the indexer's front end (fa_mla_index_prepare.hip): the 128-point Hadamard rotation of index
// queries and index keys, their e4m3 quantiser, and the placement of the keys into the index-key cache.  Filled and validated by fa_capi.hip
// (fa_run_mla_index_prepare_queries / fa_run_mla_index_prepare_append).  A block of its own: no other kernel's kernarg segment changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_mla_cache_io.hpp"

namespace fa {

constexpr int kIdxPrepThreads = 256;    // four waves; a wave owns 16 rows of 128
constexpr int kIdxPrepRows = 64;        // rows of a workgroup

// Query rows: row r = token r / heads, head r % heads.  q strides in BYTES, weights strides in elements; codes and w8 are contiguous.
struct MlaIndexPrepareQParams {
    const void* q;          // (tokens, heads, 128) of the 16-bit dtype
    const float* weights;   // (tokens, heads)
    void* codes;            // uint8 (tokens, heads, 128)
    float* w8;              // (tokens, heads): weights * scale
    int64_t q_token, q_head;
    int64_t w_token, w_head;
    int64_t total;          // tokens * heads, below 2^31
    int heads;
};

// p.total > 0 and every field checked by the caller.
hipError_t launch_mla_index_prepare_queries(const MlaIndexPrepareQParams& p, int dtype, bool hadamard, bool ue8m0, hipStream_t stream);
// The fields of launch_mla_index_cache_append over an FP8 cache (p.k_scale set): rows are rotated, quantised and placed.
hipError_t launch_mla_index_prepare_append(const MlaCacheIoParams& p, int dtype, bool ue8m0, hipStream_t stream);

}  // namespace fa
