// fa_merge_states.hpp — kernel parameters and launcher of the attention-state merge (fa_merge_states.hip): N partial results (o_i, lse_i) of the same query
// rows, each with strides of its own, into one (out, lse).  Filled and validated by fa_capi.hip (fa_run_merge_states).  A block of its own: no other
// kernel's kernarg segment changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

constexpr int kMergeMaxParts = 8;       // parts of one call (FA_MERGE_MAX_PARTS of the header)
constexpr int kMergeThreads = 256;      // four waves; a group of d_v / 8 lanes owns one (row, head)

struct MergeStatesParams {
    const void* o_ptr[kMergeMaxParts];          // (b, rows, h, d_v) of the call's dtype, last dimension contiguous
    const float* lse_ptr[kMergeMaxParts];       // fp32, addressed (batch, head, row)
    int64_t o_batch[kMergeMaxParts], o_row[kMergeMaxParts], o_head[kMergeMaxParts];     // elements
    int64_t l_batch[kMergeMaxParts], l_head[kMergeMaxParts], l_row[kMergeMaxParts];     // elements
    void* out_ptr;
    float* lse_out_ptr;
    int64_t out_batch, out_row, out_head;
    int64_t lo_batch, lo_head, lo_row;
    int64_t total;                              // b * rows * h: the (row, head) pairs of the call
    int n_parts, rows, h;
};

// total > 0, 2 <= n_parts <= kMergeMaxParts, d_v in {64, 128, 256, 512}: checked by the caller
hipError_t launch_merge_states(const MergeStatesParams& p, int dtype, int d_v, hipStream_t stream);

}  // namespace fa
