// fa_fwd_prefill.hpp — kernel parameters and launcher of the sliding-window prompt forward with attention sinks (fa_fwd_prefill.hip, fa_run_prefill_fwd).
// Filled and validated by fa_capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_params.hpp"

namespace fa {

// The fields MlapSeq (fa_mla_prefill_tile.hpp) reads carry MlaPrefillParams' names: the tile lookup, the packed bounds and the row addressing are that file's.
struct PrefillFwdParams {
    const void* q_ptr;          // fp16 / bf16; dense (b, sq, h, d) or packed (total_q, h, d)
    const void* k_ptr;          // (b, sk, h_k, d) or (total_k, h_k, d)
    const void* v_ptr;
    void* o_ptr;                // shaped like q
    float* lse_ptr;             // (b, h, sq) or (h, total_q)
    const void* sinks;          // one logit per query head, in the units of the final scores; nullptr = none (-inf)
    const int32_t* cu_q;        // (b + 1,) or NULL = dense
    const int32_t* cu_k;
    TStride q, k, v, o;         // elements
    int64_t sinks_stride;       // elements
    int32_t sinks_16bit;        // 0: fp32 logits, 1: logits in the dtype of q
    int32_t b, seqlen_q, seqlen_k, h, h_k, h_ratio;
    int32_t window_left, window_right;      // < 0: unbounded on that side (a causal call arrives as right = 0)
    int32_t n_row_tiles;        // filled by the launcher (dense): row tiles of a (batch, KV head)
    int32_t slots;              // filled by the launcher (packed): tile slots per KV head, ceil(total_q * h_ratio / rows of a tile) + b
    int64_t total_q, total_k;   // packed: rows of q / o and of k / v
    float scale, scale_log2e;
};

// dtype: FA_FP16 / FA_BF16; d: 64 or 128
hipError_t launch_fwd_prefill(PrefillFwdParams p, int dtype, int d, hipStream_t stream);

}  // namespace fa
