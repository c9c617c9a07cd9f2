// fa_fwd_fp8.hpp — kernel parameters and launcher of the FP8 (e4m3) dense attention forward (fa_fwd_fp8.hip, fa_run_fp8_fwd).  Filled and validated by
// fa_capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_params.hpp"

namespace fa {

// The fields MlapSeq (fa_mla_prefill_tile.hpp) reads carry MlaPrefillParams' names: the tile lookup, the packed bounds and the row addressing are that file's.
struct Fp8FwdParams {
    const void* q_ptr;          // e4m3 codes; dense (b, sq, h, 128) or packed (total_q, h, 128)
    const void* k_ptr;          // e4m3 codes; (b, sk, h_k, 128) or (total_k, h_k, 128)
    const void* v_ptr;
    void* o_ptr;                // fp16 / bf16, shaped like q
    float* lse_ptr;             // (b, h, sq) or (h, total_q)
    const float* qd_ptr;        // (b, h) fp32 descales, nullptr = 1.0
    const float* kd_ptr;        // (b, h_k)
    const float* vd_ptr;        // (b, h_k)
    const int32_t* cu_q;        // (b + 1,) or NULL = dense
    const int32_t* cu_k;
    TStride q, k, v, o;         // q / k / v in bytes (= codes), o in elements
    int64_t qd_batch, qd_head, kd_batch, kd_head, vd_batch, vd_head;    // elements
    int32_t b, seqlen_q, seqlen_k, h, h_k, h_ratio;
    int32_t is_causal;
    int32_t n_row_tiles;        // filled by the launcher (dense): row tiles of a (batch, KV head)
    int32_t slots;              // filled by the launcher (packed): tile slots per KV head, ceil(total_q * h_ratio / rows of a tile) + b
    int64_t total_q, total_k;   // packed: rows of q / o and of k / v
    float scale;                // softmax_scale; the descales are multiplied in on the device
};

// dtype: FA_FP16 / FA_BF16 of o
hipError_t launch_fwd_fp8(Fp8FwdParams p, int dtype, hipStream_t stream);

}  // namespace fa
