// fa_merge_states.hip — merge N partial attention states of the same query rows into one (fa_run_merge_states; vLLM's merge_attn_states, FlashInfer's
// merge_state): out = sum_i w_i o_i / sum_i w_i, lse = m + log(sum_i w_i) with m = max_i lse_i, w_i = exp(lse_i - m), in fp32 over the NON-EMPTY parts
// of a (row, head), parts taken in argument order, one rounding to the dtype.
//
// EMPTY (the rule of the whole library, include/flash_attn_gfx950.h): part i is empty for a (row, head) iff lse_i is -inf, or lse_i is +-0 and every element
// of that o_i row is +-0 - what every attention call here returns for a row that sees no key.  An empty part contributes nothing and is left out of m; all
// parts empty is out = 0, lse = 0, the dead row again, so a merged state can feed another merge.  A NaN lse_i, or a NaN in a non-empty part's row, makes
// the whole (row, head) NaN, out and lse, and no other.
//
// Memory-bound streaming, no LDS, no scratch, no atomics, no workspace: a group of d_v / 8 lanes owns one (row, head); a lane issues the lse load and the one
// 16-byte load of every part before it uses any of them, and writes one 16-byte store.  (row, head) pairs run (batch, row, head) so that the lanes of a wave
// read consecutive 16-byte pieces of a contiguous o_i.  The row-wide zero test and the row-wide NaN test are ballots cut to the lane group; the zero test is
// skipped unless some lse_i of the wave is +-0.  Lane groups at or past b * rows * h leave before the first load: nothing there is read or written.
// Two bodies per (dtype, d_v): two parts (the chunked-prefill and shared-prefix merges), and up to kMergeMaxParts with the part count a runtime bound on a
// fully unrolled loop, so the loads of every part still stand in front of the first use.
#include "fa_device.hpp"
#include "fa_merge_states.hpp"

namespace fa {

namespace {

template <typename T, int DV, bool TWO>
__global__ __launch_bounds__(kMergeThreads) void fa_merge_states_kernel(const MergeStatesParams p) {
    constexpr int TPR = DV / 8;                              // lanes per (row, head), 8 columns each
    constexpr int NMAX = TWO ? 2 : kMergeMaxParts;
    static_assert(TPR >= 8 && TPR <= 64 && (TPR & (TPR - 1)) == 0, "a lane group is a power of two of lanes inside one wave");
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)blockIdx.x * (kMergeThreads / TPR) + tid / TPR;
    if (R >= p.total) return;                                // (whole lane groups leave: the ballots below see the lanes that stay)
    const int col = (tid % TPR) * 8;
    const int n = TWO ? 2 : p.n_parts;
    const int hq = (int)(R % p.h);
    const int64_t br = R / p.h;
    const int64_t t = br % p.rows, bidx = br / p.rows;

    float ls[NMAX];
    u32x4 x[NMAX];
    static_for<0, NMAX>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        ls[i] = -INFINITY;                                   // parts past n are empty
        x[i] = u32x4{0u, 0u, 0u, 0u};
        if (i < n) {
            ls[i] = p.lse_ptr[i][bidx * p.l_batch[i] + (int64_t)hq * p.l_head[i] + t * p.l_row[i]];
            x[i] = *(const u32x4*)((const char*)p.o_ptr[i] + 2 * (bidx * p.o_batch[i] + t * p.o_row[i] + (int64_t)hq * p.o_head[i] + col));
        }
    });

    const int group_shift = (tid & 63) & ~(TPR - 1);         // first lane of this lane group within its wave
    auto group_any = [&](bool flag) -> bool {
        const uint64_t all = __ballot(flag);
        if constexpr (TPR == 64) return all != 0;
        else return ((all >> group_shift) & ((1ull << TPR) - 1)) != 0;
    };

    float M = -INFINITY;
    bool nan_part = false;
    bool empty[NMAX];
    static_for<0, NMAX>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        empty[i] = true;
        if (i < n) {
            const bool zero_lse = ls[i] == 0.f;              // +-0
            bool e = ls[i] == -INFINITY;
            if (__ballot(zero_lse) != 0) {                   // wave-uniform: some (row, head) of the wave may be the library's dead row
                const bool nonzero = ((x[i][0] | x[i][1] | x[i][2] | x[i][3]) & 0x7FFF7FFFu) != 0;
                e = e || (zero_lse && !group_any(nonzero));
            }
            empty[i] = e;
            nan_part |= __builtin_isnan(ls[i]);
            if (!e) M = fmaxf(M, ls[i]);                     // (fmaxf drops a NaN: tracked on the side, as in the combine kernels)
        }
    });

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float sum = 0.f;
    static_for<0, NMAX>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        if (i < n && !empty[i]) {
            const float w = __expf(ls[i] - M);
            sum += w;
            static_for<0, 4>([&](auto ee) {
                constexpr int e = decltype(ee)::value;
                acc[2 * e] += w * LP<T>::to_float((uint16_t)(x[i][e] & 0xFFFFu));
                acc[2 * e + 1] += w * LP<T>::to_float((uint16_t)(x[i][e] >> 16));
            });
        }
    });

    bool nan_lane = false;
    static_for<0, 8>([&](auto ee) { nan_lane |= __builtin_isnan(acc[decltype(ee)::value]); });
    const bool nan_row = group_any(nan_lane) || nan_part;
    const bool live = !(sum == 0.f);
    const float inv = nan_row ? __builtin_nanf("") : (live ? 1.0f / sum : 0.f);
    char* orow = (char*)p.out_ptr + 2 * (bidx * p.out_batch + t * p.out_row + (int64_t)hq * p.out_head + col);
    u32x4 y;
    if (nan_row) {
        const uint32_t q = LP<T>::pack2(inv, inv);
        y = u32x4{q, q, q, q};
    } else {
        y = u32x4{LP<T>::pack2(acc[0] * inv, acc[1] * inv), LP<T>::pack2(acc[2] * inv, acc[3] * inv),
                  LP<T>::pack2(acc[4] * inv, acc[5] * inv), LP<T>::pack2(acc[6] * inv, acc[7] * inv)};
    }
    *(u32x4*)orow = y;
    if (tid % TPR == 0) p.lse_out_ptr[bidx * p.lo_batch + (int64_t)hq * p.lo_head + t * p.lo_row] = nan_row ? inv : (live ? M + logf(sum) : 0.f);
}

template <typename T, int DV>
void launch_dv(const MergeStatesParams& p, unsigned grid, hipStream_t stream) {
    if (p.n_parts == 2) hipLaunchKernelGGL((fa_merge_states_kernel<T, DV, true>), dim3(grid), dim3(kMergeThreads), 0, stream, p);
    else hipLaunchKernelGGL((fa_merge_states_kernel<T, DV, false>), dim3(grid), dim3(kMergeThreads), 0, stream, p);
}

template <typename T>
hipError_t launch_t(const MergeStatesParams& p, int d_v, unsigned grid, hipStream_t stream) {
    switch (d_v) {
        case 64: launch_dv<T, 64>(p, grid, stream); break;
        case 128: launch_dv<T, 128>(p, grid, stream); break;
        case 256: launch_dv<T, 256>(p, grid, stream); break;
        case 512: launch_dv<T, 512>(p, grid, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_merge_states(const MergeStatesParams& p, int dtype, int d_v, hipStream_t stream) {
    if (p.total <= 0 || p.n_parts < 2 || p.n_parts > kMergeMaxParts || p.rows <= 0 || p.h <= 0 || (d_v != 64 && d_v != 128 && d_v != 256 && d_v != 512))
        return hipErrorInvalidValue;
    const int64_t per_block = kMergeThreads / (d_v / 8);
    const int64_t grid = (p.total + per_block - 1) / per_block;
    if (grid >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    return dtype == 0 ? launch_t<_Float16>(p, d_v, (unsigned)grid, stream) : launch_t<__bf16>(p, d_v, (unsigned)grid, stream);
}

}  // namespace fa
