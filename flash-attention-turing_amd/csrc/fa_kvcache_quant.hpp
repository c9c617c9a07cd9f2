// fa_kvcache_quant.hpp — the quantiser of the append into an 8-bit (e4m3) KV cache, shared by the append kernels of fa_fwd_kvcache.hip and
// the fused rotary append of fa_kvcache_rotary.hip (one definition: the two must give the same codes for the same row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.hpp"

namespace fa {

namespace {

// One 16-bit element of k_new / v_new -> its e4m3 code under the (batch, KV head) descale: e4m3_rne(clamp(x / descale, -448, 448)).  The
// quotient is the correctly rounded fp32 one (no fast-math), the clamp is explicit so that nothing depends on the conversion's saturation
// mode, +-inf saturate with it; NaN keeps its sign and becomes 0x7f / 0xff.
template <typename T>
FA_DEV uint32_t quant_pair_e4m3(uint32_t w, float descale, uint32_t old, bool high) {
    float x[2];
    if constexpr (__is_same(T, _Float16)) {
        x[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
        x[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    } else {
        x[0] = __builtin_bit_cast(float, w << 16);
        x[1] = __builtin_bit_cast(float, w & 0xffff0000u);
    }
    float y[2];
    static_for<0, 2>([&](auto ee) {
        constexpr int e = decltype(ee)::value;
        const float qv = x[e] / descale;
        y[e] = __builtin_isnan(qv) ? qv : fminf(fmaxf(qv, -448.f), 448.f);
    });
    uint32_t r = high ? (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], (int)old, true)
                      : (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], (int)old, false);
    const int sh = high ? 16 : 0;
    static_for<0, 2>([&](auto ee) {
        constexpr int e = decltype(ee)::value;
        if (__builtin_isnan(y[e])) {
            const uint32_t code = 0x7fu | ((__builtin_bit_cast(uint32_t, x[e]) >> 24) & 0x80u);
            r = (r & ~(0xffu << (sh + 8 * e))) | (code << (sh + 8 * e));
        }
    });
    return r;
}

template <typename T>
FA_DEV u32x2 quant8_e4m3(u32x4 x, float descale) {
    u32x2 r;
    r.x = quant_pair_e4m3<T>(x.x, descale, 0u, false);
    r.x = quant_pair_e4m3<T>(x.y, descale, r.x, true);
    r.y = quant_pair_e4m3<T>(x.z, descale, 0u, false);
    r.y = quant_pair_e4m3<T>(x.w, descale, r.y, true);
    return r;
}

}  // namespace

}  // namespace fa
