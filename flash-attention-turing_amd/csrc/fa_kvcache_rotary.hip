// fa_kvcache_rotary.hip — rotary embedding fused into the append of a decode call: the kernels of fa_kvcache_rotary.hpp at head_dim 64 / 128 (the
// head_dim-256 instantiations are in fa_fwd_kvcache_d256.hip, with every other kernel of such a call).
#include "fa_kvcache_rotary.hpp"

namespace fa {

int64_t kvcache_rotary_image_bytes(const KvcacheKernelParams& kp) {
    return ((int64_t)kp.b * kp.seqlen_q * kp.h * kp.d * 2 + 15) / 16 * 16;
}

hipError_t launch_kvcache_rotary(const KvcacheRotaryParams& rp, int dtype, hipStream_t s) {
    if (rp.kp.d == 256) return launch_kvcache_rotary_d256(rp, dtype, s);
    return launch_rotary<64, 128>(rp, dtype, s);
}

}  // namespace fa
