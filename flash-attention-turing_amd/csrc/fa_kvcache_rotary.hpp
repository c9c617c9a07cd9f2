// fa_kvcache_rotary.hpp — rotary embedding fused into the append of a decode call (fa_kvcache_options_v3, KvcacheRotaryParams).
//
// When a call carries rotary_cos / rotary_sin, ONE launch of the kernel below takes the place of the append launch (fa_kvcache_launch.hpp).
// In one grid it
//   (a) rotates the k_new rows and writes them to the cache - contiguous or through the block table (same clamp of a table entry to the
//       pool, same "rows at or past the capacity are dropped" rule as the append kernels), 16-bit or quantised to e4m3 with the append's
//       quantiser (fa_kvcache_quant.hpp) applied to the rotated row AFTER it was rounded to q's dtype;
//   (b) copies / quantises the v_new rows, exactly as the append does;
//   (c) writes the rotated q into a contiguous (b, seqlen_q, h, d) image at the head of the workspace, which the attention kernels then
//       read as their q.  The attention, append and combine kernels are untouched: the call equals, bit for bit, the call without rotary on
//       pre-rotated q and k_new.
// Positions: appended row s of sequence i sits at max(cache_seqlens[i], 0) + s (its cache row); query row t at max(cache_seqlens[i], 0) + t
// when the call is causal or windowed, else every query row at max(cache_seqlens[i], 0) (upstream flash-attn's rule).  A position is
// clamped to seqlen_ro - 1, so no value of cache_seqlens reads outside the tables.
// Rotation of a row x at position p, c = cos[p, i], s = sin[p, i], i < rotary_dim / 2: the pair (a, b) is (x[i], x[i + rotary_dim / 2])
// (GPT-NeoX) or (x[2 i], x[2 i + 1]) (interleaved, GPT-J); y_a = x_a c - x_b s, y_b = x_b c + x_a s in fp32 with every operation rounded
// on its own (contraction is switched off below; for fp16, and for bf16 away from fp32's exponent limits, the products are exact and it
// could not matter anyway), then ONE rounding to nearest even into q's dtype.  Elements rotary_dim .. d - 1 pass through.
// A thread owns one 8-element (16-byte) chunk of one output row: it loads its chunk, the partner chunk (rotary_dim / 2 is a multiple of 8,
// so the partner of an aligned chunk is an aligned chunk; interleaved pairs sit inside the chunk) and the 8 (interleaved: 4) cos and sin
// values of its position, all with 16-byte (8-byte) accesses, and stores 16 bytes (8 into an e4m3 cache).
#pragma once
#include "fa_kvcache_launch.hpp"

namespace fa {

namespace {

template <typename T>
FA_DEV void unpack8(u32x4 w, float (&x)[8]) {
    static_for<0, 4>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        x[2 * j] = LP<T>::to_float((uint16_t)(w[j] & 0xffffu));
        x[2 * j + 1] = LP<T>::to_float((uint16_t)(w[j] >> 16));
    });
}

// y = x * c + sign * (xp * s), element by element; sign = -1 for the first element of a pair, +1 for the second
template <typename T>
FA_DEV u32x4 rotate8(const float (&x)[8], const float (&xp)[8], const float (&c)[8], const float (&s)[8], const bool (&second)[8]) {
#pragma clang fp contract(off)
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = x[j] * c[j], b = xp[j] * s[j];
        y[j] = second[j] ? a + b : a - b;
    }
    return u32x4{LP<T>::pack2(y[0], y[1]), LP<T>::pack2(y[2], y[3]), LP<T>::pack2(y[4], y[5]), LP<T>::pack2(y[6], y[7])};
}

template <typename T, int D, bool PAGED, bool FP8>
__global__ __launch_bounds__(256) void fa_kvcache_rotary_kernel(const KvcacheRotaryParams rp) {
    const KvcacheKernelParams& p = rp.kp;
    constexpr int SLOTS = D / 8;
    constexpr int ES = FP8 ? 1 : 2;
    const int64_t kv_rows = (int64_t)p.seqlen_new * p.h_k, q_rows = (int64_t)p.seqlen_q * p.h;
    const int64_t rows_b = 2 * kv_rows + q_rows;            // per batch entry: the k_new rows, the v_new rows, the q rows
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.b * rows_b * SLOTS) return;
    const int slot = (int)(i % SLOTS);
    const int64_t r = i / SLOTS;
    const int bidx = (int)(r / rows_b);
    int64_t rr = r - (int64_t)bidx * rows_b;
    const int cs = p.cache_seqlens[bidx];
    const int64_t first_row = cs > 0 ? cs : 0;

    const char* src;        // this thread's source row
    char* dst;              // ... and destination row (bytes; an e4m3 cache row when dst_fp8)
    int64_t pos;
    bool is_v = false, dst_fp8 = false;
    float descale = 1.f;
    if (rr >= 2 * kv_rows) {                                // a query row -> the image
        rr -= 2 * kv_rows;
        const int t = (int)(rr / p.h), hq = (int)(rr - (int64_t)t * p.h);
        src = (const char*)p.q_ptr + 2 * ((int64_t)bidx * p.q.batch + (int64_t)t * p.q.row + (int64_t)hq * p.q.head);
        dst = (char*)rp.q_image + 2 * ((((int64_t)bidx * p.seqlen_q + t) * p.h + hq) * D);
        pos = first_row + (rp.q_pos_per_row ? t : 0);
    } else {                                                // a k_new / v_new row -> its cache row
        is_v = rr >= kv_rows;
        if (is_v) rr -= kv_rows;
        const int t = (int)(rr / p.h_k), kvh = (int)(rr - (int64_t)t * p.h_k);
        const int64_t row = first_row + t;
        if (row >= p.seqlen_cache) return;                  // dropped, like the append kernels drop it
        int64_t blk = bidx, prow = row;
        if constexpr (PAGED) {
            const int col = (int)(row / p.page_size);
            prow = row - (int64_t)col * p.page_size;
            blk = (int64_t)min((uint32_t)p.block_table[(int64_t)bidx * p.bt_stride + col], (uint32_t)(p.num_blocks - 1));
        }
        const TStride& sn = is_v ? p.vn : p.kn;
        const TStride& sc = is_v ? p.vc : p.kc;
        src = (const char*)(is_v ? p.v_new : p.k_new) + 2 * ((int64_t)bidx * sn.batch + (int64_t)t * sn.row + (int64_t)kvh * sn.head);
        dst = (char*)(is_v ? p.v_cache : p.k_cache) + ES * (blk * sc.batch + prow * sc.row + (int64_t)kvh * sc.head);
        pos = row;
        if constexpr (FP8) {
            dst_fp8 = true;
            const float* ds = is_v ? p.v_descale : p.k_descale;
            if (ds != nullptr) descale = ds[(int64_t)bidx * (is_v ? p.vds_batch : p.kds_batch) + (int64_t)kvh * (is_v ? p.vds_head : p.kds_head)];
        }
    }

    u32x4 y = *(const u32x4*)(src + 16 * slot);
    if (!is_v && 8 * slot < rp.rotary_dim) {
        if (pos > rp.seqlen_ro - 1) pos = rp.seqlen_ro - 1;
        const char* crow = (const char*)rp.cos + 2 * pos * rp.row_stride;
        const char* srow = (const char*)rp.sin + 2 * pos * rp.row_stride;
        float x[8], xp[8], c[8], s[8];
        bool second[8];
        unpack8<T>(y, x);
        if (rp.interleaved) {
            const u32x2 cw = *(const u32x2*)(crow + 8 * slot), sw = *(const u32x2*)(srow + 8 * slot);
            static_for<0, 4>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                c[2 * j] = c[2 * j + 1] = LP<T>::to_float((uint16_t)((cw[j / 2] >> (16 * (j & 1))) & 0xffffu));
                s[2 * j] = s[2 * j + 1] = LP<T>::to_float((uint16_t)((sw[j / 2] >> (16 * (j & 1))) & 0xffffu));
                xp[2 * j] = x[2 * j + 1];
                xp[2 * j + 1] = x[2 * j];
                second[2 * j] = false;
                second[2 * j + 1] = true;
            });
        } else {
            const int half = rp.rotary_dim >> 1;
            const bool hi = 8 * slot >= half;
            const int i0 = hi ? 8 * slot - half : 8 * slot;         // the chunk's first index into the table row
            unpack8<T>(*(const u32x4*)(src + 2 * (hi ? i0 : i0 + half)), xp);
            unpack8<T>(*(const u32x4*)(crow + 2 * i0), c);
            unpack8<T>(*(const u32x4*)(srow + 2 * i0), s);
            static_for<0, 8>([&](auto jj) { second[decltype(jj)::value] = hi; });
        }
        y = rotate8<T>(x, xp, c, s, second);
    }
    if constexpr (FP8) {
        if (dst_fp8) {
            *(u32x2*)(dst + 8 * slot) = quant8_e4m3<T>(y, descale);
            return;
        }
    }
    *(u32x4*)(dst + 16 * slot) = y;
}

// the fused launch at a head_dim of the list
template <int... DS>
hipError_t launch_rotary(const KvcacheRotaryParams& rp, int dtype, hipStream_t s) {
    const KvcacheKernelParams& kp = rp.kp;
    kvc_dispatch<DS...>(kp, dtype, [&](auto leaf) {
        using K = decltype(leaf);
        const int64_t n = (int64_t)kp.b * (2 * (int64_t)kp.seqlen_new * kp.h_k + (int64_t)kp.seqlen_q * kp.h) * (K::D / 8);
        hipLaunchKernelGGL((fa_kvcache_rotary_kernel<typename K::T, K::D, K::PAGED, K::ES == 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rp);
    });
    return hipGetLastError();
}

}  // namespace

}  // namespace fa
