// fa_kvcache_stage.hpp — the one step of the register-staged, two-stage LDS schedule of the 64-row bodies (documented in fa_kvcache_stage_debug.hpp).
//
//   Stage n & 1 holds step n.  While step n computes, the loads of step n + 1 are in flight; they are written to the other stage behind the compute -
//   every wave left that stage's reads (step n - 1) in front of the last barrier - and ONE barrier publishes them.  The loads of step n + 2 are issued
//   behind that barrier, so nothing is outstanding when it is reached.  A body keeps its prologue (first fill of stage 0, a barrier, the loads of step 1)
//   and its `for` over pairs of steps; the step itself, with the test builds' hooks and the racy form, is written here and nowhere else.
#pragma once
#include "fa_kvcache_attn.hpp"
#include "fa_kvcache_stage_debug.hpp"

namespace fa {

// n: the step within the split (wave-uniform; the first fill of stage 0 is step -1), wave: 0 .. 3 (wave-uniform)
FA_DEV void kvc_stage_slow_reader(int n, int wave) {
#if FA_KVC_STAGE_DEBUG == 1
    if ((n & 3) == wave) asm volatile("s_sleep 64" ::: "memory");
#endif
}

FA_DEV void kvc_stage_slow_writer(int n, int wave) {
#if FA_KVC_STAGE_DEBUG == 2
    if (((n + 1) & 3) == wave) asm volatile("s_sleep 64" ::: "memory");
#endif
}

// The step at `pos` (begin <= pos < end, in keys or rows) over stage BUF: compute(bufc, pos) if the wave is active, then - if a step follows -
// store(BUF ^ 1) of the registers loaded for it, the barrier, and load(bufc, pos + 2 steps) into the registers just freed (its stage is BUF again).
// Why the racy form (the barrier in FRONT of the store) can neither hang nor fault, part (1), for every body: the barrier only changes places inside the
// same `if (pos + kKvcStep < end)`, whose condition is the workgroup's - the callers pass begin, end and pos that are the same in every wave, and `active`
// is not part of it - so every wave meets the same number of barriers on every path, in either form.  Part (2), what is read from the images and where
// those values can flow, stands next to each body's loop.
// A body passes three one-line lambdas that bind its stage registers to its load_step, store_step and compute_step - compute_step too: handed over as
// it is, or with the calls wrapped in a lambda of the body, two registers change places in the FP8 MLA decode and the MLA prefill dK/dV kernels
// (tools/isa_diff.py).  A function that owns the whole loop restructures the kernels' scalar control flow, so prologue and `for` stay with the body.
template <int BUF, typename Load, typename Store, typename Compute>
FA_DEV void kvc_stage_step(std::integral_constant<int, BUF> bufc, int pos, int begin, int end, int wave, bool active, Load&& load, Store&& store, Compute&& compute) {
    kvc_stage_slow_reader((pos - begin) / kKvcStep, wave);
    if (active) compute(bufc, pos);
    if (pos + kKvcStep < end) {
#if FA_KVC_STAGE_RACY
        __syncthreads();
#endif
        kvc_stage_slow_writer((pos - begin) / kKvcStep, wave);
        store(std::integral_constant<int, BUF ^ 1>{});
#if !FA_KVC_STAGE_RACY
        __syncthreads();
#endif
        if (pos + 2 * kKvcStep < end) load(bufc, pos + 2 * kKvcStep);
    }
}

}  // namespace fa
