// fa_kvcache_stage_debug.hpp — adversarial timing for the register-staged LDS stages of the 64-row KV-cache bodies (test builds only).
//
//   fa_fwd_kvcache_prefill.hip, fa_kvcache_mla_attn.hpp (the one MLA decode body of fa_fwd_kvcache_mla.hip, fa_fwd_kvcache_mla_sparse.hip and
//   fa_fwd_kvcache_mla_fp8.hip), fa_fwd_mla_prefill.hip and fa_bwd_mla_prefill.hip (both of its loops) run one schedule, whose step is written once, in
//   fa_kvcache_stage.hpp (kvc_stage_step, with the two hooks below); this file holds the documentation and the defaults of the switches.  Four waves
//   each write a quarter of a 32-key step into one of two LDS stages that all four read, with ONE barrier per step.  Four waves of a unit run close to
//   lockstep, so a barrier one statement too early would hand a wave the stage's previous tenant almost never, and every value test would pass.
//   tests/test_stage_protocol_gpu.py builds the same kernels with one wave held back and asks for the product's bits.
//
//   FA_KVC_STAGE_DEBUG (the product is 0: both helpers are empty and the device code does not change)
//     1 = SLOW READER: in step n wave n % 4 sleeps in front of compute_step.  A schedule that lets another wave overwrite the stage this wave is
//         about to read hands it the wrong tenant.
//     2 = SLOW WRITER: in step n wave (n + 1) % 4 sleeps in front of store_step (the first fill of stage 0 counts as step -1: wave 0).  A schedule that
//         lets another wave read the stage before the publishing barrier hands it the previous tenant in this wave's quarter.
//     The sleep is `s_sleep 64`, the instruction of the sleepy LDS-DMA builds (fa_fwd_pp16.hip: about 4000 cycles).  It is MEANT to exceed one step,
//     about 68 MFMAs per wave in the MLA bodies; neither the sleep nor the step has been measured.
//   FA_KVC_STAGE_RACY = 1 (the product is 0): the WRONG form the method exists for - the step's barrier stands in front of store_step instead of behind
//     it, so the next step reads a stage nothing has published.  Kept to show that the slow-writer build catches it (it must NOT reproduce the product);
//     nothing is claimed about it at normal timing.  Why it can neither hang nor fault: the barrier count at kvc_stage_step, the flow of the images' values next to each body's loop.
#pragma once
#include "fa_device.hpp"

#ifndef FA_KVC_STAGE_DEBUG
#define FA_KVC_STAGE_DEBUG 0
#endif
#ifndef FA_KVC_STAGE_RACY
#define FA_KVC_STAGE_RACY 0
#endif
