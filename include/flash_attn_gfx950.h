/*
 * flash_attn_gfx950.h — C ABI of the MI355X (gfx950 / CDNA4) fused attention library.
 *
 * This is the drop-in boundary for the hot path of ssiu/flash-attention-turing
 * (reference paths below are relative to the reference checkout):
 *
 *   reference entry (pybind, csrc/flash_attn/flash_api.cpp)      C-ABI replacement
 *   ---------------------------------------------------------   -----------------------------
 *   mha_fwd         flash_api.cpp:156-223  ("fwd",  :472)        fa_mha_fwd
 *   mha_bwd         flash_api.cpp:228-317  ("bwd",  :473)        fa_mha_bwd
 *   mha_varlen_fwd  flash_api.cpp:319-381  ("varlen_fwd", :474)  fa_mha_varlen_fwd
 *   mha_varlen_bwd  flash_api.cpp:383-468  ("varlen_bwd", :475)  fa_mha_varlen_bwd
 *   run_mha_fwd     flash_api.cpp:139-145  + Flash_fwd_params    fa_run_mha_fwd(fa_fwd_params)
 *   run_mha_bwd     flash_api.cpp:147-153  + Flash_bwd_params    fa_run_mha_bwd(fa_bwd_params)
 *                   (src/flash.h:6-76 are the param structs these mirror)
 *
 * Only plain pointers, integers and an opaque stream handle cross this boundary: no torch
 * types, no C++ types.  All pointers are DEVICE pointers (HBM) unless stated otherwise.
 * The library never allocates or frees device memory and never synchronises the device;
 * every kernel is enqueued on the `stream` argument (a hipStream_t passed as void*;
 * NULL = the legacy default stream, which is what the reference launches on,
 * flash_fwd_launch_template.h:68).
 *
 * Conventions (identical to the reference):
 *   q   : (batch, seqlen_q, nheads,   head_dim)   fp16 or bf16
 *   k,v : (batch, seqlen_k, nheads_k, head_dim)   same dtype, nheads % nheads_k == 0 (GQA/MQA)
 *   o   : like q, same dtype.   lse : (batch, nheads, seqlen_q) fp32, natural log.
 *   scale = 1/sqrt(head_dim) always (flash_fwd_kernel.h:351); causal mask is bottom-right
 *   aligned (mask.h:172): key j visible to query i iff j - i <= seqlen_k - seqlen_q.
 *   Rows with no visible key produce o = 0 and lse = 0.0 (flash_fwd_kernel.h:720-728,767-771).
 *   varlen: q (total_q, nheads, d), k/v (total_k, nheads_k, d) packed, cu_seqlens int32
 *   device arrays of length batch+1, lse padded to (batch, nheads, max_seqlen_q).
 *   head_dim in {64, 128} (static_switch.h:29-38); unlike the reference an unsupported
 *   head_dim is an error, not a silent no-op.  (Decode over a KV cache, fa_kvcache_params below, has
 *   head_dim 256 as well: FA_HAS_KVCACHE_HEADDIM256.)
 *   Non-finite Q / K (forward): a NaN in a query row, or a NaN or +inf score (NaN or inf in a
 *   K row the query sees) gives that row o = NaN and lse = NaN, never +-inf; a -inf score only
 *   drops its key; a row that sees no key stays o = 0, lse = 0.  Rows the bad value does not
 *   reach keep their bits, except the other rows of a +inf row's 32-row wave: the running max
 *   is refreshed per wave, so they round P differently (within the usual tolerances).
 *   Non-finite V and a non-finite backward are unspecified: a masked P = 0 still multiplies V
 *   within a key tile, and 0 x NaN is NaN.
 *   Dynamic range (backward): over the finite range the backward is the reference algorithm with
 *   its two 16-bit rounding points (P and dS = P (dP - D), rounded to nearest before the second
 *   GEMMs; D, dP and every sum in fp32; the outputs rounded once at the end).  In fp16 that means:
 *   while |dO|, |dP| and the sums stay below 65504 (a loss scale of 2^12 on unit-variance data
 *   does, 2^14 overflows dK), and down to where dS underflows - subnormal inputs, subnormal dS
 *   and subnormal outputs are honoured, not flushed (every kernel runs with both float denorm
 *   modes at 3), so a dO of 1e-5, which is made of fp16 subnormals, loses precision only as the
 *   2^-24 grid dictates.  bf16 keeps fp32's exponent range, and there scaling dO, V or the pair
 *   (q, 1 / k) by a power of two scales the results by exactly that power, bit for bit, as long
 *   as no intermediate leaves fp32's normal range.
 *   Memory: views are never read or written outside their extent (strides may leave gaps
 *   between rows, heads and batch entries).  Packed: rows of q / k / v / dout past
 *   cu_seqlens[b] (up to total_q / total_k) are never read, and the padded lse entries
 *   (t >= seqlen of the sequence) and the padding rows of o / dq / dk / dv are never written.
 *
 * Every function returns FA_OK (0) or a negative FA_ERR_* code; positive values are
 * hipError_t codes from the launch.  fa_last_error() gives a human readable message for
 * the calling thread.
 */
#ifndef FLASH_ATTN_GFX950_H
#define FLASH_ATTN_GFX950_H

#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 4   /* 2: optional total_q / total_k appended to fa_fwd_params / fa_bwd_params; 3: optional workspace appended to
                              fa_bwd_params; 4: both structs start with {struct_size, magic}, appended fields are read only if the caller's
                              struct holds them */
/* Every params struct starts with its own size AS THE CALLER COMPILED IT and this constant.  The library copies min(struct_size,
 * its own sizeof) bytes into a zeroed local struct: a caller built against an older ABI >= 4 header simply leaves the fields appended
 * since then at their defaults (0 / NULL = "not given"), and a caller built against an ABI 1-3 header (no size field: its first 8
 * bytes are the q pointer, whose upper half can never equal the magic) is rejected with FA_ERR_BAD_ABI instead of having the library
 * read past the end of its struct.  FA_PARAMS_INIT(p) zeroes a struct and fills both fields. */
#define FA_PARAMS_MAGIC 0xFA950A71u
#define FA_PARAMS_INIT(p) do { memset(&(p), 0, sizeof(p)); (p).struct_size = (uint32_t)sizeof(p); (p).magic = FA_PARAMS_MAGIC; } while (0)

enum fa_dtype { FA_FP16 = 0, FA_BF16 = 1 };

enum fa_status {
    FA_OK = 0,
    FA_ERR_NULL_POINTER = -1,
    FA_ERR_BAD_SHAPE = -2,       /* rank/size disagreement (reference: TORCH_CHECKs flash_api.cpp:178-183) */
    FA_ERR_BAD_GQA = -3,         /* nheads % nheads_k != 0 (flash_api.cpp:183) */
    FA_ERR_BAD_HEADDIM = -4,     /* head_dim not in {64,128} (decode over a KV cache: {64,128,256}) */
    FA_ERR_BAD_DTYPE = -5,
    FA_ERR_BAD_STRIDE = -6,      /* last dim not contiguous, misaligned rows, or extent > 2^31 bytes per sequence */
    FA_ERR_NO_DEVICE = -7,
    FA_ERR_BAD_ABI = -8          /* params struct without a valid {struct_size, magic} header, shorter than the ABI 4 base, or longer
                                    than this library knows (caller compiled against a newer header) */
};

/* Element strides (NOT bytes). The innermost (head_dim) stride is 1 by contract. */
typedef struct fa_strides {
    int64_t batch; /* ignored for varlen (packed) tensors */
    int64_t row;   /* between consecutive sequence positions */
    int64_t head;  /* between consecutive heads */
} fa_strides;

/* Mirrors Qkv_params + Flash_fwd_params (reference src/flash.h:6-52). */
typedef struct fa_fwd_params {
    uint32_t struct_size;       /* sizeof(fa_fwd_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;                 /* (b, h, seqlen_q) contiguous; varlen: (b, h, max_seqlen_q) */
    const int32_t* cu_seqlens_q; /* NULL for fixed-length batches */
    const int32_t* cu_seqlens_k;
    int32_t b;
    int32_t seqlen_q;           /* varlen: max_seqlen_q */
    int32_t seqlen_k;           /* varlen: max_seqlen_k */
    int32_t h;
    int32_t h_k;
    int32_t d;
    int32_t dtype;              /* enum fa_dtype */
    int32_t is_causal;
    fa_strides q_stride, k_stride, v_stride, o_stride;
    /* ABI 2, optional (0 = unknown).  varlen only: number of rows of the PACKED q / k tensors (what the reference's mha_varlen_fwd
     * sees as q.size(0) / k.size(0), flash_api.cpp:319-381).  MUST be >= cu_seqlens_q[b] / cu_seqlens_k[b] (like max_seqlen, the
     * library cannot check device values without synchronising).  When given, the launch grid is sized by the tokens actually
     * present instead of max_seqlen x batch, which matters for batches of very unequal lengths (varlen). */
    int64_t total_q;
    int64_t total_k;
} fa_fwd_params;

/* Mirrors Flash_bwd_params (reference src/flash.h:55-76). */
typedef struct fa_bwd_params {
    uint32_t struct_size;       /* sizeof(fa_bwd_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    const void* k;
    const void* v;
    const void* o;
    const void* dout;
    const float* lse;
    void* dq;
    void* dk;                   /* (b, seqlen_k, h_k, d): already summed over the GQA group */
    void* dv;
    float* dsoftmax_sum;        /* D = rowsum(dO*O), same shape as lse (the reference's do_o): written by the dQ launch, read by dK/dV */
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_k;
    int32_t h;
    int32_t h_k;
    int32_t d;
    int32_t dtype;
    int32_t is_causal;
    fa_strides q_stride, k_stride, v_stride, o_stride, do_stride, dq_stride, dk_stride, dv_stride;
    int64_t total_q;            /* ABI 2, optional, see fa_fwd_params */
    int64_t total_k;
    /* ABI 3, optional (NULL / 0 = none): fp32 scratch for the dK/dV kernel.  Its grid is b * h_k * ceil(seqlen_k / 128)
     * workgroups; with few KV heads (GQA / MQA) that underfills the chip and, under a causal mask, is unbalanced (the first key
     * block of a sequence meets every query tile, the last a single one).  Given this scratch, the h / h_k query heads of a KV
     * head are dealt to several workgroups that leave fp32 partial sums here, and a second kernel adds them in a fixed order
     * (results stay deterministic).  fa_bwd_workspace_bytes() is the size that lets the library choose freely; a smaller buffer
     * limits the split, none keeps the single-pass behaviour of ABI 2.  Contents are unspecified afterwards. */
    void* workspace;
    int64_t workspace_bytes;
} fa_bwd_params;

/* Decode attention over a KV cache (flash-attn's flash_attn_with_kvcache conventions; no counterpart in the reference).  Same ABI 4 header
 * rule as the structs above (FA_PARAMS_INIT); fields appended later will be optional.  The presence of fa_run_mha_fwd_kvcache is how a caller
 * detects the feature (FA_ABI_VERSION is unchanged).
 *   q (b, seqlen_q, h, d), seqlen_q >= 1; k_cache / v_cache (b, seqlen_cache, h_k, d), each with its own strides;
 *   cache_seqlens: int32 DEVICE array (b,), or NULL = every sequence is seqlen_cache long;
 *   k_new / v_new (b, seqlen_new, h_k, d), both or neither: written IN PLACE into the cache at rows cache_seqlens[i] .. + seqlen_new - 1
 *   (cache_seqlens is required then and is not updated), after which attention runs over the first L_i = cache_seqlens[i] + seqlen_new
 *   keys; without them over L_i = cache_seqlens[i].  causal masks key j for query t when j > L_i - seqlen_q + t.
 *   o like q, lse (b, h, seqlen_q) fp32 natural log; rows with no visible key: o = 0, lse = 0.
 * Precondition (like max_seqlen for varlen, the library cannot check device values without synchronising): cache_seqlens[i] + seqlen_new
 * <= seqlen_cache.  Broken, nothing is read or written outside the cache: lengths are clamped to seqlen_cache and appended rows that do not
 * fit are dropped.  No host synchronisation: the call can be captured in a graph and replayed with new cache_seqlens values.
 * workspace: fp32 scratch for the key split (fa_kvcache_workspace_bytes), 16-byte aligned; a smaller buffer caps the split, none (NULL / 0)
 * means one split.  num_splits > 0 overrides the library's choice (capped by the 32-key tiles of seqlen_cache and by the workspace).
 * Results are deterministic for a given split count.
 * Paged cache (optional fields after workspace_bytes; block_table == NULL = the contiguous cache above): k_cache / v_cache are pools of
 * num_blocks pages of page_block_size rows (a positive multiple of 16), k_cache_stride.batch / v_cache_stride.batch the page strides.
 * block_table: int32 DEVICE array, row i (at block_table + i * block_table_stride, block_table_stride >= seqlen_cache / page_block_size)
 * lists the pages of sequence i: logical key j is row j % page_block_size of page block_table[i][j / page_block_size].  seqlen_cache is
 * the per-sequence capacity, a positive multiple of page_block_size (the table has seqlen_cache / page_block_size columns); it plays the
 * same part as above (split, causal alignment, precondition).  The append writes through the table.  Pool rows at or past L_i, table
 * entries of pages at or past ceil(L_i / page_block_size) and pages no sequence references are never read into a result.  Pages may be
 * shared between sequences for reading.  Precondition: every entry a sequence needs lies in [0, num_blocks).  Broken, nothing outside the
 * pool is read or written: every entry the kernels use goes through min((uint32_t)entry, num_blocks - 1), so a bad entry reads (or, for
 * the append, writes) page num_blocks - 1.  A caller built against the header before these fields (struct_size = offsetof(block_table))
 * gets the contiguous cache.
 * head_dim (FA_HAS_KVCACHE_HEADDIM256): d is 64, 128 or 256; anything else is FA_ERR_BAD_HEADDIM.  d = 256 (Gemma 2 2B / 9B, Gemma 3) exists for
 * the three kvcache entry points and their _ex forms ONLY - fa_run_mha_fwd / _bwd and the varlen entry points keep rejecting it - and supports
 * everything stated here and for the options below exactly as d = 128 does: both dtypes, both layouts, GQA / MQA, causal, windows, the 8-bit cache,
 * rotary (rotary_dim up to 256), ragged batches, softmax_scale and softcap, num_splits, graph capture; same tolerances, same bit-for-bit
 * relations (paged = contiguous, ragged sequence = dense call, rotary = pre-rotated), same workspace formula (it is written in d).  Its
 * attention kernels run one workgroup per compute unit where 64 / 128 run two (a lane holds about 390 registers at d = 256). */
#define FA_HAS_KVCACHE_HEADDIM256 1
typedef struct fa_kvcache_params {
    uint32_t struct_size;       /* sizeof(fa_kvcache_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    void* k_cache;
    void* v_cache;
    const void* k_new;          /* NULL: no append */
    const void* v_new;
    void* o;
    float* lse;
    const int32_t* cache_seqlens;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t seqlen_new;         /* rows of k_new / v_new (0 without them) */
    int32_t h;
    int32_t h_k;
    int32_t d;
    int32_t dtype;
    int32_t is_causal;
    int32_t num_splits;         /* 0 = the library's choice */
    fa_strides q_stride, k_cache_stride, v_cache_stride, k_new_stride, v_new_stride, o_stride;
    void* workspace;
    int64_t workspace_bytes;
    const int32_t* block_table;     /* optional: paged cache (see above); NULL = contiguous */
    int64_t block_table_stride;     /* elements between table rows */
    int32_t page_block_size;        /* rows per page; 0 without block_table */
    int32_t num_blocks;             /* pages in the pool */
} fa_kvcache_params;

/* Options of a decode call that fa_kvcache_params does not carry (its layout is fixed; the _ex entry points below take both).  Same ABI 4
 * header rule (FA_PARAMS_INIT): a zeroed struct means the plain call, and every later option arrived as optional fields appended after these
 * (the 8-bit cache, the rotary embedding on append, ragged query batches, the softmax scale and softcap of fa_kvcache_options_v5, the attention sinks of fa_kvcache_options_v6, and the tree mask of fa_kvcache_options_v7, below).  A NULL options pointer is the same as a zeroed struct.
 * Sliding window (upstream flash-attn's window_size; is_local = 0: no window, the two sizes are not read).  Key j of sequence i (valid
 * length L_i as above) is visible to query t when
 *     L_i - seqlen_q + t - window_size_left <= j <= L_i - seqlen_q + t + window_size_right,
 * with -1 = unbounded on that side and j < L_i always; values below -1 are FA_ERR_BAD_SHAPE.  is_causal sets the right edge to 0 (the right
 * size is then ignored): (W - 1, 0) with is_causal is the usual "last W keys" window, and (0, 0) is a legitimate window of one key.  A
 * window that cannot bind (both sides -1, left >= seqlen_cache - 1 with right -1 or causal, ...) runs exactly the call without it (same
 * kernels, split, workspace and bits).  Cache rows below max(0, L_i - seqlen_q - left) and at or past L_i, and table entries of pages that
 * lie wholly outside [that row, L_i), are never read into a result.  A window with a left edge sizes the split from its span instead of the
 * capacity: the split and the workspace are never larger than without the window.  A row that sees no key gives o = 0, lse = 0.  A
 * non-finite V element in a row that another query row of the same KV head and row tile sees (the seqlen_q x h / h_k rows of a KV head go
 * through the kernels in tiles of 16) but this row does not can make this row's o NaN, as under causal with seqlen_q > 1.
 *
 * 8-bit cache: fa_kvcache_options_v2 below is fa_kvcache_options with optional fields appended after window_size_right; the _ex entry points
 * take either through the same pointer and tell them apart by struct_size (sizeof(fa_kvcache_options): the window alone, as before;
 * sizeof(fa_kvcache_options_v2): all fields; anything else is FA_ERR_BAD_ABI).  fa_kvcache_options itself keeps its layout, so a caller
 * built against it keeps working, and it and a v2 struct with a zeroed tail get the 16-bit cache.  FA_ABI_VERSION is unchanged.  cache_dtype =
 * FA_CACHE_FP8_E4M3: k_cache / v_cache hold OCP e4m3fn codes (one byte per element; torch.float8_e4m3fn - not the fnuz format, not e5m2)
 * and the k_cache_stride / v_cache_stride of fa_kvcache_params count those 1-byte elements.  q, k_new, v_new, o keep `dtype` (fp16 / bf16),
 * lse stays fp32.  k_descale / v_descale: fp32 DEVICE arrays, element (i, g) at [i * batch_stride + g * head_stride] (strides in
 * elements, 0 allowed: one value for all), NULL = 1.0.  The call equals the 16-bit call over the dequantised cache
 *     K[i, j, g, :] = float(k_cache[i, j, g, :]) * k_descale[i, g],   V likewise,
 * in exact arithmetic: the codes are widened to `dtype` without rounding (every finite e4m3 value is an fp16 and a bf16 value) in front of
 * the same matrix instructions, k_descale folds into the softmax scale of its (batch, KV head) and v_descale into the final 1 / l
 * normalisation, both in fp32; Q and P are never quantised.  Descales are read on the device (no host synchronisation; a captured call
 * replays with the values then in memory).  Precondition (not checked, it would need a synchronisation): descales are finite and > 0.
 * Append: k_new / v_new rows are quantised into the cache, code = e4m3_rne(clamp(float(x) / descale, -448, 448)) with a correctly rounded
 * fp32 quotient, round to nearest even (into the e4m3 subnormals too), NaN -> 0x7f / 0xff, +-inf saturate to +-448; attention then runs
 * over the quantised rows.  Everything stated above for the 16-bit cache holds unchanged: contiguous and paged layout (same page size
 * rule, same clamping of table entries), the window, causal, GQA / MQA, num_splits and the workspace (split count and workspace bytes are
 * those of a 16-bit cache of the same shape: they follow the capacity, not the element size), rows without a visible key o = 0, lse = 0,
 * determinism per split count, rows / pages / heads that are never read.  NaN: a NaN code (0x7f / 0xff) in a visible K row makes that row's
 * o and lse NaN (e4m3fn has no inf).  Paged and contiguous calls over the same logical cache give the same bits.
 * Alignment of an 8-bit cache (the kernels keep 16-byte loads): base pointers 16-byte aligned; row, head and batch / page strides multiples
 * of 16 elements, row stride >= d; one sequence (one page) spans less than 2^31 bytes.  Anything else is FA_ERR_BAD_STRIDE - a cache is
 * never copied.  An unknown cache_dtype, or a descale pointer without FA_CACHE_FP8_E4M3, is FA_ERR_BAD_DTYPE.
 *
 * Rotary embedding (FA_HAS_KVCACHE_ROTARY): fa_kvcache_options_v3 below is fa_kvcache_options_v2 with optional fields appended; the _ex entry
 * points accept exactly the three sizes, and a v3 struct with a zeroed tail is a v2 call.  FA_ABI_VERSION is unchanged.  rotary_cos /
 * rotary_sin (both or neither; NULL = off): DEVICE tables (seqlen_ro, rotary_dim / 2) of `dtype` (the dtype of q - not fp32), last dim
 * contiguous, rows rotary_row_stride elements apart.  rotary_dim is a multiple of 16 with 16 <= rotary_dim <= d; elements rotary_dim .. d - 1
 * of a row pass through.  seqlen_ro >= seqlen_cache.  Rotary needs k_new / v_new (the rotation belongs to the append).  With
 * c = cos[p, i], s = sin[p, i], i < rotary_dim / 2, a row x at position p becomes y with, for the pair (a, b) = (i, i + rotary_dim / 2)
 * (rotary_interleaved = 0, GPT-NeoX) or (2 i, 2 i + 1) (rotary_interleaved != 0, GPT-J),
 *     y_a = x_a * c - x_b * s,    y_b = x_b * c + x_a * s,
 * every operation in fp32, rounded on its own (no contraction), and y rounded once, to nearest even, to `dtype`.  Position of appended row s
 * of sequence i: max(cache_seqlens[i], 0) + s, its cache row.  Position of query row t: max(cache_seqlens[i], 0) + t when is_causal != 0 or
 * the options carry a window other than (-1, -1) - as the caller states them, before a window that cannot bind is normalised away - else
 * max(cache_seqlens[i], 0) for every t.  On the device a position is clamped to seqlen_ro - 1: no value of cache_seqlens reads outside the
 * tables.  THE CONTRACT: the call equals, bit for bit in o, lse and every cache byte, the same call without rotary on q and k_new rotated by
 * the formula above (v_new is appended as is), for the same num_splits; with an 8-bit cache the rotated row, already rounded to `dtype`,
 * goes through the quantiser above.  So everything stated for the plain call carries over.  q, k_new, v_new and the tables are not written;
 * table rows other than the positions above are never read.  One fused launch takes the place of the append (rotate k_new into the cache,
 * copy / quantise v_new, write the rotated q into an image); the call stays at up to three launches.  The image comes out of the workspace:
 * fa_kvcache_workspace_bytes_ex returns align16(b * seqlen_q * h * d * 2) plus what it returns without rotary; the image sits first, the
 * split partials behind it, and "a smaller workspace caps the split" applies to what remains.  Split count and split workspace are those of
 * the same call without rotary.  A workspace too small for the image is FA_ERR_BAD_SHAPE (there is no path without the image).  One table
 * without the other, rotary_dim not a multiple of 16 or outside [16, d], seqlen_ro < max(seqlen_cache, 1), rotary without k_new / v_new:
 * FA_ERR_BAD_SHAPE; a table pointer that is not 16-byte aligned, or a row stride that is not a multiple of 8 elements or is below
 * rotary_dim / 2 (with more than one row): FA_ERR_BAD_STRIDE. */
typedef struct fa_kvcache_options {
    uint32_t struct_size;       /* sizeof(fa_kvcache_options) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* != 0: the window below applies */
    int32_t window_size_left;   /* >= -1 */
    int32_t window_size_right;  /* >= -1; ignored under is_causal */
} fa_kvcache_options;
#define FA_CACHE_FP8_E4M3 1
typedef struct fa_kvcache_options_v2 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v2) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the five fields of fa_kvcache_options, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;        /* optional: 0 = the dtype of q, FA_CACHE_FP8_E4M3 = 8-bit codes (see above) */
    const float* k_descale;     /* optional: fp32 device array, NULL = 1.0; FA_CACHE_FP8_E4M3 only */
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;   /* in elements */
    int64_t v_descale_batch_stride, v_descale_head_stride;
} fa_kvcache_options_v2;
#define FA_HAS_KVCACHE_ROTARY 1
typedef struct fa_kvcache_options_v3 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v3) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the fields of fa_kvcache_options_v2, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;
    const float* k_descale;
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    const void* rotary_cos;     /* optional: device table (seqlen_ro, rotary_dim / 2) of `dtype`; NULL = no rotary (the fields below are not read) */
    const void* rotary_sin;
    int64_t rotary_row_stride;  /* elements between table rows (both tables) */
    int32_t seqlen_ro;          /* table rows, >= seqlen_cache */
    int32_t rotary_dim;         /* a multiple of 16 in [16, d] */
    int32_t rotary_interleaved; /* 0: pairs (i, i + rotary_dim / 2); != 0: pairs (2 i, 2 i + 1) */
    int32_t reserved_;          /* 0 (pads the struct to a multiple of 8 bytes) */
} fa_kvcache_options_v3;

/* Ragged query batches (FA_HAS_KVCACHE_RAGGED): fa_kvcache_options_v4 below is fa_kvcache_options_v3 with optional fields appended; the _ex
 * entry points accept exactly the four sizes (20, 72, 112, 144 bytes), and a v4 struct with a zeroed tail is a v3 call.  FA_ABI_VERSION is
 * unchanged.  cu_seqlens_q (int32 DEVICE array (b + 1,), non-decreasing from 0; NULL = off, the fields below are not read): q and o are PACKED,
 * (total_q, h, d) with row and head strides (q_stride.batch / o_stride.batch are ignored), sequence i owns rows cu_seqlens_q[i] ..
 * cu_seqlens_q[i + 1] - 1 (sq_i rows, 0 allowed), and lse is (h, total_q): entry [hq * total_q + cu_seqlens_q[i] + t].  In fa_kvcache_params,
 * b is the number of sequences (cache_seqlens, block_table rows, the contiguous cache's batch, the descales), seqlen_q carries max_seqlen_q
 * (>= 1; precondition sq_i <= max_seqlen_q, a device value and not checked - it sizes the launch and the split, never which keys a row sees);
 * total_q below is the rows of q / o: it may exceed cu_seqlens_q[b]; the rows past it are never read and their o / lse entries are never written.
 * k_new / v_new, if given, are packed as well, (total_k_new, h_k, d) under cu_seqlens_k_new (same rules; it may be the same array as
 * cu_seqlens_q), k_new_stride.batch / v_new_stride.batch are ignored and seqlen_new carries the largest sn_i allowed (<= seqlen_cache).
 * Sequence i appends its sn_i rows at cache rows max(cache_seqlens[i], 0) .. + sn_i - 1 (through the table when paged, quantised into an 8-bit
 * cache); rows that would land at or past seqlen_cache are dropped, nothing is written outside the sequence's capacity or the pool.  Then
 * L_i = min(max(cache_seqlens[i], 0) + sn_i, seqlen_cache) and row t of sequence i sees key j < L_i, under is_causal only j <= L_i - sq_i + t,
 * under a window only L_i - sq_i + t - left <= j <= L_i - sq_i + t + right: the formulas above with sq_i in place of seqlen_q.  THE CONTRACT:
 * sequence i of a ragged call equals, bit for bit in o, lse and every cache byte, the dense call on that sequence alone (b = 1, seqlen_q = sq_i)
 * with the same key split (num_splits = 1 always; a forced num_splits = n cuts the keys at the same places unless a window with a left edge
 * shortens the span, which the ragged call sizes from max_seqlen_q).  Everything stated above carries over: both cache layouts, the clamping of
 * table entries, GQA / MQA, the 8-bit cache, windows, rows without a visible key o = 0, lse = 0, the NaN rules, determinism per split count,
 * no host synchronisation, what is never read.  The automatic split counts the tile slots of the launch in place of b x row tiles:
 * min(ceil(total_q * (h / h_k) / 16) + b, b * ceil(max_seqlen_q * (h / h_k) / 16)) per KV head; the workspace is that of h * total_q rows.
 * Errors: cu_seqlens_k_new without cu_seqlens_q or without k_new, k_new in a ragged call without cu_seqlens_k_new: FA_ERR_NULL_POINTER;
 * total_q < 0, total_k_new < 0, a grid past 2^31 - 1 workgroups, rotary together with cu_seqlens_q (not supported): FA_ERR_BAD_SHAPE; a
 * cu_seqlens pointer that is not 4-byte aligned: FA_ERR_BAD_STRIDE. */
#define FA_HAS_KVCACHE_RAGGED 1
typedef struct fa_kvcache_options_v4 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v4) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the fields of fa_kvcache_options_v3, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;
    const float* k_descale;
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    const void* rotary_cos;
    const void* rotary_sin;
    int64_t rotary_row_stride;
    int32_t seqlen_ro;
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t reserved_;
    const int32_t* cu_seqlens_q;        /* optional: device array (b + 1,); NULL = the dense call (the fields below are not read) */
    const int32_t* cu_seqlens_k_new;    /* device array (b + 1,) for packed k_new / v_new; NULL without them */
    int64_t total_q;                    /* packed rows of q / o */
    int64_t total_k_new;                /* packed rows of k_new / v_new */
} fa_kvcache_options_v4;

/* Softmax scale and soft-capped scores (FA_HAS_KVCACHE_SOFTCAP; upstream flash-attn's softmax_scale / softcap): fa_kvcache_options_v5 below is
 * fa_kvcache_options_v4 with optional fields appended; the _ex entry points accept exactly the five sizes (20, 72, 112, 144, 168 bytes), and a
 * v5 struct with a zeroed tail is a v4 call: same kernels, split, workspace and bits.  FA_ABI_VERSION is unchanged.
 *   softmax_scale: 0 = the default 1 / sqrt(d), computed as 1.0f / sqrtf((float)d); otherwise the scores are (q . k) * softmax_scale.  A value
 *   equal to the default gives the default's bits (the value is the same and so are the kernels).
 *   softcap: 0 = off.  > 0: score = softcap * tanh((q . k) * softmax_scale / softcap); the mask (length, causal, window) comes after the cap, the
 *   softmax runs over the capped scores and lse is their natural-log logsumexp.  tanh is built from the exponential and reciprocal
 *   instructions, 1 - 2 / (exp(2 x) + 1): absolute error about 1e-7, times softcap in the score.
 * A negative, NaN or infinite value of either is FA_ERR_BAD_SHAPE (fa_last_error names the field), as is a pair whose ratio softmax_scale /
 * softcap is zero or infinite in fp32; a non-zero `reserved` is FA_ERR_BAD_ABI (a
 * newer caller's field this library does not know).  Errors of fa_kvcache_params and of the older option fields come first.  Both are host
 * values baked into the call like the window: no synchronisation, and a captured call replays with them.  Everything stated above carries over
 * for both: contiguous and paged layout and the clamping of table entries, GQA / MQA, fp16 / bf16, head_dim 64 / 128 / 256, windows, causal,
 * num_splits (the split count and the workspace do not depend on the two values), the 8-bit cache (k_descale multiplies the score inside the
 * tanh, v_descale stays in the final normalisation), rotary (a launch of its own in front of attention), ragged batches (sequence i of a
 * soft-capped ragged call equals the soft-capped dense call on it alone, bit for bit, under the split rule above), rows without a visible key
 * o = 0, lse = 0, determinism per split count, what is never read.  Paged and contiguous soft-capped calls over the same logical cache give the
 * same bits.  Plain, causal and windowed soft-capped calls are all served by the window kernels (an unbounded window is the plain call).
 * Non-finite inputs: with softcap = 0 the rules above hold under any softmax_scale.  With softcap > 0 the contract is fp32 math on the CAPPED
 * scores, which differs in two places: a NaN score still makes the row's o and lse NaN, but a raw score of +inf caps to +softcap - finite, the
 * row is no longer NaN - and a raw score of -inf caps to -softcap - the key is no longer dropped.
 * sizeof is 168, not 152: the sizes 145, 148, 152, 160, 176 and 256 are pinned as FA_ERR_BAD_ABI by callers' tests of the v4 library, and 168 is
 * the smallest multiple of 8 that clears them; the two reserved words are the room that leaves. */
#define FA_HAS_KVCACHE_SOFTCAP 1
typedef struct fa_kvcache_options_v5 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v5) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the fields of fa_kvcache_options_v4, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;
    const float* k_descale;
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    const void* rotary_cos;
    const void* rotary_sin;
    int64_t rotary_row_stride;
    int32_t seqlen_ro;
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t reserved_;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k_new;
    int64_t total_q;
    int64_t total_k_new;
    float softmax_scale;        /* optional: 0 = 1 / sqrt(d); else finite and > 0 */
    float softcap;              /* optional: 0 = off; else finite and > 0 */
    int64_t reserved[2];        /* 0 */
} fa_kvcache_options_v5;

/* Attention sinks (FA_HAS_KVCACHE_SINKS; `sinks` of transformers / the gpt-oss reference, `s_aux` of vLLM's flash-attn): fa_kvcache_options_v6
 * below is fa_kvcache_options_v5 with optional fields appended; the _ex entry points accept exactly the six sizes (20, 72, 112, 144, 168, 200
 * bytes), and a v6 struct with a zeroed tail is a v5 call: same kernels, split, workspace and bits.  FA_ABI_VERSION is unchanged.
 *   sinks: NULL = off.  Otherwise fp32 device memory, 4-byte aligned (else FA_ERR_BAD_STRIDE), one logit per QUERY head: head hq reads
 *   sinks[hq * sinks_stride] (elements; any value, 0 broadcasts one logit).  The logit is in the units of the final scores - behind softmax_scale
 *   and k_descale, natural-log - and is never scaled.  It joins the softmax denominator and contributes no value: with the visible scores s_j
 *   of a row and M = max(max_j s_j, sink), in fp32 math
 *       o = sum_j exp(s_j - M) v_j / (sum_j exp(s_j - M) + exp(sink - M)),   lse = M + log(sum_j exp(s_j - M) + exp(sink - M)).
 *   The returned lse INCLUDES the sink, so exp(s_j - lse) are the probabilities actually used (they sum to less than 1: the rest sits on the
 *   sink).  The maximum covers the sink: a sink far above every score gives o near 0 and lse near the sink without overflow, one far below
 *   gives the call without sinks.  The values are read on the device like the descales: no synchronisation, and a captured call replays with
 *   the values then in memory.
 *   Rows that see no key: a finite sink holds all the mass, o = 0 and lse = the sink exactly; with a sink of -inf the row is dead as ever, o =
 *   0, lse = 0.  A sink of -inf on every head gives the call without sinks bit for bit, o and lse, for every num_splits.  A NaN sink makes the
 *   rows of its head NaN in o and lse and leaves the other heads' bits alone; +inf breaks the precondition: the result is unspecified, nothing
 *   is read or written out of bounds.  The NaN / +inf score rules are unchanged.
 * Everything stated above carries over: contiguous and paged layout and the clamping of table entries, GQA / MQA (packed row r of a KV head's
 * tile belongs to query head kv_head * h_ratio + r % h_ratio), fp16 / bf16, head_dim 64 / 128, windows, causal, num_splits (the split count and
 * the workspace do not depend on sinks: a split call runs the attention kernels of the call without sinks and a combine that adds the sink as
 * one more term of the merge), the 8-bit cache (k_descale does not touch the sink, v_descale stays in the final normalisation), softmax_scale,
 * rotary (a launch of its own in front of attention), ragged batches (sequence i of a ragged sink call equals the dense sink call on it alone,
 * bit for bit, under the split rule above), paged == contiguous bit for bit, determinism per split count, what is never read.  Plain, causal and
 * windowed unsplit sink calls are all served by the window kernels (an unbounded window is the plain call).
 * Not supported, FA_ERR_BAD_SHAPE with the field named by fa_last_error: sinks together with softcap > 0 (no model has both), and sinks at d =
 * 256.  A non-zero `reserved2` is FA_ERR_BAD_ABI (a newer caller's field this library does not know).  Errors of fa_kvcache_params and of the
 * older option fields come first, then those of sinks, then reserved2.
 * sizeof is 200: the sizes 169 .. 192 and 256 are pinned as FA_ERR_BAD_ABI by callers' tests of the v5 library, and 200 is the next multiple of
 * 8 that clears them; the two reserved words are the room that leaves. */
#define FA_HAS_KVCACHE_SINKS 1
typedef struct fa_kvcache_options_v6 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v6) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the fields of fa_kvcache_options_v5, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;
    const float* k_descale;
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    const void* rotary_cos;
    const void* rotary_sin;
    int64_t rotary_row_stride;
    int32_t seqlen_ro;
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t reserved_;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k_new;
    int64_t total_q;
    int64_t total_k_new;
    float softmax_scale;
    float softcap;
    int64_t reserved[2];        /* 0 */
    const float* sinks;         /* optional: NULL = off; (h,) fp32 on the device, one logit per query head */
    int64_t sinks_stride;       /* elements between consecutive heads' logits */
    int64_t reserved2[2];       /* 0 */
} fa_kvcache_options_v6;

/* Tree attention masks (FA_HAS_KVCACHE_TREE_MASK; the draft trees of EAGLE / Medusa / SpecInfer, the tree-attention backend of vLLM, the custom
 * mask of SGLang and FlashInfer): fa_kvcache_options_v7 below is fa_kvcache_options_v6 with optional fields appended; the _ex entry points accept
 * exactly the seven sizes (20, 72, 112, 144, 168, 200, 240 bytes), and a v7 struct with a zeroed tail is a v6 call: same kernels, split,
 * workspace and bits.  FA_ABI_VERSION is unchanged.
 *   tree_mask: NULL = off.  Otherwise int64 device memory, 8-byte aligned (else FA_ERR_BAD_STRIDE), one word per query row: row t of sequence i
 *   reads tree_mask[i * tree_mask_batch_stride + t * tree_mask_row_stride] (elements, any values); a ragged call (cu_seqlens_q) reads
 *   tree_mask[r * tree_mask_row_stride] for packed row r and uses tree_mask_row_stride only; rows at or past cu_seqlens_q[b] are never read.
 *   With L_i the valid length, sq_i the query rows of the sequence (seqlen_q; ragged: cu_seqlens_q[i + 1] - cu_seqlens_q[i]) and base_i = L_i -
 *   sq_i, query row t sees key j iff 0 <= j < L_i and
 *       j < base_i   or   bit (j - base_i) of the row's word is set.
 *   Bit u of row t means "draft token t sees draft token u": the draft tokens are the last sq_i keys of the sequence, in the usual call the
 *   rows just appended through k_new / v_new, and every row sees the whole prefix in front of them.  Bits at or above sq_i are ignored, and so
 *   are bits whose key index would be negative (L_i < sq_i: the first draft token the cache holds is key 0 and bit sq_i - L_i).  Bit 63 is the
 *   sign bit and an ordinary bit.  Any bit pattern is legal: it need not be a tree, and the diagonal need not be set.  A row that sees no key
 *   (L_i = 0, or no prefix and no bit set) is o = 0, lse = 0, as everywhere else.  The words are read on the device like lengths and descales:
 *   no synchronisation, and a captured call replays with the words then in memory.  seqlen_q (ragged: the max_seqlen_q it carries) must be at
 *   most 64.
 *   Two relations hold bit for bit, o and lse, for every num_splits: the lower-triangle mask (bit u of row t set iff u <= t) gives the
 *   is_causal call, and the mask with bits 0 .. sq - 1 all set gives the call with neither.  The tree kernels are the plain attention body
 *   over the same 32-key steps [0, L_i); only the select of a score differs.
 * Everything stated above carries over: contiguous and paged layout and the clamping of table entries, GQA / MQA (the query heads of a token
 * share its mask word: packed row r of a KV head's tile reads the word of token r / h_ratio), fp16 / bf16, head_dim 64 / 128, the 8-bit cache and
 * its descales, softmax_scale, num_splits (the split count and the workspace do not depend on the mask: they are those of the call without it;
 * append, partial planes and combine are the unchanged kernels), ragged batches (sequence i of a ragged tree call equals the dense tree call on
 * it alone, bit for bit, under the split rule above), paged == contiguous bit for bit, determinism per split count, the NaN rules over the
 * visible keys (a NaN or +inf score a row sees makes the row NaN; a key no row of a tile sees cannot reach its rows, whatever K holds there,
 * while V rows below L_i are multiplied by a probability of 0 and must be finite), what is never read (cache rows at or past L_i, table entries
 * of blocks past L_i, mask words of rows a sequence does not have).
 * Not supported, FA_ERR_BAD_SHAPE with the field named by fa_last_error: tree_mask together with is_causal, with a window other than (-1, -1),
 * with softcap > 0, with sinks, with rotary_cos / rotary_sin (a node's position is its depth, not its index: the engine rotates), at d = 256,
 * and with seqlen_q / max_seqlen_q above 64.  A non-zero `reserved3` is FA_ERR_BAD_ABI (a newer caller's field this library does not know).
 * Errors of fa_kvcache_params and of the older option fields come first, then those of tree_mask, then reserved3.
 * sizeof is 240: the sizes 201 .. 232 and 256 are pinned as FA_ERR_BAD_ABI by callers' tests of the v6 library, and 240 is the next multiple of
 * 8 that clears them; the two reserved words are the room that leaves. */
#define FA_HAS_KVCACHE_TREE_MASK 1
typedef struct fa_kvcache_options_v7 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v7) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the fields of fa_kvcache_options_v6, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;
    const float* k_descale;
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    const void* rotary_cos;
    const void* rotary_sin;
    int64_t rotary_row_stride;
    int32_t seqlen_ro;
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t reserved_;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k_new;
    int64_t total_q;
    int64_t total_k_new;
    float softmax_scale;
    float softcap;
    int64_t reserved[2];        /* 0 */
    const float* sinks;
    int64_t sinks_stride;
    int64_t reserved2[2];       /* 0 */
    const int64_t* tree_mask;   /* optional: NULL = off; (b, seqlen_q) int64 on the device, ragged: (total_q,); one word per query row */
    int64_t tree_mask_batch_stride, tree_mask_row_stride;       /* elements; a ragged call uses the row stride only */
    int64_t reserved3[2];       /* 0 */
} fa_kvcache_options_v7;

/* 64-row workgroups for prompt chunks (FA_HAS_KVCACHE_PREFILL): fa_kvcache_options_v8 below is fa_kvcache_options_v7 with optional fields
 * appended; the _ex entry points accept exactly the eight sizes (20, 72, 112, 144, 168, 200, 240, 288 bytes), and a v8 struct with a zeroed
 * tail is a v7 call: same kernels, split, workspace and bits.  FA_ABI_VERSION is unchanged.
 *   row_tile: 0 = the 16-row kernels (every call above), 64 = the wide kernels; anything else is FA_ERR_BAD_SHAPE.
 *   The decode kernels cut the seqlen_q x (h / h_k) packed query rows of a KV head into tiles of 16, and every tile streams the visible K / V
 *   of its head on its own: right for decode, wrong for a chunk of a prompt (a 2048-token chunk at h / h_k = 4 is 512 tiles per KV head).  With
 *   row_tile = 64 the attention launch of the call uses kernels whose workgroup serves 64 packed rows of one (sequence, KV head, key split):
 *   four waves of 16 rows each walk the same 32-key steps, and the K / V rows of a step are loaded once per workgroup into LDS images all four
 *   read.  Everything in front (the append) and behind (the partial planes, the combine) is the existing code.  Each sequence is tiled on its
 *   own from its first packed row; the ragged grid has min(ceil(total_q * h_ratio / 64) + b, b * tiles64(max_seqlen_q)) slots per KV head.  The
 *   automatic key split is the existing rule evaluated with the wide grid's workgroup count; a forced num_splits cuts the keys where it cuts
 *   them with row_tile = 0; the workspace formula is unchanged.  Under is_causal a tile's key range ends at the last key its last row sees.
 *   Values: fp32 math over the visible keys, the tolerances of the 16-row path.  The bits may differ from row_tile = 0 (the summation order
 *   differs); no bit relation between the two is promised.  Bit for bit: paged == contiguous over the same logical cache; sequence i of a
 *   ragged row_tile = 64 call == the dense row_tile = 64 call on it alone, in o, lse and every cache byte, for num_splits = 1 and for any forced
 *   split (there is no window, so the cuts coincide); run-to-run determinism per split count.  Unchanged: a row that sees no key is o = 0,
 *   lse = 0; a NaN query row, or a NaN / +inf score, gives a NaN row; cache rows at or past L_i, packed rows past cu_seqlens_q[b] and table
 *   entries of pages wholly past L_i never reach a result; a non-finite V element within the 16 keys of an MFMA block that another row of the
 *   tile sees can make a row NaN that does not see it (0 x NaN), as with row_tile = 0.  row_tile applies to the whole call: a decoding
 *   sequence in such a call fills 4 of 64 rows at h / h_k = 4.  Choosing the tile automatically is out of scope.
 * Supported with row_tile = 64: dense and cu_seqlens_q calls, contiguous and paged caches, the 8-bit cache with descales (read and append side),
 * k_new / v_new, is_causal, GQA / MQA, fp16 / bf16, d = 64 / 128, softmax_scale, num_splits; no host synchronisation (lengths, tables, descales
 * and cu_seqlens are read on the device: a captured call replays with the values then in memory).
 * Not supported, FA_ERR_BAD_SHAPE with the field named by fa_last_error: row_tile = 64 together with a window other than (-1, -1), with
 * softcap > 0, with sinks, with tree_mask, with rotary_cos / rotary_sin, and at d = 256.  A non-zero `reserved4_` / `reserved4` is
 * FA_ERR_BAD_ABI (a newer caller's field this library does not know).  Errors of fa_kvcache_params and of the older option fields come first,
 * then those of row_tile, then the reserved words.
 * sizeof is 288: the sizes 241 .. 280 and 1024 are pinned as FA_ERR_BAD_ABI by callers' tests of the v7 library, and 288 is the next multiple
 * of 8 that clears them; the reserved words are the room that leaves. */
#define FA_HAS_KVCACHE_PREFILL 1
typedef struct fa_kvcache_options_v8 {      /* FA_PARAMS_INIT(o); then fa_..._ex(&p, (const fa_kvcache_options*)&o, ...) */
    uint32_t struct_size;       /* sizeof(fa_kvcache_options_v8) */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t is_local;           /* the fields of fa_kvcache_options_v7, same offsets */
    int32_t window_size_left;
    int32_t window_size_right;
    int32_t cache_dtype;
    const float* k_descale;
    const float* v_descale;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    const void* rotary_cos;
    const void* rotary_sin;
    int64_t rotary_row_stride;
    int32_t seqlen_ro;
    int32_t rotary_dim;
    int32_t rotary_interleaved;
    int32_t reserved_;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k_new;
    int64_t total_q;
    int64_t total_k_new;
    float softmax_scale;
    float softcap;
    int64_t reserved[2];        /* 0 */
    const float* sinks;
    int64_t sinks_stride;
    int64_t reserved2[2];       /* 0 */
    const int64_t* tree_mask;
    int64_t tree_mask_batch_stride, tree_mask_row_stride;
    int64_t reserved3[2];       /* 0 */
    int32_t row_tile;           /* optional: 0 = the 16-row kernels, 64 = the 64-row kernels for prompt chunks */
    int32_t reserved4_;         /* 0 */
    int64_t reserved4[5];       /* 0 */
} fa_kvcache_options_v8;

/* Multi-head latent attention (MLA) decode over a latent KV cache (FA_HAS_MLA_KVCACHE; DeepSeek-V2 / V3 / R1, Kimi K2; the FlashMLA call).  After
 * weight absorption a decode step is MQA over ONE KV head whose key is the d_qk = 576 wide latent row (512 compressed-KV elements, then 64 rope
 * elements, RoPE already applied) and whose value is the first d_v = 512 elements of the SAME row.  FA_ABI_VERSION is unchanged; the presence of
 * fa_run_mla_fwd_kvcache is how a caller detects the feature.  The struct is versioned by its size (FA_PARAMS_INIT): every field below is
 * mandatory in this version, fields appended later will be optional.
 *   q (b, seqlen_q, h, 576), seqlen_q >= 1, h >= 1; kv_cache (b, seqlen_cache, 576) with batch and row strides (its head stride is not read), or with
 *   block_table a pool (num_blocks, page_block_size, 576) exactly as in fa_kvcache_params: page_block_size a positive multiple of 16, seqlen_cache the
 *   per-sequence capacity and a multiple of it, entries clamped min((uint32_t)entry, num_blocks - 1);
 *   cache_seqlens: int32 DEVICE array (b,), or NULL = every sequence is seqlen_cache long;
 *   kv_new (b, seqlen_new, 576) or NULL: written IN PLACE at rows cache_seqlens[i] .. + seqlen_new - 1 (cache_seqlens is required then and is not
 *   updated; rows at or past seqlen_cache are dropped), after which L_i = cache_seqlens[i] + seqlen_new; without it L_i = cache_seqlens[i];
 *   o (b, seqlen_q, h, 512), lse (b, h, seqlen_q) fp32 natural log.
 * In fp32 math over the visible keys: s_tj = (q_t . kv_j[0:576]) * softmax_scale; key j is visible iff j < L_i and, under is_causal,
 * j <= L_i - seqlen_q + t; o_t = softmax_j(s_tj) @ kv_j[0:512]; a row that sees no key is o = 0, lse = 0; a NaN query row, or a NaN / +inf
 * score, gives a NaN row.  softmax_scale: finite and > 0, or 0 = the default 576 ** -0.5 (models pass their own, e.g. 192 ** -0.5 * mscale).
 * workspace / num_splits as in fa_kvcache_params: fa_mla_workspace_bytes states n_split x rows x 512 x 4 + align16(n_split x rows x 4) bytes
 * with rows = b * h * seqlen_q; the automatic split is the rule of fa_kvcache_num_splits over this grid's b x ceil(seqlen_q * h / 64) workgroups.
 * No host synchronisation; paged == contiguous over the same logical cache bit for bit; deterministic per split count; rows at or past L_i,
 * pages wholly past L_i and pages no sequence references never reach a result.
 * Errors, the argument named by fa_last_error: d_qk != 576 or d_v != 512 FA_ERR_BAD_HEADDIM, dtype FA_ERR_BAD_DTYPE, sizes / page_block_size /
 * softmax_scale / num_splits FA_ERR_BAD_SHAPE, pointers FA_ERR_NULL_POINTER, strides and alignment FA_ERR_BAD_STRIDE, the header FA_ERR_BAD_ABI.
 * b == 0 is FA_OK without a launch.  No window, softcap, sinks, tree mask, rotary or ragged batch: the struct has no field for them.  An FP8 latent
 * cache is fa_mla_params_v2 below. */
#define FA_HAS_MLA_KVCACHE 1
typedef struct fa_mla_params {
    uint32_t struct_size;       /* sizeof(fa_mla_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    void* kv_cache;
    const void* kv_new;         /* NULL: no append */
    void* o;
    float* lse;
    const int32_t* cache_seqlens;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t seqlen_new;         /* rows of kv_new (0 without it) */
    int32_t h;
    int32_t d_qk;               /* 576 */
    int32_t d_v;                /* 512 */
    int32_t dtype;
    int32_t is_causal;
    int32_t num_splits;         /* 0 = the library's choice */
    float softmax_scale;        /* 0 = 576 ** -0.5 */
    int32_t reserved_;          /* 0 */
    fa_strides q_stride, kv_cache_stride, kv_new_stride, o_stride;     /* kv_cache_stride.head / kv_new_stride.head are not read */
    void* workspace;
    int64_t workspace_bytes;
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int64_t block_table_stride;
    int32_t page_block_size;
    int32_t num_blocks;
} fa_mla_params;

/* Sparse MLA decode over a latent KV cache (FA_HAS_MLA_SPARSE_KVCACHE; DeepSeek-V3.2 "DeepSeek Sparse Attention"; FlashMLA's sparse call).  The cache, q, o
 * and lse are those of fa_mla_params above; in place of every key below L_i, query token t of sequence i attends to the rows its list names:
 *   indices: int32 DEVICE array, entry (i, t, s) at indices[i * indices_batch_stride + t * indices_row_stride + s], s < topk (strides in elements, the last
 *   dim contiguous); topk a positive multiple of 32 (callers pad with -1).  An entry is a LOGICAL key position of sequence i (it goes through block_table
 *   when the cache is paged) and belongs to the token: all h heads share it.
 * With L_i = min(max(cache_seqlens[i], 0), seqlen_cache) (cache_seqlens NULL: seqlen_cache), slot s of row (i, t) is valid iff 0 <= entry < L_i.  The
 * valid slots form a multiset (a position listed twice counts twice).  In fp32 math: s_ts = (q_t . kv[entry][0:576]) * softmax_scale,
 * o_t = softmax over the valid slots @ kv[entry][0:512], lse the natural-log logsumexp over them; a row without a valid slot is o = 0, lse = 0.  There is
 * no is_causal: the list is the mask.  An invalid entry of any value (-1, >= L_i, INT32_MIN, INT32_MAX) reads nothing and contributes exactly nothing;
 * cache rows, pages and table entries that no valid slot names are never read.  A NaN query row, or a NaN / +inf score of a valid slot, gives NaN rows for
 * that token and no other.  No host synchronisation (indices, lengths and tables are read on the device); paged == contiguous bit for bit; deterministic per
 * split count.  The list 0 .. n - 1 followed by -1 gives the bits of fa_run_mla_fwd_kvcache without is_causal at cache_seqlens = n for one split (and for a
 * forced num_splits when topk == seqlen_cache).
 * workspace / num_splits as in fa_mla_params: fa_mla_sparse_workspace_bytes states n_split x rows x 512 x 4 + align16(n_split x rows x 4) bytes with
 * rows = b * h * seqlen_q; the split runs over the slots [0, topk) in multiples of 32 (a forced count is at most topk / 32), the automatic one by the rule
 * of fa_kvcache_num_splits with topk in the place of seqlen_cache over this grid's b x seqlen_q x ceil(h / 64) workgroups.
 * Errors as for fa_mla_params; indices NULL (b > 0) FA_ERR_NULL_POINTER, topk / the index strides FA_ERR_BAD_SHAPE / FA_ERR_BAD_STRIDE naming them.
 * b == 0 is FA_OK without a launch.  No kv_new, ragged batch, sinks or physical (pool-wide) indices: the struct has no field for them.  An FP8 latent
 * cache is fa_mla_sparse_params_v2 below. */
#define FA_HAS_MLA_SPARSE_KVCACHE 1
typedef struct fa_mla_sparse_params {
    uint32_t struct_size;       /* sizeof(fa_mla_sparse_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    const void* kv_cache;
    void* o;
    float* lse;
    const int32_t* cache_seqlens;
    const int32_t* indices;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t topk;               /* a positive multiple of 32 */
    int32_t h;
    int32_t d_qk;               /* 576 */
    int32_t d_v;                /* 512 */
    int32_t dtype;
    int32_t num_splits;         /* 0 = the library's choice */
    float softmax_scale;        /* 0 = 576 ** -0.5 */
    int64_t reserved_;          /* 0 */
    fa_strides q_stride, kv_cache_stride, o_stride;     /* kv_cache_stride.head is not read */
    int64_t indices_batch_stride;
    int64_t indices_row_stride;
    void* workspace;
    int64_t workspace_bytes;
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int64_t block_table_stride;
    int32_t page_block_size;
    int32_t num_blocks;
} fa_mla_sparse_params;

/* FP8 latent cache for both MLA calls (FA_HAS_MLA_FP8_KVCACHE; the cache of DeepSeek-V3.2 / FlashMLA's sparse decode, vLLM's fp8_ds_mla).  The _v2 structs
 * are fa_mla_params / fa_mla_sparse_params with kv_format appended; the same entry points take either struct through the same pointer and tell them apart
 * by struct_size (any other size stays FA_ERR_BAD_ABI).  FA_ABI_VERSION is unchanged.
 * kv_format = FA_MLA_KV_16BIT: exactly the call of the first struct.  kv_format = FA_MLA_KV_FP8_ROWS656: kv_cache holds 656-byte latent rows and
 * kv_cache_stride is in BYTES (batch / page and row strides and the pointer multiples of 16, row >= 656; the head stride is not read):
 *   bytes 0 .. 511    code[c], OCP e4m3 (float8_e4m3fn), columns 0 .. 511 of the latent row
 *   bytes 512 .. 527  scale[g], four fp32 (little endian), g = c / 128
 *   bytes 528 .. 655  columns 512 .. 575 (the rope part), 64 elements of `dtype`, unscaled
 * The row means kv[c] = round_to_dtype(fp32(code[c]) * scale[c / 128]) for c < 512 - the fp32 product rounded once, to nearest-even - and kv[512 + r] =
 * the stored rope element; everything else is the contract of the 16-bit call over kv, and the two calls agree BIT FOR BIT: a call on an FP8 cache
 * equals the 16-bit call on the dequantised cache in o and lse for every split count.  A NaN code (0x7f / 0xff) is NaN.  Scales are used as they are and
 * are not checked; precondition: every fp32(code) * scale is zero or a normal fp32 number (for fp16 a product beyond 65504 becomes inf by the rounding).
 * Rows at or past L_i, pages wholly past L_i or unreferenced and (sparse) whatever no valid slot names are never read: they may hold 0xff bytes.
 * kv_new (dense call) stays (b, seqlen_new, 576) of `dtype` with kv_new_stride in elements and is QUANTISED into whole 656-byte rows, drop and clamp rules
 * unchanged; attention runs over the quantised rows.  Per tile g of a new row: amax_g = max |x_c| over the tile's finite elements (0 if none),
 * scale_g = max(amax_g, 2^-24) / 448 (the correctly rounded fp32 quotient), code[c] = e4m3_rne(clamp(float(x_c) / scale_g, -448, 448)) with NaN kept
 * (0x7f | sign) and +-inf saturating; the rope part is copied bit for bit.
 * Workspace and split are those of kv_format = 0.  Errors: an unknown kv_format or a non-zero reserved2_ FA_ERR_BAD_SHAPE naming the field; a stride or
 * pointer of the FP8 cache that is no multiple of 16 bytes FA_ERR_BAD_STRIDE. */
#define FA_HAS_MLA_FP8_KVCACHE 1
#define FA_MLA_KV_16BIT 0
#define FA_MLA_KV_FP8_ROWS656 1
typedef struct fa_mla_params_v2 {
    uint32_t struct_size;       /* sizeof(fa_mla_params_v2) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    void* kv_cache;
    const void* kv_new;
    void* o;
    float* lse;
    const int32_t* cache_seqlens;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t seqlen_new;
    int32_t h;
    int32_t d_qk;
    int32_t d_v;
    int32_t dtype;
    int32_t is_causal;
    int32_t num_splits;
    float softmax_scale;
    int32_t reserved_;
    fa_strides q_stride, kv_cache_stride, kv_new_stride, o_stride;
    void* workspace;
    int64_t workspace_bytes;
    const int32_t* block_table;
    int64_t block_table_stride;
    int32_t page_block_size;
    int32_t num_blocks;
    int32_t kv_format;          /* FA_MLA_KV_16BIT / FA_MLA_KV_FP8_ROWS656 */
    int32_t reserved2_;         /* 0 */
} fa_mla_params_v2;

typedef struct fa_mla_sparse_params_v2 {
    uint32_t struct_size;       /* sizeof(fa_mla_sparse_params_v2) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    const void* kv_cache;
    void* o;
    float* lse;
    const int32_t* cache_seqlens;
    const int32_t* indices;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t topk;
    int32_t h;
    int32_t d_qk;
    int32_t d_v;
    int32_t dtype;
    int32_t num_splits;
    float softmax_scale;
    int64_t reserved_;
    fa_strides q_stride, kv_cache_stride, o_stride;
    int64_t indices_batch_stride;
    int64_t indices_row_stride;
    void* workspace;
    int64_t workspace_bytes;
    const int32_t* block_table;
    int64_t block_table_stride;
    int32_t page_block_size;
    int32_t num_blocks;
    int32_t kv_format;          /* FA_MLA_KV_16BIT / FA_MLA_KV_FP8_ROWS656 */
    int32_t reserved2_;         /* 0 */
} fa_mla_sparse_params_v2;

/* The DeepSeek-V3.2 indexer in front of sparse MLA decode (FA_HAS_MLA_INDEXER): index logits over an index-key cache, and the top-k selection that
 * turns them into the `indices` of fa_mla_sparse_params.  Two launches, two structs; both carry the {struct_size, magic} header, struct_size must be
 * the struct's own size.  FA_ABI_VERSION is unchanged.
 * Visibility, shared by both: L_i = min(max(cache_seqlens[i], 0), seqlen_cache) (cache_seqlens NULL: seqlen_cache); token t of sequence i sees the
 * keys j < n_t, n_t = L_i without is_causal, else min(L_i, max(L_i - seqlen_q + t + 1, 0)): the rule of fa_mla_params.
 * fa_mla_indexer_params.  q_idx (b, seqlen_q, h, 128) of `dtype`, h 16, 32 or 64, strides in elements (multiples of 8, pointer 16-byte aligned);
 * weights fp32 (b, seqlen_q, h), any strides in elements; k_idx_cache (b, seqlen_cache, 128) - k_cache_batch_stride / k_cache_row_stride - or, with
 * block_table, a pool (num_blocks, page_block_size, 128) whose page stride is k_cache_batch_stride, entries clamped min(uint32(entry), num_blocks - 1).
 * k_format FA_MLA_KV_16BIT: elements of `dtype`, strides in elements, multiples of 8.  k_format FA_IDX_K_FP8_E4M3: OCP e4m3 codes, strides in BYTES,
 * multiples of 16; pointer 16-byte aligned either way; one sequence (one page) spans less than 2^31 bytes.  k_scale: NULL (= 1.0) or one fp32 per
 * cached token at k_scale[i * k_scale_batch_stride + j * k_scale_row_stride] (a page in the place of i when paged), strides in elements, any value.
 * In fp32 math, for j < n_t:  logit[i, t, j] = k_scale[j] * sum_h weights[t, h] * relu(q_idx[t, h, :] . k[j, :]),  relu(x) = x > 0 ? x : 0, written to
 * logits[i * logits_batch_stride + t * logits_row_stride + j] (strides in elements, 64-bit offsets).  An entry at j >= n_t is never written; cache rows
 * and scales at or past L_i, pages wholly past L_i and pages no sequence references are never read.  FP8 codes are widened exactly and multiplied in
 * `dtype`; nothing is quantised.  Non-finite inputs have no value contract.  No host synchronisation; paged == contiguous bit for bit; deterministic.
 * fa_mla_topk_params.  logits as written above (seqlen_cache = its last dimension); indices int32 (b, seqlen_q, topk) contiguous, topk a positive
 * multiple of 32.  fp32 values are ordered by u(x) = bits(x) ^ (bits(x) >> 31 ? 0xffffffff : 0x80000000).  Row (i, t): n_t <= topk gives 0, 1, ..,
 * n_t - 1 followed by -1; otherwise the topk positions below n_t with the largest keys, ties at the threshold to the lower positions, in ascending
 * position order.  Entries at j >= n_t are never read.  Exact and deterministic: what fa_run_mla_sparse_fwd_kvcache takes as it is.
 * Errors name the field: NULL pointers FA_ERR_NULL_POINTER, h / d FA_ERR_BAD_HEADDIM, dtype / k_format FA_ERR_BAD_DTYPE, sizes, topk, paging and
 * non-zero reserved words FA_ERR_BAD_SHAPE, strides and alignment FA_ERR_BAD_STRIDE, the header FA_ERR_BAD_ABI.  b == 0 is FA_OK without a launch. */
#define FA_HAS_MLA_INDEXER 1
#define FA_IDX_K_FP8_E4M3 1
typedef struct fa_mla_indexer_params {
    uint32_t struct_size;       /* sizeof(fa_mla_indexer_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q_idx;
    const float* weights;
    const void* k_idx_cache;
    const float* k_scale;       /* NULL = 1.0 */
    float* logits;
    const int32_t* cache_seqlens;
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t h;                  /* 16, 32 or 64 */
    int32_t d;                  /* 128 */
    int32_t dtype;
    int32_t k_format;           /* FA_MLA_KV_16BIT / FA_IDX_K_FP8_E4M3 */
    int32_t is_causal;
    int32_t page_block_size;
    int32_t num_blocks;
    int64_t reserved_;          /* 0 */
    fa_strides q_idx_stride, weights_stride;
    int64_t k_cache_batch_stride;
    int64_t k_cache_row_stride;
    int64_t k_scale_batch_stride;
    int64_t k_scale_row_stride;
    int64_t logits_batch_stride;
    int64_t logits_row_stride;
    int64_t block_table_stride;
} fa_mla_indexer_params;

typedef struct fa_mla_topk_params {
    uint32_t struct_size;       /* sizeof(fa_mla_topk_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const float* logits;
    int32_t* indices;
    const int32_t* cache_seqlens;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t topk;               /* a positive multiple of 32 */
    int32_t is_causal;
    int32_t reserved_;          /* 0 */
    int64_t logits_batch_stride;
    int64_t logits_row_stride;
} fa_mla_topk_params;

/* Index logits for a prompt chunk (FA_HAS_MLA_INDEXER_PREFILL; fp8_mqa_logits next to fp8_paged_mqa_logits in DeepGEMM).  fa_run_mla_indexer_prefill_logits
 * takes the fa_mla_indexer_params of fa_run_mla_indexer_logits - the same struct, the same checks, the same errors - and writes exactly the entries
 * that call writes, with the same bits (but for a NaN key below L_i, which gives NaN in its column here and 0 there): a workgroup serves a tile of several consecutive tokens of one sequence and stages each 32-key step once for
 * all of them, where fa_run_mla_indexer_logits gives a workgroup one token (right for seqlen_q = 1).  Entries at j >= n_t are never written; cache rows
 * and scales at or past L_i, pages wholly past L_i, pages no sequence references and keys at or past the n_t of a tile's last token are never read.  One
 * launch, no workspace, no atomics, no host synchronisation, deterministic.  b == 0 is FA_OK without a launch.  FA_ABI_VERSION is unchanged.
 * fa_mla_indexer_prefill_launch says on the host what that launch would use. */
#define FA_HAS_MLA_INDEXER_PREFILL 1

/* FP8 (e4m3) index queries (FA_HAS_MLA_INDEXER_FP8_Q; both sides of DeepGEMM's fp8_paged_mqa_logits / fp8_mqa_logits).  fa_mla_indexer_params_v2 is
 * fa_mla_indexer_params with q_format appended.  It goes to three entry points of its own, fa_run_mla_indexer_logits_v2, fa_run_mla_indexer_prefill_logits_v2
 * and fa_mla_indexer_prefill_launch_v2, which take either struct through their pointer and tell them apart by struct_size (any other size is FA_ERR_BAD_ABI).
 * The entry points without _v2 keep accepting the 216-byte struct alone, with their errors: a struct_size of 224 there stays FA_ERR_BAD_ABI, because a
 * 216-byte struct mislabelled by 8 bytes cannot be told from a _v2 and would be read past its end.  FA_ABI_VERSION is unchanged.
 * q_format = FA_IDX_Q_16BIT: exactly the call of the first struct.  q_format = FA_IDX_Q_FP8_E4M3: q_idx holds OCP e4m3 codes, q_idx_stride counts BYTES
 * (multiples of 16, pointer 16-byte aligned), k_format must be FA_IDX_K_FP8_E4M3, and `dtype` must still be a valid value but is not used.  The scale of the
 * quantised queries, one per (token, head), is the caller's: fold it into weights.  For j < n_t:
 *   logit[i, t, j] = k_scale[j] * sum_h weights[t, h] * relu(sum_d float(qcode[t, h, d]) * float(kcode[j, d]))
 * on v_mfma_f32_16x16x128_f8f6f4: every product is exact in fp32, the 128-term sum is the instruction's; relu is the IEEE 754-2019 maximum in both calls (a NaN
 * code gives NaN), so the prefill call writes the entries of the decode call with the same bits for every input.  Visibility, what is never read or written,
 * paging, determinism and the launch rule reported by fa_mla_indexer_prefill_launch are those of the first struct.
 * Errors: an unknown q_format FA_ERR_BAD_DTYPE naming q_format; q_format = 1 with another k_format FA_ERR_BAD_DTYPE naming k_format; a non-zero reserved2_
 * FA_ERR_BAD_SHAPE naming it; a q_idx stride or pointer that is no multiple of 16 bytes FA_ERR_BAD_STRIDE. */
#define FA_HAS_MLA_INDEXER_FP8_Q 1
#define FA_IDX_Q_16BIT 0
#define FA_IDX_Q_FP8_E4M3 1
typedef struct fa_mla_indexer_params_v2 {
    uint32_t struct_size;       /* sizeof(fa_mla_indexer_params_v2) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q_idx;
    const float* weights;
    const void* k_idx_cache;
    const float* k_scale;       /* NULL = 1.0 */
    float* logits;
    const int32_t* cache_seqlens;
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_cache;
    int32_t h;                  /* 16, 32 or 64 */
    int32_t d;                  /* 128 */
    int32_t dtype;
    int32_t k_format;           /* FA_MLA_KV_16BIT / FA_IDX_K_FP8_E4M3 */
    int32_t is_causal;
    int32_t page_block_size;
    int32_t num_blocks;
    int64_t reserved_;          /* 0 */
    fa_strides q_idx_stride, weights_stride;
    int64_t k_cache_batch_stride;
    int64_t k_cache_row_stride;
    int64_t k_scale_batch_stride;
    int64_t k_scale_row_stride;
    int64_t logits_batch_stride;
    int64_t logits_row_stride;
    int64_t block_table_stride;
    int32_t q_format;           /* FA_IDX_Q_16BIT / FA_IDX_Q_FP8_E4M3 */
    int32_t reserved2_;         /* 0 */
} fa_mla_indexer_params_v2;

/* MLA prefill attention (FA_HAS_MLA_PREFILL; DeepSeek-V2 / V3 / R1, Kimi K2 before weight absorption; the (192, 128) forward of flash-attn and FlashMLA).
 * Ordinary multi-head attention with d_qk = 192 wide queries and keys (128 no-rope columns, then 64 rope columns, RoPE already applied) and d_v = 128
 * wide values.  FA_ABI_VERSION is unchanged; the presence of fa_run_mla_prefill_fwd is how a caller detects the feature.  struct_size must be
 * sizeof(fa_mla_prefill_params) (FA_PARAMS_INIT).
 *   dense (cu_seqlens_q = cu_seqlens_k = NULL): q (b, seqlen_q, h, 192), k (b, seqlen_k, h_k, 192), v (b, seqlen_k, h_k, 128), o (b, seqlen_q, h, 128),
 *   lse (b, h, seqlen_q) fp32; total_q / total_k are not read.
 *   packed (both cu_seqlens given: int32 DEVICE arrays (b + 1,), non-decreasing from a value >= 0): q (total_q, h, 192), k (total_k, h_k, 192), v (total_k,
 *   h_k, 128), o (total_q, h, 128), lse (h, total_q); sequence i owns rows cu_seqlens_q[i] .. cu_seqlens_q[i + 1] - 1 of q / o and cu_seqlens_k[i] ..
 *   cu_seqlens_k[i + 1] - 1 of k / v; seqlen_q / seqlen_k and the batch strides are not read; the launch is sized from total_q.  Rows of o / lse at or
 *   past cu_seqlens_q[b] are left untouched; rows of k / v at or past cu_seqlens_k[b], or of another sequence, never reach a result.
 *   h % h_k == 0 (GQA / MQA); strides in elements, multiples of 8, row strides at least the row widths, pointers 16-byte aligned; one sequence (packed: the
 *   whole tensor, as no max_seqlen is stated) spans less than 2^31 bytes, the limit and the error of fa_fwd_params.
 * In fp32 math over the visible keys, per sequence with sq_i query rows and sk_i keys: s_tj = (q_t . k_j) * softmax_scale; key j is visible to row t iff
 * j < sk_i and, under is_causal, j <= sk_i - sq_i + t (bottom-right aligned); o_t = softmax_j(s_tj) @ v_j; lse the natural-log logsumexp.  A row that sees no
 * key (sq_i > sk_i under is_causal, sk_i = 0) is o = 0, lse = 0; empty query sequences are allowed.  A NaN in a query row, or a NaN / +inf score, gives a NaN
 * row; a -inf score only drops the key.  softmax_scale: finite and > 0, or 0 = the default 192 ** -0.5.
 * One launch on `stream`, no workspace (there is no key split), no host synchronisation, deterministic.  Sequence i of a packed call equals the dense call
 * on that sequence alone bit for bit, and so does a batch entry of a dense call.
 * Errors, the argument named by fa_last_error: d_qk != 192 or d_v != 128 FA_ERR_BAD_HEADDIM, h % h_k FA_ERR_BAD_GQA, dtype FA_ERR_BAD_DTYPE, sizes /
 * total_q / total_k / softmax_scale FA_ERR_BAD_SHAPE, pointers (one cu_seqlens without the other included) FA_ERR_NULL_POINTER, strides and alignment
 * FA_ERR_BAD_STRIDE, the header FA_ERR_BAD_ABI.  b == 0 or no query row (total_q == 0; dense: seqlen_q == 0) is FA_OK without a launch.  The backward is
 * fa_run_mla_prefill_bwd (fa_mla_prefill_bwd_params below).  No FP8
 * or paged inputs, other widths, window, softcap or sinks: the struct has no field for them. */
#define FA_HAS_MLA_PREFILL 1
typedef struct fa_mla_prefill_params {
    uint32_t struct_size;       /* sizeof(fa_mla_prefill_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;
    const int32_t* cu_seqlens_q;    /* both NULL = dense */
    const int32_t* cu_seqlens_k;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_k;
    int32_t h;
    int32_t h_k;
    int32_t d_qk;               /* 192 */
    int32_t d_v;                /* 128 */
    int32_t dtype;
    int32_t is_causal;
    float softmax_scale;        /* 0 = 192 ** -0.5 */
    fa_strides q_stride, k_stride, v_stride, o_stride;     /* packed: the batch strides are not read */
    int64_t total_q;            /* packed: rows of q / o */
    int64_t total_k;            /* packed: rows of k / v */
} fa_mla_prefill_params;

/* The backward of MLA prefill attention (FA_HAS_MLA_PREFILL_BWD): dq (192 wide), dk (192 wide) and dv (128 wide) from dout, q, k, v and the forward's o
 * and lse.  FA_ABI_VERSION is unchanged; the presence of fa_run_mla_prefill_bwd is how a caller detects the feature.  struct_size must be
 * sizeof(fa_mla_prefill_bwd_params) (FA_PARAMS_INIT).  The fields of fa_mla_prefill_params with the same meaning, dense or packed, plus:
 *   o, lse          the forward's outputs (read); lse fp32, (b, h, seqlen_q) dense or (h, total_q) packed
 *   dout            the gradient of o, shaped like o, with strides of its own
 *   dq, dk, dv      outputs shaped like q, k, v, with strides of their own
 *   dsoftmax_sum    fp32, the layout of lse: D_t = sum_c dout_tc * o_tc, WRITTEN by the first launch and read by the second (the only workspace)
 *   phases          0 = the call (both launches); FA_MLA_PREFILL_BWD_DQ (1) / _DKDV (2) = only that launch, any other value is refused (measurements; _DKDV reads the dsoftmax_sum an earlier _DQ call left)
 * In fp32 math over the visible pairs (visibility exactly the forward's): P_tj = exp(s_tj - lse_t), exactly 0 on hidden pairs (selected to 0: whatever the exponential gives there is discarded);
 * dP_tj = dout_t . v_j; dS = P (dP - D); dq_t = softmax_scale * sum_j dS_tj k_j; dk_j = softmax_scale * sum over the h / h_k heads of the group and t of
 * dS_tj q_t; dv_j = sum over the group and t of P_tj dout_t.  Accumulated in fp32, each output rounded once; P and dS are rounded to dtype in front of their
 * second matrix products.  A row the forward gave o = 0, lse = 0 (it sees no key) gets dq = 0, written; a key no row sees gets dk = dv = 0, written; empty
 * sequences on either side are allowed.  Packed rows of dq at or past cu_seqlens_q[b] and of dk / dv at or past cu_seqlens_k[b] keep the caller's bytes.
 * Two launches on `stream` (dq, then dk / dv), no atomics, no key or head split, no host synchronisation, deterministic; one workgroup owns an output row
 * from start to end.  Sequence i of a packed call equals the dense call on it alone bit for bit, and so does a batch entry of a dense call.  Non-finite
 * inputs have no value contract (as for fa_run_mha_bwd) but never change which addresses are touched.
 * Errors as for the forward, the argument named by fa_last_error.  b == 0 or no query row is FA_OK without a launch (dk / dv are not touched); with query
 * rows but no key anywhere dq is zeroed.  Out of scope: a head-group or key split with a workspace, other widths, window / softcap / sinks, FP8 or paged
 * inputs, a fused single-kernel backward. */
#define FA_HAS_MLA_PREFILL_BWD 1
#define FA_MLA_PREFILL_BWD_DQ 1
#define FA_MLA_PREFILL_BWD_DKDV 2
typedef struct fa_mla_prefill_bwd_params {
    uint32_t struct_size;       /* sizeof(fa_mla_prefill_bwd_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* q;
    const void* k;
    const void* v;
    const void* o;
    const float* lse;
    const void* dout;
    void* dq;
    void* dk;
    void* dv;
    float* dsoftmax_sum;
    const int32_t* cu_seqlens_q;    /* both NULL = dense */
    const int32_t* cu_seqlens_k;
    int32_t b;
    int32_t seqlen_q;
    int32_t seqlen_k;
    int32_t h;
    int32_t h_k;
    int32_t d_qk;               /* 192 */
    int32_t d_v;                /* 128 */
    int32_t dtype;
    int32_t is_causal;
    float softmax_scale;        /* 0 = 192 ** -0.5 */
    int32_t phases;             /* 0 = both launches */
    int32_t reserved_;          /* 0 */
    fa_strides q_stride, k_stride, v_stride, o_stride, dout_stride, dq_stride, dk_stride, dv_stride;     /* packed: the batch strides are not read */
    int64_t total_q;            /* packed: rows of q / o / dout / dq */
    int64_t total_k;            /* packed: rows of k / v / dk / dv */
} fa_mla_prefill_bwd_params;

/* Merging attention states (FA_HAS_MERGE_STATES; merge_attn_states of vLLM, merge_state of FlashInfer): every attention call of this library returns
 * (o, lse), and n_parts such results over DISJOINT key sets of the same query rows combine into the result over the union.  FA_ABI_VERSION is unchanged; the
 * presence of fa_run_merge_states is how a caller detects the feature.  struct_size must be sizeof(fa_merge_params) (FA_PARAMS_INIT).
 *   o[i]            part i, (b, rows, h, d_v) of `dtype`, last dimension contiguous, with o_stride[i] (batch / row / head, elements, multiples of 8) of its
 *                   own and a 16-byte aligned base; 2 <= n_parts <= FA_MERGE_MAX_PARTS, entries at or past n_parts are not read
 *   lse[i]          fp32, entry (batch, head, row) at lse[i][batch * lse_stride[i].batch + head * lse_stride[i].head + row * lse_stride[i].row]: strides in
 *                   elements, ANY values.  One form covers the dense (b, h, rows) layout, the packed (h, total) layout (b = 1) and the LSE (1, h, b * rows)
 *                   of a call that took the b * rows query rows as one sequence (batch stride = rows, head stride = b * rows, row stride = 1)
 *   out, lse_out    the results, shaped and addressed like the parts, with out_stride / lse_out_stride of their own
 *   d_v             64, 128, 256 or 512
 * In fp32 over the NON-EMPTY parts of a (row, head), in argument order: m = max_i lse_i, w_i = exp(lse_i - m), out = (sum_i w_i o_i) / (sum_i w_i) rounded
 * once to dtype, lse_out = m + log(sum_i w_i).
 * EMPTY, the one rule: part i is empty for a (row, head) iff lse_i is -inf, or lse_i is +-0 and every element of that o_i row is +-0.  The second form is
 * what every attention call of this library returns for a row that sees no key.  (A live row can look like that only when its scores sum to exactly one
 * and its V rows are all zero: it is then taken as empty.)  An empty part contributes nothing; all parts empty gives out = 0, lse_out = 0 - the dead row
 * again, so a merged state can feed another merge.  A part merged with empty parts comes back bit for bit, out and lse.  A NaN lse_i, or a NaN in a
 * non-empty part's row, makes that (row, head) NaN in out and lse_out, and no other.  lse_i = +inf has no contract.  Nothing at or past row b * rows, and
 * nothing between the rows, heads and batch entries the strides skip, is read or written.
 * One launch on `stream`, no workspace, no atomics, no host synchronisation, deterministic.  out must not overlap a part unless it is that part's very view.
 * Errors, the field named by fa_last_error: n_parts FA_ERR_BAD_SHAPE, d_v FA_ERR_BAD_HEADDIM, dtype FA_ERR_BAD_DTYPE, b / rows / h FA_ERR_BAD_SHAPE,
 * pointers FA_ERR_NULL_POINTER, strides and alignment FA_ERR_BAD_STRIDE, the header FA_ERR_BAD_ABI.  b * rows * h == 0 is FA_OK without a launch. */
#define FA_HAS_MERGE_STATES 1
#define FA_MERGE_MAX_PARTS 8
typedef struct fa_lse_strides {
    int64_t batch;
    int64_t head;
    int64_t row;
} fa_lse_strides;
typedef struct fa_merge_params {
    uint32_t struct_size;       /* sizeof(fa_merge_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    int32_t dtype;
    int32_t n_parts;            /* 2 .. FA_MERGE_MAX_PARTS */
    int32_t b;
    int32_t rows;
    int32_t h;
    int32_t d_v;                /* 64, 128, 256, 512 */
    const void* o[FA_MERGE_MAX_PARTS];
    fa_strides o_stride[FA_MERGE_MAX_PARTS];
    const float* lse[FA_MERGE_MAX_PARTS];
    fa_lse_strides lse_stride[FA_MERGE_MAX_PARTS];
    void* out;
    fa_strides out_stride;
    float* lse_out;
    fa_lse_strides lse_out_stride;
    void* stream;               /* the stream of fa_run_merge_states (hipStream_t; NULL = the default stream) */
} fa_merge_params;

/* Stand-alone append and gather for the MLA latent cache and the index-key cache (FA_HAS_MLA_CACHE_IO; concat_and_cache_mla and
 * gather_and_maybe_dequant_cache / cp_gather_and_upconvert_fp8_kv_cache of vLLM): the rows that fa_run_mla_fwd_kvcache, fa_run_mla_sparse_fwd_kvcache and
 * fa_run_mla_indexer_logits read, written and read back without an attention call.  FA_ABI_VERSION is unchanged.  Three structs with the {struct_size, magic}
 * header; struct_size must be the struct's own size.  One launch each on `stream`, no workspace, no host synchronisation: lengths, tables, cu_seqlens and starts
 * are read on the device.  The unit conventions are those of fa_mla_params_v2 / fa_mla_indexer_params: the strides of a 16-bit tensor count elements (multiples of
 * 8, pointer 16-byte aligned), those of an FP8 cache count BYTES (multiples of 16).
 * Rows.  Dense: (b, seqlen_new, ..) / (b, seqlen_out, ..) with batch and row strides.  Packed (cu_seqlens_* given, int32 (b + 1,)): total_* rows with the row
 * stride alone, rows cu[i] .. cu[i + 1] - 1 those of sequence i; rows at or past cu[b] are neither read nor written.
 * Placement (both appends): new row s of sequence i goes to logical row max(cache_seqlens[i], 0) + s, dropped at or past seqlen_cache; paged, to row (.) %
 * page_block_size of page min((uint32_t)block_table[i][(.) / page_block_size], num_blocks - 1): the rules of the append of fa_run_mla_fwd_kvcache.  Nothing is
 * written outside the cache / the pool, and every byte that is not a target row keeps its value.  The caller advances the lengths.
 * fa_mla_cache_append_params.  kv_new (.., 576) of `dtype`, or with k_pe: kv_new 512 wide and k_pe 64 wide with strides of its own, the row being their
 * concatenation.  kv_format FA_MLA_KV_16BIT: the 1152 bytes are copied.  FA_MLA_KV_FP8_ROWS656: the row is quantised by the rule stated with fa_mla_params_v2.
 * fa_mla_cache_gather_params.  out (.., 576) of `dtype`, last dimension contiguous.  Row r of sequence i is the cache row at logical position start_i + r,
 * start_i = max(seq_starts[i], 0) (NULL: 0).  L_i = min(max(cache_seqlens[i], 0), seqlen_cache) (NULL: seqlen_cache).  Below L_i: the row's 1152 bytes, or for
 * FP8 rows kv[c] = round_to_dtype(fp32(code[c]) * scale[c / 128]) and the stored rope elements - what the attention kernels compute with, bit for bit.  At or
 * past L_i: a row of +0, and neither the table nor the cache is read.  Rows at or past L_i, pages and table entries no requested row needs and pages no sequence
 * references are never read; out rows at or past cu_seqlens_out[b] and the gaps of a strided out are never written.
 * fa_mla_index_cache_append_params.  k_idx_new (.., 128) of `dtype` into the cache of fa_mla_indexer_params.  k_format FA_MLA_KV_16BIT: rows are copied, k_scale
 * must be NULL.  FA_IDX_K_FP8_E4M3: k_scale (strides in elements, any value) is required and takes one scale per token: amax = max |x| over the row's finite
 * elements (0 if none), scale = max(amax, 2^-24) / 448 (the correctly rounded fp32 quotient), under scale_format FA_IDX_SCALE_UE8M0 rounded up to a power of
 * two on its bits ((bits + 0x007fffff) & 0x7f800000); code = e4m3_rne(clamp(float(x) / scale, -448, 448)), NaN kept with its sign (0x7f / 0xff), +-inf
 * saturating.
 * Errors name the field: NULL pointers FA_ERR_NULL_POINTER, dtype / k_format / scale_format FA_ERR_BAD_DTYPE, sizes, totals, kv_format (as in
 * fa_mla_params_v2), paging, non-zero reserved words and a k_scale given with FA_MLA_KV_16BIT FA_ERR_BAD_SHAPE, strides and alignment FA_ERR_BAD_STRIDE, the
 * header FA_ERR_BAD_ABI.  b == 0 or no row to move is FA_OK without a launch. */
#define FA_HAS_MLA_CACHE_IO 1
#define FA_IDX_SCALE_FP32 0
#define FA_IDX_SCALE_UE8M0 1
typedef struct fa_mla_cache_append_params {
    uint32_t struct_size;       /* sizeof(fa_mla_cache_append_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    void* kv_cache;
    const void* kv_new;
    const void* k_pe;           /* NULL: kv_new is 576 wide */
    const int32_t* cache_seqlens;
    const int32_t* cu_seqlens_new;      /* NULL: dense */
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int32_t b;
    int32_t seqlen_new;         /* dense: new rows per sequence */
    int32_t seqlen_cache;
    int32_t dtype;
    int32_t kv_format;          /* FA_MLA_KV_16BIT / FA_MLA_KV_FP8_ROWS656 */
    int32_t page_block_size;
    int32_t num_blocks;
    int32_t reserved_;          /* 0 */
    int64_t total_new;          /* packed: rows of kv_new / k_pe */
    fa_strides kv_cache_stride, kv_new_stride, k_pe_stride;     /* head strides are not read */
    int64_t block_table_stride;
} fa_mla_cache_append_params;

typedef struct fa_mla_cache_gather_params {
    uint32_t struct_size;       /* sizeof(fa_mla_cache_gather_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    const void* kv_cache;
    void* out;
    const int32_t* cache_seqlens;       /* NULL = seqlen_cache */
    const int32_t* cu_seqlens_out;      /* NULL: dense */
    const int32_t* seq_starts;  /* NULL = 0 */
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int32_t b;
    int32_t seqlen_out;         /* dense: rows per sequence */
    int32_t seqlen_cache;
    int32_t dtype;              /* of out (and of a 16-bit cache) */
    int32_t kv_format;          /* FA_MLA_KV_16BIT / FA_MLA_KV_FP8_ROWS656 */
    int32_t page_block_size;
    int32_t num_blocks;
    int32_t reserved_;          /* 0 */
    int64_t total_out;          /* packed: rows of out */
    fa_strides kv_cache_stride; /* the head stride is not read */
    int64_t out_batch_stride;   /* elements; dense only */
    int64_t out_row_stride;     /* elements, a multiple of 8, >= 576 */
    int64_t block_table_stride;
} fa_mla_cache_gather_params;

typedef struct fa_mla_index_cache_append_params {
    uint32_t struct_size;       /* sizeof(fa_mla_index_cache_append_params) in the caller's translation unit */
    uint32_t magic;             /* FA_PARAMS_MAGIC */
    void* k_idx_cache;
    float* k_scale;             /* FA_IDX_K_FP8_E4M3: required; FA_MLA_KV_16BIT: NULL */
    const void* k_idx_new;
    const int32_t* cache_seqlens;
    const int32_t* cu_seqlens_new;      /* NULL: dense */
    const int32_t* block_table; /* paged cache; NULL = contiguous */
    int32_t b;
    int32_t seqlen_new;         /* dense: new rows per sequence */
    int32_t seqlen_cache;
    int32_t dtype;
    int32_t k_format;           /* FA_MLA_KV_16BIT / FA_IDX_K_FP8_E4M3 */
    int32_t scale_format;       /* FA_IDX_SCALE_FP32 / FA_IDX_SCALE_UE8M0 */
    int32_t page_block_size;
    int32_t num_blocks;
    int64_t total_new;          /* packed: rows of k_idx_new */
    int64_t reserved_;          /* 0 */
    int64_t k_cache_batch_stride;
    int64_t k_cache_row_stride;
    int64_t k_scale_batch_stride;
    int64_t k_scale_row_stride;
    int64_t k_new_batch_stride; /* elements; dense only */
    int64_t k_new_row_stride;   /* elements */
    int64_t block_table_stride;
} fa_mla_index_cache_append_params;

/* ---- library info ---------------------------------------------------------------------- */
int fa_abi_version(void);
const char* fa_last_error(void);
const char* fa_build_info(void);          /* e.g. "gfx950 hipcc ..." */

/* ---- param-struct entry points (replace run_mha_fwd / run_mha_bwd) ---------------------- */
int fa_run_mha_fwd(const fa_fwd_params* params, void* stream);
int fa_run_mha_bwd(const fa_bwd_params* params, void* stream);

/* ---- flat entry points for contiguous tensors (replace mha_fwd / mha_bwd / varlen_*) ---- */
/* q (b,sq,h,d), k/v (b,sk,hk,d), o (b,sq,h,d), lse (b,h,sq); all contiguous. */
int fa_mha_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
               int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t h_k, int32_t d,
               int32_t dtype, int32_t is_causal, void* stream);

int fa_mha_bwd(const void* q, const void* k, const void* v, const void* o, const float* lse,
               const void* dout, void* dq, void* dk, void* dv, float* dsoftmax_sum,
               int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t h_k, int32_t d,
               int32_t dtype, int32_t is_causal, void* stream);

/* q (total_q,h,d), k/v (total_k,hk,d) packed; lse (b,h,max_seqlen_q). */
int fa_mha_varlen_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                      const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                      int32_t b, int32_t max_seqlen_q, int32_t max_seqlen_k,
                      int32_t h, int32_t h_k, int32_t d,
                      int32_t dtype, int32_t is_causal, void* stream);

int fa_mha_varlen_bwd(const void* q, const void* k, const void* v, const void* o, const float* lse,
                      const void* dout, void* dq, void* dk, void* dv, float* dsoftmax_sum,
                      const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                      int32_t b, int32_t max_seqlen_q, int32_t max_seqlen_k,
                      int32_t h, int32_t h_k, int32_t d,
                      int32_t dtype, int32_t is_causal, void* stream);

/* D = rowsum(dO * O) alone (replaces flash_bwd_dot_do_o_kernel, flash_bwd_preprocess_kernel.h:23-96): the one HBM-bound kernel of
 * the reference's path.  Since round 2 fa_run_mha_bwd no longer launches it (the dQ kernel computes D in its prologue); it stays as a
 * stand-alone entry point and is measured separately. */
int fa_bwd_dot_do_o(const fa_bwd_params* params, void* stream);
/* The other two launches of run_flash_bwd, individually (flash_bwd_launch_template.h:95-146): dQ and dK/dV.  fa_bwd_dq computes D for
 * its rows itself (from O and dO) and WRITES params->dsoftmax_sum; fa_bwd_dkdv READS it, i.e. fa_bwd_dq (or fa_bwd_dot_do_o) must
 * have run on the same stream before.  fa_run_mha_bwd == fa_bwd_dq then fa_bwd_dkdv; exposed so that each kernel can be timed /
 * profiled against its own roofline (bench.py `roofline_bwd`). */
int fa_bwd_dq(const fa_bwd_params* params, void* stream);
int fa_bwd_dkdv(const fa_bwd_params* params, void* stream);
/* Bytes of fa_bwd_params.workspace the dK/dV launch of these params would use (0: it would not split).  The `workspace` /
 * `workspace_bytes` fields of the argument are ignored (a stale or unaligned pointer left in a reused struct is not an error here).
 * Host-only arithmetic; the split target follows the CU count of the current device (256 when there is none).  Negative = error code. */
int64_t fa_bwd_workspace_bytes(const fa_bwd_params* params);

/* ---- decode over a KV cache (fa_kvcache_params above) ----------------------------------------- */
/* Append (if k_new / v_new), split-KV attention, and the combine of the splits: up to three launches on `stream`, no host synchronisation. */
int fa_run_mha_fwd_kvcache(const fa_kvcache_params* params, void* stream);
/* Bytes of workspace the launch would use with the split the library chooses (or num_splits, if set); 0 = one split.  The `workspace` /
 * `workspace_bytes` fields are ignored.  Host-only arithmetic; the split target follows the CU count of the current device (256 without one).
 * Negative = error code. */
int64_t fa_kvcache_workspace_bytes(const fa_kvcache_params* params);
/* Key splits the launch of these params would use, workspace fields included (NULL / 0 -> 1).  Host-only.  Negative = error code. */
int32_t fa_kvcache_num_splits(const fa_kvcache_params* params);
/* The same three with options (fa_kvcache_options / _v2 / _v3 / _v4 / _v5 / _v6 / _v7 above; NULL = the plain calls).  Their presence is how a caller detects the window.
 * Options are validated before anything is launched: a bad header is FA_ERR_BAD_ABI, a window size below -1 FA_ERR_BAD_SHAPE, an unknown
 * cache_dtype or a descale without FA_CACHE_FP8_E4M3 FA_ERR_BAD_DTYPE, an 8-bit cache view that breaks the alignment rule FA_ERR_BAD_STRIDE,
 * the rotary fields as listed with fa_kvcache_options_v3, the ragged fields with _v4, softmax_scale / softcap with _v5, sinks with _v6, tree_mask with _v7.  With rotary, fa_kvcache_num_splits_ex answers for the workspace behind the image
 * (a workspace that cannot hold the image is FA_ERR_BAD_SHAPE there as in the launch). */
int fa_run_mha_fwd_kvcache_ex(const fa_kvcache_params* params, const fa_kvcache_options* options, void* stream);
int64_t fa_kvcache_workspace_bytes_ex(const fa_kvcache_params* params, const fa_kvcache_options* options);
int32_t fa_kvcache_num_splits_ex(const fa_kvcache_params* params, const fa_kvcache_options* options);
/* Packed query rows per workgroup of the attention launch these params and options would make: 16, or 64 with fa_kvcache_options_v8.row_tile =
 * 64 (FA_HAS_KVCACHE_PREFILL).  The `workspace` fields are ignored.  Host-only.  Negative = error code, exactly those of the launch. */
int32_t fa_kvcache_row_tile_ex(const fa_kvcache_params* params, const fa_kvcache_options* options);

/* ---- MLA decode over a latent KV cache (fa_mla_params above) ----------------------------------- */
/* Append (if kv_new), split-KV attention, and the combine of the splits: up to three launches on `stream`, no host synchronisation.  The three entry
 * points take a fa_mla_params or (cast to it) a fa_mla_params_v2, told apart by struct_size. */
int fa_run_mla_fwd_kvcache(const fa_mla_params* params, void* stream);
/* Host-only, like fa_kvcache_workspace_bytes / fa_kvcache_num_splits: the bytes the split the library chooses (or num_splits) needs, the
 * `workspace` fields ignored; and the splits the launch would use, the workspace fields included (NULL / 0 -> 1).  Negative = error code. */
int64_t fa_mla_workspace_bytes(const fa_mla_params* params);
int32_t fa_mla_num_splits(const fa_mla_params* params);

/* ---- sparse MLA decode over a latent KV cache (fa_mla_sparse_params above) ------------------- */
/* Split attention over the token lists, and the combine of the splits: up to two launches on `stream`, no host synchronisation.  The three entry points
 * take a fa_mla_sparse_params or (cast to it) a fa_mla_sparse_params_v2, told apart by struct_size. */
int fa_run_mla_sparse_fwd_kvcache(const fa_mla_sparse_params* params, void* stream);
/* Host-only, like fa_mla_workspace_bytes / fa_mla_num_splits.  Negative = error code, exactly those of the launch. */
int64_t fa_mla_sparse_workspace_bytes(const fa_mla_sparse_params* params);
int32_t fa_mla_sparse_num_splits(const fa_mla_sparse_params* params);

/* ---- the indexer in front of sparse MLA decode (fa_mla_indexer_params / fa_mla_topk_params above) --- */
/* One launch each on `stream`, no workspace, no host synchronisation: lengths, tables and scales are read on the device. */
int fa_run_mla_indexer_logits(const fa_mla_indexer_params* params, void* stream);
int fa_run_mla_indexer_topk(const fa_mla_topk_params* params, void* stream);
/* The same logits for a prompt chunk (FA_HAS_MLA_INDEXER_PREFILL): the struct, the checks and the bits of fa_run_mla_indexer_logits. */
int fa_run_mla_indexer_prefill_logits(const fa_mla_indexer_params* params, void* stream);
/* Host-only, like fa_kvcache_row_tile_ex / fa_mla_num_splits: the tokens of a workgroup's tile (4 or 8), the keys of a workgroup's range (a multiple of
 * 32) and the ranges per tile of the launch fa_run_mla_indexer_prefill_logits would make; its grid is b x ceil(seqlen_q / tokens_per_wg) x n_chunks.
 * Any of the three pointers may be NULL.  Returns FA_OK or the error code of the launch (then nothing is written). */
int fa_mla_indexer_prefill_launch(const fa_mla_indexer_params* params, int32_t* tokens_per_wg, int32_t* wg_keys, int32_t* n_chunks);
/* The three entry points above for fa_mla_indexer_params_v2 (FA_HAS_MLA_INDEXER_FP8_Q): they take a fa_mla_indexer_params_v2 or (cast to it) a
 * fa_mla_indexer_params, told apart by struct_size; with q_format = FA_IDX_Q_16BIT, or the 216-byte struct, they are the calls above. */
int fa_run_mla_indexer_logits_v2(const fa_mla_indexer_params_v2* params, void* stream);
int fa_run_mla_indexer_prefill_logits_v2(const fa_mla_indexer_params_v2* params, void* stream);
int fa_mla_indexer_prefill_launch_v2(const fa_mla_indexer_params_v2* params, int32_t* tokens_per_wg, int32_t* wg_keys, int32_t* n_chunks);

/* ---- MLA prefill attention (fa_mla_prefill_params above) -------------------------------------- */
/* One launch on `stream`, no workspace, no host synchronisation: cu_seqlens are read on the device. */
int fa_run_mla_prefill_fwd(const fa_mla_prefill_params* params, void* stream);
/* Its backward (fa_mla_prefill_bwd_params above): two launches on `stream`, dsoftmax_sum the only workspace, no host synchronisation. */
int fa_run_mla_prefill_bwd(const fa_mla_prefill_bwd_params* params, void* stream);

/* ---- merging attention states (fa_merge_params above) ------------------------------------------ */
/* One launch on params->stream, no workspace, no host synchronisation. */
int fa_run_merge_states(const fa_merge_params* params);

/* ---- append and gather for the MLA caches (fa_mla_cache_append_params / _gather_params / fa_mla_index_cache_append_params above) --- */
/* One launch each on `stream`, no workspace, no host synchronisation. */
int fa_run_mla_cache_append(const fa_mla_cache_append_params* params, void* stream);
int fa_run_mla_cache_gather(const fa_mla_cache_gather_params* params, void* stream);
int fa_run_mla_index_cache_append(const fa_mla_index_cache_append_params* params, void* stream);

/* ---- measurement helpers ----------------------------------------------------------------- */
/* Algorithmic FLOPs of one forward call (4*b*h*sq*sk*d, causal counts only visible pairs);
 * backward = 2.5x this. Host-only arithmetic, no GPU needed. */
double fa_fwd_flops(int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t d, int32_t is_causal);
/* Algorithmic HBM bytes of one forward call: q,k,v,o once + lse. */
double fa_fwd_bytes(int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t h_k, int32_t d);
/* Name of the forward kernel the library dispatches LARGE problems of this head_dim to (what a profiler's kernel trace of the
 * BASELINE configurations will show; lets a benchmark tie a committed PMC profile to the kernel that actually ran).  head_dim 128
 * has two kernels: fa_fwd_pp16_kernel serves problems of seqlen_q * seqlen_k >= 2^20 whose launch fills the chip (fa_set_kernel_policy below), fa_fwd_pp_kernel
 * the others; head_dim 64 likewise for fp16 inputs from 2^24 (2^26 under a causal mask) - the answer given here - while bf16
 * inputs stay on fa_fwd_pp_kernel at every size (fa_kernel_name_dtype answers per dtype). */
const char* fa_fwd_kernel_name(int32_t d);
/* head_dim 128 has two sets of kernels, tiled for v_mfma_f32_32x32x16 and for v_mfma_f32_16x16x32.  Both meet the same tolerances;
 * they differ in speed only: the 16x16x32 shape draws less power per FLOP and wins where the chip's power cap binds (long launches),
 * the 32x32x16 forward needs fewer cycles and wins short ones and launches that leave compute units idle.  FA_POLICY_AUTO (the default, head_dim 128, round 6): the
 * forward and dQ go to the 16x16x32 set when the launch has at least one 256-row workgroup per compute unit (batch x heads x ceil(seqlen_q / 256) >= CUs; under a causal
 * mask two per unit, or one with seqlen_q * seqlen_k >= 2^26) and, forward and causal dQ, seqlen_q * seqlen_k >= 2^20; dK/dV from seqlen_q * seqlen_k >= 2^20 whatever the
 * launch (from 2^18 when it brings two 128-key workgroups per compute unit).  Because the choice follows the LAUNCH, a (batch, head) shard of a problem may get the other kernel set than the whole problem would: a caller that wants the
 * whole problem's kernels, hence its bits, on every shard states the whole problem's batch x heads with fa_set_policy_problem_heads() before it runs the shards (rounds
 * 3-5 chose per head only; flash_attn_turing/sharding.py:problem_policy does it for the Python surface).  One more exception stays: dK / dV of a GQA / MQA call that is given a
 * workspace - how far a head group is split, hence the order its partial sums are added in, follows the launch's workgroup count and the
 * device's CU count; shards then agree with the whole problem to a last rounding, not bit for bit.  FA_POLICY_MFMA32 / FA_POLICY_MFMA16 pin one set for every launch.  Process-wide, thread-safe; returns the
 * previous policy, -1 (and changes nothing) for an unknown value.  head_dim 64 has both forward kernels since round 4 and both backward sets since round 5; there the
 * launch matters the other way round: the 32x32x16 kernels live off two co-resident workgroups per compute unit, so FA_POLICY_AUTO keeps them for launches that fill the
 * chip with short sequences and gives the 16x16x32 set (one workgroup per unit) the long sequences - fp16 forward from 2^24 pairs per head (2^26 causal), dQ without a mask
 * from 2^18 and under one from 2^26, dK/dV from 2^24 (2^28 causal) - AND, since round 6, every launch that leaves the second workgroup slot empty (forward: at most one
 * 256-row workgroup per unit from 2^22 pairs, two under a mask, half a one from 2^20; dQ / dK/dV under a mask: at most two per unit; 5-25 % there), never when a causal
 * problem has fewer keys than queries; bf16 forwards stay on the 32x32x16 kernel (-8..-11 % / -4..-6 %
 * where it serves; both dtypes).  The pinned policies apply to every head_dim, stage and dtype.  The reference has no counterpart.
 * Precision contract of the forward's softmax row sums: fp16 inputs on the 16x16x32 kernel sum the ROUNDED P in the matrix pipe after an exactly
 * summed prefix of 1024 keys (LSE within 5e-5 of fp32 math at the BASELINE sizes); bf16 inputs keep exact fp32 VALU sums on every kernel (LSE within
 * 2e-6): with bf16's 8-bit P the same construction measured 1.2e-4 even behind a 4096-key exact prefix, for -0.9 % at configs[3] - refused
 * (profiles/r5_fwd_bf16_mfma_rowsum_ab.log, r5_lse_error_bf16_mfma_rowsum.json). */
#define FA_POLICY_MFMA32 0
#define FA_POLICY_MFMA16 1
#define FA_POLICY_AUTO 2
int32_t fa_set_kernel_policy(int32_t policy);
/* The batch x heads FA_POLICY_AUTO sizes every following launch with, instead of the launch's own: the WHOLE problem's, stated by a caller that runs (batch, head) shards of
 * it one after the other or on several devices and wants every shard served by the kernels the whole problem would get (bit-identical results).  0 (the initial value) = the
 * launch's own batch x heads.  Process-wide, thread-safe; returns the previous value, -1 (and changes nothing) for a negative argument.  Round 6; the reference has no counterpart. */
int64_t fa_set_policy_problem_heads(int64_t batch_times_heads);
/* Name of the kernel a launch of this shape is dispatched to under the current policy (what a profiler's kernel trace will show):
 * stage FA_STAGE_FWD / FA_STAGE_DQ / FA_STAGE_DKDV; seqlen_* = the max_seqlen_* of a packed call.  "" for an unknown stage. */
#define FA_STAGE_FWD 0
#define FA_STAGE_DQ 1
#define FA_STAGE_DKDV 2
const char* fa_kernel_name(int32_t stage, int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t d, int32_t is_causal);
/* The same per input dtype (enum fa_dtype; fa_kernel_name answers for FA_FP16): the only choice that depends on it is the head_dim-64 forward
 * under FA_POLICY_AUTO.  "" for an unknown stage or dtype. */
const char* fa_kernel_name_dtype(int32_t stage, int32_t dtype, int32_t b, int32_t seqlen_q, int32_t seqlen_k, int32_t h, int32_t d, int32_t is_causal);
/* Peak shader clock of `device` in kHz (hipDeviceAttributeClockRate), or a negative HIP error code: with 256 CUs x 4096 FLOP/clk/CU
 * it derives the dense fp16 MFMA peak a benchmark quotes (256 x 2.4 GHz x 4096 = 2.5 PFLOP/s). */
int fa_device_clock_khz(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_GFX950_H */
