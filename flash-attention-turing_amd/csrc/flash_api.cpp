// flash_api.cpp — PyTorch host module `flash_attn_turing._C` for the MI355X attention library.
//
// Same Python surface as the reference extension (csrc/flash_attn/flash_api.cpp:471-476):
//     fwd(q, k, v, is_causal)                               -> [o, l]
//     bwd(q, k, v, out, l, dout, is_causal)                 -> [dq, dk, dv]
//     varlen_fwd(q, k, v, cu_q, cu_k, max_sq, max_sk, is_causal)            -> [out, l]
//     varlen_bwd(q, k, v, out, l, dout, cu_q, cu_k, max_sq, max_sk, causal) -> [dq, dk, dv]
// Shape checks and their messages follow the reference's TORCH_CHECKs (:178-183, :252-259,
// :329-345, :396-423).  Deliberate hardening over the reference: dtype / device /
// head_dim checks (the reference silently returns zeros for head_dim not in {64,128},
// static_switch.h:29-38), bf16 accepted in addition to fp16, kernels enqueued on the CURRENT
// stream of q's device under a device guard (the reference uses the legacy default stream of
// device 0), launch errors surfaced.  This file contains no device code: it is compiled by
// plain g++ and calls the C ABI in include/flash_attn_gfx950.h; PyTorch is only plumbing
// (allocation, streams).
#include <atomic>

#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "flash_attn_gfx950.h"

namespace {

int fa_dtype_of(const at::Tensor& t) {
    if (t.scalar_type() == at::kHalf) return FA_FP16;
    if (t.scalar_type() == at::kBFloat16) return FA_BF16;
    TORCH_CHECK(false, "flash_attn_turing: only fp16 and bf16 are supported, got ", t.scalar_type());
    return -1;
}

void check_qkv_common(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
    TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(), "q, k, v must be GPU (HIP) tensors");
    TORCH_CHECK(k.device() == q.device() && v.device() == q.device(), "q, k, v must be on the same device");
    TORCH_CHECK(k.scalar_type() == q.scalar_type() && v.scalar_type() == q.scalar_type(), "q, k, v must have the same dtype");
}

void check_status(int rc) {
    TORCH_CHECK(rc == FA_OK, "flash_attn_turing (gfx950): ", fa_last_error(), " [code ", rc, "]");
}

void* current_stream(const at::Tensor& t) {
    return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

// (b, s, h, d) tensor -> element strides; the innermost dim must be dense.
fa_strides strides4(const at::Tensor& t) {
    TORCH_CHECK(t.stride(3) == 1, "last dimension must be contiguous");
    return fa_strides{t.stride(0), t.stride(1), t.stride(2)};
}
fa_strides strides3(const at::Tensor& t) {
    TORCH_CHECK(t.stride(2) == 1, "last dimension must be contiguous");
    return fa_strides{0, t.stride(0), t.stride(1)};
}
fa_strides strides34(const at::Tensor& t) { return t.dim() == 3 ? strides3(t) : strides4(t); }      // packed (rows, h, d) or dense (b, rows, h, d)
// The kernels take real strides, but rows/heads must stay 16-byte aligned; anything else is
// densified (the reference assumes contiguous input without checking, flash_api.cpp:38-54).
// NOTE: the densifying copy is a hidden extra HBM pass the reference never makes (it never checks); it only
// triggers for layouts the kernels cannot address (unaligned base / strides, broadcast rows) and is counted in
// g_densify_copies (exported as `densify_copies()`) so that a caller can see it happened.
std::atomic<int64_t> g_densify_copies{0};       // autograd may run backward on several threads / devices at once
at::Tensor dense_last(const at::Tensor& t) {
    bool ok = t.stride(-1) == 1 && (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0);
    for (int i = 0; i < t.dim() - 1 && ok; ++i) ok = (t.stride(i) % 8 == 0);
    // the row (sequence) dimension is dim -3: an expand()-ed / overlapping row stride (< head_dim) is not addressable
    if (ok && t.dim() >= 3 && t.size(-3) > 1) ok = t.stride(-3) >= t.size(-1);
    if (ok) return t;
    g_densify_copies.fetch_add(1, std::memory_order_relaxed);
    return t.contiguous();
}
void check_same_device(const at::Tensor& q, const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == q.device(), name, " must be on the same GPU device as q");
}

void check_cu_seqlens(const at::Tensor& cu_q, const at::Tensor& cu_k) {
    TORCH_CHECK(cu_q.is_cuda() && cu_k.is_cuda(), "cu_seqlens_q/cu_seqlens_k must be CUDA tensors");
    TORCH_CHECK(cu_q.scalar_type() == torch::kInt32 && cu_k.scalar_type() == torch::kInt32,
                "cu_seqlens_q/cu_seqlens_k must be int32 tensors");
    TORCH_CHECK(cu_q.is_contiguous() && cu_k.is_contiguous(), "cu_seqlens_q/cu_seqlens_k must be contiguous");
    TORCH_CHECK(cu_q.dim() == 1 && cu_k.dim() == 1, "cu_seqlens_q/cu_seqlens_k must be rank-1");
    TORCH_CHECK(cu_q.numel() >= 2 && cu_k.numel() >= 2, "cu_seqlens_q/cu_seqlens_k must have at least 2 elements");
    TORCH_CHECK(cu_k.numel() == cu_q.numel(), "cu_seqlens_k must have shape [batch_size + 1] with cumulative offsets");
}

// ---- argument rules that several functions below share: each is stated once and called at the caller's place in its order of checks.  The words and the place
// of a refusal are part of the interface; where the callers differ, the difference is an argument.

// A block_table argument: int32 (batch_size, max_blocks_per_seq) on q's device, last dimension contiguous, over the page pool `pool` (num_blocks, page_block_size,
// ..).  Fills the four paging fields of the C struct `p` and returns the capacity.  one_check: mla_indexer_logits states dtype, rank and batch in one check of its
// own words (its Python layer has checked them before).
template <typename P>
int64_t attach_block_table(P& p, const at::Tensor& q, int64_t batch_size, const at::Tensor& block_table, const at::Tensor& pool, bool one_check = false) {
    check_same_device(q, block_table, "block_table");
    if (one_check) {
        TORCH_CHECK(block_table.scalar_type() == torch::kInt32 && block_table.dim() == 2 && block_table.size(0) == batch_size, "block_table must be int32 [batch_size, max_blocks_per_seq]");
    } else {
        TORCH_CHECK(block_table.scalar_type() == torch::kInt32, "block_table must be an int32 tensor");
        TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == batch_size, "block_table must have shape [batch_size, max_blocks_per_seq]");
    }
    TORCH_CHECK(block_table.stride(1) == 1 || block_table.size(1) <= 1, "block_table: last dimension must be contiguous");
    const int64_t capacity = block_table.size(1) * pool.size(1);        // max_blocks_per_seq pages of page_block_size rows
    TORCH_CHECK(pool.size(0) <= INT32_MAX && capacity <= INT32_MAX, "block_table: pool pages and capacity must fit in int32");
    p.block_table = block_table.data_ptr<int32_t>();
    // (a one-row table's row stride is never used; a view may report anything there)
    p.block_table_stride = batch_size > 1 ? block_table.stride(0) : std::max<int64_t>(block_table.stride(0), block_table.size(1));
    p.page_block_size = (int32_t)pool.size(1); p.num_blocks = (int32_t)pool.size(0);
    return capacity;
}

// An optional cache_seqlens: int32 (batch_size,), contiguous, on q's device -> its pointer (NULL without it); it stays on the device
const int32_t* cache_seqlens_ptr(const at::Tensor& q, int64_t batch_size, const c10::optional<at::Tensor>& cache_seqlens) {
    if (!cache_seqlens.has_value()) return nullptr;
    check_same_device(q, *cache_seqlens, "cache_seqlens");
    TORCH_CHECK(cache_seqlens->scalar_type() == torch::kInt32, "cache_seqlens must be an int32 tensor");
    TORCH_CHECK(cache_seqlens->dim() == 1 && cache_seqlens->size(0) == batch_size && cache_seqlens->is_contiguous(),
                "cache_seqlens must be a contiguous tensor of shape [batch_size]");
    return cache_seqlens->data_ptr<int32_t>();
}

// softmax_scale -> the float of the C ABI, rounded once to fp32; 0 means "the default" there (None here; dflt: its text), so a given scale that is or rounds to 0 is refused
float softmax_scale_fp32(const c10::optional<double>& softmax_scale, const char* dflt) {
    TORCH_CHECK(!softmax_scale.has_value() || (std::isfinite(*softmax_scale) && (float)*softmax_scale > 0.f && std::isfinite((float)*softmax_scale)),
                "softmax_scale must be a finite fp32 value > 0 (or None = ", dflt, ")");
    return softmax_scale.has_value() ? (float)*softmax_scale : 0.f;
}

// ws_bytes: what the library's *_workspace_bytes query answered for `p` (negative: its error).  The fp32 scratch comes from the caching allocator and is attached
// to `p`; the returned tensor keeps it alive.
template <typename P>
at::Tensor attach_workspace(P& p, int64_t ws_bytes, const at::Tensor& q) {
    at::Tensor workspace;
    if (ws_bytes < 0) check_status((int)ws_bytes);
    if (ws_bytes > 0) {
        workspace = torch::empty({ws_bytes / 4}, q.options().dtype(torch::kFloat32));
        p.workspace = workspace.data_ptr(); p.workspace_bytes = ws_bytes;
    }
    return workspace;
}

}  // namespace

// reference: mha_fwd, flash_api.cpp:156-223
std::vector<at::Tensor> mha_fwd(at::Tensor q, at::Tensor k, at::Tensor v, bool is_causal) {
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q, k, v must be rank-4 tensors");
    check_qkv_common(q, k, v);
    const int64_t batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), head_size = q.size(3);
    const int64_t seqlen_k = k.size(1), num_heads_k = k.size(2);
    TORCH_CHECK(k.size(0) == batch_size && v.size(0) == batch_size, "k/v batch size must match q");
    TORCH_CHECK(v.size(1) == seqlen_k, "k and v seqlen_k must match");
    TORCH_CHECK(v.size(2) == num_heads_k, "k and v num_heads must match");
    TORCH_CHECK(k.size(3) == head_size && v.size(3) == head_size, "q/k/v head_dim must match");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "num_heads_q must be divisible by num_heads_k for GQA/MQA");

    c10::DeviceGuard guard(q.device());   // resolves to the ROCm (cuda-masquerading) guard impl
    q = dense_last(q); k = dense_last(k); v = dense_last(v);
    // every element of o and l is written by the kernel (dead rows included), so no zero fill
    at::Tensor o = torch::empty(q.sizes(), q.options());
    at::Tensor l = torch::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(torch::kFloat32));

    fa_fwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = o.data_ptr(); p.lse = l.data_ptr<float>();
    p.b = (int32_t)batch_size; p.seqlen_q = (int32_t)seqlen_q; p.seqlen_k = (int32_t)seqlen_k;
    p.h = (int32_t)num_heads; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.dtype = fa_dtype_of(q); p.is_causal = is_causal;
    p.q_stride = strides4(q); p.k_stride = strides4(k); p.v_stride = strides4(v); p.o_stride = strides4(o);
    check_status(fa_run_mha_fwd(&p, current_stream(q)));
    return {o, l};
}

// reference: mha_bwd, flash_api.cpp:228-317
std::vector<at::Tensor> mha_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor out, at::Tensor l, at::Tensor dout,
                                bool is_causal) {
    TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "q, k, v must be rank-4 tensors");
    TORCH_CHECK(out.dim() == 4 && dout.dim() == 4, "out and dout must be rank-4 tensors");
    check_qkv_common(q, k, v);
    check_same_device(q, out, "out"); check_same_device(q, dout, "dout"); check_same_device(q, l, "l");
    const int64_t batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2), head_size = q.size(3);
    const int64_t seqlen_k = k.size(1), num_heads_k = k.size(2);
    TORCH_CHECK(k.size(0) == batch_size && v.size(0) == batch_size, "k/v batch size must match q");
    TORCH_CHECK(v.size(1) == seqlen_k, "k and v seqlen_k must match");
    TORCH_CHECK(v.size(2) == num_heads_k, "k and v num_heads must match");
    TORCH_CHECK(k.size(3) == head_size && v.size(3) == head_size, "q/k/v head_dim must match");
    TORCH_CHECK(out.sizes() == q.sizes() && dout.sizes() == q.sizes(), "out and dout must match q shape");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "num_heads_q must be divisible by num_heads_k for GQA/MQA");
    TORCH_CHECK(out.scalar_type() == q.scalar_type() && dout.scalar_type() == q.scalar_type(), "out/dout dtype must match q");
    TORCH_CHECK(l.scalar_type() == torch::kFloat32 && l.dim() == 3 && l.size(0) == batch_size && l.size(1) == num_heads &&
                    l.size(2) == seqlen_q, "l must be fp32 with shape [batch_size, nheads_q, seqlen_q]");

    c10::DeviceGuard guard(q.device());   // resolves to the ROCm (cuda-masquerading) guard impl
    q = dense_last(q); k = dense_last(k); v = dense_last(v); out = dense_last(out); dout = dense_last(dout);
    l = l.contiguous();
    at::Tensor dq = torch::empty(q.sizes(), q.options());
    at::Tensor dk = torch::empty(k.sizes(), k.options());
    at::Tensor dv = torch::empty(v.sizes(), v.options());
    at::Tensor do_o = torch::empty_like(l);   // D = rowsum(dO * O), the reference's do_o (:274)

    fa_bwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = out.data_ptr(); p.dout = dout.data_ptr();
    p.lse = l.data_ptr<float>(); p.dsoftmax_sum = do_o.data_ptr<float>();
    p.dq = dq.data_ptr(); p.dk = dk.data_ptr(); p.dv = dv.data_ptr();
    p.b = (int32_t)batch_size; p.seqlen_q = (int32_t)seqlen_q; p.seqlen_k = (int32_t)seqlen_k;
    p.h = (int32_t)num_heads; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.dtype = fa_dtype_of(q); p.is_causal = is_causal;
    p.q_stride = strides4(q); p.k_stride = strides4(k); p.v_stride = strides4(v); p.o_stride = strides4(out);
    p.do_stride = strides4(dout); p.dq_stride = strides4(dq); p.dk_stride = strides4(dk); p.dv_stride = strides4(dv);
    // fp32 scratch (ABI 3) that lets the dK/dV launch split a KV head's query-head group over several workgroups (GQA / MQA with few
    // workgroups, causal imbalance); 0 bytes for MHA and for grids that fill the chip anyway
    at::Tensor workspace = attach_workspace(p, fa_bwd_workspace_bytes(&p), q);
    check_status(fa_run_mha_bwd(&p, current_stream(q)));
    return {dq, dk, dv};
}

// reference: mha_varlen_fwd, flash_api.cpp:319-381
std::vector<at::Tensor> mha_varlen_fwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor& cu_seqlens_q,
                                       at::Tensor& cu_seqlens_k, const int max_seqlen_q, const int max_seqlen_k,
                                       bool is_causal) {
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3, "q, k, v must be rank-3 packed tensors");
    check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    check_qkv_common(q, k, v);
    check_same_device(q, cu_seqlens_q, "cu_seqlens_q"); check_same_device(q, cu_seqlens_k, "cu_seqlens_k");
    const int64_t batch_size = cu_seqlens_q.numel() - 1;
    TORCH_CHECK(k.size(0) == v.size(0), "k and v total tokens must match");
    TORCH_CHECK(k.size(1) == v.size(1), "k and v num_heads must match");
    TORCH_CHECK(k.size(2) == v.size(2), "k and v head_dim must match");
    TORCH_CHECK(q.size(2) == k.size(2), "q/k/v head_dim must match");
    TORCH_CHECK(k.size(1) > 0 && q.size(1) % k.size(1) == 0, "num_heads_q must be divisible by num_heads_k for GQA/MQA");
    TORCH_CHECK(max_seqlen_q >= 0 && max_seqlen_k >= 0, "max_seqlen_q/max_seqlen_k must be non-negative");
    const int64_t num_heads = q.size(1), num_heads_k = k.size(1), head_size = q.size(2);

    c10::DeviceGuard guard(q.device());   // resolves to the ROCm (cuda-masquerading) guard impl
    q = dense_last(q); k = dense_last(k); v = dense_last(v);
    // tokens past cu_seqlens_q[-1] belong to no sequence and are not touched by the kernel: keep
    // the reference's zero fill (flash_api.cpp:351) for them
    at::Tensor out = torch::zeros_like(q);
    // padded LSE: entries past a sequence's length are never written by the kernel -> keep the
    // reference's zero fill for those (flash_api.cpp:352)
    at::Tensor l = torch::zeros({batch_size, num_heads, max_seqlen_q}, q.options().dtype(torch::kFloat32));

    fa_fwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = out.data_ptr(); p.lse = l.data_ptr<float>();
    p.cu_seqlens_q = cu_seqlens_q.data_ptr<int32_t>(); p.cu_seqlens_k = cu_seqlens_k.data_ptr<int32_t>();
    p.b = (int32_t)batch_size; p.seqlen_q = max_seqlen_q; p.seqlen_k = max_seqlen_k;
    p.h = (int32_t)num_heads; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.dtype = fa_dtype_of(q); p.is_causal = is_causal;
    p.q_stride = strides3(q); p.k_stride = strides3(k); p.v_stride = strides3(v); p.o_stride = strides3(out);
    p.total_q = q.size(0); p.total_k = k.size(0);   // packed row counts >= cu_seqlens[b]: lets the library size the grid by tokens present
    check_status(fa_run_mha_fwd(&p, current_stream(q)));
    return {out, l};
}

// reference: mha_varlen_bwd, flash_api.cpp:383-468
std::vector<at::Tensor> mha_varlen_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor out, at::Tensor l,
                                       at::Tensor dout, at::Tensor cu_seqlens_q, at::Tensor cu_seqlens_k,
                                       const int max_seqlen_q, const int max_seqlen_k, bool is_causal) {
    TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3, "q, k, v must be rank-3 packed tensors");
    check_cu_seqlens(cu_seqlens_q, cu_seqlens_k);
    check_qkv_common(q, k, v);
    check_same_device(q, cu_seqlens_q, "cu_seqlens_q"); check_same_device(q, cu_seqlens_k, "cu_seqlens_k");
    check_same_device(q, out, "out"); check_same_device(q, dout, "dout"); check_same_device(q, l, "l");
    const int64_t batch_size = cu_seqlens_q.numel() - 1;
    TORCH_CHECK(k.size(0) == v.size(0), "k and v total tokens must match");
    TORCH_CHECK(k.size(1) == v.size(1), "k and v num_heads must match");
    TORCH_CHECK(k.size(2) == v.size(2), "k and v head_dim must match");
    TORCH_CHECK(q.size(2) == k.size(2), "q/k/v head_dim must match");
    TORCH_CHECK(k.size(1) > 0 && q.size(1) % k.size(1) == 0, "num_heads_q must be divisible by num_heads_k for GQA/MQA");
    TORCH_CHECK(out.sizes() == q.sizes(), "out must match q shape");
    TORCH_CHECK(dout.sizes() == q.sizes(), "dout must match q shape");
    TORCH_CHECK(l.dim() == 3, "l must be rank-3 for varlen_bwd");
    const int64_t num_heads = q.size(1), num_heads_k = k.size(1), head_size = q.size(2);
    TORCH_CHECK(l.size(0) == batch_size && l.size(1) == num_heads && l.size(2) == max_seqlen_q,
                "l must have shape [batch_size, nheads_q, max_seqlen_q]");
    TORCH_CHECK(l.scalar_type() == torch::kFloat32, "l must be fp32");
    TORCH_CHECK(out.scalar_type() == q.scalar_type() && dout.scalar_type() == q.scalar_type(), "out/dout dtype must match q");

    c10::DeviceGuard guard(q.device());   // resolves to the ROCm (cuda-masquerading) guard impl
    q = dense_last(q); k = dense_last(k); v = dense_last(v); out = dense_last(out); dout = dense_last(dout);
    l = l.contiguous();
    at::Tensor dq = torch::zeros_like(q);
    // tokens of k/v that belong to no sequence (beyond cu_seqlens_k[-1]) are not touched by
    // the kernels -> zero fill like the reference (:425-427)
    at::Tensor dk = torch::zeros_like(k);
    at::Tensor dv = torch::zeros_like(v);
    at::Tensor do_o = torch::zeros_like(l);

    fa_bwd_params p;
    FA_PARAMS_INIT(p);
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = out.data_ptr(); p.dout = dout.data_ptr();
    p.lse = l.data_ptr<float>(); p.dsoftmax_sum = do_o.data_ptr<float>();
    p.dq = dq.data_ptr(); p.dk = dk.data_ptr(); p.dv = dv.data_ptr();
    p.cu_seqlens_q = cu_seqlens_q.data_ptr<int32_t>(); p.cu_seqlens_k = cu_seqlens_k.data_ptr<int32_t>();
    p.b = (int32_t)batch_size; p.seqlen_q = max_seqlen_q; p.seqlen_k = max_seqlen_k;
    p.h = (int32_t)num_heads; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.dtype = fa_dtype_of(q); p.is_causal = is_causal;
    p.q_stride = strides3(q); p.k_stride = strides3(k); p.v_stride = strides3(v); p.o_stride = strides3(out);
    p.do_stride = strides3(dout); p.dq_stride = strides3(dq); p.dk_stride = strides3(dk); p.dv_stride = strides3(dv);
    p.total_q = q.size(0); p.total_k = k.size(0);
    // fp32 scratch (ABI 3) that lets the dK/dV launch split a KV head's query-head group over several workgroups (GQA / MQA with few
    // workgroups, causal imbalance); 0 bytes for MHA and for grids that fill the chip anyway
    at::Tensor workspace = attach_workspace(p, fa_bwd_workspace_bytes(&p), q);
    check_status(fa_run_mha_bwd(&p, current_stream(q)));
    return {dq, dk, dv};
}

// Decode attention over a KV cache (upstream flash-attn's flash_attn_with_kvcache; the reference has no counterpart).  k_cache / v_cache are
// used in place with their own strides (no copy: k_new / v_new are appended INTO them); cache_seqlens stays on the device (no host sync, the
// call can be captured in a graph).  The split workspace comes from the caching allocator.  With block_table (int32, (b, max_blocks_per_seq))
// k_cache / v_cache are page pools (num_blocks, page_block_size, h_k, d), addressed through the table in place as well.  window_size_left /
// _right: a sliding window (fa_kvcache_options; (-1, -1) = none, the plain entry points).  A torch.float8_e4m3fn cache is the 8-bit cache of
// fa_kvcache_options_v2 with its optional fp32 (batch, h_k) descales (any strides, read on the device); a cache is never copied, so a view
// that breaks the alignment rule of the 8-bit loads is an error.  rotary_cos / rotary_sin ((seqlen_ro, rotary_dim / 2), q's dtype): rotary
// embedding of q and of the appended k (fa_kvcache_options_v3), fused into the append launch; the image of the rotated q lives in the
// workspace, whose size fa_kvcache_workspace_bytes_ex states, so the allocation below serves it as well.  cu_seqlens_q (int32 (b + 1,)): a ragged
// batch (fa_kvcache_options_v4) - q is packed (total_q, h, d), k_new / v_new (total_new, h_k, d) under cu_seqlens_k_new, max_seqlen_q sizes the
// launch; out comes back packed and lse as (h, total_q).  The cu_seqlens tensors stay on the device like cache_seqlens.  softmax_scale (None = 1 /
// sqrt(d)) and softcap (0 = off) are the two host scalars of fa_kvcache_options_v5; they are validated by the library.  sinks (float32 (nheads,), any stride): the
// attention sinks of fa_kvcache_options_v6, one logit per query head, read on the device like the descales.  tree_mask (int64 (batch, seqlen_q), ragged
// (total_q,), any strides): the tree attention mask of fa_kvcache_options_v7, one word per query row, read on the device in place.  prefill: the
// 64-row attention kernels for prompt chunks (fa_kvcache_options_v8.row_tile = 64); what they do not serve is refused by the library.
std::vector<at::Tensor> mha_fwd_kvcache(at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, c10::optional<at::Tensor> k_new_,
                                        c10::optional<at::Tensor> v_new_, c10::optional<at::Tensor> cache_seqlens_, bool is_causal,
                                        int64_t num_splits, c10::optional<at::Tensor> block_table_, int64_t window_size_left,
                                        int64_t window_size_right, c10::optional<at::Tensor> k_descale_, c10::optional<at::Tensor> v_descale_,
                                        c10::optional<at::Tensor> rotary_cos_, c10::optional<at::Tensor> rotary_sin_, bool rotary_interleaved,
                                        c10::optional<at::Tensor> cu_seqlens_q_, int64_t max_seqlen_q, c10::optional<at::Tensor> cu_seqlens_k_new_,
                                        c10::optional<double> softmax_scale, double softcap, c10::optional<at::Tensor> sinks_,
                                        c10::optional<at::Tensor> tree_mask_, bool prefill) {
    const bool ragged = cu_seqlens_q_.has_value();
    at::Tensor cu_seqlens_q, cu_seqlens_k_new;
    auto cu_tensor = [&](const at::Tensor& t, const char* name) {
        TORCH_CHECK(t.device() == q.device(), name, " must be on the same device as q");
        TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be an int32 tensor");
        TORCH_CHECK(t.dim() == 1 && t.size(0) >= 1 && t.is_contiguous(), name, " must be a contiguous tensor of shape [batch_size + 1]");
    };
    if (ragged) {
        // packed q (total_q, h, d) -> a batch of one with total_q rows: the strides and the output shape below follow, the batch is the cu's
        TORCH_CHECK(q.dim() == 3, "q must be a packed rank-3 tensor (total_q, nheads, head_dim) with cu_seqlens_q");
        TORCH_CHECK(max_seqlen_q >= 1 && max_seqlen_q <= INT32_MAX, "max_seqlen_q must be an int32 >= 1 with cu_seqlens_q");
        TORCH_CHECK(!rotary_cos_.has_value() && !rotary_sin_.has_value(), "rotary_cos / rotary_sin together with cu_seqlens_q are not supported");
        cu_seqlens_q = *cu_seqlens_q_;
        cu_tensor(cu_seqlens_q, "cu_seqlens_q");
        q = q.unsqueeze(0);
        if (k_new_.has_value() && v_new_.has_value()) {
            TORCH_CHECK(k_new_->dim() == 3 && v_new_->dim() == 3, "k and v must be packed rank-3 tensors (total_new, nheads_k, head_dim) with cu_seqlens_q");
            TORCH_CHECK(cu_seqlens_k_new_.has_value(), "packed k and v need cu_seqlens_k_new");
            cu_seqlens_k_new = *cu_seqlens_k_new_;
            cu_tensor(cu_seqlens_k_new, "cu_seqlens_k_new");
            TORCH_CHECK(cu_seqlens_k_new.size(0) == cu_seqlens_q.size(0), "cu_seqlens_k_new must have the shape of cu_seqlens_q");
            k_new_ = k_new_->unsqueeze(0); v_new_ = v_new_->unsqueeze(0);
        } else {
            TORCH_CHECK(!cu_seqlens_k_new_.has_value(), "cu_seqlens_k_new given without k and v");
        }
    } else {
        TORCH_CHECK(!cu_seqlens_k_new_.has_value(), "cu_seqlens_k_new given without cu_seqlens_q");
    }
    TORCH_CHECK(q.dim() == 4 && k_cache.dim() == 4 && v_cache.dim() == 4, "q, k_cache, v_cache must be rank-4 tensors");
    TORCH_CHECK(q.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda(), "q, k, v must be GPU (HIP) tensors");
    TORCH_CHECK(k_cache.device() == q.device() && v_cache.device() == q.device(), "q, k, v must be on the same device");
    TORCH_CHECK(k_cache.scalar_type() == v_cache.scalar_type(), "k_cache and v_cache must have the same dtype");
    const bool fp8 = k_cache.scalar_type() == at::kFloat8_e4m3fn;
    TORCH_CHECK(fp8 || k_cache.scalar_type() == q.scalar_type(),
                "k_cache / v_cache must have the dtype of q or be torch.float8_e4m3fn (OCP e4m3; float8_e4m3fnuz, float8_e5m2 and other dtypes are not supported), got ",
                k_cache.scalar_type());
    TORCH_CHECK(fp8 || (!k_descale_.has_value() && !v_descale_.has_value()), "k_descale / v_descale need a torch.float8_e4m3fn cache");
    const int64_t total_q = q.size(1);         // (ragged: the packed rows)
    const int64_t batch_size = ragged ? cu_seqlens_q.size(0) - 1 : q.size(0), seqlen_q = ragged ? max_seqlen_q : q.size(1), num_heads = q.size(2), head_size = q.size(3);
    const int64_t num_heads_k = k_cache.size(2);
    int64_t seqlen_cache = k_cache.size(1);
    TORCH_CHECK(seqlen_q >= 1, "seqlen_q must be >= 1");
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    if (block_table_.has_value()) {
        seqlen_cache = attach_block_table(p, q, batch_size, *block_table_, k_cache);
    } else {
        TORCH_CHECK(k_cache.size(0) == batch_size && v_cache.size(0) == batch_size, "k_cache/v_cache batch size must match q");
    }
    TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), "k_cache and v_cache must have the same shape");
    TORCH_CHECK(k_cache.size(3) == head_size, "q/k_cache/v_cache head_dim must match");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "num_heads_q must be divisible by num_heads_k for GQA/MQA");
    TORCH_CHECK(k_cache.stride(3) == 1 && v_cache.stride(3) == 1, "k_cache/v_cache: last dimension must be contiguous");
    TORCH_CHECK(num_splits >= 0, "num_splits must be >= 0 (0 = automatic)");
    TORCH_CHECK(window_size_left >= -1 && window_size_right >= -1 && window_size_left <= INT32_MAX && window_size_right <= INT32_MAX,
                "window_size: each side must be an int32 >= -1 (-1 = unbounded)");
    TORCH_CHECK(k_new_.has_value() == v_new_.has_value(), "k and v must both be given or both be None");
    at::Tensor k_new, v_new;
    p.cache_seqlens = cache_seqlens_ptr(q, batch_size, cache_seqlens_);
    c10::DeviceGuard guard(q.device());
    if (k_new_.has_value()) {
        TORCH_CHECK(cache_seqlens_.has_value(), "cache_seqlens is required when k and v are appended");
        k_new = *k_new_; v_new = *v_new_;
        TORCH_CHECK(k_new.dim() == 4 && v_new.dim() == 4, "k and v must be rank-4 tensors");
        check_same_device(q, k_new, "k"); check_same_device(q, v_new, "v");
        TORCH_CHECK(k_new.scalar_type() == q.scalar_type() && v_new.scalar_type() == q.scalar_type(), "k and v must have the dtype of q");
        TORCH_CHECK((ragged || k_new.size(0) == batch_size) && k_new.size(2) == num_heads_k && k_new.size(3) == head_size && v_new.sizes() == k_new.sizes(),
                    ragged ? "k and v must have shape [total_new, num_heads_k, head_dim]" : "k and v must have shape [batch_size, seqlen_new, num_heads_k, head_dim]");
        TORCH_CHECK(ragged || k_new.size(1) <= seqlen_cache, "seqlen_new must not exceed the cache capacity");
        k_new = dense_last(k_new); v_new = dense_last(v_new);
    }
    q = dense_last(q);
    at::Tensor o = torch::empty(q.sizes(), q.options());
    at::Tensor l = ragged ? torch::empty({num_heads, total_q}, q.options().dtype(torch::kFloat32))
                          : torch::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(torch::kFloat32));

    p.q = q.data_ptr(); p.k_cache = k_cache.data_ptr(); p.v_cache = v_cache.data_ptr(); p.o = o.data_ptr(); p.lse = l.data_ptr<float>();
    p.b = (int32_t)batch_size; p.seqlen_q = (int32_t)seqlen_q; p.seqlen_cache = (int32_t)seqlen_cache;
    p.h = (int32_t)num_heads; p.h_k = (int32_t)num_heads_k; p.d = (int32_t)head_size;
    p.dtype = fa_dtype_of(q); p.is_causal = is_causal; p.num_splits = (int32_t)num_splits;
    p.q_stride = strides4(q); p.k_cache_stride = strides4(k_cache); p.v_cache_stride = strides4(v_cache); p.o_stride = strides4(o);
    if (k_new.defined()) {
        // (ragged: the largest append the call allows - no sequence can append more rows than there are, or than its capacity holds)
        p.k_new = k_new.data_ptr(); p.v_new = v_new.data_ptr(); p.seqlen_new = (int32_t)(ragged ? std::min<int64_t>(k_new.size(1), seqlen_cache) : k_new.size(1));
        p.k_new_stride = strides4(k_new); p.v_new_stride = strides4(v_new);
    }
    fa_kvcache_options_v8 opt;
    FA_PARAMS_INIT(opt);
    opt.softmax_scale = softmax_scale_fp32(softmax_scale, "1 / sqrt(head_dim)");
    TORCH_CHECK(std::isfinite(softcap) && softcap >= 0.0 && std::isfinite((float)softcap) && (softcap == 0.0 || (float)softcap > 0.f),
                "softcap must be a finite fp32 value >= 0 (0 = no cap)");
    const bool scaled = softmax_scale.has_value() || softcap != 0.0;
    opt.softcap = (float)softcap;
    if (ragged) {
        opt.cu_seqlens_q = cu_seqlens_q.data_ptr<int32_t>(); opt.total_q = total_q;
        if (k_new.defined()) { opt.cu_seqlens_k_new = cu_seqlens_k_new.data_ptr<int32_t>(); opt.total_k_new = k_new.size(1); }
    }
    opt.is_local = window_size_left != -1 || window_size_right != -1;
    opt.window_size_left = (int32_t)window_size_left; opt.window_size_right = (int32_t)window_size_right;
    at::Tensor k_descale, v_descale;
    if (fp8) {
        opt.cache_dtype = FA_CACHE_FP8_E4M3;
        auto descale = [&](const c10::optional<at::Tensor>& t_, const char* name, at::Tensor& keep, const float*& ptr, int64_t& sb, int64_t& sh) {
            if (!t_.has_value()) return;
            keep = *t_;
            check_same_device(q, keep, name);
            TORCH_CHECK(keep.scalar_type() == torch::kFloat32, name, " must be a float32 tensor");
            TORCH_CHECK(keep.dim() == 2 && keep.size(0) == batch_size && keep.size(1) == num_heads_k, name, " must have shape [batch_size, num_heads_k]");
            ptr = keep.data_ptr<float>(); sb = keep.stride(0); sh = keep.stride(1);
        };
        descale(k_descale_, "k_descale", k_descale, opt.k_descale, opt.k_descale_batch_stride, opt.k_descale_head_stride);
        descale(v_descale_, "v_descale", v_descale, opt.v_descale, opt.v_descale_batch_stride, opt.v_descale_head_stride);
    }
    TORCH_CHECK(rotary_cos_.has_value() == rotary_sin_.has_value(), "rotary_cos and rotary_sin must both be given or both be None");
    at::Tensor rotary_cos, rotary_sin;
    if (rotary_cos_.has_value()) {
        rotary_cos = *rotary_cos_; rotary_sin = *rotary_sin_;
        TORCH_CHECK(k_new.defined(), "rotary_cos / rotary_sin are only applicable if k and v are passed in");
        check_same_device(q, rotary_cos, "rotary_cos"); check_same_device(q, rotary_sin, "rotary_sin");
        TORCH_CHECK(rotary_cos.scalar_type() == q.scalar_type() && rotary_sin.scalar_type() == q.scalar_type(), "rotary_cos / rotary_sin must have the dtype of q");
        TORCH_CHECK(rotary_cos.dim() == 2 && rotary_sin.sizes() == rotary_cos.sizes(), "rotary_cos / rotary_sin must both have shape [seqlen_ro, rotary_dim / 2]");
        TORCH_CHECK(rotary_cos.size(0) <= INT32_MAX && rotary_cos.size(1) <= INT32_MAX / 2, "rotary_cos / rotary_sin: sizes must fit in int32");
        TORCH_CHECK(rotary_cos.stride(1) == 1 && rotary_sin.stride(1) == 1, "rotary_cos / rotary_sin: last dimension must be contiguous");
        // one row stride serves both tables in the C ABI; a table whose row stride differs from the other's is made dense (tables are small)
        if (rotary_cos.size(0) > 1 && rotary_cos.stride(0) != rotary_sin.stride(0)) { rotary_cos = rotary_cos.contiguous(); rotary_sin = rotary_sin.contiguous(); }
        opt.rotary_cos = rotary_cos.data_ptr(); opt.rotary_sin = rotary_sin.data_ptr();
        opt.rotary_row_stride = rotary_cos.size(0) > 1 ? rotary_cos.stride(0) : rotary_cos.size(1);
        opt.seqlen_ro = (int32_t)rotary_cos.size(0); opt.rotary_dim = (int32_t)(2 * rotary_cos.size(1));
        opt.rotary_interleaved = rotary_interleaved ? 1 : 0;
    }
    at::Tensor sinks;
    if (sinks_.has_value()) {
        sinks = *sinks_;
        check_same_device(q, sinks, "sinks");
        TORCH_CHECK(sinks.scalar_type() == torch::kFloat32, "sinks must be a float32 tensor");
        TORCH_CHECK(sinks.dim() == 1 && sinks.size(0) == num_heads, "sinks must have shape [num_heads]");
        opt.sinks = sinks.data_ptr<float>(); opt.sinks_stride = num_heads > 1 ? sinks.stride(0) : 1;
    }
    at::Tensor tree_mask;
    if (tree_mask_.has_value()) {
        tree_mask = *tree_mask_;
        check_same_device(q, tree_mask, "tree_mask");
        TORCH_CHECK(tree_mask.scalar_type() == torch::kInt64, "tree_mask must be an int64 tensor");
        if (ragged) {
            TORCH_CHECK(tree_mask.dim() == 1 && tree_mask.size(0) == total_q, "tree_mask must have shape [total_q] with cu_seqlens_q");
            opt.tree_mask_row_stride = tree_mask.stride(0);
        } else {
            TORCH_CHECK(tree_mask.dim() == 2 && tree_mask.size(0) == batch_size && tree_mask.size(1) == seqlen_q, "tree_mask must have shape [batch_size, seqlen_q]");
            opt.tree_mask_batch_stride = tree_mask.stride(0); opt.tree_mask_row_stride = tree_mask.stride(1);
        }
        opt.tree_mask = tree_mask.data_ptr<int64_t>();
    }
    if (prefill) opt.row_tile = 64;
    const fa_kvcache_options* opts = (opt.is_local || fp8 || rotary_cos.defined() || ragged || scaled || sinks.defined() || tree_mask.defined() || prefill) ? (const fa_kvcache_options*)&opt : nullptr;
    at::Tensor workspace = attach_workspace(p, fa_kvcache_workspace_bytes_ex(&p, opts), q);
    check_status(fa_run_mha_fwd_kvcache_ex(&p, opts, current_stream(q)));
    if (ragged) return {o.squeeze(0), l};
    return {o, l};
}

// kv_cache of the two MLA calls below in the FP8 format (FA_MLA_KV_FP8_ROWS656): a 1-byte dtype and 656-byte rows; anything else is the 16-bit cache
static bool mla_cache_is_fp8(const at::Tensor& kv_cache) {
    return (kv_cache.scalar_type() == torch::kUInt8 || kv_cache.scalar_type() == at::ScalarType::Float8_e4m3fn) && kv_cache.dim() == 4 && kv_cache.size(3) == 656;
}

// ---- what mha_fwd_mla_kvcache and mha_fwd_mla_sparse_kvcache share (PV: fa_mla_params_v2 or fa_mla_sparse_params_v2, which name these fields alike), in the
// three places where their orders of checks coincide: q and kv_cache; the table and the lengths; q made dense, the outputs and the struct.
static void check_mla_decode_inputs(const at::Tensor& q, const at::Tensor& kv_cache, int64_t num_splits, int64_t head_dim_v) {
    TORCH_CHECK(q.dim() == 4 && kv_cache.dim() == 4, "q and kv_cache must be rank-4 tensors");
    TORCH_CHECK(q.is_cuda() && kv_cache.is_cuda(), "q, kv_cache must be GPU (HIP) tensors");
    TORCH_CHECK(kv_cache.device() == q.device(), "q, kv_cache must be on the same device");
    const bool fp8 = mla_cache_is_fp8(kv_cache);
    TORCH_CHECK(fp8 || kv_cache.scalar_type() == q.scalar_type(), "kv_cache must have the dtype of q, got ", kv_cache.scalar_type());
    TORCH_CHECK(q.size(1) >= 1 && q.size(2) >= 1, "seqlen_q and the number of heads must be >= 1");
    TORCH_CHECK(kv_cache.size(2) == 1, "kv_cache must have exactly one head (the latent row)");
    TORCH_CHECK(fp8 || kv_cache.size(3) == q.size(3), "q / kv_cache head_dim must match");
    TORCH_CHECK(kv_cache.stride(3) == 1, "kv_cache: last dimension must be contiguous");
    TORCH_CHECK(num_splits >= 0 && num_splits <= INT32_MAX, "num_splits must be >= 0 (0 = automatic)");
    TORCH_CHECK(head_dim_v >= 0 && head_dim_v <= INT32_MAX && q.size(3) <= INT32_MAX, "head dims must fit in int32");
}

// block_table (or the batch of a contiguous cache) and cache_seqlens -> pv; returns the capacity
template <typename PV>
static int64_t mla_decode_table_and_lengths(PV& pv, const at::Tensor& q, const at::Tensor& kv_cache, const c10::optional<at::Tensor>& block_table,
                                            const c10::optional<at::Tensor>& cache_seqlens) {
    int64_t seqlen_cache = kv_cache.size(1);
    if (block_table.has_value()) {
        seqlen_cache = attach_block_table(pv, q, q.size(0), *block_table, kv_cache);
    } else {
        TORCH_CHECK(kv_cache.size(0) == q.size(0), "kv_cache batch size must match q");
    }
    pv.cache_seqlens = cache_seqlens_ptr(q, q.size(0), cache_seqlens);
    pv.seqlen_cache = (int32_t)seqlen_cache;
    return seqlen_cache;
}

// Under the caller's device guard: q with addressable strides, out (b, sq, h, head_dim_v) and lse (b, h, sq) allocated, and every field of pv the two structs
// share filled from them.  The cache is never copied.
template <typename PV>
static std::vector<at::Tensor> mla_decode_outputs(PV& pv, at::Tensor& q, const at::Tensor& kv_cache, int64_t num_splits, const c10::optional<double>& softmax_scale,
                                                  int64_t head_dim_v) {
    q = dense_last(q);
    const int64_t batch_size = q.size(0), seqlen_q = q.size(1), num_heads = q.size(2);
    at::Tensor o = torch::empty({batch_size, seqlen_q, num_heads, head_dim_v}, q.options());
    at::Tensor l = torch::empty({batch_size, num_heads, seqlen_q}, q.options().dtype(torch::kFloat32));
    pv.kv_format = mla_cache_is_fp8(kv_cache) ? FA_MLA_KV_FP8_ROWS656 : FA_MLA_KV_16BIT;     // (FP8: a 1-byte dtype, so strides4(kv_cache) is in bytes, as the format asks)
    pv.q = q.data_ptr(); pv.kv_cache = kv_cache.data_ptr(); pv.o = o.data_ptr(); pv.lse = l.data_ptr<float>();
    pv.b = (int32_t)batch_size; pv.seqlen_q = (int32_t)seqlen_q;
    pv.h = (int32_t)num_heads; pv.d_qk = (int32_t)q.size(3); pv.d_v = (int32_t)head_dim_v;
    pv.dtype = fa_dtype_of(q); pv.num_splits = (int32_t)num_splits;
    pv.softmax_scale = softmax_scale_fp32(softmax_scale, "576 ** -0.5");
    pv.q_stride = strides4(q); pv.kv_cache_stride = strides4(kv_cache); pv.o_stride = strides4(o);
    return {o, l};
}

// MLA decode over a latent KV cache (fa_run_mla_fwd_kvcache): q (b, sq, h, 576), kv_cache (b, capacity, 1, 576) or a page pool (num_blocks,
// page_block_size, 1, 576) with block_table, kv_new (b, s_new, 1, 576) appended in place; out (b, sq, h, 512) and lse (b, h, sq).  The cache is never
// copied; lengths and tables are read on the device.  softmax_scale: rounded once to fp32, None = the library's default 576 ** -0.5.
std::vector<at::Tensor> mha_fwd_mla_kvcache(at::Tensor q, at::Tensor kv_cache, c10::optional<at::Tensor> kv_new_, c10::optional<at::Tensor> cache_seqlens_,
                                            bool is_causal, int64_t num_splits, c10::optional<at::Tensor> block_table_, c10::optional<double> softmax_scale,
                                            int64_t head_dim_v) {
    fa_mla_params_v2 pv;
    FA_PARAMS_INIT(pv);
    check_mla_decode_inputs(q, kv_cache, num_splits, head_dim_v);
    const int64_t seqlen_cache = mla_decode_table_and_lengths(pv, q, kv_cache, block_table_, cache_seqlens_);
    const int64_t batch_size = q.size(0), head_size = q.size(3);
    c10::DeviceGuard guard(q.device());
    at::Tensor kv_new;
    if (kv_new_.has_value()) {
        TORCH_CHECK(cache_seqlens_.has_value(), "cache_seqlens is required when kv_new is appended");
        kv_new = *kv_new_;
        TORCH_CHECK(kv_new.dim() == 4, "kv_new must be a rank-4 tensor");
        check_same_device(q, kv_new, "kv_new");
        TORCH_CHECK(kv_new.scalar_type() == q.scalar_type(), "kv_new must have the dtype of q");
        TORCH_CHECK(kv_new.size(0) == batch_size && kv_new.size(2) == 1 && kv_new.size(3) == head_size, "kv_new must have shape [batch_size, seqlen_new, 1, head_dim]");
        TORCH_CHECK(kv_new.size(1) <= seqlen_cache, "seqlen_new must not exceed the cache capacity");
        kv_new = dense_last(kv_new);
    }
    pv.is_causal = is_causal;
    std::vector<at::Tensor> out = mla_decode_outputs(pv, q, kv_cache, num_splits, softmax_scale, head_dim_v);
    if (kv_new.defined()) {
        pv.kv_new = kv_new.data_ptr(); pv.seqlen_new = (int32_t)kv_new.size(1);
        pv.kv_new_stride = strides4(kv_new);
    }
    fa_mla_params& p = reinterpret_cast<fa_mla_params&>(pv);
    at::Tensor workspace = attach_workspace(p, fa_mla_workspace_bytes(&p), q);
    check_status(fa_run_mla_fwd_kvcache(&p, current_stream(q)));
    return out;
}

// ---- what mha_fwd_mla_prefill and mha_bwd_mla_prefill share: the q / k / v section of their checks (the backward's out / dout / lse checks stand between its
// two halves) and the fields fa_mla_prefill_params and fa_mla_prefill_bwd_params name alike
struct MlaPrefillShape {
    bool packed;
    int64_t batch_size, rows_q, rows_k, num_heads, num_heads_k;
};

// cu_seqlens both or neither; q / k / v of the rank that follows, on one GPU, of one dtype.  Returns whether the call is packed.
static bool check_mla_prefill_qkv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const c10::optional<at::Tensor>& cu_q, const c10::optional<at::Tensor>& cu_k) {
    const bool packed = cu_q.has_value() || cu_k.has_value();
    TORCH_CHECK(cu_q.has_value() == cu_k.has_value(), "cu_seqlens_q and cu_seqlens_k come both or neither");
    const int64_t rank = packed ? 3 : 4;
    TORCH_CHECK(q.dim() == rank && k.dim() == rank && v.dim() == rank, "q, k, v must be rank-", rank, " tensors");
    check_qkv_common(q, k, v);
    return packed;
}

static MlaPrefillShape check_mla_prefill_shapes(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, bool packed, const c10::optional<at::Tensor>& cu_q) {
    const int64_t batch_size = packed ? cu_q->numel() - 1 : q.size(0);
    const int64_t rows_q = q.size(-3), rows_k = k.size(-3), num_heads = q.size(-2), num_heads_k = k.size(-2);
    TORCH_CHECK(v.size(-3) == rows_k && v.size(-2) == num_heads_k, "k and v must agree in rows and heads");
    TORCH_CHECK(packed || (k.size(0) == batch_size && v.size(0) == batch_size), "k/v batch size must match q");
    TORCH_CHECK(k.size(-1) == q.size(-1), "q / k head_dim must match");
    TORCH_CHECK(num_heads_k > 0 && num_heads % num_heads_k == 0, "num_heads_q must be divisible by num_heads_k for GQA/MQA");
    TORCH_CHECK(batch_size <= INT32_MAX && (packed || (rows_q <= INT32_MAX && rows_k <= INT32_MAX)) && num_heads <= INT32_MAX && q.size(-1) <= INT32_MAX && v.size(-1) <= INT32_MAX,
                "sizes must fit in int32");
    return MlaPrefillShape{packed, batch_size, rows_q, rows_k, num_heads, num_heads_k};
}

static void check_mla_prefill_cu(const at::Tensor& q, bool packed, const c10::optional<at::Tensor>& cu_q, const c10::optional<at::Tensor>& cu_k) {
    if (!packed) return;
    check_cu_seqlens(*cu_q, *cu_k);
    check_same_device(q, *cu_q, "cu_seqlens_q"); check_same_device(q, *cu_k, "cu_seqlens_k");
}

// o: the forward's output, allocated (forward) or given (backward); lse likewise.  Nothing is copied.
template <typename P>
static void fill_mla_prefill(P& p, const MlaPrefillShape& s, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& o, const at::Tensor& lse,
                             const c10::optional<at::Tensor>& cu_q, const c10::optional<at::Tensor>& cu_k, bool is_causal, const c10::optional<double>& softmax_scale) {
    p.q = q.data_ptr(); p.k = k.data_ptr(); p.v = v.data_ptr(); p.o = o.data_ptr(); p.lse = lse.data_ptr<float>();
    p.b = (int32_t)s.batch_size; p.h = (int32_t)s.num_heads; p.h_k = (int32_t)s.num_heads_k; p.d_qk = (int32_t)q.size(-1); p.d_v = (int32_t)v.size(-1);
    p.dtype = fa_dtype_of(q); p.is_causal = is_causal;
    p.softmax_scale = softmax_scale_fp32(softmax_scale, "192 ** -0.5");
    if (s.packed) {
        p.cu_seqlens_q = cu_q->data_ptr<int32_t>(); p.cu_seqlens_k = cu_k->data_ptr<int32_t>();
        p.total_q = s.rows_q; p.total_k = s.rows_k;
    } else {
        p.seqlen_q = (int32_t)s.rows_q; p.seqlen_k = (int32_t)s.rows_k;
    }
    p.q_stride = strides34(q); p.k_stride = strides34(k); p.v_stride = strides34(v); p.o_stride = strides34(o);
}

// MLA prefill attention (fa_run_mla_prefill_fwd): dense q (b, sq, h, 192), k (b, sk, h_k, 192), v (b, sk, h_k, 128) -> out (b, sq, h, 128), lse (b, h, sq);
// packed (both cu_seqlens) q (total_q, h, 192), k (total_k, h_k, 192), v (total_k, h_k, 128) -> out (total_q, h, 128), lse (h, total_q).  Nothing is copied:
// the tensors go to the library with the strides they have, and a view it cannot address is its error.  softmax_scale: rounded once to fp32, None =
// the library's default 192 ** -0.5.
std::vector<at::Tensor> mha_fwd_mla_prefill(at::Tensor q, at::Tensor k, at::Tensor v, c10::optional<at::Tensor> cu_seqlens_q_, c10::optional<at::Tensor> cu_seqlens_k_,
                                            bool is_causal, c10::optional<double> softmax_scale) {
    const bool packed = check_mla_prefill_qkv(q, k, v, cu_seqlens_q_, cu_seqlens_k_);
    const MlaPrefillShape s = check_mla_prefill_shapes(q, k, v, packed, cu_seqlens_q_);
    check_mla_prefill_cu(q, packed, cu_seqlens_q_, cu_seqlens_k_);
    c10::DeviceGuard guard(q.device());
    // dense: every element of o and l is written (dead rows included); packed: the rows past cu_seqlens_q[-1] are not touched
    at::Tensor o = packed ? torch::empty({s.rows_q, s.num_heads, v.size(-1)}, q.options()) : torch::empty({s.batch_size, s.rows_q, s.num_heads, v.size(-1)}, q.options());
    at::Tensor l = packed ? torch::empty({s.num_heads, s.rows_q}, q.options().dtype(torch::kFloat32))
                          : torch::empty({s.batch_size, s.num_heads, s.rows_q}, q.options().dtype(torch::kFloat32));

    fa_mla_prefill_params p;
    FA_PARAMS_INIT(p);
    fill_mla_prefill(p, s, q, k, v, o, l, cu_seqlens_q_, cu_seqlens_k_, is_causal, softmax_scale);
    check_status(fa_run_mla_prefill_fwd(&p, current_stream(q)));
    return {o, l};
}

// Merging attention states (fa_run_merge_states): dense outs[i] (b, rows, h, d_v) / lses[i] (b, h, rows) -> [out (b, rows, h, d_v), lse (b, h, rows)]; packed
// outs[i] (total, h, d_v) / lses[i] (h, total) -> [out (total, h, d_v), lse (h, total)].  Nothing is copied: every part goes to the library with the strides it
// has (an LSE with any strides at all), and a view it cannot address is its error.
std::vector<at::Tensor> merge_states(std::vector<at::Tensor> outs, std::vector<at::Tensor> lses) {
    TORCH_CHECK(outs.size() >= 2 && outs.size() <= FA_MERGE_MAX_PARTS && lses.size() == outs.size(), "merge_states takes 2 .. ", FA_MERGE_MAX_PARTS,
                " parts, as many lses as outs");
    const at::Tensor& o0 = outs[0];
    const bool packed = o0.dim() == 3;
    TORCH_CHECK(packed || o0.dim() == 4, "outs[0] must be (b, rows, h, d_v) or (total, h, d_v)");
    TORCH_CHECK(o0.is_cuda(), "outs / lses must be GPU (HIP) tensors");
    const int64_t b = packed ? 1 : o0.size(0), rows = o0.size(-3), h = o0.size(-2), dv = o0.size(-1);
    TORCH_CHECK(b <= INT32_MAX && rows <= INT32_MAX && h <= INT32_MAX && dv <= INT32_MAX, "sizes must fit in int32");
    fa_merge_params p;
    FA_PARAMS_INIT(p);
    p.dtype = fa_dtype_of(o0); p.n_parts = (int32_t)outs.size(); p.b = (int32_t)b; p.rows = (int32_t)rows; p.h = (int32_t)h; p.d_v = (int32_t)dv;
    auto lse_strides = [&](const at::Tensor& l) { return packed ? fa_lse_strides{0, l.stride(0), l.stride(1)} : fa_lse_strides{l.stride(0), l.stride(1), l.stride(2)}; };
    for (size_t i = 0; i < outs.size(); ++i) {
        const at::Tensor& o = outs[i];
        const at::Tensor& l = lses[i];
        TORCH_CHECK(o.sizes() == o0.sizes() && o.scalar_type() == o0.scalar_type(), "outs[", i, "] must have the shape and dtype of outs[0]");
        TORCH_CHECK(l.scalar_type() == torch::kFloat32 && l.dim() == o0.dim() - 1 && l.size(-1) == rows && l.size(-2) == h && (packed || l.size(0) == b),
                    "lses[", i, "] must be a float32 tensor ", packed ? "(h, total)" : "(b, h, rows)");
        check_same_device(o0, o, "outs[i]"); check_same_device(o0, l, "lses[i]");
        p.o[i] = o.data_ptr(); p.o_stride[i] = packed ? strides3(o) : strides4(o);
        p.lse[i] = l.data_ptr<float>(); p.lse_stride[i] = lse_strides(l);
    }
    c10::DeviceGuard guard(o0.device());
    at::Tensor out = torch::empty(o0.sizes(), o0.options());
    at::Tensor lse = packed ? torch::empty({h, rows}, o0.options().dtype(torch::kFloat32)) : torch::empty({b, h, rows}, o0.options().dtype(torch::kFloat32));
    p.out = out.data_ptr(); p.out_stride = packed ? strides3(out) : strides4(out);
    p.lse_out = lse.data_ptr<float>(); p.lse_out_stride = lse_strides(lse);
    p.stream = current_stream(o0);
    check_status(fa_run_merge_states(&p));
    return {out, lse};
}

// The backward of MLA prefill attention (fa_run_mla_prefill_bwd): dout / out shaped like the forward's out, lse as the forward returned it -> [dq, dk, dv],
// contiguous and shaped like q / k / v.  Nothing is copied: the tensors go to the library with the strides they have.  D (dsoftmax_sum) is allocated here.
// phases: 0 = the call; 1 / 2 = only the dq or the dk / dv launch (measurements; 2 takes the D of an earlier call as `dsoftmax_sum`).
std::vector<at::Tensor> mha_bwd_mla_prefill(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor out, at::Tensor lse, c10::optional<at::Tensor> cu_seqlens_q_,
                                            c10::optional<at::Tensor> cu_seqlens_k_, bool is_causal, c10::optional<double> softmax_scale, int64_t phases,
                                            c10::optional<at::Tensor> dsoftmax_sum_) {
    const bool packed = check_mla_prefill_qkv(q, k, v, cu_seqlens_q_, cu_seqlens_k_);
    check_same_device(q, out, "out"); check_same_device(q, dout, "dout"); check_same_device(q, lse, "lse");
    TORCH_CHECK(out.scalar_type() == q.scalar_type() && dout.scalar_type() == q.scalar_type(), "out and dout must have the dtype of q");
    const MlaPrefillShape s = check_mla_prefill_shapes(q, k, v, packed, cu_seqlens_q_);
    const int64_t batch_size = s.batch_size, rows_q = s.rows_q, num_heads = s.num_heads;
    std::vector<int64_t> o_shape = q.sizes().vec();
    o_shape.back() = v.size(-1);
    TORCH_CHECK(out.sizes() == at::IntArrayRef(o_shape) && dout.sizes() == at::IntArrayRef(o_shape), "out and dout must have the shape of the forward's out");
    std::vector<int64_t> l_shape = packed ? std::vector<int64_t>{num_heads, rows_q} : std::vector<int64_t>{batch_size, num_heads, rows_q};
    TORCH_CHECK(lse.scalar_type() == torch::kFloat32 && lse.is_contiguous() && lse.sizes() == at::IntArrayRef(l_shape), "lse must be the forward's: fp32, contiguous, (b, h, seqlen_q) or (h, total_q)");
    TORCH_CHECK(phases >= 0 && phases <= 2, "phases: 0 (both launches), 1 (dq) or 2 (dk / dv)");
    check_mla_prefill_cu(q, packed, cu_seqlens_q_, cu_seqlens_k_);
    c10::DeviceGuard guard(q.device());
    // dense: every element of dq / dk / dv is written; packed: the rows past cu_seqlens[-1] are not touched.  Without a query row nothing is launched and
    // dk / dv are zero by definition.
    const bool no_rows = batch_size == 0 || rows_q == 0;
    at::Tensor dq = torch::empty(q.sizes(), q.options()), dk = no_rows ? torch::zeros(k.sizes(), k.options()) : torch::empty(k.sizes(), k.options()),
               dv = no_rows ? torch::zeros(v.sizes(), v.options()) : torch::empty(v.sizes(), v.options());
    at::Tensor dsum;
    if (dsoftmax_sum_.has_value()) {
        dsum = *dsoftmax_sum_;
        check_same_device(q, dsum, "dsoftmax_sum");
        TORCH_CHECK(dsum.scalar_type() == torch::kFloat32 && dsum.is_contiguous() && dsum.sizes() == lse.sizes(), "dsoftmax_sum must be fp32, contiguous and shaped like lse");
    } else {
        dsum = torch::empty(lse.sizes(), lse.options());
    }

    fa_mla_prefill_bwd_params p;
    FA_PARAMS_INIT(p);
    p.dout = dout.data_ptr(); p.dq = dq.data_ptr(); p.dk = dk.data_ptr(); p.dv = dv.data_ptr(); p.dsoftmax_sum = dsum.data_ptr<float>();
    p.phases = (int32_t)phases;
    fill_mla_prefill(p, s, q, k, v, out, lse, cu_seqlens_q_, cu_seqlens_k_, is_causal, softmax_scale);
    p.dout_stride = strides34(dout); p.dq_stride = strides34(dq); p.dk_stride = strides34(dk); p.dv_stride = strides34(dv);
    check_status(fa_run_mla_prefill_bwd(&p, current_stream(q)));
    return {dq, dk, dv, dsum};
}

// Sparse MLA decode over a latent KV cache (fa_run_mla_sparse_fwd_kvcache): q, kv_cache, block_table, cache_seqlens as in mha_fwd_mla_kvcache; indices
// int32 (b, sq, topk), last dim contiguous, any batch / row strides: the logical key positions of each query token.  out (b, sq, h, 512) and lse (b, h, sq).
// Indices, lengths and tables are read on the device.
std::vector<at::Tensor> mha_fwd_mla_sparse_kvcache(at::Tensor q, at::Tensor kv_cache, at::Tensor indices, c10::optional<at::Tensor> cache_seqlens_, int64_t num_splits,
                                                   c10::optional<at::Tensor> block_table_, c10::optional<double> softmax_scale, int64_t head_dim_v) {
    fa_mla_sparse_params_v2 pv;
    FA_PARAMS_INIT(pv);
    check_mla_decode_inputs(q, kv_cache, num_splits, head_dim_v);
    check_same_device(q, indices, "indices");
    TORCH_CHECK(indices.scalar_type() == torch::kInt32, "indices must be an int32 tensor");
    TORCH_CHECK(indices.dim() == 3 && indices.size(0) == q.size(0) && indices.size(1) == q.size(1), "indices must have shape [batch_size, seqlen_q, topk]");
    TORCH_CHECK(indices.size(2) >= 1 && indices.size(2) <= INT32_MAX && indices.stride(2) == 1, "indices: topk must be >= 1 and the last dimension contiguous");
    mla_decode_table_and_lengths(pv, q, kv_cache, block_table_, cache_seqlens_);
    c10::DeviceGuard guard(q.device());
    pv.indices = indices.data_ptr<int32_t>(); pv.topk = (int32_t)indices.size(2);
    pv.indices_batch_stride = indices.stride(0); pv.indices_row_stride = indices.stride(1);
    std::vector<at::Tensor> out = mla_decode_outputs(pv, q, kv_cache, num_splits, softmax_scale, head_dim_v);
    fa_mla_sparse_params& p = reinterpret_cast<fa_mla_sparse_params&>(pv);
    at::Tensor workspace = attach_workspace(p, fa_mla_sparse_workspace_bytes(&p), q);
    check_status(fa_run_mla_sparse_fwd_kvcache(&p, current_stream(q)));
    return out;
}

// The DeepSeek-V3.2 indexer (fa_run_mla_indexer_logits / fa_run_mla_indexer_topk).  The Python layer has checked shapes and views; here the tensors become
// pointers and strides.  logits (b, sq, capacity) fp32 is the caller's buffer: entries at or past a token's visible length are not written.
// run: fa_run_mla_indexer_logits (a workgroup per token) or fa_run_mla_indexer_prefill_logits (a workgroup per tile of tokens): one struct, one set of checks.
static void mla_indexer_logits_with(int (*run)(const fa_mla_indexer_params_v2*, void*), at::Tensor q_idx, at::Tensor weights, at::Tensor k_idx_cache, at::Tensor cache_seqlens,
                                    at::Tensor logits, c10::optional<at::Tensor> k_scale_, c10::optional<at::Tensor> block_table_, bool is_causal) {
    TORCH_CHECK(q_idx.dim() == 4 && weights.dim() == 3 && k_idx_cache.dim() == 3 && logits.dim() == 3, "q_idx (b, sq, h, 128), weights (b, sq, h), k_idx_cache (b, capacity, 128), logits (b, sq, capacity)");
    TORCH_CHECK(q_idx.is_cuda(), "q_idx must be a GPU (HIP) tensor");
    for (const at::Tensor* t : {&weights, &k_idx_cache, &cache_seqlens, &logits}) TORCH_CHECK(t->device() == q_idx.device(), "every tensor must be on q_idx's device");
    TORCH_CHECK(weights.scalar_type() == torch::kFloat32 && logits.scalar_type() == torch::kFloat32, "weights and logits must be float32");
    TORCH_CHECK(cache_seqlens.scalar_type() == torch::kInt32 && cache_seqlens.dim() == 1 && cache_seqlens.size(0) == q_idx.size(0) && cache_seqlens.is_contiguous(),
                "cache_seqlens must be a contiguous int32 tensor of shape [batch_size]");
    const bool fp8 = k_idx_cache.element_size() == 1, q8 = q_idx.element_size() == 1;      // (q8: e4m3 codes; the strides below then count bytes, as q_format asks)
    TORCH_CHECK(fp8 || (!q8 && k_idx_cache.scalar_type() == q_idx.scalar_type()), "k_idx_cache must have the dtype of q_idx or hold e4m3 codes; e4m3 q_idx needs an e4m3 cache");
    TORCH_CHECK(q_idx.stride(3) == 1 && k_idx_cache.stride(2) == 1 && logits.stride(2) == 1, "q_idx, k_idx_cache, logits: last dimension must be contiguous");
    const int64_t batch_size = q_idx.size(0), seqlen_q = q_idx.size(1);
    int64_t seqlen_cache = k_idx_cache.size(1);
    c10::DeviceGuard guard(q_idx.device());
    fa_mla_indexer_params_v2 p;
    FA_PARAMS_INIT(p);
    if (block_table_.has_value()) seqlen_cache = attach_block_table(p, q_idx, batch_size, *block_table_, k_idx_cache, true);
    TORCH_CHECK(logits.size(0) == batch_size && logits.size(1) == seqlen_q && logits.size(2) == seqlen_cache, "logits must have shape [batch_size, seqlen_q, capacity]");
    p.q_idx = q_idx.data_ptr(); p.weights = weights.data_ptr<float>(); p.k_idx_cache = k_idx_cache.data_ptr(); p.logits = logits.data_ptr<float>();
    p.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
    if (k_scale_.has_value()) {
        const at::Tensor& ks = *k_scale_;
        check_same_device(q_idx, ks, "k_scale");
        TORCH_CHECK(ks.scalar_type() == torch::kFloat32 && ks.dim() == 2, "k_scale must be a float32 tensor with one value per cached token");
        p.k_scale = ks.data_ptr<float>(); p.k_scale_batch_stride = ks.stride(0); p.k_scale_row_stride = ks.stride(1);
    }
    p.b = (int32_t)batch_size; p.seqlen_q = (int32_t)seqlen_q; p.seqlen_cache = (int32_t)seqlen_cache;
    p.h = (int32_t)q_idx.size(2); p.d = (int32_t)q_idx.size(3); p.dtype = q8 ? FA_BF16 : fa_dtype_of(q_idx);      // (q8: a valid value that is not used)
    p.k_format = fp8 ? FA_IDX_K_FP8_E4M3 : FA_MLA_KV_16BIT; p.q_format = q8 ? FA_IDX_Q_FP8_E4M3 : FA_IDX_Q_16BIT; p.is_causal = is_causal;
    p.q_idx_stride = strides4(q_idx);
    p.weights_stride = fa_strides{weights.stride(0), weights.stride(1), weights.stride(2)};
    p.k_cache_batch_stride = k_idx_cache.stride(0); p.k_cache_row_stride = k_idx_cache.stride(1);      // (FP8: a 1-byte dtype, so these are bytes, as the format asks)
    p.logits_batch_stride = logits.stride(0); p.logits_row_stride = logits.stride(1);
    check_status(run(&p, current_stream(q_idx)));
}

void mla_indexer_logits(at::Tensor q_idx, at::Tensor weights, at::Tensor k_idx_cache, at::Tensor cache_seqlens, at::Tensor logits,
                        c10::optional<at::Tensor> k_scale_, c10::optional<at::Tensor> block_table_, bool is_causal) {
    mla_indexer_logits_with(fa_run_mla_indexer_logits_v2, q_idx, weights, k_idx_cache, cache_seqlens, logits, k_scale_, block_table_, is_causal);
}

void mla_indexer_prefill_logits(at::Tensor q_idx, at::Tensor weights, at::Tensor k_idx_cache, at::Tensor cache_seqlens, at::Tensor logits,
                                c10::optional<at::Tensor> k_scale_, c10::optional<at::Tensor> block_table_, bool is_causal) {
    mla_indexer_logits_with(fa_run_mla_indexer_prefill_logits_v2, q_idx, weights, k_idx_cache, cache_seqlens, logits, k_scale_, block_table_, is_causal);
}

void mla_indexer_topk(at::Tensor logits, at::Tensor cache_seqlens, at::Tensor indices, bool is_causal) {
    TORCH_CHECK(logits.dim() == 3 && indices.dim() == 3 && logits.is_cuda(), "logits (b, sq, capacity) and indices (b, sq, topk) must be GPU (HIP) tensors");
    TORCH_CHECK(indices.device() == logits.device() && cache_seqlens.device() == logits.device(), "every tensor must be on logits' device");
    TORCH_CHECK(logits.scalar_type() == torch::kFloat32 && (logits.stride(2) == 1 || logits.size(2) <= 1), "logits must be float32 with a contiguous last dimension");
    TORCH_CHECK(indices.scalar_type() == torch::kInt32 && indices.is_contiguous(), "indices must be a contiguous int32 tensor");
    TORCH_CHECK(indices.size(0) == logits.size(0) && indices.size(1) == logits.size(1), "indices must have shape [batch_size, seqlen_q, topk]");
    TORCH_CHECK(cache_seqlens.scalar_type() == torch::kInt32 && cache_seqlens.dim() == 1 && cache_seqlens.size(0) == logits.size(0) && cache_seqlens.is_contiguous(),
                "cache_seqlens must be a contiguous int32 tensor of shape [batch_size]");
    TORCH_CHECK(logits.size(2) <= INT32_MAX && indices.size(2) <= INT32_MAX, "capacity and topk must fit in int32");
    c10::DeviceGuard guard(logits.device());
    fa_mla_topk_params p;
    FA_PARAMS_INIT(p);
    p.logits = logits.data_ptr<float>(); p.indices = indices.data_ptr<int32_t>(); p.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
    p.b = (int32_t)logits.size(0); p.seqlen_q = (int32_t)logits.size(1); p.seqlen_cache = (int32_t)logits.size(2); p.topk = (int32_t)indices.size(2);
    p.is_causal = is_causal;
    p.logits_batch_stride = logits.stride(0); p.logits_row_stride = logits.stride(1);
    check_status(fa_run_mla_indexer_topk(&p, current_stream(logits)));
}

// Stand-alone append and gather for the MLA caches (fa_run_mla_cache_append / fa_run_mla_cache_gather / fa_run_mla_index_cache_append).  The Python layer has
// checked shapes, dtypes and views; here the tensors become pointers and strides.  Dense rows are (b, n, ..), packed rows (total, ..) with cu_seqlens.
void mla_cache_append(at::Tensor kv_cache, at::Tensor kv_new, at::Tensor cache_seqlens, c10::optional<at::Tensor> k_pe_, c10::optional<at::Tensor> block_table_,
                      c10::optional<at::Tensor> cu_seqlens_new_) {
    TORCH_CHECK(kv_cache.is_cuda() && kv_new.is_cuda(), "kv_cache, kv_new must be GPU (HIP) tensors");
    const bool packed = cu_seqlens_new_.has_value();
    TORCH_CHECK(kv_cache.dim() == 4 && kv_new.dim() == (packed ? 3 : 4), "kv_cache (b, capacity, 1, 576 | 656), kv_new (b, s_new, 1, w) or packed (total_new, 1, w)");
    const int64_t batch_size = cache_seqlens.size(0);
    c10::DeviceGuard guard(kv_cache.device());
    fa_mla_cache_append_params p;
    FA_PARAMS_INIT(p);
    int64_t seqlen_cache = kv_cache.size(1);
    if (block_table_.has_value()) seqlen_cache = attach_block_table(p, kv_cache, batch_size, *block_table_, kv_cache);
    p.kv_cache = kv_cache.data_ptr(); p.kv_new = kv_new.data_ptr();
    p.cache_seqlens = cache_seqlens_ptr(kv_cache, batch_size, cache_seqlens);
    p.b = (int32_t)batch_size; p.seqlen_cache = (int32_t)seqlen_cache; p.dtype = fa_dtype_of(kv_new);
    p.kv_format = kv_cache.element_size() == 1 ? FA_MLA_KV_FP8_ROWS656 : FA_MLA_KV_16BIT;
    p.kv_cache_stride = fa_strides{kv_cache.stride(0), kv_cache.stride(1), 0};
    auto rows = [&](const at::Tensor& t) { return packed ? fa_strides{0, t.stride(0), 0} : fa_strides{t.stride(0), t.stride(1), 0}; };
    p.kv_new_stride = rows(kv_new);
    if (k_pe_.has_value()) {
        check_same_device(kv_cache, *k_pe_, "k_pe");
        p.k_pe = k_pe_->data_ptr(); p.k_pe_stride = rows(*k_pe_);
    }
    if (packed) {
        check_same_device(kv_cache, *cu_seqlens_new_, "cu_seqlens_new");
        p.cu_seqlens_new = cu_seqlens_new_->data_ptr<int32_t>(); p.total_new = kv_new.size(0);
    } else {
        p.seqlen_new = (int32_t)kv_new.size(1);
    }
    check_status(fa_run_mla_cache_append(&p, current_stream(kv_cache)));
}

void mla_cache_gather(at::Tensor kv_cache, c10::optional<at::Tensor> cache_seqlens_, at::Tensor out, c10::optional<at::Tensor> block_table_,
                      c10::optional<at::Tensor> cu_seqlens_out_, c10::optional<at::Tensor> seq_starts_, int64_t batch_size) {
    TORCH_CHECK(kv_cache.is_cuda() && out.is_cuda(), "kv_cache, out must be GPU (HIP) tensors");
    const bool packed = cu_seqlens_out_.has_value();
    TORCH_CHECK(kv_cache.dim() == 4 && out.dim() == (packed ? 2 : 3), "kv_cache (b, capacity, 1, 576 | 656), out (b, n, 576) or packed (total, 576)");
    c10::DeviceGuard guard(kv_cache.device());
    fa_mla_cache_gather_params p;
    FA_PARAMS_INIT(p);
    int64_t seqlen_cache = kv_cache.size(1);
    if (block_table_.has_value()) seqlen_cache = attach_block_table(p, kv_cache, batch_size, *block_table_, kv_cache);
    p.kv_cache = kv_cache.data_ptr(); p.out = out.data_ptr();
    p.cache_seqlens = cache_seqlens_ptr(kv_cache, batch_size, cache_seqlens_);
    p.b = (int32_t)batch_size; p.seqlen_cache = (int32_t)seqlen_cache; p.dtype = fa_dtype_of(out);
    p.kv_format = kv_cache.element_size() == 1 ? FA_MLA_KV_FP8_ROWS656 : FA_MLA_KV_16BIT;
    p.kv_cache_stride = fa_strides{kv_cache.stride(0), kv_cache.stride(1), 0};
    if (packed) {
        check_same_device(kv_cache, *cu_seqlens_out_, "cu_seqlens_out");
        p.cu_seqlens_out = cu_seqlens_out_->data_ptr<int32_t>(); p.total_out = out.size(0); p.out_row_stride = out.stride(0);
    } else {
        p.seqlen_out = (int32_t)out.size(1); p.out_batch_stride = out.stride(0); p.out_row_stride = out.stride(1);
    }
    if (seq_starts_.has_value()) {
        check_same_device(kv_cache, *seq_starts_, "seq_starts");
        p.seq_starts = seq_starts_->data_ptr<int32_t>();
    }
    check_status(fa_run_mla_cache_gather(&p, current_stream(kv_cache)));
}

void mla_index_cache_append(at::Tensor k_idx_cache, at::Tensor k_idx_new, at::Tensor cache_seqlens, c10::optional<at::Tensor> k_scale_,
                            c10::optional<at::Tensor> block_table_, c10::optional<at::Tensor> cu_seqlens_new_, int64_t scale_format) {
    TORCH_CHECK(k_idx_cache.is_cuda() && k_idx_new.is_cuda(), "k_idx_cache, k_idx_new must be GPU (HIP) tensors");
    const bool packed = cu_seqlens_new_.has_value();
    TORCH_CHECK(k_idx_cache.dim() == 3 && k_idx_new.dim() == (packed ? 2 : 3), "k_idx_cache (b, capacity, 128), k_idx_new (b, s_new, 128) or packed (total_new, 128)");
    const int64_t batch_size = cache_seqlens.size(0);
    c10::DeviceGuard guard(k_idx_cache.device());
    fa_mla_index_cache_append_params p;
    FA_PARAMS_INIT(p);
    int64_t seqlen_cache = k_idx_cache.size(1);
    if (block_table_.has_value()) seqlen_cache = attach_block_table(p, k_idx_cache, batch_size, *block_table_, k_idx_cache);
    p.k_idx_cache = k_idx_cache.data_ptr(); p.k_idx_new = k_idx_new.data_ptr();
    p.cache_seqlens = cache_seqlens_ptr(k_idx_cache, batch_size, cache_seqlens);
    p.b = (int32_t)batch_size; p.seqlen_cache = (int32_t)seqlen_cache; p.dtype = fa_dtype_of(k_idx_new);
    p.k_format = k_idx_cache.element_size() == 1 ? FA_IDX_K_FP8_E4M3 : FA_MLA_KV_16BIT; p.scale_format = (int32_t)scale_format;
    p.k_cache_batch_stride = k_idx_cache.stride(0); p.k_cache_row_stride = k_idx_cache.stride(1);      // (FP8: a 1-byte dtype, so these are bytes, as the format asks)
    if (k_scale_.has_value()) {
        const at::Tensor& ks = *k_scale_;
        check_same_device(k_idx_cache, ks, "k_scale");
        TORCH_CHECK(ks.scalar_type() == torch::kFloat32 && ks.dim() == 2, "k_scale must be a float32 tensor with one value per cached token");
        p.k_scale = ks.data_ptr<float>(); p.k_scale_batch_stride = ks.stride(0); p.k_scale_row_stride = ks.stride(1);
    }
    if (packed) {
        check_same_device(k_idx_cache, *cu_seqlens_new_, "cu_seqlens_new");
        p.cu_seqlens_new = cu_seqlens_new_->data_ptr<int32_t>(); p.total_new = k_idx_new.size(0); p.k_new_row_stride = k_idx_new.stride(0);
    } else {
        p.seqlen_new = (int32_t)k_idx_new.size(1); p.k_new_batch_stride = k_idx_new.stride(0); p.k_new_row_stride = k_idx_new.stride(1);
    }
    check_status(fa_run_mla_index_cache_append(&p, current_stream(k_idx_cache)));
}

// ---- autograd nodes in C++ ------------------------------------------------------------------------------------------------------
// The reference ships the four raw functions only; its README's flash_attn_func is an older Python-level API.  The differentiable wrappers
// of this package used to be torch.autograd.Function subclasses in Python: ~85 us of host time per forward + backward, more than the GPU
// work of a b1 x 512-token call (58 us).  As C++ nodes the same pair costs the host 42-52 us (tools/host_overhead.py, profiles/r4_host_overhead.log).
class FlashAttnNode : public torch::autograd::Function<FlashAttnNode> {
public:
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor q, at::Tensor k, at::Tensor v, bool is_causal) {
        at::AutoDispatchBelowADInplaceOrView below;
        std::vector<at::Tensor> r = mha_fwd(q, k, v, is_causal);
        ctx->save_for_backward({q, k, v, r[0], r[1]});
        ctx->saved_data["causal"] = is_causal;
        return r[0];
    }
    static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list grads) {
        const torch::autograd::variable_list s = ctx->get_saved_variables();
        std::vector<at::Tensor> g = mha_bwd(s[0], s[1], s[2], s[3], s[4], grads[0], ctx->saved_data["causal"].toBool());      // strided dout is fine
        return {g[0], g[1], g[2], at::Tensor()};
    }
};
class FlashAttnVarlenNode : public torch::autograd::Function<FlashAttnVarlenNode> {
public:
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor cu_seqlens_q, at::Tensor cu_seqlens_k,
                              int64_t max_seqlen_q, int64_t max_seqlen_k, bool is_causal) {
        at::AutoDispatchBelowADInplaceOrView below;
        std::vector<at::Tensor> r = mha_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, (int)max_seqlen_q, (int)max_seqlen_k, is_causal);
        ctx->save_for_backward({q, k, v, r[0], r[1], cu_seqlens_q, cu_seqlens_k});
        ctx->saved_data["causal"] = is_causal;
        ctx->saved_data["max_q"] = max_seqlen_q;
        ctx->saved_data["max_k"] = max_seqlen_k;
        return r[0];
    }
    static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list grads) {
        const torch::autograd::variable_list s = ctx->get_saved_variables();
        std::vector<at::Tensor> g = mha_varlen_bwd(s[0], s[1], s[2], s[3], s[4], grads[0], s[5], s[6], (int)ctx->saved_data["max_q"].toInt(),
                                                   (int)ctx->saved_data["max_k"].toInt(), ctx->saved_data["causal"].toBool());
        return {g[0], g[1], g[2], at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};
static at::Tensor attn_autograd(at::Tensor q, at::Tensor k, at::Tensor v, bool is_causal) { return FlashAttnNode::apply(q, k, v, is_causal); }
static at::Tensor attn_varlen_autograd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor cu_seqlens_q, at::Tensor cu_seqlens_k, int64_t max_seqlen_q,
                                       int64_t max_seqlen_k, bool is_causal) {
    return FlashAttnVarlenNode::apply(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "MI355X (gfx950) fused attention behind the flash_attn_turing surface";
    m.def("fwd", &mha_fwd, "Forward pass");
    m.def("bwd", &mha_bwd,
          "Backward pass.\n\n"
          "Dynamic range: over the finite range the result is the reference algorithm with its two 16-bit rounding points (P and dS = P (dP - D),\n"
          "rounded to nearest before the second GEMMs; D, dP and every sum in fp32; dQ, dK, dV rounded once at the end).  In fp16: while |dO|, |dP|\n"
          "and the sums stay below 65504, and down to where dS underflows - subnormal inputs, subnormal dS and subnormal outputs are honoured, not\n"
          "flushed (a dO of 1e-5 is made of fp16 subnormals).  bf16 keeps fp32's exponent range: scaling dO, V or the pair (q, 1 / k) by a power of\n"
          "two scales the results by exactly that power, bit for bit.  A non-finite backward is unspecified (include/flash_attn_gfx950.h).");
    m.def("varlen_fwd", &mha_varlen_fwd, "Varlen forward pass");
    m.def("varlen_bwd", &mha_varlen_bwd, "Varlen backward pass");
    m.def("fwd_mla_kvcache", &mha_fwd_mla_kvcache, "MLA decode over a latent KV cache: q (b, sq, h, 576), kv_cache (b, capacity, 1, 576) -> [out (b, sq, h, 512), lse]",
          py::arg("q"), py::arg("kv_cache"), py::arg("kv_new") = py::none(), py::arg("cache_seqlens") = py::none(), py::arg("is_causal") = false,
          py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("softmax_scale") = py::none(), py::arg("head_dim_v") = 512);
    m.def("fwd_mla_sparse_kvcache", &mha_fwd_mla_sparse_kvcache,
          "Sparse MLA decode over a latent KV cache: q (b, sq, h, 576), kv_cache (b, capacity, 1, 576), indices int32 (b, sq, topk) -> [out (b, sq, h, 512), lse]",
          py::arg("q"), py::arg("kv_cache"), py::arg("indices"), py::arg("cache_seqlens") = py::none(), py::arg("num_splits") = 0,
          py::arg("block_table") = py::none(), py::arg("softmax_scale") = py::none(), py::arg("head_dim_v") = 512);
    m.def("fwd_mla_prefill", &mha_fwd_mla_prefill,
          "MLA prefill attention: q (b, sq, h, 192), k (b, sk, h_k, 192), v (b, sk, h_k, 128) -> [out (b, sq, h, 128), lse]; packed with both cu_seqlens",
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("cu_seqlens_q") = py::none(), py::arg("cu_seqlens_k") = py::none(), py::arg("is_causal") = false,
          py::arg("softmax_scale") = py::none());
    m.def("bwd_mla_prefill", &mha_bwd_mla_prefill,
          "MLA prefill backward: dout, q, k, v, out, lse -> [dq, dk, dv, dsoftmax_sum]; packed with both cu_seqlens",
          py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("lse"), py::arg("cu_seqlens_q") = py::none(),
          py::arg("cu_seqlens_k") = py::none(), py::arg("is_causal") = false, py::arg("softmax_scale") = py::none(), py::arg("phases") = 0,
          py::arg("dsoftmax_sum") = py::none());
    m.def("merge_states", &merge_states, "merge 2 .. 8 partial attention states (outs[i], lses[i]) of the same query rows -> [out, lse]; dense or packed", py::arg("outs"),
          py::arg("lses"));
    m.def("mla_indexer_logits", &mla_indexer_logits,"index logits of the DeepSeek-V3.2 indexer into the caller's fp32 buffer (b, sq, capacity)", py::arg("q_idx"), py::arg("weights"),
          py::arg("k_idx_cache"), py::arg("cache_seqlens"), py::arg("logits"), py::arg("k_scale") = py::none(), py::arg("block_table") = py::none(), py::arg("is_causal") = true);
    m.def("mla_indexer_prefill_logits", &mla_indexer_prefill_logits, "the same index logits for a prompt chunk: a workgroup per tile of tokens, the bits of mla_indexer_logits",
          py::arg("q_idx"), py::arg("weights"), py::arg("k_idx_cache"), py::arg("cache_seqlens"), py::arg("logits"), py::arg("k_scale") = py::none(),
          py::arg("block_table") = py::none(), py::arg("is_causal") = true);
    m.def("mla_cache_append", &mla_cache_append, "append latent rows (16-bit, or quantised to 656-byte FP8 rows) to the MLA latent cache, in place", py::arg("kv_cache"),
          py::arg("kv_new"), py::arg("cache_seqlens"), py::arg("k_pe") = py::none(), py::arg("block_table") = py::none(), py::arg("cu_seqlens_new") = py::none());
    m.def("mla_cache_gather", &mla_cache_gather, "gather (and dequantise) rows of the MLA latent cache into the caller's buffer", py::arg("kv_cache"),
          py::arg("cache_seqlens"), py::arg("out"), py::arg("block_table") = py::none(), py::arg("cu_seqlens_out") = py::none(), py::arg("seq_starts") = py::none(),
          py::arg("batch_size") = 0);
    m.def("mla_index_cache_append", &mla_index_cache_append, "append index keys (16-bit, or e4m3 codes with one scale per token) to the index-key cache, in place",
          py::arg("k_idx_cache"), py::arg("k_idx_new"), py::arg("cache_seqlens"), py::arg("k_scale") = py::none(), py::arg("block_table") = py::none(),
          py::arg("cu_seqlens_new") = py::none(), py::arg("scale_format") = 0);
    m.def("mla_indexer_topk", &mla_indexer_topk, "top-k positions of every logits row into the caller's int32 buffer (b, sq, topk)", py::arg("logits"), py::arg("cache_seqlens"),
          py::arg("indices"), py::arg("is_causal") = true);
    // three overloads: the signature as it was (every existing call, positional or keyword, resolves to it), the one that continues it with the
    // ragged-batch keywords after rotary_interleaved, and the one that continues that with softmax_scale / softcap
    m.def("fwd_kvcache",
          [](at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new, c10::optional<at::Tensor> cache_seqlens,
             bool is_causal, int64_t num_splits, c10::optional<at::Tensor> block_table, int64_t window_size_left, int64_t window_size_right,
             c10::optional<at::Tensor> k_descale, c10::optional<at::Tensor> v_descale, c10::optional<at::Tensor> rotary_cos, c10::optional<at::Tensor> rotary_sin,
             bool rotary_interleaved) {
              return mha_fwd_kvcache(q, k_cache, v_cache, k_new, v_new, cache_seqlens, is_causal, num_splits, block_table, window_size_left, window_size_right, k_descale,
                                     v_descale, rotary_cos, rotary_sin, rotary_interleaved, c10::nullopt, 0, c10::nullopt, c10::nullopt, 0.0, c10::nullopt, c10::nullopt, false);
          },
          "Decode forward over a KV cache (in-place append of k / v, split-KV attention)", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k_new") = py::none(), py::arg("v_new") = py::none(), py::arg("cache_seqlens") = py::none(),
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("window_size_left") = -1,
          py::arg("window_size_right") = -1, py::kw_only(), py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(),
          py::arg("rotary_cos") = py::none(), py::arg("rotary_sin") = py::none(), py::arg("rotary_interleaved") = true);
    m.def("fwd_kvcache",
          [](at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new, c10::optional<at::Tensor> cache_seqlens,
             bool is_causal, int64_t num_splits, c10::optional<at::Tensor> block_table, int64_t window_size_left, int64_t window_size_right,
             c10::optional<at::Tensor> k_descale, c10::optional<at::Tensor> v_descale, c10::optional<at::Tensor> rotary_cos, c10::optional<at::Tensor> rotary_sin,
             bool rotary_interleaved, c10::optional<at::Tensor> cu_seqlens_q, int64_t max_seqlen_q, c10::optional<at::Tensor> cu_seqlens_k_new) {
              return mha_fwd_kvcache(q, k_cache, v_cache, k_new, v_new, cache_seqlens, is_causal, num_splits, block_table, window_size_left, window_size_right, k_descale,
                                     v_descale, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new, c10::nullopt, 0.0, c10::nullopt, c10::nullopt, false);
          },
          "The same with a ragged query batch: packed q / k / v under cu_seqlens_q / cu_seqlens_k_new", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k_new") = py::none(), py::arg("v_new") = py::none(), py::arg("cache_seqlens") = py::none(),
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("window_size_left") = -1,
          py::arg("window_size_right") = -1, py::kw_only(), py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(),
          py::arg("rotary_cos") = py::none(), py::arg("rotary_sin") = py::none(), py::arg("rotary_interleaved") = true,
          py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 0, py::arg("cu_seqlens_k_new") = py::none());
    m.def("fwd_kvcache",
          [](at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new, c10::optional<at::Tensor> cache_seqlens,
             bool is_causal, int64_t num_splits, c10::optional<at::Tensor> block_table, int64_t window_size_left, int64_t window_size_right,
             c10::optional<at::Tensor> k_descale, c10::optional<at::Tensor> v_descale, c10::optional<at::Tensor> rotary_cos, c10::optional<at::Tensor> rotary_sin,
             bool rotary_interleaved, c10::optional<at::Tensor> cu_seqlens_q, int64_t max_seqlen_q, c10::optional<at::Tensor> cu_seqlens_k_new,
             c10::optional<double> softmax_scale, double softcap) {
              return mha_fwd_kvcache(q, k_cache, v_cache, k_new, v_new, cache_seqlens, is_causal, num_splits, block_table, window_size_left, window_size_right, k_descale,
                                     v_descale, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new, softmax_scale, softcap, c10::nullopt, c10::nullopt, false);
          },
          "The same with a softmax scale other than 1 / sqrt(head_dim) and / or soft-capped scores", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k_new") = py::none(), py::arg("v_new") = py::none(), py::arg("cache_seqlens") = py::none(),
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("window_size_left") = -1,
          py::arg("window_size_right") = -1, py::kw_only(), py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(),
          py::arg("rotary_cos") = py::none(), py::arg("rotary_sin") = py::none(), py::arg("rotary_interleaved") = true,
          py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 0, py::arg("cu_seqlens_k_new") = py::none(),
          py::arg("softmax_scale") = py::none(), py::arg("softcap") = 0.0);
    // Attention sinks: the same arguments continued by `sinks`.  A function of its own and not a fourth overload of fwd_kvcache - the overload set
    // of that name is what its callers resolve against, and it stays the three signatures it was: a call without sinks never comes here.
    m.def("fwd_kvcache_sinks",
          [](at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new, c10::optional<at::Tensor> cache_seqlens,
             bool is_causal, int64_t num_splits, c10::optional<at::Tensor> block_table, int64_t window_size_left, int64_t window_size_right,
             c10::optional<at::Tensor> k_descale, c10::optional<at::Tensor> v_descale, c10::optional<at::Tensor> rotary_cos, c10::optional<at::Tensor> rotary_sin,
             bool rotary_interleaved, c10::optional<at::Tensor> cu_seqlens_q, int64_t max_seqlen_q, c10::optional<at::Tensor> cu_seqlens_k_new,
             c10::optional<double> softmax_scale, double softcap, c10::optional<at::Tensor> sinks) {
              return mha_fwd_kvcache(q, k_cache, v_cache, k_new, v_new, cache_seqlens, is_causal, num_splits, block_table, window_size_left, window_size_right, k_descale,
                                     v_descale, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new, softmax_scale, softcap, sinks, c10::nullopt, false);
          },
          "fwd_kvcache with attention sinks: one float32 logit per query head in the softmax denominator", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k_new") = py::none(), py::arg("v_new") = py::none(), py::arg("cache_seqlens") = py::none(),
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("window_size_left") = -1,
          py::arg("window_size_right") = -1, py::kw_only(), py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(),
          py::arg("rotary_cos") = py::none(), py::arg("rotary_sin") = py::none(), py::arg("rotary_interleaved") = true,
          py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 0, py::arg("cu_seqlens_k_new") = py::none(),
          py::arg("softmax_scale") = py::none(), py::arg("softcap") = 0.0, py::arg("sinks") = py::none());
    // Tree attention masks: the same arguments continued by `tree_mask`, again on a function of its own - fwd_kvcache keeps its three overloads and
    // fwd_kvcache_sinks its signature, and a call without tree_mask never comes here.
    m.def("fwd_kvcache_tree",
          [](at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new, c10::optional<at::Tensor> cache_seqlens,
             bool is_causal, int64_t num_splits, c10::optional<at::Tensor> block_table, int64_t window_size_left, int64_t window_size_right,
             c10::optional<at::Tensor> k_descale, c10::optional<at::Tensor> v_descale, c10::optional<at::Tensor> rotary_cos, c10::optional<at::Tensor> rotary_sin,
             bool rotary_interleaved, c10::optional<at::Tensor> cu_seqlens_q, int64_t max_seqlen_q, c10::optional<at::Tensor> cu_seqlens_k_new,
             c10::optional<double> softmax_scale, double softcap, c10::optional<at::Tensor> sinks, c10::optional<at::Tensor> tree_mask) {
              return mha_fwd_kvcache(q, k_cache, v_cache, k_new, v_new, cache_seqlens, is_causal, num_splits, block_table, window_size_left, window_size_right, k_descale,
                                     v_descale, rotary_cos, rotary_sin, rotary_interleaved, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new, softmax_scale, softcap, sinks, tree_mask, false);
          },
          "fwd_kvcache with a tree attention mask: one int64 word per query row over the last seqlen_q keys", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k_new") = py::none(), py::arg("v_new") = py::none(), py::arg("cache_seqlens") = py::none(),
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("window_size_left") = -1,
          py::arg("window_size_right") = -1, py::kw_only(), py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(),
          py::arg("rotary_cos") = py::none(), py::arg("rotary_sin") = py::none(), py::arg("rotary_interleaved") = true,
          py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 0, py::arg("cu_seqlens_k_new") = py::none(),
          py::arg("softmax_scale") = py::none(), py::arg("softcap") = 0.0, py::arg("sinks") = py::none(), py::arg("tree_mask") = py::none());
    // 64-row kernels for prompt chunks: the same arguments continued by `prefill`, once more on a function of its own - fwd_kvcache keeps its three
    // overloads, fwd_kvcache_sinks and fwd_kvcache_tree their signatures, and a call without prefill=True never comes here.
    m.def("fwd_kvcache_prefill", &mha_fwd_kvcache, "fwd_kvcache on the 64-row attention kernels for prompt chunks (prefill=True)", py::arg("q"),
          py::arg("k_cache"), py::arg("v_cache"), py::arg("k_new") = py::none(), py::arg("v_new") = py::none(), py::arg("cache_seqlens") = py::none(),
          py::arg("is_causal") = false, py::arg("num_splits") = 0, py::arg("block_table") = py::none(), py::arg("window_size_left") = -1,
          py::arg("window_size_right") = -1, py::kw_only(), py::arg("k_descale") = py::none(), py::arg("v_descale") = py::none(),
          py::arg("rotary_cos") = py::none(), py::arg("rotary_sin") = py::none(), py::arg("rotary_interleaved") = true,
          py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 0, py::arg("cu_seqlens_k_new") = py::none(),
          py::arg("softmax_scale") = py::none(), py::arg("softcap") = 0.0, py::arg("sinks") = py::none(), py::arg("tree_mask") = py::none(),
          py::arg("prefill") = false);
    m.def("attn_autograd", &attn_autograd, "differentiable forward (C++ autograd node over fwd / bwd)");
    m.def("attn_varlen_autograd", &attn_varlen_autograd, "differentiable packed forward (C++ autograd node over varlen_fwd / varlen_bwd)");
    m.def("abi_version", []() { return fa_abi_version(); });
    m.def("build_info", []() { return std::string(fa_build_info()); });
    m.def("densify_copies", []() { return g_densify_copies.load(std::memory_order_relaxed); }, "number of hidden .contiguous() copies made so far (0 for addressable layouts)");
}
