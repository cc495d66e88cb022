// runtime_paged_varlen.hip -- the C ABI of packed variable-length queries over a paged / static KV cache (include/umfa_abi.h):
// umfa_varlen_kvcache_attention_forward_stream, with the rotary embedding of q and k_new fused into the append launch
// (fa_paged_rope.h) umfa_varlen_kvcache_attention_rope_forward_stream, and over an fp8 (e4m3fn) cache with per-(sequence, KV head)
// descales, with or without rotary (fa_paged_varlen_fp8.h), umfa_varlen_kvcache_attention_fp8_forward_stream, and with a sliding window
// over a 16-bit cache (fa_paged_varlen_window.h) umfa_varlen_kvcache_attention_window_forward_stream.  In-stream, never synchronising: cu_seqlens_q, cache_seqlens and the block table stay on
// the device, so a captured graph follows their contents on replay.  Launch order on the stream: the packed append of k_new / v_new
// (when given), the item-list pre-pass, the attention, and with split-KV the fold.  The item list and the split partials come from the
// stream's pooled workspace (a capture that would have to grow it returns MFA_ERROR_MEMORY_ALLOCATION: warm up first).  Anything
// outside the kernels' scope is MFA_ERROR_INVALID_ARGS: no silent fall-back.
#include <string.h>

#include "runtime_paged_common.h"
#include "fa_paged_varlen.h"
#include "fa_paged_rope.h"
#include "fa_paged_varlen_fp8.h"
#include "fa_paged_varlen_window.h"

using namespace umfa;
using namespace umfa_rt;

namespace {

constexpr size_t PV_HDR_B = 256;  // the tally's words at the front of the workspace block

}  // namespace

namespace {

// every entry; rope != NULL: the fused pre-pass (fa_paged_rope.h) stands in for the packed append and the attention reads its q image;
// f8 != NULL: the cache is e4m3fn with f8's descales (cache strides in bytes) and the kernels are fa_fwd_16_paged_varlen_fp8.hip's;
// win != NULL (16-bit caches): the banded kernel (fa_paged_varlen_window.h) stands in for the attention, `causal` then only places the
// rotary positions of q
mfa_error_t varlen_kvcache_forward(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache,
                                   const int64_t* k_cache_strides, void* v_cache, const int64_t* v_cache_strides, const void* k_new,
                                   const int64_t* k_new_strides, const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                   int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q, uint32_t batch,
                                   uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads,
                                   uint32_t num_kv_heads, uint16_t head_dim, uint32_t page_size, uint32_t num_pages,
                                   uint32_t max_pages_per_seq, float softmax_scale, bool causal, int32_t input_precision, void* out,
                                   int32_t out_precision, float* lse, int32_t num_splits, const RopeArgs* rope,
                                   const PagedVarlenFp8Params* f8 = nullptr, const WindowArgs* win = nullptr) {
    Context* ctx = as_ctx(context);
    if (win && f8) return MFA_ERROR_INVALID_ARGS;
    if (rope && (!has_new || !rope->cos || !rope->sin || rope->table_f32 < 0))
        return MFA_ERROR_INVALID_ARGS;
    if (!ctx || !out || !q || !k_cache || !v_cache || !cache_seqlens || !cu_seqlens_q || !k_cache_strides || !v_cache_strides)
        return MFA_ERROR_INVALID_ARGS;
    if (input_precision != MFA_PRECISION_FP16 && input_precision != MFA_PRECISION_BF16) return MFA_ERROR_INVALID_ARGS;
    if (out_precision != MFA_PRECISION_FP32 && out_precision != input_precision) return MFA_ERROR_INVALID_ARGS;
    if (!(softmax_scale > 0.0f) || ((uintptr_t)cache_seqlens & 3) || ((uintptr_t)block_table & 3) || ((uintptr_t)cu_seqlens_q & 3) || num_splits < 0)
        return MFA_ERROR_INVALID_ARGS;
    if (has_new && (!k_new || !v_new || !k_new_strides || !v_new_strides)) return MFA_ERROR_INVALID_ARGS;
    if (block_table && block_table_stride < (int64_t)max_pages_per_seq) return MFA_ERROR_INVALID_ARGS;
    if (max_seqlen_q > total_q) return MFA_ERROR_INVALID_ARGS;
    PagedVarlenFp8Params f;
    memset(&f, 0, sizeof(f));
    if (f8) f = *f8;
    PagedVarlenParams& v = f.v;
    memset(&v, 0, sizeof(v));
    PagedParams& p = v.p;
    p.q = q; p.kc = k_cache; p.vc = v_cache; p.bt = block_table; p.seqlens = cache_seqlens;
    p.out = out; p.lse = lse;
    v.cu = cu_seqlens_q; v.Tq = total_q;
    p.B = batch; p.Sq = max_seqlen_q; p.Snew = has_new ? 1 : 0; p.H = num_heads; p.Hkv = num_kv_heads; p.D = head_dim;
    p.page_size = page_size;
    // static cache: page b is sequence b's row of S_max = page_size tokens
    p.num_pages = block_table ? num_pages : batch;
    p.max_pages = block_table ? max_pages_per_seq : 1;
    p.bt_stride = block_table ? block_table_stride : 0;
    p.page_shift = (page_size && !(page_size & (page_size - 1))) ? __builtin_ctz(page_size) : -1;
    p.qst = q_strides ? q_strides[0] : (int64_t)num_heads * head_dim;
    p.qsh = q_strides ? q_strides[1] : (int64_t)head_dim;
    p.kpg = k_cache_strides[0]; p.kst = k_cache_strides[1]; p.ksh = k_cache_strides[2];
    p.vpg = v_cache_strides[0]; p.vst = v_cache_strides[1]; p.vsh = v_cache_strides[2];
    if (has_new) {
        p.kn = k_new; p.vn = v_new;
        p.knt = k_new_strides[0]; p.knh = k_new_strides[1];
        p.vnt = v_new_strides[0]; p.vnh = v_new_strides[1];
    }
    p.scale = softmax_scale;
    p.causal = causal ? 1 : 0;
    p.in_prec = dense_prec(input_precision);
    p.out_prec = dense_prec(out_precision);
    if (num_kv_heads == 0 || num_heads % num_kv_heads) return MFA_ERROR_INVALID_ARGS;
    p.nsplit = 1;
    v.n_items = paged_varlen_item_bound(v);
    auto supported = [&]() {
        return f8 ? paged_varlen_fp8_supported(f) : win ? paged_varlen_window_supported(PagedVarlenWindowParams{v, win->left, win->right}) : paged_varlen_supported(v);
    };
    if (!supported() || ((uintptr_t)out & 15) || ((uintptr_t)lse & 3)) return MFA_ERROR_INVALID_ARGS;
    const char* name = "none";
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    // (automatic: kvcache_attention's rule on the item bound -- runtime_paged_common.h)
    p.nsplit = num_splits > 0 ? (uint32_t)(num_splits < 256 ? num_splits : 256) : paged_auto_splits(p, v.n_items, win, paged_cu_count(dev));
    if (!supported()) return MFA_ERROR_INVALID_ARGS;
    PagedRopeParams r;
    memset(&r, 0, sizeof(r));
    if (rope) {
        paged_rope_fill(r, *rope);
        r.packed = 1;
        r.v = v;
    }
    if (v.n_items || (rope && total_q)) {
        // one block of the pooled workspace: the form tally (PV_HDR_B bytes), the item list, (split) the partials, then (rotary) the
        // rotated q image; every check and the allocation come before the first launch
        StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);
        const size_t list_b = ((size_t)v.n_items * 2 * sizeof(int32_t) + 255) & ~(size_t)255;
        const size_t part_b = p.nsplit > 1 ? (size_t)p.nsplit * total_q * num_heads * (p.D + 2) * sizeof(float) : 0;  // (a multiple of 8 bytes)
        const size_t img_at = (PV_HDR_B + list_b + part_b + 255) & ~(size_t)255;
        const size_t need = rope ? img_at + paged_rope_qimg_bytes(r) : PV_HDR_B + list_b + part_b;  // without rotary: the size it always was
        char* const ws = (char*)sc.workspace.ensure(need, (hipStream_t)stream);
        if (!ws) return MFA_ERROR_MEMORY_ALLOCATION;
        v.counts = (uint32_t*)ws;
        v.items = (int32_t*)(ws + PV_HDR_B);
        if (part_b) p.part = (float*)(ws + PV_HDR_B + list_b);
        r.qimg = ws + img_at;
    }
    if (rope) {
        if (total_q) {
            hipError_t e;
            if (f8) {
                const PagedVarlenFp8RopeParams r8 = {f, r.cos, r.sin, r.qimg, r.rstride, r.seqlen_ro, r.rdim, r.interleaved, r.table_f32};
                if (!paged_varlen_fp8_rope_supported(r8)) return MFA_ERROR_INVALID_ARGS;
                e = launch_paged_varlen_fp8_rope(r8, (hipStream_t)stream);
            } else {
                if (!paged_rope_supported(r)) return MFA_ERROR_INVALID_ARGS;
                e = launch_paged_rope(r, (hipStream_t)stream);
            }
            if (e != hipSuccess) return rc_paged(e);
            p.q = r.qimg;
            p.qst = (int64_t)num_heads * head_dim; p.qsh = head_dim;
        }
    } else if (has_new) {
        const hipError_t e = f8 ? launch_paged_varlen_fp8_append(f, (hipStream_t)stream) : launch_paged_varlen_append(v, (hipStream_t)stream);
        if (e != hipSuccess) return rc_paged(e);
    }
    // (v as it stands here: the rotary path has pointed p.q at its image by now)
    const hipError_t e = f8    ? launch_fwd_16_paged_varlen_fp8(f, (hipStream_t)stream, &name)
                         : win ? launch_fwd_16_paged_varlen_window(PagedVarlenWindowParams{v, win->left, win->right}, (hipStream_t)stream, &name)
                               : launch_fwd_16_paged_varlen(v, (hipStream_t)stream, &name);
    ctx->last_kernel = name;
    return rc_paged(e);
}

}  // namespace

mfa_error_t umfa_varlen_kvcache_attention_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                         void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                         const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                         const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                         int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
                                                         uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new,
                                                         uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, uint32_t page_size,
                                                         uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
                                                         int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                         int32_t num_splits) {
    return varlen_kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides,
                                  v_new, v_new_strides, block_table, block_table_stride, cache_seqlens, total_q, batch, max_seqlen_q,
                                  cu_seqlens_q, has_new, num_heads, num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq,
                                  softmax_scale, causal, input_precision, out, out_precision, lse, num_splits, nullptr);
}

mfa_error_t umfa_varlen_kvcache_attention_rope_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache, const int64_t* k_cache_strides,
    void* v_cache, const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides, const void* v_new,
    const int64_t* v_new_strides, const int32_t* block_table, int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
    uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads, uint32_t num_kv_heads,
    uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
    int32_t input_precision, void* out, int32_t out_precision, float* lse, int32_t num_splits, const void* rotary_cos,
    const void* rotary_sin, int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro, uint32_t rotary_dim,
    bool rotary_interleaved) {
    const RopeArgs rope = paged_rope_args(rotary_cos, rotary_sin, rotary_table_precision == MFA_PRECISION_FP32,
                                          rotary_table_precision == input_precision, rotary_row_stride, seqlen_ro, rotary_dim, rotary_interleaved);
    return varlen_kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides,
                                  v_new, v_new_strides, block_table, block_table_stride, cache_seqlens, total_q, batch, max_seqlen_q,
                                  cu_seqlens_q, has_new, num_heads, num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq,
                                  softmax_scale, causal, input_precision, out, out_precision, lse, num_splits, &rope);
}

mfa_error_t umfa_varlen_kvcache_attention_fp8_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache, const int64_t* k_cache_strides,
    void* v_cache, const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides, const void* v_new,
    const int64_t* v_new_strides, const int32_t* block_table, int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
    uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads, uint32_t num_kv_heads,
    uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
    int32_t input_precision, void* out, int32_t out_precision, float* lse, int32_t num_splits, const float* k_descale,
    const int64_t* k_descale_strides, const float* v_descale, const int64_t* v_descale_strides, const void* rotary_cos,
    const void* rotary_sin, int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro, uint32_t rotary_dim,
    bool rotary_interleaved) {
    PagedVarlenFp8Params f8;
    memset(&f8, 0, sizeof(f8));
    if (!paged_fill_descales(f8, k_descale, k_descale_strides, v_descale, v_descale_strides)) return MFA_ERROR_INVALID_ARGS;
    if ((rotary_cos == nullptr) != (rotary_sin == nullptr)) return MFA_ERROR_INVALID_ARGS;
    const RopeArgs rope = paged_rope_args(rotary_cos, rotary_sin, rotary_table_precision == MFA_PRECISION_FP32,
                                          rotary_table_precision == input_precision, rotary_row_stride, seqlen_ro, rotary_dim, rotary_interleaved);
    return varlen_kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides,
                                  v_new, v_new_strides, block_table, block_table_stride, cache_seqlens, total_q, batch, max_seqlen_q,
                                  cu_seqlens_q, has_new, num_heads, num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq,
                                  softmax_scale, causal, input_precision, out, out_precision, lse, num_splits, rotary_cos ? &rope : nullptr,
                                  &f8);
}

mfa_error_t umfa_varlen_kvcache_attention_window_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache, const int64_t* k_cache_strides,
    void* v_cache, const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides, const void* v_new,
    const int64_t* v_new_strides, const int32_t* block_table, int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
    uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads, uint32_t num_kv_heads,
    uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
    int32_t input_precision, void* out, int32_t out_precision, float* lse, int32_t num_splits, const void* rotary_cos,
    const void* rotary_sin, int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro, uint32_t rotary_dim,
    bool rotary_interleaved, int32_t window_left, int32_t window_right) {
    if (window_left < -1 || window_right < -1) return MFA_ERROR_INVALID_ARGS;
    if ((rotary_cos == nullptr) != (rotary_sin == nullptr)) return MFA_ERROR_INVALID_ARGS;
    const uint64_t cap = block_table ? (uint64_t)max_pages_per_seq * page_size : (uint64_t)page_size;
    if (cap >= (1ull << 30) || max_seqlen_q >= (1u << 30)) return MFA_ERROR_INVALID_ARGS;
    bool plain;
    const WindowArgs w = paged_window_normalise(window_left, window_right, causal, cap, max_seqlen_q, plain);
    const RopeArgs rope = paged_rope_args(rotary_cos, rotary_sin, rotary_table_precision == MFA_PRECISION_FP32,
                                          rotary_table_precision == input_precision, rotary_row_stride, seqlen_ro, rotary_dim, rotary_interleaved);
    return varlen_kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides,
                                  v_new, v_new_strides, block_table, block_table_stride, cache_seqlens, total_q, batch, max_seqlen_q,
                                  cu_seqlens_q, has_new, num_heads, num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq,
                                  softmax_scale, causal, input_precision, out, out_precision, lse, num_splits, rotary_cos ? &rope : nullptr,
                                  nullptr, plain ? nullptr : &w);
}

// debug: the tally of the last umfa_varlen_kvcache_attention_forward_stream call on `stream` (nothing else may have used the stream's
// workspace since).  Synchronises the stream.
mfa_error_t umfa_varlen_kvcache_item_counts(mfa_context_t context, void* stream, uint32_t* decode_items, uint32_t* block_items) {
    Context* ctx = as_ctx(context);
    if (!ctx || !decode_items || !block_items) return MFA_ERROR_INVALID_ARGS;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);
    if (!sc.workspace.ptr || sc.workspace.bytes < PV_HDR_B) return MFA_ERROR_INVALID_ARGS;
    uint32_t host[2] = {0, 0};
    if (hipMemcpyAsync(host, sc.workspace.ptr, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return MFA_ERROR_EXECUTION_FAILED;
    }
    *decode_items = host[0];
    *block_items = host[1];
    return MFA_SUCCESS;
}
