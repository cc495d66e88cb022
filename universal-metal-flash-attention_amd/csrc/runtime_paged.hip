// runtime_paged.hip -- the C ABI of KV-cache attention for inference (include/umfa_abi.h): umfa_kvcache_attention_forward_stream, over an
// fp8 (e4m3fn) cache with per-(batch, KV head) descales (fa_paged_fp8.h) umfa_kvcache_attention_fp8_forward_stream, and with the rotary
// embedding of q and k_new fused into the append launch (fa_paged_rope.h) umfa_kvcache_attention_rope_forward_stream, and with a sliding
// window over a 16-bit cache (fa_paged_window.h) umfa_kvcache_attention_window_forward_stream.
// In-stream, never synchronising: cache_seqlens and the block table stay on the device (the kernels read them when they run), so a
// captured graph follows their contents on replay.  Launch order on the stream: the append of k_new / v_new (when given), the attention,
// and with split-KV the fold.  Split partials come from the stream's pooled workspace (a capture that would have to grow it returns
// MFA_ERROR_MEMORY_ALLOCATION: warm up first).  Anything outside the kernels' scope is MFA_ERROR_INVALID_ARGS: no silent fall-back.
#include <string.h>

#include "runtime_paged_common.h"
#include "fa_paged_fp8.h"
#include "fa_paged_rope.h"
#include "fa_paged_window.h"

using namespace umfa;
using namespace umfa_rt;

namespace {

// every entry: fp8 = the cache is e4m3fn with the descales in f8 (cache strides in bytes), else 16-bit in input_precision; rope != NULL:
// the fused pre-pass (fa_paged_rope.h) stands in for the append and the attention reads its q image; win != NULL (16-bit caches): the
// banded kernel (fa_paged_window.h) stands in for the attention, `causal` then only places the rotary positions of q
mfa_error_t kvcache_forward(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache,
                            const int64_t* k_cache_strides, void* v_cache, const int64_t* v_cache_strides, const void* k_new,
                            const int64_t* k_new_strides, const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                            int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t batch, uint32_t seqlen_q,
                            uint32_t seqlen_new, uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, uint32_t page_size,
                            uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal, int32_t input_precision,
                            void* out, int32_t out_precision, float* lse, int32_t num_splits, bool fp8, PagedFp8Params f8, const RopeArgs* rope = nullptr,
                            const WindowArgs* win = nullptr) {
    Context* ctx = as_ctx(context);
    if (win && fp8) return MFA_ERROR_INVALID_ARGS;
    if (rope && (!seqlen_new || !rope->cos || !rope->sin || rope->table_f32 < 0))
        return MFA_ERROR_INVALID_ARGS;
    if (!ctx || !out || !q || !k_cache || !v_cache || !cache_seqlens || !k_cache_strides || !v_cache_strides) return MFA_ERROR_INVALID_ARGS;
    if (input_precision != MFA_PRECISION_FP16 && input_precision != MFA_PRECISION_BF16) return MFA_ERROR_INVALID_ARGS;
    if (out_precision != MFA_PRECISION_FP32 && out_precision != input_precision) return MFA_ERROR_INVALID_ARGS;
    if (!(softmax_scale > 0.0f) || ((uintptr_t)cache_seqlens & 3) || ((uintptr_t)block_table & 3) || num_splits < 0) return MFA_ERROR_INVALID_ARGS;
    if (seqlen_new && (!k_new || !v_new || !k_new_strides || !v_new_strides)) return MFA_ERROR_INVALID_ARGS;
    if (block_table && block_table_stride < (int64_t)max_pages_per_seq) return MFA_ERROR_INVALID_ARGS;
    PagedParams& p = f8.p;
    memset(&p, 0, sizeof(p));
    p.q = q; p.kc = k_cache; p.vc = v_cache; p.kn = k_new; p.vn = v_new; p.bt = block_table; p.seqlens = cache_seqlens;
    p.out = out; p.lse = lse;
    p.B = batch; p.Sq = seqlen_q; p.Snew = seqlen_new; p.H = num_heads; p.Hkv = num_kv_heads; p.D = head_dim;
    p.page_size = page_size;
    // static cache: page b is sequence b's row of S_max = page_size tokens
    p.num_pages = block_table ? num_pages : batch;
    p.max_pages = block_table ? max_pages_per_seq : 1;
    p.bt_stride = block_table ? block_table_stride : 0;
    p.page_shift = (page_size && !(page_size & (page_size - 1))) ? __builtin_ctz(page_size) : -1;
    p.qsb = q_strides ? q_strides[0] : (int64_t)seqlen_q * num_heads * head_dim;
    p.qst = q_strides ? q_strides[1] : (int64_t)num_heads * head_dim;
    p.qsh = q_strides ? q_strides[2] : (int64_t)head_dim;
    p.kpg = k_cache_strides[0]; p.kst = k_cache_strides[1]; p.ksh = k_cache_strides[2];
    p.vpg = v_cache_strides[0]; p.vst = v_cache_strides[1]; p.vsh = v_cache_strides[2];
    if (seqlen_new) {
        p.knb = k_new_strides[0]; p.knt = k_new_strides[1]; p.knh = k_new_strides[2];
        p.vnb = v_new_strides[0]; p.vnt = v_new_strides[1]; p.vnh = v_new_strides[2];
    }
    p.scale = softmax_scale;
    p.causal = causal ? 1 : 0;
    p.in_prec = dense_prec(input_precision);
    p.out_prec = dense_prec(out_precision);
    if (num_kv_heads == 0 || num_heads % num_kv_heads) return MFA_ERROR_INVALID_ARGS;
    const uint64_t R = (uint64_t)(num_heads / num_kv_heads) * seqlen_q;
    if (R >= (1ull << 31)) return MFA_ERROR_INVALID_ARGS;
    p.R = (uint32_t)R;
    p.ks4 = R <= 32 ? 1 : 0;
    p.nrb = p.ks4 ? 1u : (uint32_t)((R + 127) / 128);
    p.nsplit = 1;
    auto supported = [&]() {
        return fp8 ? paged_fp8_supported(f8) : win ? paged_window_supported(PagedWindowParams{p, win->left, win->right}) : paged_supported(p);
    };
    auto attend = [&](const char** nm) {  // (p as it stands at the launch: the rotary path has pointed p.q at its image by then)
        if (win) return launch_fwd_16_paged_window(PagedWindowParams{p, win->left, win->right}, (hipStream_t)stream, nm);
        return fp8 ? launch_fwd_16_paged_fp8(f8, (hipStream_t)stream, nm) : launch_fwd_16_paged(p, (hipStream_t)stream, nm);
    };
    if (!supported() || ((uintptr_t)out & 15) || ((uintptr_t)lse & 3)) return MFA_ERROR_INVALID_ARGS;
    const char* name = "none";
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    p.nsplit = num_splits > 0 ? (uint32_t)(num_splits < 256 ? num_splits : 256)
                              : paged_auto_splits(p, (uint64_t)p.B * p.Hkv * p.nrb, win, paged_cu_count(dev));
    if (!supported()) return MFA_ERROR_INVALID_ARGS;
    if (rope) {
        // one block of the pooled workspace: the rotated q image, then (split) the partials; every check and the allocation come before
        // the first launch
        PagedRopeParams r;
        memset(&r, 0, sizeof(r));
        r.v.p = p;
        r.kd = f8.kd; r.vd = f8.vd; r.kdb = f8.kdb; r.kdh = f8.kdh; r.vdb = f8.vdb; r.vdh = f8.vdh;
        paged_rope_fill(r, *rope);
        r.fp8 = fp8 ? 1 : 0;
        const size_t img_b = (paged_rope_qimg_bytes(r) + 255) & ~(size_t)255;
        const size_t part_b = p.nsplit > 1 ? (size_t)p.nsplit * p.B * p.Hkv * p.R * (p.D + 2) * sizeof(float) : 0;
        StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);
        char* const ws = (char*)sc.workspace.ensure(img_b + part_b ? img_b + part_b : 256, (hipStream_t)stream);
        if (!ws) return MFA_ERROR_MEMORY_ALLOCATION;
        r.qimg = ws;
        if (part_b) p.part = (float*)(ws + img_b);
        if (!paged_rope_supported(r)) return MFA_ERROR_INVALID_ARGS;
        if (const hipError_t e = launch_paged_rope(r, (hipStream_t)stream); e != hipSuccess) return rc_paged(e);
        p.q = r.qimg;
        p.qsb = (int64_t)seqlen_q * num_heads * head_dim; p.qst = (int64_t)num_heads * head_dim; p.qsh = head_dim;
        const hipError_t e = attend(&name);
        ctx->last_kernel = name;
        return rc_paged(e);
    }
    if (p.nsplit > 1 && R) {
        StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);
        const size_t bytes = (size_t)p.nsplit * p.B * p.Hkv * p.R * (p.D + 2) * sizeof(float);
        p.part = (float*)sc.workspace.ensure(bytes, (hipStream_t)stream);
        if (!p.part) return MFA_ERROR_MEMORY_ALLOCATION;
    }
    if (seqlen_new) {
        const hipError_t e = fp8 ? launch_paged_fp8_append(f8, (hipStream_t)stream) : launch_paged_append(p, (hipStream_t)stream);
        if (e != hipSuccess) return rc_paged(e);
    }
    const hipError_t e = attend(&name);
    ctx->last_kernel = name;
    return rc_paged(e);
}

}  // namespace

mfa_error_t umfa_kvcache_attention_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                  void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                  const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                  const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                  int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t batch,
                                                  uint32_t seqlen_q, uint32_t seqlen_new, uint32_t num_heads, uint32_t num_kv_heads,
                                                  uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq,
                                                  float softmax_scale, bool causal, int32_t input_precision, void* out,
                                                  int32_t out_precision, float* lse, int32_t num_splits) {
    return kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides, v_new,
                           v_new_strides, block_table, block_table_stride, cache_seqlens, batch, seqlen_q, seqlen_new, num_heads,
                           num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq, softmax_scale, causal, input_precision, out,
                           out_precision, lse, num_splits, false, PagedFp8Params{});
}

mfa_error_t umfa_kvcache_attention_fp8_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                      void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                      const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                      const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                      int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t batch,
                                                      uint32_t seqlen_q, uint32_t seqlen_new, uint32_t num_heads, uint32_t num_kv_heads,
                                                      uint16_t head_dim, uint32_t page_size, uint32_t num_pages,
                                                      uint32_t max_pages_per_seq, float softmax_scale, bool causal,
                                                      int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                      int32_t num_splits, const float* k_descale, const int64_t* k_descale_strides,
                                                      const float* v_descale, const int64_t* v_descale_strides) {
    PagedFp8Params f8;
    memset(&f8, 0, sizeof(f8));
    if (!paged_fill_descales(f8, k_descale, k_descale_strides, v_descale, v_descale_strides)) return MFA_ERROR_INVALID_ARGS;
    return kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides, v_new,
                           v_new_strides, block_table, block_table_stride, cache_seqlens, batch, seqlen_q, seqlen_new, num_heads,
                           num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq, softmax_scale, causal, input_precision, out,
                           out_precision, lse, num_splits, true, f8);
}

mfa_error_t umfa_kvcache_attention_rope_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                       void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                       const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                       const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                       int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t batch,
                                                       uint32_t seqlen_q, uint32_t seqlen_new, uint32_t num_heads, uint32_t num_kv_heads,
                                                       uint16_t head_dim, uint32_t page_size, uint32_t num_pages,
                                                       uint32_t max_pages_per_seq, float softmax_scale, bool causal,
                                                       int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                       int32_t num_splits, bool cache_fp8, const float* k_descale,
                                                       const int64_t* k_descale_strides, const float* v_descale,
                                                       const int64_t* v_descale_strides, const void* rotary_cos, const void* rotary_sin,
                                                       int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro,
                                                       uint32_t rotary_dim, bool rotary_interleaved) {
    PagedFp8Params f8;
    memset(&f8, 0, sizeof(f8));
    if (cache_fp8) {
        if (!paged_fill_descales(f8, k_descale, k_descale_strides, v_descale, v_descale_strides)) return MFA_ERROR_INVALID_ARGS;
    } else if (k_descale || v_descale || k_descale_strides || v_descale_strides) {
        return MFA_ERROR_INVALID_ARGS;
    }
    const RopeArgs rope = paged_rope_args(rotary_cos, rotary_sin, rotary_table_precision == MFA_PRECISION_FP32,
                                          rotary_table_precision == input_precision, rotary_row_stride, seqlen_ro, rotary_dim, rotary_interleaved);
    return kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides, v_new,
                           v_new_strides, block_table, block_table_stride, cache_seqlens, batch, seqlen_q, seqlen_new, num_heads,
                           num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq, softmax_scale, causal, input_precision, out,
                           out_precision, lse, num_splits, cache_fp8, f8, &rope);
}

mfa_error_t umfa_kvcache_attention_window_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                         void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                         const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                         const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                         int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t batch,
                                                         uint32_t seqlen_q, uint32_t seqlen_new, uint32_t num_heads, uint32_t num_kv_heads,
                                                         uint16_t head_dim, uint32_t page_size, uint32_t num_pages,
                                                         uint32_t max_pages_per_seq, float softmax_scale, bool causal,
                                                         int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                         int32_t num_splits, bool cache_fp8, const float* k_descale,
                                                         const int64_t* k_descale_strides, const float* v_descale,
                                                         const int64_t* v_descale_strides, const void* rotary_cos, const void* rotary_sin,
                                                         int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro,
                                                         uint32_t rotary_dim, bool rotary_interleaved, int32_t window_left,
                                                         int32_t window_right) {
    if (cache_fp8 || k_descale || v_descale || k_descale_strides || v_descale_strides) return MFA_ERROR_INVALID_ARGS;
    if (window_left < -1 || window_right < -1) return MFA_ERROR_INVALID_ARGS;
    if ((rotary_cos == nullptr) != (rotary_sin == nullptr)) return MFA_ERROR_INVALID_ARGS;
    const uint64_t cap = block_table ? (uint64_t)max_pages_per_seq * page_size : (uint64_t)page_size;
    if (cap >= (1ull << 30)) return MFA_ERROR_INVALID_ARGS;
    bool plain;
    const WindowArgs w = paged_window_normalise(window_left, window_right, causal, cap, seqlen_q, plain);
    const RopeArgs rope = paged_rope_args(rotary_cos, rotary_sin, rotary_table_precision == MFA_PRECISION_FP32,
                                          rotary_table_precision == input_precision, rotary_row_stride, seqlen_ro, rotary_dim, rotary_interleaved);
    PagedFp8Params f8;
    memset(&f8, 0, sizeof(f8));
    return kvcache_forward(context, stream, q, q_strides, k_cache, k_cache_strides, v_cache, v_cache_strides, k_new, k_new_strides, v_new,
                           v_new_strides, block_table, block_table_stride, cache_seqlens, batch, seqlen_q, seqlen_new, num_heads,
                           num_kv_heads, head_dim, page_size, num_pages, max_pages_per_seq, softmax_scale, causal, input_precision, out,
                           out_precision, lse, num_splits, false, f8, rotary_cos ? &rope : nullptr, plain ? nullptr : &w);
}
