// runtime_dropout.hip -- the C ABI of attention dropout (include/umfa_abi.h): umfa_attention_forward_dropout_stream,
// umfa_attention_backward_dropout_stream, umfa_dropout_keep_mask_stream.  In-stream, never synchronising; the kernels read
// rng_state = {seed, offset} on the device, so a captured graph whose rng_state tensor is rewritten between replays draws new masks.
// Anything outside the kernels' scope is MFA_ERROR_INVALID_ARGS: no silent fall-back.
#include <string.h>

#include "runtime_internal.h"
#include "fa_dropout.h"

using namespace umfa;
using namespace umfa_rt;

namespace {

bool dropout_args_ok(float dropout_p, const int64_t* rng_state) {
    return rng_state && dropout_p > 0.0f && dropout_p < 1.0f && ((uintptr_t)rng_state & 7) == 0;
}

mfa_error_t rc_drop(hipError_t e) {
    return e == hipSuccess ? MFA_SUCCESS : e == hipErrorInvalidValue ? MFA_ERROR_INVALID_ARGS
                                         : e == hipErrorOutOfMemory ? MFA_ERROR_MEMORY_ALLOCATION : MFA_ERROR_EXECUTION_FAILED;
}

}  // namespace

mfa_error_t umfa_attention_forward_dropout_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                  const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                                                  void* out, int32_t out_precision, float* lse, uint32_t batch_size, uint32_t seq_len_q,
                                                  uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale,
                                                  bool causal, int32_t input_precision, int32_t intermediate_precision,
                                                  float dropout_p, const int64_t* rng_state) {
    Context* ctx = as_ctx(context);
    if (!ctx || !q || !k || !v || !out || !dropout_args_ok(dropout_p, rng_state)) return MFA_ERROR_INVALID_ARGS;
    if (input_precision != MFA_PRECISION_FP16 && input_precision != MFA_PRECISION_BF16) return MFA_ERROR_INVALID_ARGS;
    if (dense_prec(intermediate_precision) == P_FP32 || !(softmax_scale > 0.0f)) return MFA_ERROR_INVALID_ARGS;
    DropFwdParams p;
    memset(&p, 0, sizeof(p));
    p.B = batch_size; p.H = num_heads; p.Sq = seq_len_q; p.Skv = seq_len_kv; p.D = head_dim;
    p.scale = softmax_scale;
    p.causal = causal ? 1 : 0;
    p.in_prec = dense_prec(input_precision);
    p.out_prec = dense_prec(out_precision);
    auto take = [&](int64_t* dst, const int64_t* src, uint32_t S) {
        if (src) {
            for (int i = 0; i < 4; ++i) dst[i] = src[i];
        } else {  // dense BHSD
            dst[0] = (int64_t)num_heads * S * head_dim; dst[1] = (int64_t)S * head_dim; dst[2] = head_dim; dst[3] = 1;
        }
        return dst[0] >= 0 && dst[1] >= 0 && dst[2] >= 0;
    };
    if (!take(p.qs, q_strides, seq_len_q) || !take(p.ks, k_strides, seq_len_kv) || !take(p.vs, v_strides, seq_len_kv)) return MFA_ERROR_INVALID_ARGS;
    p.q = q; p.k = k; p.v = v; p.o = out; p.lse = lse;
    if (!fwd_16_dropout_supported(p)) return MFA_ERROR_INVALID_ARGS;
    if ((size_t)batch_size * num_heads * seq_len_q * seq_len_kv == 0) return MFA_SUCCESS;
    p.rng = rng_state;
    p.thresh = drop_threshold((double)dropout_p);
    p.dscale = drop_scale(p.thresh);
    const char* name = "none";
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    if (p.in_prec == P_BF16) {
        // the P V product runs in fp16 as on the no-dropout 128-row launch: V as the fp16 image of the cast pre-pass, shifted by one power of
        // two per (batch, head) slab (broadcast batch / head dimensions of V stay broadcast: the slab is cast once)
        StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);
        const uint32_t vB = p.vs[0] == 0 ? 1u : p.B, vH = p.vs[1] == 0 ? 1u : p.H;
        const size_t slabs = (size_t)vB * vH;
        char* blk = sc.ensure_v16(slabs, slabs * p.Skv * p.D * 2, (hipStream_t)stream);
        if (!blk) return MFA_ERROR_MEMORY_ALLOCATION;
        void* v16 = blk + sc.v16_cnt_bytes;
        const hipError_t e = launch_cast_rows_bf16_to_f16(p.v, p.vs, v16, vB, vH, p.Skv, p.D, (uint32_t*)blk, (hipStream_t)stream);
        if (e != hipSuccess) return rc_drop(e);
        const int64_t vs0 = p.vs[0], vs1 = p.vs[1];
        p.v = v16;
        p.vs[0] = vs0 == 0 ? 0 : (int64_t)vH * p.Skv * p.D; p.vs[1] = vs1 == 0 ? 0 : (int64_t)p.Skv * p.D; p.vs[2] = p.D; p.vs[3] = 1;
        p.vsc = (const float*)blk;
        p.vsc_bs = vs0 == 0 ? 0u : vH; p.vsc_hs = vs1 == 0 ? 0u : 1u;
        p.pv16 = 2;
    }
    const hipError_t e = launch_fwd_16_dropout(p, (hipStream_t)stream, &name);
    ctx->last_kernel = name;
    return rc_drop(e);
}

mfa_error_t umfa_attention_backward_dropout_stream(mfa_context_t context, void* stream, const void* dout, const void* q, const void* k,
                                                   const void* v, const void* out, const float* softmax_lse, void* dq, void* dk, void* dv,
                                                   float* d_buffer, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
                                                   uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
                                                   int32_t input_precision, int32_t intermediate_precision, bool grads_in_input_type,
                                                   bool out_in_input_type, float dropout_p, const int64_t* rng_state) {
    Context* ctx = as_ctx(context);
    if (!ctx || !dout || !q || !k || !v || !out || !softmax_lse || !dq || !dk || !dv || !d_buffer) return MFA_ERROR_INVALID_ARGS;
    if (!dropout_args_ok(dropout_p, rng_state)) return MFA_ERROR_INVALID_ARGS;
    if (input_precision != MFA_PRECISION_FP16 && input_precision != MFA_PRECISION_BF16) return MFA_ERROR_INVALID_ARGS;
    if (dense_prec(intermediate_precision) == P_FP32) return MFA_ERROR_INVALID_ARGS;
    DropBwdParams p;
    memset(&p, 0, sizeof(p));
    p.dout = dout; p.q = q; p.k = k; p.v = v; p.o = (const float*)out; p.lse = softmax_lse;
    p.dq = (float*)dq; p.dk = (float*)dk; p.dv = (float*)dv; p.dvec = d_buffer;
    p.B = batch_size; p.H = num_heads; p.Sq = seq_len_q; p.Skv = seq_len_kv; p.D = head_dim;
    p.scale = softmax_scale; p.causal = causal ? 1 : 0;
    p.in_prec = dense_prec(input_precision); p.dout_prec = p.in_prec;
    p.grad_in_type = grads_in_input_type ? 1 : 0;
    p.o_in_type = out_in_input_type ? 1 : 0;
    if (!bwd_16_dropout_supported(p)) return MFA_ERROR_INVALID_ARGS;
    if ((size_t)batch_size * num_heads * seq_len_q * seq_len_kv == 0) return MFA_SUCCESS;
    p.rng = rng_state;
    p.thresh = drop_threshold((double)dropout_p);
    p.dscale = drop_scale(p.thresh);
    const char* name = "none";
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);  // row constants of the dK / dV kernel
    p.rowc = (float*)sc.rowc.ensure((size_t)2 * batch_size * num_heads * seq_len_q * sizeof(float), (hipStream_t)stream);
    if (!p.rowc) return MFA_ERROR_MEMORY_ALLOCATION;
    const hipError_t e = launch_bwd_16_dropout(p, (hipStream_t)stream, &name);
    ctx->last_kernel = name;
    return rc_drop(e);
}

mfa_error_t umfa_dropout_keep_mask_stream(mfa_context_t context, void* stream, uint8_t* keep, uint32_t batch_size, uint32_t num_heads,
                                          uint32_t seq_len_q, uint32_t seq_len_kv, float dropout_p, const int64_t* rng_state) {
    Context* ctx = as_ctx(context);
    if (!ctx || !keep || !dropout_args_ok(dropout_p, rng_state)) return MFA_ERROR_INVALID_ARGS;
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    const hipError_t e = launch_dropout_keep_mask(keep, batch_size, num_heads, seq_len_q, seq_len_kv, rng_state,
                                                  drop_threshold((double)dropout_p), (hipStream_t)stream);
    ctx->last_kernel = "fa_dropout_keep";
    return rc_drop(e);
}
