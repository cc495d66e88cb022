// runtime_varlen.hip -- the C ABI of packed variable-length attention (include/umfa_abi.h): umfa_varlen_attention_forward_stream,
// umfa_varlen_attention_backward_stream and their sliding-window forms (..._window_stream).  In-stream, never synchronising: the sequence offsets stay on the device (the kernels read them
// when they run), so a captured graph follows the contents of cu_seq_q / cu_seq_k on replay.  Scratch comes from the stream's pools only
// (a capture that would have to grow one returns MFA_ERROR_MEMORY_ALLOCATION: warm up first).  Anything outside the kernels' scope is
// MFA_ERROR_INVALID_ARGS: no silent fall-back.
#include <string.h>

#include "runtime_internal.h"
#include "fa_varlen.h"

using namespace umfa;
using namespace umfa_rt;

namespace {

mfa_error_t rc_varlen(hipError_t e) {
    return e == hipSuccess ? MFA_SUCCESS : e == hipErrorInvalidValue ? MFA_ERROR_INVALID_ARGS
                                         : e == hipErrorOutOfMemory ? MFA_ERROR_MEMORY_ALLOCATION : MFA_ERROR_EXECUTION_FAILED;
}

// the shared part of both entries: shapes, element strides ([token, head]; NULL = dense [T, heads, D]) and scope
bool varlen_take(VarlenParams& p, const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                 const int64_t* v_strides, const int32_t* cu_seq_q, const int32_t* cu_seq_k, uint32_t num_seqs, uint32_t total_q,
                 uint32_t total_k, uint32_t max_q, uint32_t max_k, uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim,
                 float softmax_scale, bool causal, int32_t input_precision) {
    if (!q || !k || !v || !cu_seq_q || !cu_seq_k) return false;
    if (input_precision != MFA_PRECISION_FP16 && input_precision != MFA_PRECISION_BF16) return false;
    if (!(softmax_scale > 0.0f) || ((uintptr_t)cu_seq_q & 3) || ((uintptr_t)cu_seq_k & 3)) return false;
    memset(&p, 0, sizeof(p));
    p.q = q; p.k = k; p.v = v; p.cu_q = cu_seq_q; p.cu_k = cu_seq_k;
    p.N = num_seqs; p.Tq = total_q; p.Tk = total_k; p.max_q = max_q; p.max_k = max_k;
    p.H = num_heads; p.Hkv = num_kv_heads; p.D = head_dim;
    p.scale = softmax_scale; p.causal = causal ? 1 : 0;
    p.in_prec = dense_prec(input_precision);
    p.qst = q_strides ? q_strides[0] : (int64_t)num_heads * head_dim;
    p.qsh = q_strides ? q_strides[1] : (int64_t)head_dim;
    p.kst = k_strides ? k_strides[0] : (int64_t)num_kv_heads * head_dim;
    p.ksh = k_strides ? k_strides[1] : (int64_t)head_dim;
    p.vst = v_strides ? v_strides[0] : (int64_t)num_kv_heads * head_dim;
    p.vsh = v_strides ? v_strides[1] : (int64_t)head_dim;
    return varlen_supported(p);
}

// flash-attention's window_size (left, right), -1 = unbounded, normalised on the host: causal sets right = 0; a side that cannot bound
// any row is unbounded (left >= max_k: row i's lower bound i + L_k - L_q - left <= L_k - 1 - max_k < 0 for every row; right >= max_q
// alike), which also keeps every bound the kernels compute inside int32.  No band left ((-1, -1), or (-1, 0): bottom-right causal) ->
// *banded = false and p.causal set for the unwindowed kernels, so such a call is bit for bit the unwindowed one.  Else p.win_left /
// p.win_right for the window kernels.  A value below -1: false.
bool varlen_window(VarlenParams& p, int32_t left, int32_t right, bool* banded) {
    if (left < -1 || right < -1) return false;
    if (p.causal) right = 0;
    if (left >= 0 && (uint32_t)left >= p.max_k) left = -1;
    if (right >= 0 && (uint32_t)right >= p.max_q) right = -1;
    *banded = !(left == -1 && right <= 0);
    if (!*banded) {
        p.causal = right == 0 ? 1 : 0;
        return true;
    }
    p.win_left = left < 0 ? VARLEN_WIN_OPEN : left;
    p.win_right = right < 0 ? VARLEN_WIN_OPEN : right;
    return true;
}

mfa_error_t varlen_forward(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, const void* k,
                           const int64_t* k_strides, const void* v, const int64_t* v_strides, const int32_t* cu_seq_q, const int32_t* cu_seq_k,
                           uint32_t num_seqs, uint32_t total_q, uint32_t total_k, uint32_t max_q, uint32_t max_k, uint32_t num_heads,
                           uint32_t num_kv_heads, uint16_t head_dim, float softmax_scale, bool causal, int32_t input_precision, void* out,
                           int32_t out_precision, float* lse, int32_t window_left, int32_t window_right) {
    Context* ctx = as_ctx(context);
    VarlenParams p;
    bool banded = false;
    if (!ctx || !out) return MFA_ERROR_INVALID_ARGS;
    if (!varlen_take(p, q, q_strides, k, k_strides, v, v_strides, cu_seq_q, cu_seq_k, num_seqs, total_q, total_k, max_q, max_k, num_heads,
                     num_kv_heads, head_dim, softmax_scale, causal, input_precision))
        return MFA_ERROR_INVALID_ARGS;
    if (!varlen_window(p, window_left, window_right, &banded)) return MFA_ERROR_INVALID_ARGS;

    if (out_precision != MFA_PRECISION_FP32 && out_precision != input_precision) return MFA_ERROR_INVALID_ARGS;
    p.out_prec = dense_prec(out_precision);
    p.out = out; p.lse = lse;
    if (((uintptr_t)out & 15) || ((uintptr_t)lse & 3)) return MFA_ERROR_INVALID_ARGS;
    const char* name = "none";
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    if (p.in_prec == P_BF16) {
        // the P V product runs in fp16 as on the other 128-row launches: V as the fp16 image of the cast pass over the packed V, read as
        // B = 1, H = H_kv, S = T_k with its token stride -- one power of two per KV head, taken back in the epilogue
        StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);
        const size_t slabs = p.Hkv;
        char* blk = sc.ensure_v16(slabs, slabs * p.Tk * p.D * 2, (hipStream_t)stream);
        if (!blk) return MFA_ERROR_MEMORY_ALLOCATION;
        void* v16 = blk + sc.v16_cnt_bytes;
        const int64_t vstr[4] = {0, p.vsh, p.vst, 1};
        const hipError_t e = launch_cast_rows_bf16_to_f16(p.v, vstr, v16, 1, p.Hkv, p.Tk, p.D, (uint32_t*)blk, (hipStream_t)stream);
        if (e != hipSuccess) return rc_varlen(e);
        p.v = v16;
        p.vst = p.D; p.vsh = (int64_t)p.Tk * p.D;
        p.vsc = (const float*)blk;
        if (!varlen_supported(p)) return MFA_ERROR_INVALID_ARGS;  // (the image's strides: dense rows, in range whenever V's were)
    }
    const hipError_t e = banded ? launch_fwd_16_varlen_window(p, (hipStream_t)stream, &name) : launch_fwd_16_varlen(p, (hipStream_t)stream, &name);
    ctx->last_kernel = name;
    return rc_varlen(e);
}

mfa_error_t varlen_backward(mfa_context_t context, void* stream, const void* dout, const void* q, const int64_t* q_strides, const void* k,
                            const int64_t* k_strides, const void* v, const int64_t* v_strides, const void* out, bool out_in_input_type,
                            const float* softmax_lse, const int32_t* cu_seq_q, const int32_t* cu_seq_k, uint32_t num_seqs, uint32_t total_q,
                            uint32_t total_k, uint32_t max_q, uint32_t max_k, uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim,
                            float softmax_scale, bool causal, int32_t input_precision, void* dq, void* dk, void* dv,
                            bool grads_in_input_type, int32_t window_left, int32_t window_right) {
    Context* ctx = as_ctx(context);
    VarlenParams p;
    bool banded = false;
    if (!ctx || !dout || !out || !softmax_lse || !dq || !dk || !dv) return MFA_ERROR_INVALID_ARGS;
    if (!varlen_take(p, q, q_strides, k, k_strides, v, v_strides, cu_seq_q, cu_seq_k, num_seqs, total_q, total_k, max_q, max_k, num_heads,
                     num_kv_heads, head_dim, softmax_scale, causal, input_precision))
        return MFA_ERROR_INVALID_ARGS;
    if (!varlen_window(p, window_left, window_right, &banded)) return MFA_ERROR_INVALID_ARGS;
    p.dout = dout; p.o = out; p.lse = (float*)softmax_lse;
    p.dq = dq; p.dk = dk; p.dv = dv;
    p.o_in_type = out_in_input_type ? 1 : 0;
    p.grad_in_type = grads_in_input_type ? 1 : 0;
    const char* name = "none";
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int dev = stream_device((hipStream_t)stream);
    DeviceGuard guard(dev);
    StreamScratch& sc = ctx->pool(dev, (hipStream_t)stream);  // row constants of the dK / dV kernel
    p.rowc = (float*)sc.rowc.ensure((size_t)2 * num_heads * (total_q ? total_q : 1) * sizeof(float), (hipStream_t)stream);
    if (!p.rowc) return MFA_ERROR_MEMORY_ALLOCATION;
    const hipError_t e = banded ? launch_bwd_16_varlen_window(p, (hipStream_t)stream, &name) : launch_bwd_16_varlen(p, (hipStream_t)stream, &name);
    ctx->last_kernel = name;
    return rc_varlen(e);
}

}  // namespace

mfa_error_t umfa_varlen_attention_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, const void* k,
                                                 const int64_t* k_strides, const void* v, const int64_t* v_strides, const int32_t* cu_seq_q,
                                                 const int32_t* cu_seq_k, uint32_t num_seqs, uint32_t total_q, uint32_t total_k, uint32_t max_q,
                                                 uint32_t max_k, uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim,
                                                 float softmax_scale, bool causal, int32_t input_precision, void* out,
                                                 int32_t out_precision, float* lse) {
    return varlen_forward(context, stream, q, q_strides, k, k_strides, v, v_strides, cu_seq_q, cu_seq_k, num_seqs, total_q, total_k, max_q,
                          max_k, num_heads, num_kv_heads, head_dim, softmax_scale, causal, input_precision, out, out_precision, lse, -1, -1);
}

mfa_error_t umfa_varlen_attention_forward_window_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                        const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                                                        const int32_t* cu_seq_q, const int32_t* cu_seq_k, uint32_t num_seqs,
                                                        uint32_t total_q, uint32_t total_k, uint32_t max_q, uint32_t max_k,
                                                        uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, float softmax_scale,
                                                        bool causal, int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                        int32_t window_left, int32_t window_right) {
    return varlen_forward(context, stream, q, q_strides, k, k_strides, v, v_strides, cu_seq_q, cu_seq_k, num_seqs, total_q, total_k, max_q,
                          max_k, num_heads, num_kv_heads, head_dim, softmax_scale, causal, input_precision, out, out_precision, lse,
                          window_left, window_right);
}

mfa_error_t umfa_varlen_attention_backward_stream(mfa_context_t context, void* stream, const void* dout, const void* q, const int64_t* q_strides,
                                                  const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                                                  const void* out, bool out_in_input_type, const float* softmax_lse, const int32_t* cu_seq_q,
                                                  const int32_t* cu_seq_k, uint32_t num_seqs, uint32_t total_q, uint32_t total_k,
                                                  uint32_t max_q, uint32_t max_k, uint32_t num_heads, uint32_t num_kv_heads,
                                                  uint16_t head_dim, float softmax_scale, bool causal, int32_t input_precision, void* dq,
                                                  void* dk, void* dv, bool grads_in_input_type) {
    return varlen_backward(context, stream, dout, q, q_strides, k, k_strides, v, v_strides, out, out_in_input_type, softmax_lse, cu_seq_q,
                           cu_seq_k, num_seqs, total_q, total_k, max_q, max_k, num_heads, num_kv_heads, head_dim, softmax_scale, causal,
                           input_precision, dq, dk, dv, grads_in_input_type, -1, -1);
}

mfa_error_t umfa_varlen_attention_backward_window_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                                         const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                                         const int64_t* v_strides, const void* out, bool out_in_input_type,
                                                         const float* softmax_lse, const int32_t* cu_seq_q, const int32_t* cu_seq_k,
                                                         uint32_t num_seqs, uint32_t total_q, uint32_t total_k, uint32_t max_q,
                                                         uint32_t max_k, uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim,
                                                         float softmax_scale, bool causal, int32_t input_precision, void* dq, void* dk,
                                                         void* dv, bool grads_in_input_type, int32_t window_left, int32_t window_right) {
    return varlen_backward(context, stream, dout, q, q_strides, k, k_strides, v, v_strides, out, out_in_input_type, softmax_lse, cu_seq_q,
                           cu_seq_k, num_seqs, total_q, total_k, max_q, max_k, num_heads, num_kv_heads, head_dim, softmax_scale, causal,
                           input_precision, dq, dk, dv, grads_in_input_type, window_left, window_right);
}
