/*
 * umfa_abi.h -- the C ABI of libMFAFFI.so for AMD Instinct MI355X (gfx950).
 *
 * Drop-in boundary: every entry point below keeps the name, argument order,
 * argument widths and return convention of the symbol the reference exports
 * from its Swift bridge, so the existing ctypes / bindgen / C++ callers bind
 * unchanged.  Citations are to the reference tree
 * (bghira/universal-metal-flash-attention):
 *   [H]  Sources/MFAFFI/include/mfa_ffi.h            (29 declared symbols)
 *   [B]  Sources/MFABridge/MFABridge.swift           (@_cdecl bodies)
 *   [Q]  Sources/MFABridge/MFABridge+Quantized.swift
 *   [L]  Sources/MFABridge/QuantizedLayoutManifest+FFI.swift
 *   [T]  examples/pytorch-custom-op-ffi/include/metal_sdpa_backend.h (13 undeclared symbols)
 *   [M]  examples/pytorch-custom-op-ffi/src/mps_utils.mm
 *
 * ROCm reading of the opaque pointers (ABI-preserving):
 *   "command_buffer"              -> hipStream_t the work is enqueued on
 *   "*_buffer" in *_encode_mtl    -> raw device pointer
 *   "metal_buffer" in *_from_mtl_buffer* -> raw device pointer (borrowed)
 *   data_ptr in mfa_buffer_from_ptr*     -> host OR device pointer (detected);
 *       host memory is staged to HBM before and copied back after each
 *       synchronous op so results are visible in the caller's memory on return.
 *
 * Tensor layout is contiguous [batch, heads, seq, head_dim] ("BHSD",
 * metal_sdpa_backend.cpp:188-193); attention outputs and gradients are always
 * fp32 ([B] 1074-1433 ignores output_precision; MultiHeadFFITests.swift:171-173).
 * The library never throws across the boundary and never falls back to the CPU:
 * without a usable gfx950 device mfa_create_context returns 3.
 */
#ifndef UMFA_ABI_H
#define UMFA_ABI_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the 61 entry points declared between this push and its pop are the ONLY
 * dynamic symbols of libMFAFFI.so (tests/test_abi_symbols.py checks `nm -D`).  Harmless for callers. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* ---- status codes, [H]:17-26 -------------------------------------------- */
typedef int mfa_error_t;
enum {
    MFA_SUCCESS = 0,
    MFA_ERROR_INVALID_ARGS = 1,
    MFA_ERROR_MEMORY_ALLOCATION = 2,
    MFA_ERROR_DEVICE_NOT_SUPPORTED = 3,
    MFA_ERROR_KERNEL_COMPILATION = 4,
    MFA_ERROR_EXECUTION_FAILED = 5
};

/* ---- element encodings, [H]:33-41 ---------------------------------------- */
typedef int mfa_precision_t;
enum {
    MFA_PRECISION_FP16 = 0,
    MFA_PRECISION_BF16 = 1,
    MFA_PRECISION_FP32 = 2,
    MFA_PRECISION_INT8 = 3,
    MFA_PRECISION_INT4 = 4
};

/* ---- attention masks, [H]:46-64; semantics [B]:157-242 -------------------- */
typedef int mfa_mask_type_t;
enum { MFA_MASK_TYPE_NONE = 0, MFA_MASK_TYPE_BOOL = 1, MFA_MASK_TYPE_ADDITIVE = 2 };
typedef int mfa_mask_scalar_t;
enum {
    MFA_MASK_SCALAR_BYTE = 0,
    MFA_MASK_SCALAR_FP16 = 1,
    MFA_MASK_SCALAR_BF16 = 2,
    MFA_MASK_SCALAR_FP32 = 3
};

/* ---- opaque handles, [H]:69,74,633 ---------------------------------------- */
typedef void* mfa_context_t;
typedef void* mfa_buffer_t;
typedef void* mfa_mla_context_t;

/* ---- quantised-kernel introspection, [H]:76-135, [L]:1-156 ---------------- */
typedef enum {
    MFA_QUANT_KERNEL_FORWARD = 0,
    MFA_QUANT_KERNEL_BACKWARD_QUERY = 1,
    MFA_QUANT_KERNEL_BACKWARD_KEY_VALUE = 2
} mfa_quantized_kernel_t;

/* 38 x int32 binding slots; the reference fills every slot with -1 ([L]:47-49). */
typedef struct {
    int32_t qData, kData, vData, output, gradOutput, logsumexp, gradQuery, dValues, gradKey,
        gradValue;
    int32_t qScale, qZeroPoint, kScale, kZeroPoint, vScale, vZeroPoint;
    int32_t dims, steClipRange;
    int32_t qBlockScales, qBlockZeroPoints, kBlockScales, kBlockZeroPoints, vBlockScales,
        vBlockZeroPoints;
    int32_t qPrecomputedSums, kPrecomputedSums, vPrecomputedSums;
    int32_t qStrides, kStrides, vStrides, oStrides;
    int32_t maskBuffer, numHeads, numKeyValueHeads, headDimension, sequenceLength;
    int32_t scratch0, scratch1;
} mfa_quantized_layout_t;

typedef struct {
    bool supports_multi_head_backward;
    bool supports_blockwise_backward;
    uint32_t max_heads;
    uint32_t max_block_size;
} mfa_quantized_capabilities_t;

void mfa_get_quantized_layout(mfa_quantized_kernel_t kernel, mfa_quantized_layout_t* out_layout); /* [H]:123 */
void mfa_get_quantized_capabilities(void* out_capabilities); /* [H]:135 -> {1,1,128,256}, [L]:126-131 */

/* ---- context: process-wide singleton, +1 per create, [B]:782-805 ---------- */
mfa_error_t mfa_create_context(mfa_context_t* context);   /* [H]:147 */
void mfa_destroy_context(mfa_context_t context);          /* [H]:154 */

/* ---- buffers, [B]:850-1070.  Wrapped memory is never freed by the library. - */
mfa_error_t mfa_create_buffer(mfa_context_t context, size_t size_bytes, mfa_buffer_t* buffer); /* [H]:168 */
mfa_error_t mfa_buffer_from_ptr(mfa_context_t context, void* data_ptr, size_t size_bytes,
                                mfa_buffer_t* buffer); /* [H]:183 */
mfa_error_t mfa_buffer_from_ptr_with_strides(mfa_context_t context, void* data_ptr,
                                             size_t size_bytes, const int64_t* shape,
                                             const int64_t* strides, uint32_t ndim,
                                             mfa_buffer_t* buffer); /* [H]:193 */
mfa_error_t mfa_buffer_from_mtl_buffer(mfa_context_t context, void* metal_buffer,
                                       size_t size_bytes, mfa_buffer_t* buffer); /* [H]:206 */
mfa_error_t mfa_buffer_from_mtl_buffer_with_strides(mfa_context_t context, void* metal_buffer,
                                                    size_t size_bytes, const int64_t* shape,
                                                    const int64_t* strides, uint32_t ndim,
                                                    mfa_buffer_t* buffer); /* [H]:216 */
void* mfa_buffer_contents(mfa_buffer_t buffer); /* [H]:232: host-visible pointer */
void mfa_destroy_buffer(mfa_buffer_t buffer);   /* [H]:239 */

/* ---- dense forward, synchronous, [H]:273-300, [B]:1074-1433 ---------------- */
mfa_error_t mfa_attention_forward(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t out,
    uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,
    uint16_t head_dim, float softmax_scale, bool causal, mfa_precision_t input_precision,
    mfa_precision_t intermediate_precision, mfa_precision_t output_precision, bool transpose_q,
    bool transpose_k, bool transpose_v, bool transpose_o, const void* mask_ptr,
    size_t mask_size_bytes, const int64_t* mask_shape, const int64_t* mask_strides,
    uint32_t mask_ndim, mfa_mask_type_t mask_type, mfa_mask_scalar_t mask_scalar_type);

/* Same, precisions as strings ("fp16","float16","bf16","bfloat16","fp32","float32","int8","int4";
 * NULL/unknown -> fp32).  [T]:311-327, [B]:1438-1522. */
mfa_error_t mfa_attention_forward_str(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t out,
    uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,
    uint16_t head_dim, float softmax_scale, bool causal, const char* input_precision,
    const char* intermediate_precision, const char* output_precision, bool transpose_q,
    bool transpose_k, bool transpose_v, bool transpose_o, const void* mask_ptr,
    size_t mask_size_bytes, const int64_t* mask_shape, const int64_t* mask_strides,
    uint32_t mask_ndim, mfa_mask_type_t mask_type, mfa_mask_scalar_t mask_scalar_type);

/* ---- dense forward, asynchronous on the caller's stream, [H]:312-334, [B]:2377-2543.
 * command_buffer = hipStream_t; *_buffer = device pointers; offsets in BYTES;
 * q/k/v_strides = 4 x int64 ELEMENT strides in BHSD order (last must be 1) or NULL = dense;
 * out is dense fp32 [B,H,Sq,D].  Never synchronises. */
mfa_error_t mfa_attention_encode_mtl(
    mfa_context_t context, void* command_buffer, void* q_buffer, int64_t q_offset,
    const int64_t* q_strides, void* k_buffer, int64_t k_offset, const int64_t* k_strides,
    void* v_buffer, int64_t v_offset, const int64_t* v_strides, void* out_buffer,
    int64_t out_offset, void* mask_buffer, int64_t mask_offset, const int64_t* mask_shape,
    const int64_t* mask_strides, uint32_t mask_ndim, mfa_mask_type_t mask_type,
    mfa_mask_scalar_t mask_scalar_type, uint32_t batch_size, uint32_t seq_len_q,
    uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    const char* input_precision, const char* intermediate_precision);

/* ---- forward + log-sum-exp (fp32 [B*H*Sq], natural log), [T]:471-480, [B]:3078-3166 */
int32_t mfa_attention_forward_with_lse(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t out,
    mfa_buffer_t lse, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
    uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    int32_t input_precision, int32_t intermediate_precision, bool transpose_q, bool transpose_k,
    bool transpose_v, bool transpose_o);

/* ---- dense backward, [H]:407-438, [B]:3171-3282.  dq/dk/dv fp32; d_buffer fp32 [B*H*Sq]. */
mfa_error_t mfa_attention_backward(
    mfa_context_t context, mfa_buffer_t dout, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v,
    mfa_buffer_t out, mfa_buffer_t softmax_lse, mfa_buffer_t dq, mfa_buffer_t dk, mfa_buffer_t dv,
    mfa_buffer_t d_buffer, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
    uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    mfa_precision_t input_precision, mfa_precision_t intermediate_precision, bool transpose_q,
    bool transpose_k, bool transpose_v, bool transpose_o);

/* ---- runtime-quantised forward / backward, [T]:498-531, [Q]:227-533.
 * target_precision 3 = INT8, 4 = INT4; quant_mode 0 = per tensor, 2 = block-wise;
 * mask: fp32 additive [B,H,Sq,Skv] buffer or NULL.
 * MI355X extra value (additive; the reference reads every value other than 2 as per-tensor):
 *   quant_mode 3 = UMFA_QUANT_BLOCKWISE_FP8PV: block-wise int8 Q K^T as mode 2, P and V in fp8 e4m3 (V with one
 *   power-of-two scale per 64-key tile), P V on the 2x-rate fp8 MFMA -- SageAttention2's arithmetic, coarser than the
 *   reference's int8-storage / fp32-math; served for head_dim 128 without mask, anything else runs mode 2. */
#define UMFA_QUANT_BLOCKWISE_FP8PV 3
int32_t mfa_quantized_forward_with_lse(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t out,
    mfa_buffer_t lse, mfa_buffer_t mask, uint32_t batch_size, uint32_t seq_len_q,
    uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    int32_t target_precision, int32_t quant_mode, int32_t input_precision);
int32_t mfa_quantized_backward(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t out,
    mfa_buffer_t grad_out, mfa_buffer_t lse, mfa_buffer_t grad_q, mfa_buffer_t grad_k,
    mfa_buffer_t grad_v, mfa_buffer_t mask, uint32_t batch_size, uint32_t seq_len_q,
    uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    int32_t target_precision, int32_t quant_mode, int32_t input_precision);

/* ---- legacy "quantized" forwards.  In the reference all five funnel into
 * mfa_attention_forward_quantized_direct, which ignores every quantisation
 * argument and runs the dense forward ([Q]:12-218, [B]:2671-2899); kept so. ---- */
#define UMFA_QUANT_LEGACY_ARGS                                                                    \
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t out,      \
        uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,         \
        uint16_t head_dim, float softmax_scale, bool causal, float q_scale, int32_t q_zero_point, \
        float k_scale, int32_t k_zero_point, float v_scale, int32_t v_zero_point
mfa_error_t mfa_attention_forward_quantized(UMFA_QUANT_LEGACY_ARGS, mfa_precision_t q_precision,
                                            mfa_precision_t k_precision,
                                            mfa_precision_t v_precision,
                                            mfa_precision_t output_precision, bool transpose_q,
                                            bool transpose_k, bool transpose_v,
                                            bool transpose_o); /* [H]:364 */
mfa_error_t mfa_attention_forward_quantized_unified(
    UMFA_QUANT_LEGACY_ARGS, mfa_precision_t q_precision, mfa_precision_t k_precision,
    mfa_precision_t v_precision, mfa_precision_t output_precision, int32_t granularity,
    uint32_t q_block_size, uint32_t k_block_size, uint32_t v_block_size,
    bool enable_mixed_precision, bool force_symmetric_quantization, bool transpose_q,
    bool transpose_k, bool transpose_v, bool transpose_o); /* [T]:380-395 */
mfa_error_t mfa_attention_forward_quantized_enhanced(
    UMFA_QUANT_LEGACY_ARGS, mfa_precision_t q_precision, mfa_precision_t k_precision,
    mfa_precision_t v_precision, mfa_precision_t output_precision, int32_t granularity,
    uint32_t q_block_size, uint32_t k_block_size, uint32_t v_block_size,
    bool enable_mixed_precision, bool force_symmetric_quantization, bool transpose_q,
    bool transpose_k, bool transpose_v, bool transpose_o); /* [T]:412-427 */
mfa_error_t mfa_attention_forward_quantized_direct(UMFA_QUANT_LEGACY_ARGS, int32_t q_precision,
                                                   int32_t k_precision, int32_t v_precision,
                                                   int32_t output_precision, bool transpose_q,
                                                   bool transpose_k, bool transpose_v,
                                                   bool transpose_o); /* [T]:430-444, [Q]:12-218 */
mfa_error_t mfa_multihead_attention_quantized_direct(UMFA_QUANT_LEGACY_ARGS, int32_t q_precision,
                                                     int32_t k_precision,
                                                     int32_t v_precision); /* [T]:446-455 */
mfa_error_t mfa_set_scale_arrays(mfa_context_t context, const float* q_scales,
                                 uint32_t q_scales_count, const float* k_scales,
                                 uint32_t k_scales_count, const float* v_scales,
                                 uint32_t v_scales_count); /* [T]:370-375, [B]:807-848 */

/* ---- pre-quantised backward ABI ([H]:480-624, [B]:1623-2163).  Built: Q, K, V arrive quantised (INT8 / INT4) or in
 * fp16 / bf16 / fp32 (`*_precision` = mfa_precision_t) with per-tensor scale / zero point or, when `*_block_size` > 0 and
 * a scale buffer is passed, one fp32 scale (+ optional int32 zero point) per block of `*_block_size` consecutive rows of
 * a (batch, head) slab, laid out [batch][head][block].  O, dO, LSE, D and the gradients are fp32 dense BHSD; softmax
 * scale 1/sqrt(head_dim); num_kv_heads may divide num_heads (grouped K/V: dK / dV are summed over the group).  The
 * query call writes dQ and D, the kv call reads D.  head_dim <= 1024 (257 ... 1024: the wide fp32 backward); transpose_o must be false. -- */
#define UMFA_QBWD_TAIL                                                                            \
    float q_scale, int32_t q_zero_point, float k_scale, int32_t k_zero_point, float v_scale,      \
        int32_t v_zero_point, int32_t q_precision, int32_t k_precision, int32_t v_precision,      \
        bool causal, bool transpose_q, bool transpose_k, bool transpose_v, bool transpose_o
#define UMFA_QBWD_BLOCKS                                                                          \
    mfa_buffer_t q_block_scales, mfa_buffer_t q_block_zero_points, mfa_buffer_t k_block_scales,   \
        mfa_buffer_t k_block_zero_points, mfa_buffer_t v_block_scales,                            \
        mfa_buffer_t v_block_zero_points, uint32_t q_block_size, uint32_t k_block_size,           \
        uint32_t v_block_size, uint32_t options
int32_t mfa_attention_backward_query_quantized(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t output,
    mfa_buffer_t grad_output, mfa_buffer_t logsumexp, mfa_buffer_t grad_query,
    mfa_buffer_t d_values, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
    uint32_t num_heads, uint16_t head_dim, UMFA_QBWD_TAIL); /* [H]:480 */
int32_t mfa_attention_backward_kv_quantized(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v,
    mfa_buffer_t grad_output, mfa_buffer_t logsumexp, mfa_buffer_t d_values, mfa_buffer_t grad_key,
    mfa_buffer_t grad_value, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
    uint32_t num_heads, uint16_t head_dim, UMFA_QBWD_TAIL); /* [H]:511 */
int32_t mfa_attention_backward_query_quantized_ex(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v, mfa_buffer_t output,
    mfa_buffer_t grad_output, mfa_buffer_t logsumexp, mfa_buffer_t grad_query,
    mfa_buffer_t d_values, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
    uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, UMFA_QBWD_TAIL,
    UMFA_QBWD_BLOCKS); /* [H]:542 */
int32_t mfa_attention_backward_kv_quantized_ex(
    mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k, mfa_buffer_t v,
    mfa_buffer_t grad_output, mfa_buffer_t logsumexp, mfa_buffer_t d_values, mfa_buffer_t grad_key,
    mfa_buffer_t grad_value, uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv,
    uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, UMFA_QBWD_TAIL,
    UMFA_QBWD_BLOCKS); /* [H]:584 */

/* ---- utilities, [B]:1526-1617 ----------------------------------------------- */
const char* mfa_error_string(mfa_error_t error); /* [H]:450; strdup'd, caller free()s */
bool mfa_is_device_supported(void);              /* [H]:457: true iff a gfx950 device is usable */
void mfa_get_version(int* major, int* minor, int* patch); /* [H]:466 -> 1.0.0 */
double mfa_get_gpu_latency(mfa_context_t context); /* [H]:478: seconds, last synchronous op */
int32_t mfa_has_native_bfloat(void);               /* [T]:458: 1 on gfx950 */
int32_t mfa_has_native_bfloat_msl32(void);         /* [T]:459: 1 on gfx950 */

/* ---- neighbours of the attention path, SURVEY §8f rows 1 and 4 (built: csrc/fa_aux.hip) ----
 * Rotary rotation in-stream ([M]:9-22, [B]:2286-2375): src strided BHSD (element strides), dst dense BHSD,
 * fp32 cos/sin tables [S,D] (table_batch_stride 0) or [B,S,D]; negate_sin = inverse rotation. */
int mfa_rope_rotate_encode_mtl(void* context, void* command_buffer, void* src_buffer,
                               int64_t src_offset, int64_t src_batch_stride,
                               int64_t src_head_stride, int64_t src_seq_stride, void* dst_buffer,
                               int64_t dst_offset, void* cos_buffer, int64_t cos_offset,
                               void* sin_buffer, int64_t sin_offset, int64_t table_batch_stride,
                               bool negate_sin, uint32_t batch_size, uint32_t num_heads,
                               uint32_t seq_len, uint32_t head_dim,
                               const char* precision); /* [M]:9-22 */
/* In-place group-wise Walsh-Hadamard transform, 1/sqrt(N) normalised ([B]:3433-3459); element type inferred from
 * the buffer size (4 B/elt fp32, 2 B/elt fp16); block_size a power of two <= 32768. */
int32_t mfa_hadamard_rotate(mfa_buffer_t data, uint32_t block_size, uint32_t num_blocks); /* [T]:462-465 */

/* ---- other ops of the reference that are NOT built (GEMMs, not SDPA):
 * the symbols exist so existing callers link; each returns 3. ------------------ */
mfa_error_t mfa_sparse_indexer_scores(mfa_context_t context, mfa_buffer_t q, mfa_buffer_t k,
                                      uint32_t batch_size, uint32_t num_heads, uint32_t seq_len_q,
                                      uint32_t seq_len_k, uint16_t head_dim, float scale,
                                      mfa_buffer_t scores_in, mfa_buffer_t* scores_out); /* [H]:393 */
mfa_error_t mfa_mla_create_context(mfa_mla_context_t* context); /* [H]:644 */
void mfa_mla_destroy_context(mfa_mla_context_t context);        /* [H]:651 */
mfa_error_t mfa_mla_init_weights(mfa_mla_context_t context, uint32_t num_heads, uint32_t head_dim,
                                 uint32_t kv_latent_dim); /* [H]:665 */
mfa_error_t mfa_mla_load_weights(mfa_mla_context_t context, mfa_buffer_t wk, mfa_buffer_t wv); /* [H]:682 */
mfa_error_t mfa_mla_forward(mfa_mla_context_t context, mfa_context_t mfa_context,
                            mfa_buffer_t kv_latent, mfa_buffer_t* decompressed_k,
                            mfa_buffer_t* decompressed_v, uint32_t batch_size, uint32_t num_heads,
                            uint32_t sequence_length, uint32_t head_dim,
                            uint32_t kv_latent_dim); /* [H]:709 */

/* ---- MI355X additions (not in the reference; prefixed umfa_, safe to ignore) --
 * Asynchronous launch of the bf16/fp16 forward with a caller-chosen output
 * element type (0 = fp16, 1 = bf16, 2 = fp32) and optional LSE, so a PyTorch
 * binding can skip the fp32-O round trip (metal_sdpa_backend.cpp:1418-1445). */
/* umfa_attention_forward_stream only: mask_type value for a sliding window WITHOUT a mask tensor.  mask_shape points at
 * int64 {left, right}: key attends iff row - left <= key <= row + right; mask / mask_strides / mask_ndim are ignored. */
#define UMFA_MASK_TYPE_WINDOW 3

mfa_error_t umfa_attention_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, const void* k,
    const int64_t* k_strides, const void* v, const int64_t* v_strides, void* out,
    int32_t out_precision, float* lse, const void* mask, const int64_t* mask_shape,
    const int64_t* mask_strides, uint32_t mask_ndim, mfa_mask_type_t mask_type,
    mfa_mask_scalar_t mask_scalar_type, uint32_t batch_size, uint32_t seq_len_q,
    uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    int32_t input_precision, int32_t intermediate_precision);

/* MI355X extra: RoPE + SDPA in one in-stream call.  Replaces the reference's sequence of two rotary launches into dense
 * Q_rot / K_rot copies and the attention encode after them (metal_sdpa_backend.cpp:1472-1641): K is rotated once into the
 * stream's workspace, Q is rotated in registers behind the attention kernel's Q fragment load.  Bit-identical to the
 * unfused sequence (rotate q, rotate k, attend).  cos / sin: fp32 [S, D] (table_batch_stride 0) or [B, S, D]
 * (table_batch_stride S * D), pair-duplicated; seq_len_q == seq_len_kv, head_dim even; no mask. */
mfa_error_t umfa_rope_attention_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, const void* k,
    const int64_t* k_strides, const void* v, const int64_t* v_strides, void* out, int32_t out_precision, float* lse,
    const float* cos_table, const float* sin_table, int64_t table_batch_stride, uint32_t batch_size, uint32_t seq_len_q,
    uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale, bool causal,
    int32_t input_precision, int32_t intermediate_precision);
/* Name of the kernel variant the last forward on this context dispatched to (static string). */
/* MI355X extra: the runtime quantiser alone, on a device tensor [batch_heads, rows, head_dim]; writes the int8 image
 * (rows padded to *padded_row_bytes = 64 / 128 / 256) and one fp32 scale per 64-row block to device buffers.  Exists so
 * that the integer half of the quantised path can be compared bit-for-bit with the oracle. */
/* MI355X extra: mfa_attention_backward in-stream (raw device pointers, caller's stream, never synchronises).
 * dq / dk / dv are fp32 [B,H,S,D] (the ABI contract) or, with grads_in_input_type, the operand type (16-bit MFMA
 * backward only: head_dim 64 / 128 / 256, 16-bit intermediates; otherwise error 1). d_buffer: fp32 [B*H*Sq] scratch.
 * out: O in fp32 (as for mfa_attention_backward) or, with out_in_input_type, O in the operand type. */
mfa_error_t umfa_attention_backward_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                           const void* k, const void* v, const void* out, const float* softmax_lse,
                                           void* dq, void* dk, void* dv, float* d_buffer, uint32_t batch_size,
                                           uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,
                                           uint16_t head_dim, float softmax_scale, bool causal, int32_t input_precision,
                                           int32_t intermediate_precision, bool grads_in_input_type,
                                           bool out_in_input_type);

/* MI355X extra: umfa_attention_backward_stream with the mask of the forward call (the reference's backward takes none,
 * metal_sdpa_backend.cpp:1798-1803).  (mask, mask_shape, mask_strides, mask_ndim, mask_type, mask_scalar_type) exactly as
 * umfa_attention_forward_stream takes them: bool / fp32 / fp16 / bf16 of <= 4 dims broadcast onto [B, H, Sq, Skv] with any
 * strides, or UMFA_MASK_TYPE_WINDOW with {left, right} in mask_shape and no tensor; `causal` combines with either.
 * MFA_MASK_TYPE_NONE is umfa_attention_backward_stream.  16-bit operands at head_dim 64 / 128 / 256 with 16-bit
 * intermediates run the masked MFMA backward (tiles the mask closes entirely are skipped); other calls up to head_dim 256
 * the fp32-exact one; beyond 256: MFA_ERROR_INVALID_ARGS.  A row whose forward LSE is -inf (nothing visible) gets a zero
 * dQ row and adds nothing to dK / dV.  Tensor masks take a per-call tile-flag pass whose scratch grows on first use;
 * under stream capture without a warm-up call it cannot grow and the call returns MFA_ERROR_MEMORY_ALLOCATION. */
mfa_error_t umfa_attention_backward_masked_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                                  const void* k, const void* v, const void* out, const float* softmax_lse,
                                                  void* dq, void* dk, void* dv, float* d_buffer, uint32_t batch_size,
                                                  uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,
                                                  uint16_t head_dim, float softmax_scale, bool causal,
                                                  int32_t input_precision, int32_t intermediate_precision,
                                                  bool grads_in_input_type, bool out_in_input_type, const void* mask,
                                                  const int64_t* mask_shape, const int64_t* mask_strides,
                                                  uint32_t mask_ndim, mfa_mask_type_t mask_type,
                                                  mfa_mask_scalar_t mask_scalar_type);

/* MI355X extra: attention dropout (torch's dropout_p).  The keep mask is a pure function of (query row i, key j, b * H + h) and
 * rng_state, a DEVICE int64[2] = {seed, offset} the kernels read when they run (so a captured graph whose rng_state is rewritten between
 * replays draws a new mask each time): w = Philox4x32-10(ctr = (j >> 2, i, b*H + h, lo32(offset)), key = (lo32(seed), hi32(seed)))[j & 3],
 * t = min(round(p 2^32), 2^32 - 1), keep = (w >= t), scale s = 2^32 / (2^32 - t).
 * The forward: the arguments of umfa_attention_forward_stream without the mask group.  O = s * sum_j keep_ij P_ij V_j with P the
 * softmax over the visible keys (causal first); lse receives the UNDROPPED log-sum-exp (may be NULL).  Scope: fp16 / bf16 operands,
 * head_dim 64 / 128, 16-bit intermediates, K / V rows contiguous (strides {*, *, head_dim, 1}), 16-byte aligned, out fp32 or the operand
 * type, 0 < dropout_p < 1, rng_state non-NULL; anything else is MFA_ERROR_INVALID_ARGS (never a silent fall-back).
 * In-stream, never synchronises; valid under stream capture after a warm-up call (bf16 takes a V image from the stream's scratch). */
mfa_error_t umfa_attention_forward_dropout_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, const void* k,
    const int64_t* k_strides, const void* v, const int64_t* v_strides, void* out, int32_t out_precision, float* lse,
    uint32_t batch_size, uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim,
    float softmax_scale, bool causal, int32_t input_precision, int32_t intermediate_precision, float dropout_p,
    const int64_t* rng_state);

/* MI355X extra: the backward of umfa_attention_forward_dropout_stream: the arguments of umfa_attention_backward_stream plus the
 * forward's dropout_p and rng_state (the same mask, bit for bit).  out is the dropped O the forward returned, softmax_lse its LSE;
 * dense BHSD operands.  Scope as the forward (fp16 / bf16, head_dim 64 / 128, 16-bit intermediates), else MFA_ERROR_INVALID_ARGS.
 * No atomics: bitwise repeatable.  In-stream; the row-constant scratch grows on first use (warm up before capturing). */
mfa_error_t umfa_attention_backward_dropout_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                                   const void* k, const void* v, const void* out, const float* softmax_lse,
                                                   void* dq, void* dk, void* dv, float* d_buffer, uint32_t batch_size,
                                                   uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,
                                                   uint16_t head_dim, float softmax_scale, bool causal,
                                                   int32_t input_precision, int32_t intermediate_precision,
                                                   bool grads_in_input_type, bool out_in_input_type, float dropout_p,
                                                   const int64_t* rng_state);

/* MI355X extra: the dropout keep mask itself as 0 / 1 bytes, dense [B, H, Sq, Skv], from the same definition the kernels use
 * (tests, debugging).  0 < dropout_p < 1 and rng_state non-NULL, else MFA_ERROR_INVALID_ARGS.  In-stream. */
mfa_error_t umfa_dropout_keep_mask_stream(mfa_context_t context, void* stream, uint8_t* keep, uint32_t batch_size,
                                          uint32_t num_heads, uint32_t seq_len_q, uint32_t seq_len_kv, float dropout_p,
                                          const int64_t* rng_state);

/* MI355X extra: packed variable-length attention (flash-attention's varlen form, torch.nn.attention.varlen.varlen_attn).
 *   Layout: q [total_q, num_heads, D], k and v [total_k, num_kv_heads, D]; *_strides = {token, head} in ELEMENTS (NULL: dense), both
 *   multiples of 8, head_dim contiguous, bases 16-byte aligned -- so qkv[:, 0] of a [T, 3, H, D] projection is accepted as it is.
 *   cu_seq_q, cu_seq_k: DEVICE int32 [num_seqs + 1]; sequence n owns rows cu[n] .. cu[n+1]-1 (zero-length sequences allowed).  The
 *   offsets are read by the kernels when they run and never by the host: the calls never synchronise, and a captured graph follows the
 *   CONTENTS of cu_seq_* on replay.  Only num_seqs, total_*, max_q, max_k are host values.
 *   GQA: num_heads % num_kv_heads == 0, query head h reads KV head h / (num_heads / num_kv_heads).
 *   Causal is BOTTOM-RIGHT aligned per sequence: query i sees key j iff j <= i + (L_k - L_q) (flash-attention's varlen convention,
 *   torch.nn.attention.bias.causal_lower_right); with L_q == L_k it is the top-left is_causal of the dense entries.
 *   A row that sees no key (L_k = 0, or causal with L_q > L_k) gives O = 0 exactly, LSE = -inf, and dQ = 0.
 *   Memory safety: each sequence's range is clamped on the device into [0, total) and its length to max_q / max_k, so no offsets make the
 *   kernels read or write outside the tensors; rows of a sequence longer than max_q / max_k, and rows no sequence covers, are undefined.
 *   Scope: fp16 / bf16, head_dim 64 / 128, softmax_scale > 0 (callers pass D^-0.5 for the default); else MFA_ERROR_INVALID_ARGS.
 *   Scratch from the stream's pools (bf16: the fp16 V image; backward: row constants): valid under stream capture after a warm-up
 *   call, a capture that would have to grow a pool returns MFA_ERROR_MEMORY_ALLOCATION.
 * Forward: out dense [total_q, num_heads, D] in out_precision (fp32 or the input type); lse (optional) fp32 [num_heads, total_q],
 * natural log (torch's varlen layout). */
mfa_error_t umfa_varlen_attention_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                 const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                                                 const int32_t* cu_seq_q, const int32_t* cu_seq_k, uint32_t num_seqs, uint32_t total_q,
                                                 uint32_t total_k, uint32_t max_q, uint32_t max_k, uint32_t num_heads,
                                                 uint32_t num_kv_heads, uint16_t head_dim, float softmax_scale, bool causal,
                                                 int32_t input_precision, void* out, int32_t out_precision, float* lse);

/* MI355X extra: the backward of umfa_varlen_attention_forward_stream, the same layout and scope.  dout and out dense
 * [total_q, num_heads, D] (dout in the input type, out in the input type or fp32: out_in_input_type), softmax_lse the forward's
 * [num_heads, total_q].  dq dense [total_q, num_heads, D], dk and dv dense [total_k, num_kv_heads, D], in the input type or fp32
 * (grads_in_input_type); grouped query heads are summed inside the dK / dV kernel in a fixed order.  No atomics: bitwise repeatable. */
mfa_error_t umfa_varlen_attention_backward_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                                  const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                                  const int64_t* v_strides, const void* out, bool out_in_input_type,
                                                  const float* softmax_lse, const int32_t* cu_seq_q, const int32_t* cu_seq_k,
                                                  uint32_t num_seqs, uint32_t total_q, uint32_t total_k, uint32_t max_q, uint32_t max_k,
                                                  uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, float softmax_scale,
                                                  bool causal, int32_t input_precision, void* dq, void* dk, void* dv,
                                                  bool grads_in_input_type);

/* MI355X extra: umfa_varlen_attention_forward_stream / umfa_varlen_attention_backward_stream with a sliding window, flash-attention's
 * window_size = (window_left, window_right), bottom-right per sequence.  For sequence n with lengths L_q, L_k and off = L_k - L_q,
 * query row i sees key j iff 0 <= j < L_k, and (window_left < 0 or j >= i + off - window_left), and
 * (window_right < 0 or j <= i + off + window_right).  -1 is unbounded on that side; a value below -1 is MFA_ERROR_INVALID_ARGS.
 * causal sets window_right = 0 (so (left, -1) with causal is a causal look-back window of left keys).  With L_q == L_k this is the
 * dense sliding window i - left <= j <= i + right.  A row that sees no key gives O = 0 exactly, LSE = -inf and dQ = 0; a key no row
 * sees gets dK = dV = 0.  The host normalises without touching the device: window_left >= max_k and window_right >= max_q are
 * unbounded, and a call whose window bounds nothing ((-1, -1), or (-1, 0): bottom-right causal) runs the unwindowed kernels, bit for
 * bit the unwindowed entries' results.  Everything else as the unwindowed entries; the backward takes the forward's window. */
mfa_error_t umfa_varlen_attention_forward_window_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                        const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                                                        const int32_t* cu_seq_q, const int32_t* cu_seq_k, uint32_t num_seqs,
                                                        uint32_t total_q, uint32_t total_k, uint32_t max_q, uint32_t max_k,
                                                        uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, float softmax_scale,
                                                        bool causal, int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                        int32_t window_left, int32_t window_right);

mfa_error_t umfa_varlen_attention_backward_window_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                                         const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v,
                                                         const int64_t* v_strides, const void* out, bool out_in_input_type,
                                                         const float* softmax_lse, const int32_t* cu_seq_q, const int32_t* cu_seq_k,
                                                         uint32_t num_seqs, uint32_t total_q, uint32_t total_k, uint32_t max_q,
                                                         uint32_t max_k, uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim,
                                                         float softmax_scale, bool causal, int32_t input_precision, void* dq, void* dk,
                                                         void* dv, bool grads_in_input_type, int32_t window_left, int32_t window_right);

/* MI355X extra: attention over a paged or static KV cache for inference (flash-attention's flash_attn_with_kvcache), forward only.
 *   q [batch, seqlen_q, num_heads, D]; q_strides = {batch, token, head} in ELEMENTS (NULL: dense).
 *   Paged cache (block_table != NULL): k_cache / v_cache [num_pages, page_size, num_kv_heads, D], *_cache_strides = {page, token, head};
 *   block_table DEVICE int32 [batch][block_table_stride]: sequence b's logical page lp is physical page block_table[b * stride + lp],
 *   lp < max_pages_per_seq; page_size a multiple of 16.
 *   Static cache (block_table == NULL): page b is sequence b's whole row of page_size = S_max tokens, so
 *   [batch, S_max, H_kv, D] and [batch, H_kv, S_max, D] are both taken through their strides ({batch, token, head}), without a copy;
 *   num_pages and max_pages_per_seq are ignored.
 *   cache_seqlens DEVICE int32 [batch], contiguous (entry b at cache_seqlens + b): the cached length of each sequence, never read by the
 *   host.  Every stride is a multiple of 8
 *   elements with head_dim contiguous; bases 16-byte aligned.
 *   Append (seqlen_new > 0): k_new / v_new [batch, seqlen_new, num_kv_heads, D] ({batch, token, head} strides) are written into the cache
 *   in place at positions cache_seqlens[b] .. + seqlen_new - 1, through the block table, on `stream` before the attention; cache_seqlens
 *   itself is not modified.  Attention then covers L_k = cache_seqlens[b] + seqlen_new keys.
 *   Causal is BOTTOM-RIGHT aligned per sequence: query i sees key j iff j <= i + L_k - seqlen_q.  A row that sees no key gives O = 0
 *   exactly and LSE = -inf.  GQA: num_heads % num_kv_heads == 0, query head h reads KV head h / (num_heads / num_kv_heads).
 *   Memory safety, on the device: cache_seqlens[b] and L_k are clamped into [0, max_pages_per_seq * page_size] (static: [0, S_max]);
 *   a block-table entry outside [0, num_pages) is never dereferenced -- its keys count as masked and the append skips its rows; append
 *   rows past the capacity are dropped.  No table or length contents make a kernel touch memory outside q, the cache pools, k_new /
 *   v_new, out and lse.  Pages shared between sequences may be read; appending into a page another sequence also reads or appends to is
 *   the caller's race.
 *   num_splits: 0 = the library picks the split-KV parts from max_pages_per_seq * page_size and the CU count; > 0 forces that many.
 *   Split partials come from the stream's pooled workspace: valid under stream capture after a warm-up call, a capture that would have
 *   to grow it returns MFA_ERROR_MEMORY_ALLOCATION.  Never synchronises; a captured graph follows the contents of cache_seqlens and
 *   block_table on replay.
 *   Scope: fp16 / bf16, head_dim 64 / 128, softmax_scale > 0; else MFA_ERROR_INVALID_ARGS.
 * out dense [batch, seqlen_q, num_heads, D] in out_precision (fp32 or the input type); lse (optional) fp32 [batch, num_heads, seqlen_q],
 * natural log. */
mfa_error_t umfa_kvcache_attention_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                  void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                  const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                  const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                  int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t batch,
                                                  uint32_t seqlen_q, uint32_t seqlen_new, uint32_t num_heads, uint32_t num_kv_heads,
                                                  uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq,
                                                  float softmax_scale, bool causal, int32_t input_precision, void* out,
                                                  int32_t out_precision, float* lse, int32_t num_splits);

/* MI355X extra: umfa_kvcache_attention_forward_stream over an fp8 KV cache.  k_cache / v_cache hold OCP e4m3fn bytes (gfx950's fp8, torch's
 * float8_e4m3fn; not e4m3fnuz, not e5m2), both of them; q, k_new / v_new and out stay fp16 / bf16 (input_precision describes q and k_new /
 * v_new).  k_descale / v_descale: DEVICE fp32, entry (b, h_kv) at descale[b * strides[0] + h_kv * strides[1]] with ELEMENT strides >= 0 that
 * may be 0 (a scalar, [H_kv], [B, 1], [B, H_kv]); never read by the host, so a captured graph follows their contents on replay.  The value
 * a cache byte stands for is e4m3fn(byte) * descale[b, h_kv], and the call computes
 *   softmax(q (K8 k_descale)^T softmax_scale [bottom-right causal]) (V8 v_descale),
 * LSE that of the dequantised scores; the expansions to the 16-bit operand types are exact and the arithmetic is the 16-bit entry's.
 *   Append: element x of k_new / v_new is stored as e4m3fn_rne(clamp(fp32(x) / descale[b, h_kv], -448, +448)) -- IEEE fp32 division, the
 *   clamp before the conversion, round to nearest even (bit for bit torch's (x.float() / d).clamp(-448, 448).to(float8_e4m3fn)).  NaN
 *   inputs and descales that are zero, negative or non-finite give unspecified values but never touch memory outside the pools.
 *   Cache strides are in elements = bytes: multiples of 16 with head_dim contiguous, bases 16-byte aligned; q / k_new / v_new strides as
 *   in the 16-bit entry.  Every layout, clamp, masking and memory-safety rule, num_splits, the pooled split workspace, the capture rule
 *   and the error codes are umfa_kvcache_attention_forward_stream's.  Scope: head_dim 64 / 128, page_size a multiple of 16; anything
 *   else MFA_ERROR_INVALID_ARGS -- no fall-back. */
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
                                                      const float* v_descale, const int64_t* v_descale_strides);

/* MI355X extra: PACKED variable-length queries over the paged or static KV cache of umfa_kvcache_attention_forward_stream
 * (flash-attention's flash_attn_varlen_func(..., block_table=...): continuous batching, chunked prefill beside decode), forward only.
 *   q [total_q, num_heads, D]; q_strides = {token, head} in ELEMENTS (NULL: dense), head_dim contiguous -- a slice of a fused QKV
 *   projection goes in without a copy.  cu_seqlens_q DEVICE int32 [batch + 1]: sequence b owns rows cu[b] .. cu[b+1] - 1,
 *   L_q,b = cu[b+1] - cu[b]; max_seqlen_q is a host bound on L_q,b (<= total_q).  k_cache, v_cache, their strides, block_table,
 *   block_table_stride, cache_seqlens, page_size, num_pages, max_pages_per_seq and the static form (block_table == NULL) are exactly
 *   umfa_kvcache_attention_forward_stream's.
 *   Append (has_new): k_new / v_new [total_q, num_kv_heads, D] ({token, head} strides), packed by the SAME cu_seqlens_q; sequence b's
 *   rows are written into the cache in place at positions cache_seqlens[b] .. on `stream` before the attention, and
 *   L_k,b = min(L0_b + L_q,b, cap); without, L_k,b = L0_b.  L0_b is cache_seqlens[b] clamped into [0, cap],
 *   cap = max_pages_per_seq * page_size (static: S_max).  cache_seqlens is not modified.
 *   Causal is BOTTOM-RIGHT aligned per sequence: query i of sequence b sees key j iff j <= i + L_k,b - L_q,b and j's page entry lies in
 *   [0, num_pages); non-causal sees every such key below L_k,b.  A row that sees no key gives O = 0 exactly and LSE = -inf.  Rows of
 *   out / lse that no sequence covers are not written.
 *   Memory safety, on the device, for any contents of cu_seqlens_q, cache_seqlens and the block table: cu values are clamped into
 *   [0, total_q] and L_q,b to max_seqlen_q; lengths and table entries are treated as in umfa_kvcache_attention_forward_stream; append
 *   rows past the capacity or into a page the table does not hold are dropped.  Results are DEFINED only for non-decreasing cu with
 *   cu[batch] <= total_q; for anything else the only promise is that nothing outside q, the pools, k_new / v_new, out, lse and the
 *   library's own scratch is touched.
 *   Work follows the rows that exist: a sequence with (num_heads / num_kv_heads) * L_q,b <= 32 is one work item per KV head in the decode
 *   form, any other ceil(that / 128) items of 128 rows, both in one launch; a pre-pass launch writes the item list (at most
 *   num_kv_heads * min(floor(g total_q / 128) + batch, batch * ceil(g max_seqlen_q / 128)) entries) into the stream's pooled workspace.
 *   num_splits: 0 = the library picks the split-KV parts from that bound, the CU count and the capacity; > 0 forces that many for every
 *   item.  The list and the split partials come from the stream's pooled workspace: valid under stream capture after a warm-up call, a
 *   capture that would have to grow it returns MFA_ERROR_MEMORY_ALLOCATION.  Never synchronises; a captured graph follows the contents
 *   of cu_seqlens_q, cache_seqlens and block_table on replay (total_q, batch and max_seqlen_q are the capture's).
 *   Host-known values: total_q, batch, max_seqlen_q, the head counts, D, the page geometry, num_splits, has_new -- nothing else.
 *   Scope: fp16 / bf16 caches, head_dim 64 / 128, softmax_scale > 0; else MFA_ERROR_INVALID_ARGS -- no fall-back.
 * out dense [total_q, num_heads, D] in out_precision (fp32 or the input type); lse (optional) fp32 [num_heads, total_q], natural log. */
mfa_error_t umfa_varlen_kvcache_attention_forward_stream(mfa_context_t context, void* stream, const void* q, const int64_t* q_strides,
                                                         void* k_cache, const int64_t* k_cache_strides, void* v_cache,
                                                         const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides,
                                                         const void* v_new, const int64_t* v_new_strides, const int32_t* block_table,
                                                         int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
                                                         uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new,
                                                         uint32_t num_heads, uint32_t num_kv_heads, uint16_t head_dim, uint32_t page_size,
                                                         uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
                                                         int32_t input_precision, void* out, int32_t out_precision, float* lse,
                                                         int32_t num_splits);

/* Debug: how many work items the last umfa_varlen_kvcache_attention_forward_stream call on `stream` ran in the decode form and in the
 * 128-row form (counted by the forward kernel itself).  Valid while nothing else has used the stream's pooled workspace since that
 * call; SYNCHRONISES the stream.  MFA_ERROR_INVALID_ARGS when the stream has no workspace yet. */
mfa_error_t umfa_varlen_kvcache_item_counts(mfa_context_t context, void* stream, uint32_t* decode_items, uint32_t* block_items);

/* MI355X extra: umfa_kvcache_attention_forward_stream / umfa_kvcache_attention_fp8_forward_stream with the rotary embedding of q and
 * k_new fused in (flash_attn_with_kvcache's rotary_cos / rotary_sin / rotary_interleaved).  ONE pre-pass launch replaces the append
 * launch: it rotates k_new into the cache, appends v_new unrotated and rotates q into a dense operand-type image in the stream's pooled
 * workspace; the unchanged attention kernel then reads that image.  A rotary call launches as many kernels as the same call without.
 *   cache_fp8: false = 16-bit caches (umfa_kvcache_attention_forward_stream's arguments; the four descale arguments must be NULL);
 *   true = e4m3fn caches (umfa_kvcache_attention_fp8_forward_stream's arguments).  seqlen_new must be > 0 (rotary needs new tokens).
 *   rotary_cos / rotary_sin: DEVICE tables [seqlen_ro, rotary_dim / 2] in rotary_table_precision (fp32, or input_precision: 16-bit
 *   entries convert exactly to fp32 on load), unit column stride, rotary_row_stride ELEMENTS between rows (>= rotary_dim / 2), bases and
 *   rows 16-byte aligned.  rotary_dim: a multiple of 16 in [16, head_dim]; elements at rotary_dim and above pass through unchanged.
 *   rotary_interleaved: element 2i pairs with 2i + 1; else (GPT-NeoX) element i pairs with i + rotary_dim / 2; table column i either way.
 *   The pair (a, b) at column i and position pos becomes a' = fma(a, cos[pos, i], -(b sin[pos, i])), b' = fma(b, cos[pos, i],
 *   a sin[pos, i]) in fp32, rounded once to the operand type; for an fp8 cache the rounded key is then quantised by the fp8 entry's rule.
 *   Positions are read on the device: new-key row t of sequence b is rotated at L0_b + t, L0_b = cache_seqlens[b] clamped into [0, cap];
 *   query row i at L0_b + i when causal, every query row at L0_b when not (flash-attention's rule).  A captured graph follows
 *   cache_seqlens on replay.  A position >= seqlen_ro uses table row seqlen_ro - 1: memory-safe and defined, but meaningless -- the
 *   caller sizes the table.
 *   The result equals, in every bit of out, lse and both pools, the plain entry called on q and k_new rotated that way and rounded to
 *   the operand type.  Every layout, clamp, masking, dropped-row and memory-safety rule, num_splits and the error codes are the plain
 *   entries'.  The q image shares the pooled workspace with the split partials: valid under stream capture after a warm-up call, a
 *   capture that would have to grow it returns MFA_ERROR_MEMORY_ALLOCATION and launches nothing.  Anything outside this scope:
 *   MFA_ERROR_INVALID_ARGS -- no fall-back. */
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
                                                       uint32_t rotary_dim, bool rotary_interleaved);

/* MI355X extra: umfa_varlen_kvcache_attention_forward_stream with the same fused rotary embedding (16-bit caches; has_new must be true).
 * Packed row t of sequence b (found on the device from cu_seqlens_q) is rotated at L0_b + (t - cu[b]) for the new keys and, when
 * causal, for the queries; every query row of sequence b at L0_b when not causal.  Rows no sequence covers are neither appended nor
 * used.  The q image [total_q, num_heads, D] shares the pooled workspace with the item list and the split partials.  Everything else:
 * umfa_kvcache_attention_rope_forward_stream and umfa_varlen_kvcache_attention_forward_stream. */
mfa_error_t umfa_varlen_kvcache_attention_rope_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache, const int64_t* k_cache_strides,
    void* v_cache, const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides, const void* v_new,
    const int64_t* v_new_strides, const int32_t* block_table, int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
    uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads, uint32_t num_kv_heads,
    uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
    int32_t input_precision, void* out, int32_t out_precision, float* lse, int32_t num_splits, const void* rotary_cos,
    const void* rotary_sin, int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro, uint32_t rotary_dim,
    bool rotary_interleaved);

/* MI355X extra: umfa_varlen_kvcache_attention_forward_stream over an fp8 KV cache -- packed variable-length queries over the e4m3fn
 * paged or static cache of umfa_kvcache_attention_fp8_forward_stream, with the quantising packed append and, optionally, the fused
 * rotary embedding.  The arguments are umfa_varlen_kvcache_attention_forward_stream's, then the four descale arguments of the fp8 entry,
 * then the rotary arguments of umfa_varlen_kvcache_attention_rope_forward_stream; rotary_cos == rotary_sin == NULL means no rotary (the
 * other rotary arguments are then ignored); exactly one of them NULL is MFA_ERROR_INVALID_ARGS.  The contract is the union of the two:
 *   Layouts and clamps: umfa_varlen_kvcache_attention_forward_stream's, word for word -- q / cu_seqlens_q / the caches / the table / the
 *   lengths, L_k,b = min(L0_b + L_q,b, cap), bottom-right causal per sequence, O = 0 / LSE = -inf for a row that sees no key, rows no
 *   sequence covers left unwritten, the work items and the item-list pre-pass, and every clamp that makes any contents of
 *   cu_seqlens_q, cache_seqlens and the block table memory-safe.
 *   Bytes and arithmetic: umfa_kvcache_attention_fp8_forward_stream's -- k_cache / v_cache hold OCP e4m3fn bytes, both of them; a byte
 *   stands for e4m3fn(byte) * descale[b, h_kv] with b the SEQUENCE (a page shared by two sequences decodes under each one's own
 *   descale); k_descale / v_descale are DEVICE fp32 at descale[b * strides[0] + h_kv * strides[1]], element strides >= 0 that may be 0,
 *   never read by the host, so a captured graph follows their contents on replay; the expansions to the 16-bit operand types are exact
 *   and the arithmetic is the 16-bit entry's.  Cache strides are in elements = bytes, multiples of 16, bases 16-byte aligned.
 *   Append (has_new): packed row t of sequence b is stored at cache position L0_b + (t - cu[b]) as
 *   e4m3fn_rne(clamp(fp32(x) / descale[b, h_kv], -448, +448)) -- IEEE fp32 division, the clamp before the conversion; rows no sequence
 *   covers, rows past the capacity and rows of pages the table does not hold are dropped.
 *   Rotary (needs has_new): umfa_kvcache_attention_rope_forward_stream's rule at positions L0_b + (t - cu[b]) for the new keys and, when
 *   causal, the queries; every query row of sequence b at L0_b when not causal.  The rotated key is rounded once to the operand type,
 *   then quantised.  ONE pre-pass launch replaces the append launch; the result equals, in every bit of out, lse and both pools, this
 *   entry without rotary called on q and k_new rotated that way and rounded to the operand type.
 *   With every L_q,b equal the result equals umfa_kvcache_attention_fp8_forward_stream's (with rotary:
 *   umfa_kvcache_attention_rope_forward_stream's with cache_fp8) bit for bit at the same num_splits.
 *   The q image, the item list and the split partials share the stream's pooled workspace: valid under stream capture after a warm-up
 *   call, a capture that would have to grow it returns MFA_ERROR_MEMORY_ALLOCATION and launches nothing.  Never synchronises;
 *   umfa_varlen_kvcache_item_counts reads this call's tally too.  Scope: fp16 / bf16 q and new tokens, head_dim 64 / 128, page_size a
 *   multiple of 16, no window; anything else MFA_ERROR_INVALID_ARGS -- no fall-back. */
mfa_error_t umfa_varlen_kvcache_attention_fp8_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache, const int64_t* k_cache_strides,
    void* v_cache, const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides, const void* v_new,
    const int64_t* v_new_strides, const int32_t* block_table, int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
    uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads, uint32_t num_kv_heads,
    uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
    int32_t input_precision, void* out, int32_t out_precision, float* lse, int32_t num_splits, const float* k_descale,
    const int64_t* k_descale_strides, const float* v_descale, const int64_t* v_descale_strides, const void* rotary_cos,
    const void* rotary_sin, int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro, uint32_t rotary_dim,
    bool rotary_interleaved);

/* MI355X extra: sliding-window attention over a 16-bit paged or static KV cache (flash_attn_with_kvcache's window_size).  The
 * arguments are umfa_kvcache_attention_rope_forward_stream's followed by the window; rotary_cos == rotary_sin == NULL means no rotary
 * (the rotary arguments are then ignored), and cache_fp8 == true or a descale argument is MFA_ERROR_INVALID_ARGS (fp8 caches with a
 * window are not built).
 *   With L_k = clamp(cache_seqlens[b]) + seqlen_new, clamped as in umfa_kvcache_attention_forward_stream, and off = L_k - seqlen_q, query
 *   token i of sequence b sees key j iff j < L_k, j's page entry lies in [0, num_pages) and i + off - window_left <= j <= i + off +
 *   window_right.  A side given as -1 is unbounded; a value below -1 is MFA_ERROR_INVALID_ARGS.  causal sets window_right = 0 (and, with
 *   rotary, places the query positions as in the rotary entry: the window does not).  A row that sees no key gives O = 0 exactly and
 *   LSE = -inf.  window_left >= capacity (max_pages_per_seq * page_size; static: page_size) and window_right >= seqlen_q cannot bind and
 *   count as unbounded.  A window with both sides unbounded -- or the left unbounded, the right 0 and causal set -- launches the
 *   unwindowed kernels of the plain / rotary entry, bit for bit; every other window takes the banded kernel: each workgroup sweeps only
 *   the 128-key steps its rows' band touches, and split-KV parts divide those steps, so the cost follows the band and not the context.
 *   num_splits 0 chooses the part count from the band's length.  Block-table entries of pages wholly below the band are never read.
 *   The capacity must be below 2^30 (MFA_ERROR_INVALID_ARGS otherwise).  The append, the clamps, the memory-safety rules, stream
 *   capture (after a warm-up call) and the error codes are the plain and rotary entries'.  In-stream, never synchronising. */
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
                                                         int32_t window_right);

/* MI355X extra: sliding-window attention for packed variable-length queries over a 16-bit paged or static KV cache
 * (flash_attn_varlen_func(..., block_table=, window_size=)): the call a continuous-batching server makes for layers that attend to a
 * local window.  The arguments are umfa_varlen_kvcache_attention_rope_forward_stream's followed by the window; rotary_cos == rotary_sin
 * == NULL means no rotary (the other rotary arguments are then ignored), exactly one of them NULL is MFA_ERROR_INVALID_ARGS.  There are
 * no fp8 arguments: fp8 caches with a window are not built.
 *   The contract is umfa_varlen_kvcache_attention_forward_stream's with umfa_kvcache_attention_window_forward_stream's bound applied per
 *   sequence.  For sequence b, L_q,b = cu[b+1] - cu[b] (cu values clamped into [0, total_q], L_q,b to max_seqlen_q), L0_b =
 *   clamp(cache_seqlens[b], 0, cap), L_k,b = min(L0_b + L_q,b, cap) with has_new and L0_b without, and off_b = L_k,b - L_q,b.  Query
 *   token i of sequence b sees key j iff j < L_k,b, j's page entry lies in [0, num_pages) and i + off_b - window_left <= j <= i + off_b +
 *   window_right.  A side given as -1 is unbounded; a value below -1 is MFA_ERROR_INVALID_ARGS.  causal sets window_right = 0 (and, with
 *   rotary, places the query positions as in the rotary entry: the window does not).  A row that sees no key gives O = 0 exactly and
 *   LSE = -inf.  Rows no sequence covers are not written.  The append, the clamps, the dropped rows, memory safety for any contents of
 *   cu_seqlens_q, cache_seqlens and the block table, and the fused rotary pre-pass are the packed and rotary entries', word for word.
 *   window_left >= capacity (max_pages_per_seq * page_size; static: page_size) and window_right >= max_seqlen_q cannot bind and count
 *   as unbounded.  A window with both sides unbounded -- or the left unbounded, the right 0 and causal set -- launches the unwindowed
 *   kernels of the packed / rotary entry, bit for bit; every other window takes the banded kernel: each work item sweeps only the
 *   128-key steps its own rows' band touches, and split-KV parts (one count per launch) divide those steps, so the cost follows the band
 *   and not the context.  num_splits 0 chooses the part count from the item bound and the band's length; with every L_q,b equal that is
 *   umfa_kvcache_attention_window_forward_stream's choice, and the result equals that entry's bit for bit at the same num_splits.
 *   Block-table entries of 16-key groups wholly outside an item's band are never read.  The capacity and max_seqlen_q must be below
 *   2^30 (MFA_ERROR_INVALID_ARGS otherwise).  Stream capture (after a warm-up call), the pooled workspace and the error codes are the
 *   packed entry's; umfa_varlen_kvcache_item_counts reads this call's tally too.  In-stream, never synchronising. */
mfa_error_t umfa_varlen_kvcache_attention_window_forward_stream(
    mfa_context_t context, void* stream, const void* q, const int64_t* q_strides, void* k_cache, const int64_t* k_cache_strides,
    void* v_cache, const int64_t* v_cache_strides, const void* k_new, const int64_t* k_new_strides, const void* v_new,
    const int64_t* v_new_strides, const int32_t* block_table, int64_t block_table_stride, const int32_t* cache_seqlens, uint32_t total_q,
    uint32_t batch, uint32_t max_seqlen_q, const int32_t* cu_seqlens_q, bool has_new, uint32_t num_heads, uint32_t num_kv_heads,
    uint16_t head_dim, uint32_t page_size, uint32_t num_pages, uint32_t max_pages_per_seq, float softmax_scale, bool causal,
    int32_t input_precision, void* out, int32_t out_precision, float* lse, int32_t num_splits, const void* rotary_cos,
    const void* rotary_sin, int32_t rotary_table_precision, int64_t rotary_row_stride, uint32_t seqlen_ro, uint32_t rotary_dim,
    bool rotary_interleaved, int32_t window_left, int32_t window_right);

/* MI355X extra: umfa_attention_backward_stream for grouped-query attention without expanded K / V copies (the reference
 * expands them with repeat_interleave before both passes, metal_sdpa_backend.cpp:1694-1702).  k, v, dk, dv:
 * [B, num_kv_heads, Skv, D]; everything else as umfa_attention_backward_stream.  16-bit MFMA backward only (16-bit
 * operands, head_dim 64 / 128 / 256): otherwise MFA_ERROR_INVALID_ARGS and the caller expands K / V itself. */
mfa_error_t umfa_attention_backward_gqa_stream(mfa_context_t context, void* stream, const void* dout, const void* q,
                                               const void* k, const void* v, const void* out, const float* softmax_lse,
                                               void* dq, void* dk, void* dv, float* d_buffer, uint32_t batch_size,
                                               uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads,
                                               uint32_t num_kv_heads, uint16_t head_dim, float softmax_scale, bool causal,
                                               int32_t input_precision, bool grads_in_input_type, bool out_in_input_type);

/* MI355X extra: mfa_quantized_forward_with_lse in-stream (dense BHSD device pointers, caller's stream, never
 * synchronises).  out fp32 [B,H,Sq,D]; lse (fp32 [B*H*Sq]) and mask (fp32 additive [B,H,Sq,Skv]) may be NULL. */
mfa_error_t umfa_quantized_forward_stream(mfa_context_t context, void* stream, const void* q, const void* k,
                                          const void* v, float* out, float* lse, const float* mask, uint32_t batch_size,
                                          uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim,
                                          float softmax_scale, bool causal, int32_t target_precision, int32_t quant_mode,
                                          int32_t input_precision);

/* MI355X extra: umfa_quantized_forward_stream with the mask the caller has: any <= 4-D broadcastable bool / fp16 / bf16 / fp32 tensor with
 * ELEMENT strides (the arguments of umfa_attention_forward_stream; mfa_prepare_mask's semantics, [B]:157-242) instead of the dense fp32
 * [B,H,Sq,Skv] expansion -- a bool [1,1,Sq,Skv] mask stays Sq Skv bytes (64 MB at S 8192) where the expansion is 4 B H Sq Skv (4.3 GB at
 * B1 H16).  mask_type MFA_MASK_TYPE_NONE or mask NULL: no mask. */
mfa_error_t umfa_quantized_forward_masked_stream(mfa_context_t context, void* stream, const void* q, const void* k, const void* v, float* out,
                                                 float* lse, const void* mask, const int64_t* mask_shape, const int64_t* mask_strides,
                                                 uint32_t mask_ndim, int32_t mask_type, int32_t mask_scalar_type, uint32_t batch_size,
                                                 uint32_t seq_len_q, uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim,
                                                 float softmax_scale, bool causal, int32_t target_precision, int32_t quant_mode,
                                                 int32_t input_precision);

/* MI355X extra: mfa_quantized_backward in-stream (dense BHSD device pointers, caller's stream, never synchronises).
 * Same engines as the blocking entry (16-bit MFMA backward on fp16 de-quantised operands at head_dim 64 / 128 / 256,
 * else fp32-exact).  Every operand enters the fp16 engine as a power-of-two multiple with its largest magnitude in [1, 2) -- the
 * de-quantised Q, K, V and dO, exponents found on the device, handed back through the softmax scale, D and the gradients' epilogues
 * -- so nothing in it can leave fp16's range (dO of 1e-9 or V of 1e12 included).  status: optional device uint32, zeroed on the
 * stream; kept for callers written against round 4, which set it to 1 for an operand outside fp16's range -- it stays 0 now. */
mfa_error_t umfa_quantized_backward_stream(mfa_context_t context, void* stream, const void* q, const void* k,
                                           const void* v, const float* out, const void* dout, const float* lse, float* dq,
                                           float* dk, float* dv, uint32_t* status, uint32_t batch_size, uint32_t seq_len_q,
                                           uint32_t seq_len_kv, uint32_t num_heads, uint16_t head_dim, float softmax_scale,
                                           bool causal, int32_t target_precision, int32_t quant_mode, int32_t input_precision);

int32_t umfa_quantize_rows(mfa_context_t context, void* stream, const void* src, int32_t input_precision,
                           uint32_t batch_heads, uint32_t rows, uint32_t head_dim, int32_t bits, int32_t quant_mode,
                           void* q8_out, void* scales_out, uint32_t* padded_row_bytes);
const char* umfa_last_kernel_name(mfa_context_t context);

/* MI355X extra: launcher switches, context-wide (the context is a process-wide singleton, MFABridge.swift:652-687).
 * They replace environment variables read on the launch path: the environment (UMFA_<NAME>) only gives the initial
 * value when the library is first used.  name / value (strings):
 *   "softmax_reference"  "default" | "exact" | "deferred" | "lazy" -- reference of the online softmax in the
 *                        64-rows-per-wave forward kernels: exact running max (every P <= 1); deferred max (the reference
 *                        moves when a row max exceeds it by 2^softmax_tau); lazy (bf16 only: no row max after a
 *                        segment's first tile, exact power-of-two rebase read off the matrix-pipe row sums).
 *                        default = lazy for bf16, deferred for fp16 and the int8 kernels.
 *   "softmax_tau"        "0" ... "16" (log2 units, default 6)
 *   "force_w64" "no_w64" "w64_grid" "no_mask_flags" "bwd_exact" "bwd_dq" "bwd_persist" "no_split" "force_split"
 *   "no_dma" "bn64" "w64_skew" "no_w64_mask" "no_w64_mask_lazy" "no_w64_bias" "no_w64_f32_mask" "ksplit" "no_pipe"
 *                        kernel-selection overrides used by tests and A/B benches ("0" / "1" or a number)
 *   "bwd_ds_store"       "0" | "1": lab -- the dS-store form of the head_dim 128 non-causal backward (5 products, a
 *                        [B H Sq Skv] scratch in the operand type); measured level with the default (round 4), kept for A/B
 *   "pv_fp16"            "1" (default) | "0": bf16 operands with the P V product in fp16 -- S = K Q^T on the bf16 MFMA, P rounded
 *                        to fp16 (11 bits instead of bf16's 8), V taken as an fp16 image: the bf16-input forward then sits inside
 *                        1e-3 of fp64 SDPA at every sequence length (the bf16 P V product cannot: its format floor is 1.6e-3 from
 *                        S = 4096 on).  Every bf16 forward kernel has the form (all head dims, masks, windows, fused rotation).
 *                        fp16 has five exponent bits where bf16 has eight, so V goes in as V * 2^-e with one power of two e per
 *                        (batch, KV head) slab, taken from the slab's largest |v| ON THE DEVICE (the cast pre-pass of the long
 *                        launches; the converting 128-row kernel checks its own outputs and sweeps a workgroup's keys again with
 *                        the slab's e when e = 0 did not do), and 2^e comes back with the row's 1 / l: exact both ways, finite
 *                        and inside the tolerance for every bf16 V, in-stream, under hipGraph replay, with no status word and no
 *                        state in the context (round 4 had both).  V values more than 2^29 below their slab's largest round into
 *                        fp16's subnormals: errors below 2^-39 of that largest value -- small against the SLAB, not against a query
 *                        row that attends only to such small rows (one exponent per slab serves values 2^29 apart; INTEGRATION.md
 *                        "Range of V", tests/test_gpu_pv16_range.py test_documented_bound_of_the_per_slab_shift).
 *                        "0": the bf16 P V kernels throughout (8-bit P, fp32's exponent range: the remedy for a V that spans more).
 *   "cast_two_pass"      "0" (default) | "1": tests -- the cast pre-pass as two launches (amax, then cast) whatever the slab size
 *                        (by default only slabs of more than 64 workgroups' worth of rows take that form)
 *   "cast_wait_us"       "100" (default): in the one-launch form a workgroup of the cast pre-pass publishes its rows' amax and waits for
 *                        the other workgroups of its (batch, KV head) slab; the wait is bounded by this many microseconds, after which
 *                        the workgroup reads the whole slab for the amax itself (the same number) -- forward progress does not depend
 *                        on the slab's workgroups being resident together (CU-masked streams, many streams).  "0": never wait (tests).
 *                        The same bound serves the runtime quantiser's exchange of a slab's largest |v| (the fp16 V image of the int8 forward).
 *   "cbal"               "0" (default) | "1" | "2": balanced causal pairs on the 128-row forward kernel -- a head's q-blocks (i, last - i) dealt to
 *                        two workgroups of EQUAL length (the long block's tail is published mid-sweep by the workgroup that goes on with the
 *                        short block, the other folds it in): short causal launches no longer end with their longest q-block alone on its CU.
 *                        0: where the plan expects a gain (head_dim 128: >= 8 q-blocks of 128 rows per head, <= 4 workgroups per CU; head_dim
 *                        64: >= 16 q-blocks, <= 2 per CU; no mask tensor; an odd count leaves the middle q-block -- as long as half a pair -- whole); 1: wherever the form exists; 2: never.
 *                        Same results to rounding (another order of the row sums); bitwise repeatable.
 *   "decode_ks"          "0" (default) | "1" | "2": the decode form of the 128-row forward kernel -- at most 32 query rows per (batch, head), no mask, not
 *                        causal, head_dim 64 / 128: the four waves of a workgroup all serve those rows, each owning a key quarter of every 128-key tile (in
 *                        the plain form three of four waves compute rows that do not exist).  0: while the items fit one round of its residency (the
 *                        split-KV plan then counts parts for it); 1: whenever the shape allows; 2: never.  Same results to rounding; bitwise repeatable.
 *   "no_w64_f32_mask"    "0" (default) | "1": fp32 ADDITIVE mask tensors.  By default a mask the one-wave-per-SIMD bias kernels could take as fp16 (<= 4-D
 *                        broadcastable, 16-byte aligned contiguous rows, whole 64 x 64 tiles, bytes within twice the call's tensor traffic -- eight times for [B,1,Sq,Skv] --) is
 *                        classified and copied to fp16 by a pre-pass that also decides ON THE DEVICE whether fp16 holds every value exactly
 *                        (0 / -inf masks, masks built in 16 bits and widened, dyadic biases: yes).  Both routes are enqueued -- the bias kernel on the copy,
 *                        the 128-row kernel on the caller's tensor -- and each checks the verdict word first: exactly one runs, with the numbers that kernel
 *                        gives an fp16 (resp. fp32) mask.  umfa_last_kernel_name then names both.  "1": the 128-row kernel alone, as before.
 *   "no_mask_realign"    "0" (default) | "1": the 128-row kernel reads a mask whose rows are not aligned to four elements (an odd sequence length, a view, strided keys) in
 *                        place, per score, as before the realigned copy (rows padded to four keys with -inf / false: 1.5-2.4 x on dense biases)
 *   "no_w64_ragged_mask" "0" (default) | "1": additive masks whose Sq or Skv is not a multiple of 64 stay on the 128-row kernel (by default Sq >= 1024 and any Skv >= 64 run on the
 *                        bias kernels through a copy padded to whole tiles with -inf; so do fp16 masks whose rows are not 16-byte aligned)
 *   "mask_pass_ratio" "f32_mask_ratio"   "0" (default: the rule's own constants): lab -- the size rule of the mask pre-passes: a float mask is read by a pre-pass (tile
 *                        flags for the 128-row kernel, classes / lists / the fp16 copy for the bias kernels) when its bytes stay within 2 x the call's
 *                        Q + K + V + O bytes, 8 x for a mask with a batch dimension and no head dimension (padding / document masks in additive form);
 *                        a positive value replaces the constant (f32_mask_ratio: for the fp32 route alone).  profiles/r6/mask_pass_rule_probe.jsonl,
 *                        f32_mask_size_rule_probe.jsonl: what larger values buy and cost
 *   "cbal_delta"         "-1" (default: the plan's choice) | "0" ... "16": key tiles by which the folding workgroup's share is shorter (tests, A/B)
 *   "sync_chunks"        "1" (default: off) | "0": by size -- about 14 MB over the link per chunk, at most 8, calls of >= 64 MB | "2" ... "16" (calls of >= 16 MB).  OPT-IN
 *                        (pinning and un-pinning caller memory per call: one of three stress runs under heap churn aborted):
 *                        the synchronous entries (mfa_attention_forward, _with_lse, mfa_attention_backward) on buffers that wrap HOST memory send the
 *                        heads through in chunks on side streams -- one chunk's download under the next ones' uploads, the kernels under both (FLUX
 *                        shape forward, host to host: 2.49 -> 1.89 ms, profiles/r6/host_boundary_probe.jsonl) -- when the operands are dense row-major,
 *                        a mask has no batch / head extent, and the host ranges (>= 1 MiB each) could be pinned: hipHostRegister by the first call
 *                        that wants chunks, for as long as the wrapper lives (mfa_destroy_buffer releases it)
 *   "sync_chunked_calls" read-out: how many synchronous forwards took the chunked form (tests)
 *   "mirror_cache_hits"  read-out: host wrappers (mfa_buffer_from_ptr*) whose HBM mirror was taken from the mirrors of destroyed wrappers (same size, same
 *                        device; at most 32 blocks / 4 GiB are kept, umfa_release_scratch(context, NULL, 1) frees them) instead of a hipMalloc (tests)
 * Returns MFA_ERROR_INVALID_ARGS for an unknown name or a value out of range.  Thread-safe; affects later launches. */
mfa_error_t umfa_set_option(mfa_context_t context, const char* name, const char* value);

/* MI355X extra: the live value of a launcher switch as text (what umfa_set_option would take).
 * MFA_ERROR_INVALID_ARGS: unknown name, NULL arguments or a buffer too small (64 bytes always suffice). */
mfa_error_t umfa_get_option(mfa_context_t context, const char* name, char* value, size_t value_size);

/* MI355X extra: free the library's device scratch (stream-K partials, mask tile flags, quantiser workspace, row constants).
 * Scratch is pooled per (device, stream) and per hipGraph capture, grows geometrically and is otherwise never freed --
 * a launch in flight or a captured graph may hold its addresses.  This call waits for the devices concerned, then frees
 * the pools of `stream` (eager and every capture made on it) or, with all_streams != 0, every pool.  The caller vouches
 * that no graph captured with those pools will be replayed again. */
mfa_error_t umfa_release_scratch(mfa_context_t context, void* stream, int32_t all_streams);

#undef UMFA_QUANT_LEGACY_ARGS
#undef UMFA_QBWD_TAIL
#undef UMFA_QBWD_BLOCKS

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* UMFA_ABI_H */
