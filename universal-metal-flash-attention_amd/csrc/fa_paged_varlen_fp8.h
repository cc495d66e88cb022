// fa_paged_varlen_fp8.h -- packed variable-length queries over an OCP fp8 (e4m3fn) paged / static KV cache
// (fa_fwd_16_paged_varlen_fp8.hip, runtime_paged_varlen.hip): the parameters of fa_paged_varlen.h with fa_paged_fp8.h's dequantisation
// scale per (SEQUENCE, KV head).  PagedVarlenParams is a kernel argument of the 16-bit packed kernels and does not grow: this struct
// wraps it, as PagedFp8Params and PagedWindowParams wrap PagedParams.  Included only by those two units.
//
// The contract is the union of the two existing ones.  Layout of q / cu_seqlens_q / the caches / the table / the lengths, L_k,b =
// min(L0_b + L_q,b, cap), bottom-right causal per sequence, dead rows (O = 0, LSE = -inf), uncovered rows left unwritten, the work
// items, the packed split partials and every clamp that makes any contents of cu_seqlens_q, cache_seqlens and the table memory-safe:
// fa_paged_varlen.h, word for word.  Bytes and arithmetic: fa_paged_fp8.h's -- a cache byte stands for e4m3fn(byte) * descale[b, h_kv]
// with b the sequence (a page shared by two sequences decodes under each one's own descale), the descales are device fp32 addressed
// through (sequence, KV head) element strides that may be 0 and are never read by the host, K8 expands exactly to q's type and V8
// exactly to fp16, k_descale folds into scale log2(e) and v_descale into the epilogue's 1 / l, cache strides are bytes and multiples
// of 16.
//
// Append: packed row t of sequence b is stored at L0_b + (t - cu[b]) as e4m3fn_rne(clamp(fp32(x) / descale[b, h_kv], -448, +448)) -- IEEE
// fp32 division, the clamp in front of the conversion; rows no sequence covers, rows past the capacity and rows of pages the table
// does not hold are dropped (fa_paged_varlen_append_kernel's rules).  Rotary: fa_paged_rope.h's rule at positions L0_b + (t - cu[b])
// (every query row of a non-causal call at L0_b); the rotated key is rounded once to the operand type, then quantised; one pre-pass
// launch replaces the append launch.
#pragma once
#include "fa_paged_fp8.h"
#include "fa_paged_varlen.h"

namespace umfa {

struct PagedVarlenFp8Params {
    PagedVarlenParams v;
    const float* kd;  // k_descale
    const float* vd;  // v_descale
    int64_t kdb, kdh, vdb, vdh;  // (sequence, KV head) element strides, >= 0
};

// the fused rotary pre-pass of a call (fa_paged_rope.h's tables and rules, its PagedRopeParams' table fields under the same names)
struct PagedVarlenFp8RopeParams {
    PagedVarlenFp8Params f;  // the call's parameters with the caller's q and its strides (items / counts unused)
    const void* cos;         // [seqlen_ro][rstride], the first rdim / 2 columns used
    const void* sin;
    void* qimg;              // dense [T_q, H, D] in the operand type, 16-byte aligned
    int64_t rstride;         // table row stride in elements
    uint32_t seqlen_ro, rdim;
    int interleaved, table_f32;
};

bool paged_varlen_fp8_supported(const PagedVarlenFp8Params& f);
hipError_t launch_paged_varlen_fp8_append(const PagedVarlenFp8Params& f, hipStream_t stream);
bool paged_varlen_fp8_rope_supported(const PagedVarlenFp8RopeParams& r);
hipError_t launch_paged_varlen_fp8_rope(const PagedVarlenFp8RopeParams& r, hipStream_t stream);
hipError_t launch_fwd_16_paged_varlen_fp8(const PagedVarlenFp8Params& f, hipStream_t stream, const char** name);  // items, forward, fold

}  // namespace umfa
