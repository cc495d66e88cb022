// fa_paged_rope.h -- rotary embedding fused into the KV-cache attention calls (fa_paged_rope.hip, runtime_paged.hip,
// runtime_paged_varlen.hip): ONE pre-pass launch that replaces the append launch of a rotary call.  It rotates k_new into the cache,
// appends v_new unrotated, and rotates q into a dense operand-type image that the unchanged attention kernels then read.  Included only
// by those three units: no existing unit's device code depends on it.
//
// Tables: cos / sin [seqlen_ro, rotary_dim / 2], fp32 or the operand type (16-bit entries convert exactly to fp32 on load), unit column
// stride, row stride `rstride` elements, rows 16-byte aligned.  Non-interleaved (GPT-NeoX): element i pairs with i + rotary_dim / 2;
// interleaved: element 2i with 2i + 1; table column i either way.  Elements at rotary_dim and above pass through unchanged.  The pair
// (a, b) at column i and position pos becomes
//   a' = fma(a, cos[pos, i], -(b sin[pos, i]))     b' = fma(b, cos[pos, i], a sin[pos, i])
// in fp32 (rope_rotate8's arithmetic, fa_common.h: products and sums pinned, the fp32 results final before the conversion), rounded once
// to the operand type.  For an fp8 cache the rounded key is then quantised by fa_paged_fp8.h's rule.
//
// Positions, read on the device: row t of sequence b's new keys is rotated at L0_b + t, L0_b = cache_seqlens[b] clamped into [0, cap]
// (paged_lens / paged_varlen_lens); query row i at L0_b + i when causal, every query row at L0_b when not (flash-attention's rule).
// A position >= seqlen_ro uses table row seqlen_ro - 1: memory-safe, defined, meaningless -- the caller sizes the table.
// Every clamp, dropped append row and masking rule is fa_paged.h's / fa_paged_varlen.h's, word for word.  Packed rows that no sequence
// covers are copied into the q image unrotated (the attention never uses them).
#pragma once
#include "fa_paged_fp8.h"
#include "fa_paged_varlen.h"

namespace umfa {

struct PagedRopeParams {
    PagedVarlenParams v;   // v.p: the call's PagedParams (q = the caller's q, its strides); packed form: cu, Tq (items / counts unused)
    const float* kd;       // fp8 cache: the descales of fa_paged_fp8.h, else NULL
    const float* vd;
    int64_t kdb, kdh, vdb, vdh;
    const void* cos;       // [seqlen_ro][rstride], the first rdim / 2 columns used
    const void* sin;
    void* qimg;            // dense [B, Sq, H, D] (packed: [T_q, H, D]) in the operand type, 16-byte aligned
    int64_t rstride;       // table row stride in elements
    uint32_t seqlen_ro, rdim;
    int interleaved, table_f32, fp8, packed;
};

// the rotary arguments of the two *_rope_forward_stream entries (include/umfa_abi.h), as the caller gave them
struct RopeArgs {
    const void* cos;
    const void* sin;
    int table_f32;  // 1: rotary_table_precision is fp32, 0: the operand type, -1: neither (the entry refuses the call)
    int64_t row_stride;
    uint32_t seqlen_ro, rotary_dim;
    bool interleaved;
};

// an entry's rotary arguments; table_fp32 / table_operand: rotary_table_precision is fp32 / is the call's input_precision
inline RopeArgs paged_rope_args(const void* cos, const void* sin, bool table_fp32, bool table_operand, int64_t row_stride, uint32_t seqlen_ro,
                                uint32_t rotary_dim, bool interleaved) {
    return RopeArgs{cos, sin, table_fp32 ? 1 : table_operand ? 0 : -1, row_stride, seqlen_ro, rotary_dim, interleaved};
}

// r's table fields from the entry's arguments (everything else of r is the runtime's)
inline void paged_rope_fill(PagedRopeParams& r, const RopeArgs& a) {
    r.cos = a.cos; r.sin = a.sin; r.rstride = a.row_stride; r.seqlen_ro = a.seqlen_ro; r.rdim = a.rotary_dim;
    r.interleaved = a.interleaved ? 1 : 0;
    r.table_f32 = a.table_f32;
}

bool paged_rope_supported(const PagedRopeParams& r);
hipError_t launch_paged_rope(const PagedRopeParams& r, hipStream_t stream);
size_t paged_rope_qimg_bytes(const PagedRopeParams& r);

}  // namespace umfa
