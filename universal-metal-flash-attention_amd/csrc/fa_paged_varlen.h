// fa_paged_varlen.h -- packed variable-length queries over a paged / static KV cache (fa_fwd_16_paged_varlen.hip,
// runtime_paged_varlen.hip): the launch parameters and the per-sequence query range and lengths every kernel resolves on the device.
// Included only by those two units: no existing unit's device code depends on it.
//
// Layout: q [T_q, H, D] with element strides (token, head), head_dim contiguous.  cu_seqlens_q device int32 [B + 1]: sequence b owns
// rows cu[b] .. cu[b+1] - 1, L_q,b = cu[b+1] - cu[b].  k_cache / v_cache, block_table, cache_seqlens and the static form: fa_paged.h.
// k_new / v_new [T_q, H_kv, D], packed by the same cu_seqlens_q: sequence b's rows are appended at cache_seqlens[b] .. before the
// attention.  L0 = clamp(cache_seqlens[b], 0, cap); L_k = min(L0 + L_q,b, cap) with new tokens, L0 without.  Causal is bottom-right
// per sequence: query i of sequence b sees key j iff j <= i + L_k - L_q,b (and j's page entry lies in [0, num_pages)).  out dense
// [T_q, H, D], lse fp32 [H, T_q] (natural log).  A row that sees no key: O = 0, LSE = -inf.  Rows no sequence covers are not written.
//
// Memory safety for any contents of cu_seqlens_q, cache_seqlens and the block table: cu values are clamped into [0, T_q] and L_q,b to
// max_seqlen_q (varlen_range), lengths and table entries as in fa_paged.h, append rows past the capacity or into a page the table does
// not hold are dropped.  Results are defined for non-decreasing cu with cu[B] <= T_q; for anything else only q, the pools, k_new /
// v_new, O, LSE and the library's scratch are touched.
//
// Work distribution: a sequence with R = g L_q,b <= 32 rows per KV head (g = H / H_kv) is one item per KV head in the decode form
// (ks4: the four waves split each step's keys); any other is ceil(R / 128) items per KV head in the 128-row form.  The host bounds
// the item count by n_items = H_kv * min(floor(g T_q / 128) + B, B * ceil(g max_q / 128)); fa_paged_varlen_items_kernel (one
// workgroup, a pre-pass on the stream) writes {sequence, hk * blocks + row block} per item into scratch, {-1, 0} past the end; the
// forward's workgroup reads its item with one scalar load and decides its form from its own L_q,b.
//
// Split-KV partials are fp32 rows in the packed order the items own disjointly: row (start_b H + hk g L_q,b + r) of part s, then the
// (m, l) pairs -- n_split * T_q * H * (D + 2) floats whatever the mix of forms.
#pragma once
#include "fa_paged.h"
#include "fa_varlen.h"  // varlen_range

namespace umfa {

struct PagedVarlenParams {
    PagedParams p;         // q / caches / table / lengths / out / lse / part, strides (qsb, knb, vnb unused), geometry; B = sequences,
                           // Sq = max_seqlen_q, Snew = has_new (0 / 1), R / nrb / ks4 unused (per item, on the device)
    const int32_t* cu;     // cu_seqlens_q, device int32 [B + 1]
    int32_t* items;        // scratch: n_items x {sequence or -1, hk * blocks + row block}
    uint32_t* counts;      // scratch: 4 words the pre-pass zeroes; the forward counts the items it ran in the decode form [0] and
                           // in the 128-row form [1] (a debug tally, umfa_varlen_kvcache_item_counts)
    uint32_t Tq, n_items;
};

bool paged_varlen_supported(const PagedVarlenParams& v);
uint32_t paged_varlen_item_bound(const PagedVarlenParams& v);  // n_items for v's T_q, B, max_seqlen_q, H, H_kv
hipError_t launch_paged_varlen_append(const PagedVarlenParams& v, hipStream_t stream);
hipError_t launch_fwd_16_paged_varlen(const PagedVarlenParams& v, hipStream_t stream, const char** name);  // items, forward, fold
hipError_t launch_paged_varlen_items(const PagedVarlenParams& v, hipStream_t stream);  // the item-list pre-pass alone
hipError_t launch_paged_varlen_fold(const PagedVarlenParams& v, hipStream_t stream);   // the split-KV fold alone (p.nsplit parts in p.part)

namespace {

// sequence b's cached length L0 and key count L_k for its Lq query rows, both clamped into [0, capacity]
__device__ __forceinline__ void paged_varlen_lens(const PagedVarlenParams& v, uint32_t b, uint32_t Lq, uint32_t& L0, uint32_t& Lk) {
    const int cap = (int)(v.p.max_pages * v.p.page_size);
    int s = v.p.seqlens[b];
    s = s < 0 ? 0 : (s > cap ? cap : s);
    const int64_t lk = (int64_t)s + (v.p.Snew ? Lq : 0u);
    L0 = (uint32_t)s;
    Lk = (uint32_t)(lk < cap ? lk : cap);
}

// the sequence whose range [start, start + len) holds packed row t, or false.  cu non-decreasing: the last b with cu[b] <= t; any
// other contents end in some b < B whose clamped range is then checked, so nothing is read past cu[B].
__device__ __forceinline__ bool paged_varlen_find(const PagedVarlenParams& v, uint32_t t, uint32_t& b, uint32_t& start, uint32_t& len) {
    uint32_t lo = 0, hi = v.p.B;  // first index in [1, B] with cu[i] > t, minus one
    while (lo + 1 < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.cu[mid] <= (int)t) lo = mid; else hi = mid;
    }
    int a = v.cu[lo], e = v.cu[lo + 1];
    a = a < 0 ? 0 : (a > (int)v.Tq ? (int)v.Tq : a);
    e = e < a ? a : (e > (int)v.Tq ? (int)v.Tq : e);
    uint32_t l = (uint32_t)(e - a);
    l = l < v.p.Sq ? l : v.p.Sq;
    b = lo; start = (uint32_t)a; len = l;
    return t >= (uint32_t)a && t - (uint32_t)a < l;
}

}  // namespace

}  // namespace umfa
