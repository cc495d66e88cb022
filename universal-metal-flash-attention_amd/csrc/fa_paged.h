// fa_paged.h -- paged / static KV-cache attention for inference (fa_fwd_16_paged.hip, runtime_paged.hip): the launch parameters and
// the per-sequence lengths and pages every kernel resolves on the device.  Included only by the paged translation units: no existing
// unit's device code depends on it.
//
// Layout: q [B, Sq, H, D] with element strides (batch, token, head); k_cache / v_cache [num_pages, page_size, H_kv, D] with element
// strides (page, token, head); head_dim contiguous everywhere.  Sequence b's logical page lp is physical page block_table[b][lp]; with
// no block table (static cache) page b is sequence b's whole row of page_size = S_max tokens.  k_new / v_new [B, S_new, H_kv, D] are
// appended at cache_seqlens[b] ..  Attention covers L_k = cache_seqlens[b] + S_new keys, causal bottom-right (query i sees key j iff
// j <= i + L_k - Sq).  out dense [B, Sq, H, D], lse fp32 [B, H, Sq].
//
// Memory safety, decided on the device: cache_seqlens[b] and L_k are clamped into [0, max_pages * page_size]; a block-table entry
// outside [0, num_pages) is never dereferenced (its keys are masked, append skips its rows).  Pages shared by several sequences may be
// read; appending into a shared page is the caller's race.
#pragma once
#include <hip/hip_runtime.h>

#include "fa_bwd_16_common.h"  // d_off, make_srd, i32x4
#include "fa_common.h"

namespace umfa {

struct PagedParams {
    const void* q;
    void* kc;              // cache pools (the append writes into them)
    void* vc;
    const void* kn;        // new tokens, may be NULL when Snew == 0
    const void* vn;
    const int32_t* bt;     // block table [B][bt_stride] (NULL: static cache)
    const int32_t* seqlens;  // [B]
    void* out;             // dense [B, Sq, H, D], out_prec
    float* lse;            // optional, [B, H, Sq]
    float* part;           // split: partial O [nsplit][B H_kv R][D] fp32, then (m, l) [nsplit][B H_kv R][2]
    int64_t qsb, qst, qsh;  // element strides
    int64_t kpg, kst, ksh, vpg, vst, vsh;
    int64_t knb, knt, knh, vnb, vnt, vnh;
    int64_t bt_stride;
    uint32_t B, Sq, Snew, H, Hkv, D, page_size, num_pages, max_pages;
    int32_t page_shift;     // log2(page_size) when a power of two, else -1
    uint32_t R, nrb, nsplit;  // rows per (batch, KV head) = (H / H_kv) Sq; row blocks; split-KV parts
    float scale;
    int causal, in_prec, out_prec, ks4;  // ks4: R <= 32, the four waves split each step's keys
};

bool paged_supported(const PagedParams& p);
hipError_t launch_paged_append(const PagedParams& p, hipStream_t stream);
hipError_t launch_fwd_16_paged(const PagedParams& p, hipStream_t stream, const char** name);
hipError_t launch_paged_fold(const PagedParams& p, hipStream_t stream);  // the split-KV fold alone (p.nsplit parts in p.part)
bool paged_fwd_args_ok(const PagedParams& p);  // out / lse alignment, out_prec and R / nrb / ks4: the checks the forward launchers share

namespace {

// sequence b's cached length L0 (before the append) and the key count L_k, both clamped into [0, capacity]
__device__ __forceinline__ void paged_lens(const PagedParams& p, uint32_t b, uint32_t& L0, uint32_t& Lk) {
    const int cap = (int)(p.max_pages * p.page_size);
    int s = p.seqlens[b];
    s = s < 0 ? 0 : (s > cap ? cap : s);
    const int64_t lk = (int64_t)s + p.Snew;
    L0 = (uint32_t)s;
    Lk = (uint32_t)(lk < cap ? lk : cap);
}

__device__ __forceinline__ uint32_t paged_lpage(const PagedParams& p, uint32_t pos) {
    return p.page_shift >= 0 ? pos >> p.page_shift : pos / p.page_size;
}

// physical page of sequence b's logical page lp, or -1 when the entry is outside [0, num_pages) (never dereferenced)
__device__ __forceinline__ int paged_page(const PagedParams& p, uint32_t b, uint32_t lp) {
    if (lp >= p.max_pages) return -1;
    const int pg = p.bt ? p.bt[(int64_t)b * p.bt_stride + lp] : (int)b;
    return pg >= 0 && (uint32_t)pg < p.num_pages ? pg : -1;
}

}  // namespace

}  // namespace umfa
