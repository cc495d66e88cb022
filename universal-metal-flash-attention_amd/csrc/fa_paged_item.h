// fa_paged_item.h -- where a KV-cache forward workgroup's coordinates come from and where its rows are stored: the one thing in which a
// dense kernel (q [B, Sq, H, D], fa_paged.h) and its packed twin (cu_seqlens_q, fa_paged_varlen.h) differ.  A body written once for
// both (fa_paged_window_body.h) is a template over one of these two types and holds everything else.
//
// An item is a plain struct of always-inline members; nothing of it is kept in memory.  What a body reads of it:
//   part, b, hk, rb   the split-KV part, the sequence, the KV head and the 128-row block (0 in the decode form)
//   R, Lq, ks4        rows per KV head g L_q, the query tokens of the sequence, the decode form (R <= 32)
//   key_count()       L_k of the sequence, clamped, wave-uniform
//   q_row(qi, h)      the query row of token qi and head h
//   part_rows(), part_row(r)   rows of one split-KV part, and row r of this item among them
//   o_row(qi, h), lse_at(qi, h)   the output row (x D: the element) and the LSE index
#pragma once
#include "fa_paged_varlen.h"

namespace umfa {

namespace {

// the item of a dense launch: decoded from blockIdx; R, ks4 and L_q = Sq are the launch's
struct PagedDenseItem {
    const PagedParams* pp;
    uint32_t part, b, hk, rb, bk, R, Lq;
    bool ks4;

    __device__ __forceinline__ void decode(const PagedParams& p) {
        pp = &p;
        part = blockIdx.x % p.nsplit;
        const uint32_t item = blockIdx.x / p.nsplit;
        rb = item % p.nrb;
        bk = item / p.nrb;
        hk = bk % p.Hkv;
        b = bk / p.Hkv;
        R = p.R;
        Lq = p.Sq;
        ks4 = p.ks4 != 0;
    }
    __device__ __forceinline__ uint32_t key_count() const {
        uint32_t L0u, Lku;
        paged_lens(*pp, b, L0u, Lku);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)Lku);
    }
    template <typename T>
    __device__ __forceinline__ const T* q_row(uint32_t qi, uint32_t h) const {
        return (const T*)pp->q + (int64_t)b * pp->qsb + (int64_t)qi * pp->qst + (int64_t)h * pp->qsh;
    }
    __device__ __forceinline__ int64_t part_rows() const { return (int64_t)pp->B * pp->Hkv * pp->R; }
    __device__ __forceinline__ int64_t part_row(uint32_t r) const { return (int64_t)bk * pp->R + r; }
    __device__ __forceinline__ int64_t o_row(uint32_t qi, uint32_t h) const { return ((int64_t)b * pp->Sq + qi) * pp->H + h; }
    __device__ __forceinline__ int64_t lse_at(uint32_t qi, uint32_t h) const { return ((int64_t)b * pp->H + h) * pp->Sq + qi; }
};

// the item of a packed launch: read from the item list (fa_paged_varlen_items_kernel) with one scalar load, the sequence's query range
// from cu_seqlens_q, the form decided from the item's own L_q; rows are cu[b] + token, the partials the packed layout of fa_paged_varlen.h
struct PagedPackedItem {
    const PagedVarlenParams* vp;
    uint32_t part, b, hk, rb, q0, R, Lq;
    bool ks4;

    // false: this workgroup has nothing to do
    __device__ __forceinline__ bool decode(const PagedVarlenParams& v) {
        const PagedParams& p = v.p;
        vp = &v;
        part = blockIdx.x % p.nsplit;
        const uint32_t item = blockIdx.x / p.nsplit;
        // {sequence or -1, hk * blocks + row block}
        const int it_b = __builtin_amdgcn_readfirstlane(v.items[2 * (size_t)item]);
        const uint32_t it_j = (uint32_t)__builtin_amdgcn_readfirstlane(v.items[2 * (size_t)item + 1]);
        if (it_b < 0 || (uint32_t)it_b >= p.B) return false;  // past the end of the list
        b = (uint32_t)it_b;
        varlen_range(v.cu, b, v.Tq, p.Sq, q0, Lq);
        R = (p.H / p.Hkv) * Lq;  // rows per KV head of this sequence
        if (R == 0) return false;
        ks4 = R <= 32;  // the decode form, from the item's own L_q
        const uint32_t nrb = ks4 ? 1u : (R + 127) / 128;
        hk = it_j / nrb;
        rb = it_j % nrb;
        if (hk >= p.Hkv) return false;  // (cu rewritten between the pre-pass and this launch: nothing to do safely)
        // debug tally of the forms this launch ran (umfa_varlen_kvcache_item_counts): one atomic per item
        if (part == 0 && threadIdx.x == 0) atomicAdd(v.counts + (ks4 ? 0 : 1), 1u);
        return true;
    }
    __device__ __forceinline__ uint32_t key_count() const {
        uint32_t L0u, Lku;
        paged_varlen_lens(*vp, b, Lq, L0u, Lku);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)Lku);
    }
    template <typename T>
    __device__ __forceinline__ const T* q_row(uint32_t qi, uint32_t h) const {
        return (const T*)vp->p.q + (int64_t)(q0 + qi) * vp->p.qst + (int64_t)h * vp->p.qsh;
    }
    __device__ __forceinline__ int64_t part_rows() const { return (int64_t)vp->Tq * vp->p.H; }
    __device__ __forceinline__ int64_t part_row(uint32_t r) const { return (int64_t)q0 * vp->p.H + (int64_t)hk * R + r; }
    __device__ __forceinline__ int64_t o_row(uint32_t qi, uint32_t h) const { return (int64_t)(q0 + qi) * vp->p.H + h; }
    __device__ __forceinline__ int64_t lse_at(uint32_t qi, uint32_t h) const { return (int64_t)h * vp->Tq + q0 + qi; }
};

}  // namespace

}  // namespace umfa
