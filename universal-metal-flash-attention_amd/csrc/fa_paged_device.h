// fa_paged_device.h -- the device leaves the six KV-cache forwards share: the plain, fp8 and sliding-window kernels, each in a dense form
// (fa_fwd_16_paged.hip, fa_fwd_16_paged_fp8.hip, fa_fwd_16_paged_window.hip) and a packed one (fa_fwd_16_paged_varlen.hip,
// fa_fwd_16_paged_varlen_fp8.hip, fa_fwd_16_paged_varlen_window.hip).  What differs between the callers (the mask predicate, the
// destination rows) comes in as an always-inline callable, an item (fa_paged_item.h) or a plain argument.  Each translation unit gets
// its own copy (internal linkage), as with fa_paged_fp8.h's pieces of the fp8 stage ring.
//
// Above the leaves, the two sliding-window kernels are one body (fa_paged_window_body.h) over the dense or the packed item.  The plain
// and the fp8 kernels keep their own shells -- parameters, item and row mapping, key range and split, step loop, staging scheme and
// barriers -- in a dense and a packed copy each, which must be edited in step: the packed kernels' bitwise agreement with the dense
// ones at equal lengths (tests/test_gpu_varlen_paged.py, tests/test_gpu_varlen_paged_fp8.py) fails otherwise.  One body for each of
// those pairs was built and measured: same registers, same loop, 0.5 - 2.5 % slower (profiles/paged_body/summary.md).
//
// paged_tile is called by five of the six: fa_fwd_16_paged_varlen.hip keeps the same step in place, because the shared function cost
// that kernel alone 1.5 % of its time (profiles/paged_shared/summary.md).  A change to one of the two must be made to the other.
//
// The workgroup: 4 waves x 32 query rows, S^T = K Q^T so a lane owns one query (ql = lane & 31) and one half of the subtile's keys
// (hi = lane >> 5); the exact running max is shared by the two halves, P V runs in fp16.  A step is 128 keys of K and of V: four 32-key
// subtiles in fa_bwd_16_common.h d_off<DP>'s image.  R <= 32 rows ("ks4", the decode form): every wave holds the same rows and takes
// one subtile of each step, and the four partial (O, m, l) meet in LDS behind the loop (paged_ks4_publish, a barrier, paged_ks4_fold).
//
// Page indirection (the 16-bit caches): a 1-KiB LDS-DMA piece holds 4 rows (D = 128) or 8 rows (D = 64); a page holds a multiple of 16
// rows, so a piece never straddles two pages and gets a buffer descriptor based at its own page, its range the rows of that page below
// the last key wanted.  A block-table entry outside [0, num_pages) gives a descriptor of zero bytes (the rows land as zeros) and its
// keys are masked in the scores.  Only (page_size + 8) x token stride x 2 bytes has to fit the descriptors' 32-bit offsets (a static
// row's last piece may start up to 8 rows before its end and run past it: paged_supported); the pool may be any size.
//
// bf16 V (the 16-bit caches): the tile lands as bf16 and every wave converts the V pieces its own DMA filled to fp16 in place
// (v * 2^-e), keeping the largest |v| it saw (paged_convert_v).  Behind the loop the 128-row kernel's range rule decides
// (fa_fwd_16_kernel.h v_range_check): outputs non-finite, or rows with keys and every output below 2^-11, sweep this workgroup's keys
// once more with e from that largest |v|; the outputs are shifted back.  The rule itself stays in the 16-bit kernels and the window
// body: as a shared function it cost each bf16 kernel 4 to 10 scalar registers, up to a spill (profiles/paged_shared/resources.md).
#pragma once
#include <type_traits>

#include "fa_paged.h"
#include "fa_fwd_16_kernel.h"

namespace umfa {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// lanes 0 .. 7 (and again 8 .. 15, ...): the physical page of 16-key group (lane & 7) of step s (keys 128 s .. 128 s + 127), -1 for an
// entry outside the pool or a group wholly outside the keys [kfirst, Le) (its entry is not read).  One vector load per step, issued a
// step ahead of its use: read one entry at a time with scalar loads, every piece and subtile waited for its own (page_size had no effect
// on the rate: all of it was these waits).
__device__ __forceinline__ int paged_table(const PagedParams& p, uint32_t b, uint32_t kfirst, uint32_t Le, uint32_t s, int lane) {
    const uint32_t key = s * 128 + 16 * (uint32_t)(lane & 7);
    return key < Le && key + 15 >= kfirst ? paged_page(p, b, paged_lpage(p, key)) : -1;
}

// LDS-DMA of step s of one cache tensor, KV head at head_b bytes, into the 128-row swizzled image at lds_dst (pgv: paged_table of step
// s): piece n (RPP rows) goes to lds_dst + n KiB, wave uw issues pieces uw, uw + 4, ...  Rows of keys at or past Le lie past the
// descriptor's range, rows of keys below kfirst are sent there: both land as zeros.
template <int DP>
__device__ __forceinline__ void paged_dma_step(const PagedParams& p, const char* pool, int64_t page_b, int64_t head_b, uint32_t tst_b,
                                               int pgv, uint32_t kfirst, uint32_t Le, uint32_t s, unsigned lds_dst, int uw, int lane) {
    constexpr int ROW_B = 2 * DP, NCH = DP / 8, RPP = 1024 / ROW_B, NP = 128 / RPP;
    const int r = lane / NCH, c = lane % NCH;
#pragma nounroll
    for (int n0 = 0; n0 < NP; n0 += 4) {  // (one piece at a time: unrolled, the descriptors of all pieces ran out of scalar registers)
        const int n = n0 + uw;
        const uint32_t key0 = s * 128 + (uint32_t)(RPP * n);
        const uint32_t lp = paged_lpage(p, key0);
        const int pg = __builtin_amdgcn_readlane(pgv, (RPP * n) / 16);  // (the step's page of this piece's 16-key group: paged_table)
        const uint32_t pstart = lp * p.page_size;
        uint32_t nv = Le > pstart ? Le - pstart : 0u;
        nv = nv < p.page_size ? nv : p.page_size;
        const uint32_t bytes = pg >= 0 && nv ? (nv - 1) * tst_b + ROW_B : 0u;
        const i32x4 srd = make_srd(pool + (int64_t)(pg >= 0 ? pg : 0) * page_b + head_b, bytes);
        const int row = RPP * n + r;
        const int voff = key0 + (uint32_t)r < kfirst ? (int)bytes
                                                     : (int)((key0 - pstart + (uint32_t)r) * tst_b) + (d_off<DP>(row, c) - row * ROW_B);
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                     ::"s"(lds_dst + n * 1024), "v"(voff), "s"(srd) : "memory");
    }
}

// bf16 -> fp16 (x vmul) in place: the pieces of the V stage at vstage that this wave's own DMA filled (its vmcnt wait is all the
// ordering needed).  vamax: the largest |v| (bits) this thread converted.
template <int DP>
__device__ __forceinline__ void paged_convert_v(char* vstage, float vmul, unsigned& vamax, int uw, int lane) {
    constexpr int NP = 128 / (1024 / (2 * DP));  // pieces per step and tensor
#pragma unroll
    for (int n0 = 0; n0 < NP; n0 += 4) {
        char* const vq = vstage + (n0 + uw) * 1024 + lane * 16;
        const u32x4 x = *(const u32x4*)vq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned a = x[j] & 0x7fff7fffu, m2 = (a & 0xffffu) > (a >> 16) ? (a & 0xffffu) : (a >> 16);
            vamax = vamax > m2 ? vamax : m2;
        }
        *(u32x4*)vq = u32x4{bf16x2_to_f16x2_scaled(x[0], vmul), bf16x2_to_f16x2_scaled(x[1], vmul),
                            bf16x2_to_f16x2_scaled(x[2], vmul), bf16x2_to_f16x2_scaled(x[3], vmul)};
    }
}

// this lane's query row as the B operand of S^T = K Q^T; a row past the last one is zeros
template <typename T, int DP>
__device__ __forceinline__ void paged_load_q(typename Mma16<T>::V8 (&qf)[DP / 16], const T* qp, bool rok, int hi) {
#pragma unroll
    for (int ks = 0; ks < DP / 16; ++ks) {
        if (rok) {
            qf[ks] = *(const typename Mma16<T>::V8*)(qp + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (T)0.0f;
        }
    }
}

// the online-softmax step on one 32-key subtile: K at Kt (T), V at Vt (fp16).  c: scale log2(e); m: running max of c S (log2 domain,
// shared by the halves), l: this half's sum of P.  On an edge subtile, masked(kr) says whether key row kr of the subtile is hidden from
// this lane's query.  (fa_fwd_16_paged_varlen.hip holds a copy of this body, its tile_body: keep the two in step.)
template <typename T, int DP, typename MASKED>
__device__ __forceinline__ void paged_tile(const char* Kt, const char* Vt, const typename Mma16<T>::V8 (&qf)[DP / 16], float c,
                                           f32x16 (&acc)[DP / 32], float& m, float& l, int ql, int hi, int tr_qq, int tr_pp, int tr_g1, bool edge,
                                           MASKED masked) {
    BWD16_GEO(DP);
    (void)TILE_PIECES;
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    typedef Mma16<_Float16> MP;  // the P V product: fp16 P, fp16 V
    typedef typename MP::V8 PV8;
    f32x16 s;
    V8 ak[NKS];
#pragma unroll
    for (int ks = 0; ks < PD; ++ks) ak[ks] = *(const V8*)(Kt + d_off<DP>(ql, 2 * ks + hi));
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (ks + PD < NKS) ak[ks + PD] = *(const V8*)(Kt + d_off<DP>(ql, 2 * (ks + PD) + hi));
        s = M::mma(ak[ks], qf[ks], ks ? s : f32x16{});
    }
    float x[16], mx = -INFINITY;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        x[rr] = s[rr] * c;
        if (edge && masked(acc_row(rr, hi))) x[rr] = -INFINITY;
        mx = fmaxf(mx, x[rr]);
    }
    mx = max_xor32(mx);
    const float mn = fmaxf(m, mx);
    const float base = mn == -INFINITY ? 0.0f : mn;
    const float alpha = __builtin_amdgcn_exp2f(m - base);  // (m = -inf: 0)
    m = mn;
    l *= alpha;
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[i][rr] *= alpha;
    PV8 pb[2];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const float pr = __builtin_amdgcn_exp2f(x[rr] - base);
        l += pr;
        pb[rr >> 3][rr & 7] = (_Float16)pr;
    }
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
            acc[i] = MP::mma(tr_frag<MP, DP>(Vt, i, s2, hi, tr_qq, tr_pp, tr_g1), pb[s2], acc[i]);
}

// the decode form's exchange: waves 1..3 publish (O^T, m, l) behind the reserved header (FWD16_EPI_HDR words, in front of which the
// range rule's words lie); behind a barrier, which the kernel places, wave 0 folds them into its own.  Every wave has passed the step
// loop's last barrier and every request has landed, so the first AREA_B bytes of LDS (the tiles, or the 16-bit image) are free.
// Which reason frees the area depends on the caller: the 16-bit kernels pass their tile area (4 stages; every DMA was waited for in front
// of the loop's last barrier), the fp8 kernels their 16-bit image (2 images; the ring behind it is not touched, and its last requests
// landed before the last expansion).  The words in front of the header are used by the 16-bit kernels' range rule only.
// The fold's roundings are written out with explicit fmas, as the parent's build made them: O a0 is rounded, then aw O_w is added with one
// fma each; l a0 + a1 l_1 rounds a1 l_1, then one fma each.  `x *= a0; x += aw * e` leaves the compiler two contractions (fma(aw, e, x a0)
// or fma(x, a0, aw e)) that round differently, and which one it took depended on where the code stood.
template <int DP, int AREA_B>
__device__ __forceinline__ void paged_ks4_publish(char* smem, const f32x16 (&acc)[DP / 32], float m, float L, int uw, int lane) {
    constexpr int NDB = DP / 32, EXW = 16 * NDB + 2;
    static_assert(FWD16_EPI_RED + 8 <= FWD16_EPI_HDR && (FWD16_EPI_HDR + 3 * EXW * 64) * 4 <= AREA_B,
                  "the exchange lies behind the range rule's words, inside the free area");
    float* const e = (float*)smem + FWD16_EPI_HDR + (uw - 1) * EXW * 64 + lane;
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) e[(16 * i + rr) * 64] = acc[i][rr];
    e[(16 * NDB) * 64] = m;
    e[(16 * NDB + 1) * 64] = L;
}
template <int DP>
__device__ __forceinline__ void paged_ks4_fold(const char* smem, f32x16 (&acc)[DP / 32], float& m, float& L, int lane) {
    constexpr int NDB = DP / 32, EXW = 16 * NDB + 2;
    const float* const ex = (const float*)smem + FWD16_EPI_HDR;
    float mw[3], Mx = m;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        mw[w] = ex[(w * EXW + 16 * NDB) * 64 + lane];
        Mx = fmaxf(Mx, mw[w]);
    }
    const float a0 = m == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m - Mx);
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[i][rr] *= a0;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const float aw = mw[w] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(mw[w] - Mx);
        const float* const e = ex + w * EXW * 64 + lane;
        const float lw = e[(16 * NDB + 1) * 64];
        L = w == 0 ? __builtin_fmaf(L, a0, aw * lw) : __builtin_fmaf(aw, lw, L);  // (wave 1's product is the one that is rounded)
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[i][rr] = __builtin_fmaf(aw, e[(16 * i + rr) * 64], acc[i][rr]);
    }
    m = Mx;
}

// one row of a split-KV part: the normalised partial O f (fp32) at row prow of the parts, and (m, l) behind the rows_parts = nsplit x
// rows partial rows; a row without keys writes m = -inf, l = 0
template <int DP>
__device__ __forceinline__ void paged_store_part(float* part, int64_t rows_parts, int64_t prow, const f32x16 (&acc)[DP / 32], float f,
                                                 float m, float L, int hi) {
    float* const po = part + prow * DP;
#pragma unroll
    for (int i = 0; i < DP / 32; ++i)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
            *(f32x4*)(po + 32 * i + 8 * gg + 4 * hi) =
                f32x4{acc[i][4 * gg] * f, acc[i][4 * gg + 1] * f, acc[i][4 * gg + 2] * f, acc[i][4 * gg + 3] * f};
    if (hi == 0) {
        typedef float F2 __attribute__((ext_vector_type(2)));
        *(F2*)(part + rows_parts * DP + prow * 2) = F2{L > 0.0f ? m : -INFINITY, L};
    }
}

// one row of the final output: O f as fp32 or OUT at element orow of out, and its LSE at lse[lse_at] when lse is given
template <int DP, typename OUT>
__device__ __forceinline__ void paged_store_out(void* out, int64_t orow, float* lse, int64_t lse_at, const f32x16 (&acc)[DP / 32], float f,
                                                float m, float L, int hi) {
#pragma unroll
    for (int i = 0; i < DP / 32; ++i)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const int64_t at = orow + 32 * i + 8 * gg + 4 * hi;
            const f32x4 val = {acc[i][4 * gg] * f, acc[i][4 * gg + 1] * f, acc[i][4 * gg + 2] * f, acc[i][4 * gg + 3] * f};
            if constexpr (std::is_same<OUT, float>::value) {
                *(f32x4*)((float*)out + at) = val;
            } else {
                typedef OUT O4 __attribute__((ext_vector_type(4)));
                *(O4*)((OUT*)out + at) = O4{(OUT)val[0], (OUT)val[1], (OUT)val[2], (OUT)val[3]};
            }
        }
    if (hi == 0 && lse) lse[lse_at] = L > 0.0f ? (m + __builtin_log2f(L)) * UMFA_LN2 : -INFINITY;
}

// row r (query token qi, head h) of item `it` (fa_paged_item.h), scaled by f: a split-KV part's row when OUT is void, else the final row
template <int DP, typename OUT, typename ITEM>
__device__ __forceinline__ void paged_store_row(const PagedParams& p, const ITEM& it, uint32_t r, uint32_t qi, uint32_t h,
                                                const f32x16 (&acc)[DP / 32], float f, float m, float L, int hi) {
    if constexpr (std::is_same<OUT, void>::value) {
        const int64_t rows_all = it.part_rows();
        paged_store_part<DP>(p.part, (int64_t)p.nsplit * rows_all, (int64_t)it.part * rows_all + it.part_row(r), acc, f, m, L, hi);
    } else {
        paged_store_out<DP, OUT>(p.out, it.o_row(qi, h) * DP, p.lse, it.lse_at(qi, h), acc, f, m, L, hi);
    }
}

}  // namespace

}  // namespace umfa
