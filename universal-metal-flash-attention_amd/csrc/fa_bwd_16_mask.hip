// fa_bwd_16_mask.hip -- bf16 / fp16 MFMA backward with an attention mask or a sliding window, head_dim 64 / 128 / 256.
//
// The products, operand orientations and LDS images of fa_bwd_16.hip (bwd16_dq, and bwd16_dkdv in the form its head_dim 64 / 256
// instantiations use), with three tile classes per wave and 32 x 32 block:
//   skip   every score masked: no MFMA, no exponential.  A tile no wave of the workgroup needs is left out of the LDS-DMA staging
//          sequence altogether (the prefetch targets the next tile with work).
//   open   every score attends with a zero term: the unmasked body (plus the end-of-range / causal test where the block crosses them).
//   mixed  P = exp2(c S + term - L2) with term = mask_term (fa_common.h) read per score, or window_term.
// Tensor masks take their classes from mask_flags_kernel (fa_aux.hip: one byte per mask batch, mask head, 32-row block, 64-key tile;
// BwdParams::mask_flags); windows need no tensor and no pre-pass: the workgroup's tile range and every block's class are arithmetic,
// so the cost follows the band.  A row whose forward LSE is -inf (nothing visible) gets P = 0: its dQ row is 0 and nothing reaches
// dK / dV.  No atomics (bitwise repeatable).
//   dQ    lane <-> query, registers <-> keys: four runs of 4 contiguous keys, read with one vector load each where the mask's key
//         stride is 1 and the run is aligned, else per score.
//   dK dV lane <-> key, registers <-> queries: the 32 lanes of a half-wave read 32 consecutive keys of one row per load (per-score
//         loads, coalesced across the lanes when the key stride is 1), issued ahead of the S / dP products of the block.
#include "fa_bwd_16_common.h"
#include "fa_fwd_16_kernel.h"  // Mma16<T>, xcd_remap
#include "kernels.h"

namespace umfa {

namespace {

constexpr int MKT = 1;           // tensor mask (bool / fp32 / fp16 / bf16: p.mask_kind)
constexpr int MKW = MK_WINDOW;   // sliding window

enum : int { TC_SKIP = 0, TC_OPEN = 1, TC_MIXED = 2 };

// class of rows [r0, r0 + 32) x keys [k0, k0 + 32) of slab bh (r0 a multiple of 32, k0 of 32; both wave-uniform)
template <int MK>
__device__ __forceinline__ int block_class(const BwdParams& p, uint32_t bh, uint32_t r0, uint32_t k0) {
    if (r0 >= p.Sq || k0 >= p.Skv) return TC_SKIP;
    if constexpr (MK == MKW) {
        // key attends to row iff row - left <= key <= row + right
        const int64_t rlo = r0, rhi = (int64_t)r0 + 31, klo = k0, khi = (int64_t)k0 + 31;
        const int64_t L = p.win_left, R = p.win_right;
        if (khi < rlo - L || klo > rhi + R) return TC_SKIP;
        if (klo >= rhi - L && khi <= rlo + R) return TC_OPEN;
        return TC_MIXED;
    } else {
        if (!p.mask_flags) return TC_MIXED;
        const uint32_t b = bh / p.H, h = bh % p.H;
        const uint8_t f = p.mask_flags[((uint64_t)b * p.mf_bs + (uint64_t)h * p.mf_hs) * ((uint64_t)p.mf_nrb * p.mf_ntiles) +
                                       (uint64_t)(r0 / 32) * p.mf_ntiles + k0 / 64];
        return f == 1 ? TC_SKIP : f == 2 ? TC_OPEN : TC_MIXED;
    }
}

// terms of four consecutive keys at element idx of a key-contiguous mask (idx aligned to four elements), as mask_term gives them
__device__ __forceinline__ f32x4 mask_terms4(const void* mask, int64_t idx, int kind) {
    f32x4 t;
    if (kind == MK_BOOL) {
        const uint32_t w = *(const uint32_t*)((const uint8_t*)mask + idx);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = ((w >> (8 * e)) & 0xffu) ? 0.0f : -INFINITY;
    } else if (kind == MK_F32) {
        const f32x4 v = *(const f32x4*)((const float*)mask + idx);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = v[e] * UMFA_LOG2E;
    } else if (kind == MK_F16) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4 v = *(const h4*)((const _Float16*)mask + idx);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = (float)v[e] * UMFA_LOG2E;
    } else {
        typedef uint16_t u4 __attribute__((ext_vector_type(4)));
        const u4 v = *(const u4*)((const uint16_t*)mask + idx);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = bf16_bits_to_float(v[e]) * UMFA_LOG2E;
    }
    return t;
}

__device__ __forceinline__ int mask_elem_bytes(int kind) { return kind == MK_BOOL ? 1 : kind == MK_F32 ? 4 : 2; }

}  // namespace

// ------------------------------------------------------------------------------------------------ dQ
// bwd16_dq (fa_bwd_16.hip) with the tile classes: workgroup = 4 waves x 32 query rows, 32-key tiles of K and V through LDS (LDS-DMA,
// double-buffered; buffer parity follows the staged tiles, not the tile index, since skipped tiles leave the sequence).
template <typename T, bool CAUSAL, int DP, int MK>
__global__ __launch_bounds__(256, DP == 256 ? 1 : 2) void bwd16_dq_masked_kernel(BwdParams p) {
    BWD16_GEO(DP);
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t nqb = (p.Sq + 127) / 128;
    const uint32_t vid = xcd_remap(blockIdx.x, nqb * p.B * p.H);
    uint32_t bh = vid / nqb;
    uint32_t qb = vid % nqb;
    if (CAUSAL) qb = nqb - 1 - causal_rank(vid, nqb, bh, DP != 256);
    const uint32_t q_row = qb * 128 + wave * 32 + ql;
    const bool qok = q_row < p.Sq;
    const T* qp = (const T*)p.q + (int64_t)bh * p.Sq * DP;
    const T* dop = (const T*)p.dout + (int64_t)bh * p.Sq * DP;
    const T* kp = (const T*)p.k + (int64_t)bh * p.Skv * DP;
    const T* vp = (const T*)p.v + (int64_t)bh * p.Skv * DP;

    V8 qf[NKS], dof[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (qok) {
            qf[ks] = *(const V8*)(qp + (int64_t)q_row * DP + 16 * ks + 8 * hi);
            dof[ks] = *(const V8*)(dop + (int64_t)q_row * DP + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { qf[ks][j] = (T)0.0f; dof[ks][j] = (T)0.0f; }
        }
    }
    const float c = p.scale * UMFA_LOG2E;
    float L2 = qok ? p.lse[(int64_t)bh * p.Sq + q_row] * UMFA_LOG2E : INFINITY;  // +inf -> P = 0
    if (L2 == -INFINITY) L2 = INFINITY;  // nothing visible in this row (forward LSE -inf): P = 0, not exp2(+inf)
    float delta = 0.0f;  // D[q] = rowsum(dO o O), as in bwd16_dq
    if (qok) {
        const int64_t orow = ((int64_t)bh * p.Sq + q_row) * DP;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int64_t at = orow + 16 * ks + 8 * hi;
            if (p.o_in_type) {
                const V8 ov = *(const V8*)((const T*)p.o + at);
#pragma unroll
                for (int j = 0; j < 8; ++j) delta = __builtin_fmaf((float)dof[ks][j], (float)ov[j], delta);
            } else {
                const f32x4 o0 = *(const f32x4*)(p.o + at), o1 = *(const f32x4*)(p.o + at + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    delta = __builtin_fmaf((float)dof[ks][j], o0[j], delta);
                    delta = __builtin_fmaf((float)dof[ks][4 + j], o1[j], delta);
                }
            }
        }
    }
    delta += __shfl_xor(delta, 32, 64);
    if (qok && hi == 0) {
        const int64_t ri = (int64_t)bh * p.Sq + q_row;
        p.dvec[ri] = delta;
        p.rowc[ri] = -L2;  // row constants of bwd16_dkdv_masked (-inf for a row with nothing visible)
        p.rowc[(int64_t)p.B * p.H * p.Sq + ri] = -delta;
    }

    const i32x4 k_srd = make_srd(kp, p.Skv * (uint32_t)ROW_B), v_srd = make_srd(vp, p.Skv * (uint32_t)ROW_B);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
#pragma unroll
    for (int i = 0; i < 4 * TILE_BYTES / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();

    // the workgroup's key tiles: causal and window bounds are arithmetic
    uint32_t t_lo = 0, t_hi = (p.Skv + 31) / 32;
    if (CAUSAL) {
        const uint32_t lim = (qb * 128 + 128 + 31) / 32;
        t_hi = t_hi < lim ? t_hi : lim;
    }
    if constexpr (MK == MKW) {
        const int64_t klo = (int64_t)qb * 128 - p.win_left, khi = (int64_t)qb * 128 + 127 + p.win_right;
        t_lo = klo > 0 ? (uint32_t)(klo / 32) : 0u;
        const int64_t lim = khi / 32 + 1;
        t_hi = (int64_t)t_hi < lim ? t_hi : (uint32_t)lim;
    }
    const uint32_t q0 = qb * 128;
    auto wave_class = [&](uint32_t w, uint32_t t) -> int {
        const uint32_t r0 = q0 + 32 * w, k0 = t * 32;
        if (CAUSAL && k0 > r0 + 31) return TC_SKIP;
        return block_class<MK>(p, bh, r0, k0);
    };
    auto next_tile = [&](uint32_t t) -> uint32_t {  // first tile >= t some wave of the workgroup has work in
        for (; t < t_hi; ++t)
            if (wave_class(0, t) != TC_SKIP || wave_class(1, t) != TC_SKIP || wave_class(2, t) != TC_SKIP || wave_class(3, t) != TC_SKIP) break;
        return __builtin_amdgcn_readfirstlane(t);
    };

    f32x16 acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;
    auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
        dma_rows<TILE_PIECES, DP>(k_srd, lds0 + par * TILE_BYTES, t * 32, uw, lane);
        dma_rows<TILE_PIECES, DP>(v_srd, lds0 + 2 * TILE_BYTES + par * TILE_BYTES, t * 32, uw, lane);
    };
    // this lane's mask row (tensor masks)
    const int64_t mrow = (int64_t)(bh / p.H) * p.ms[0] + (int64_t)(bh % p.H) * p.ms[1] + (int64_t)q_row * p.ms[2];
    const int mes = mask_elem_bytes(p.mask_kind);
    const bool mvec = p.ms[3] == 1;

    // row fragments in flight ahead of their MFMAs: one k-step fewer than bwd16_dq where the mask terms of a tile are held in registers
    // at head_dim 128 (two workgroups per CU, 256 registers: at PD the causal instantiations spilled)
    constexpr int PDM = (MK == MKT && DP == 128) ? PD - 2 : PD;
    // ONE body for every class (as compile-time variants, three inlined copies in the loop cost spills of the dQ accumulators):
    // `term` and `edge` are wave-uniform -- the mask reads are skipped for open tiles, the per-key test costs a select per score
    auto tile_body = [&](uint32_t t, int par, bool term, bool edge) __attribute__((always_inline)) {
        const char* Kt = smem + par * TILE_BYTES;
        const char* Vt = smem + 2 * TILE_BYTES + par * TILE_BYTES;
        const uint32_t key_base = t * 32;
        f32x4 tm[4] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
        if (term) {  // issued ahead of the products: their latency runs under the S / dP MFMAs
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t k0 = key_base + 8 * g + 4 * hi;  // registers 4g .. 4g+3: keys k0 .. k0+3
                if constexpr (MK != MKW) {  // (window terms are arithmetic: formed in the softmax loop below, no registers held)
                    const int64_t at = mrow + k0;
                    if (qok && mvec && k0 + 3 < p.Skv && (((uintptr_t)p.mask + at * mes) & (4 * mes - 1)) == 0) {
                        tm[g] = mask_terms4(p.mask, at, p.mask_kind);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            tm[g][e] = (qok && k0 + e < p.Skv) ? mask_term(p.mask, mrow + (int64_t)(k0 + e) * p.ms[3], p.mask_kind) : 0.0f;
                    }
                }
            }
        }
        f32x16 s, dp;
        V8 ak[NKS], av[NKS];
#pragma unroll
        for (int ks = 0; ks < PDM; ++ks) {
            ak[ks] = *(const V8*)(Kt + d_off<DP>(ql, 2 * ks + hi));
            av[ks] = *(const V8*)(Vt + d_off<DP>(ql, 2 * ks + hi));
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * PDM, 0);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (ks + PDM < NKS) {
                ak[ks + PDM] = *(const V8*)(Kt + d_off<DP>(ql, 2 * (ks + PDM) + hi));
                av[ks + PDM] = *(const V8*)(Vt + d_off<DP>(ql, 2 * (ks + PDM) + hi));
            }
            s = M::mma(ak[ks], qf[ks], ks ? s : f32x16{});
            dp = M::mma(av[ks], dof[ks], ks ? dp : f32x16{});
            if (ks + PDM < NKS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        }
        V8 ds[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t key = key_base + acc_row(r, hi);
            float x = __builtin_fmaf(s[r], c, -L2);
            if constexpr (MK == MKW) x += term ? window_term(q_row, key, p.win_left, p.win_right) : 0.0f;
            else x += tm[r >> 2][r & 3];
            float pr = __builtin_amdgcn_exp2f(x);
            if (edge && (key >= p.Skv || (CAUSAL && key > q_row))) pr = 0.0f;
            ds[r >> 3][r & 7] = (T)(pr * (dp[r] - delta));
        }
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[i] = M::mma(tr_frag<M, DP>(Kt, i, s2, hi, tr_qq, tr_pp, tr_g1), ds[s2], acc[i]);
    };

    const uint32_t wq0 = __builtin_amdgcn_readfirstlane(q0 + (uint32_t)uw * 32);
    uint32_t t = next_tile(t_lo);
    int par = 0;
    if (t < t_hi) stage(t, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    while (t < t_hi) {
        const uint32_t tn = next_tile(t + 1);
        if (tn < t_hi) stage(tn, par ^ 1);  // other buffer: its last readers passed the previous barrier
        const int cls = wave_class((uint32_t)uw, t);
        if (cls != TC_SKIP) tile_body(t, par, cls == TC_MIXED, t * 32 + 31 >= p.Skv || (CAUSAL && t * 32 + 31 > wq0));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        t = tn;
        par ^= 1;
    }
    if (qok) {
        const int64_t orow = ((int64_t)bh * p.Sq + q_row) * DP;
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 val = {acc[i][4 * g] * p.scale, acc[i][4 * g + 1] * p.scale, acc[i][4 * g + 2] * p.scale, acc[i][4 * g + 3] * p.scale};
                store_grad4<T>(p.dq, orow + 32 * i + 8 * g + 4 * hi, val, p.grad_in_type != 0);
            }
    }
}

// ------------------------------------------------------------------------------------------------ dK, dV
// bwd16_dkdv's structure in the form of its head_dim 64 / 256 instantiations (hipcc's own order, no pinned pipeline): workgroup = 4 waves
// x 32 keys, K / V fragments in registers, 64-row tiles of Q and dO through LDS (two 32-row sub-tiles, each classed per wave), row
// constants (-LSE log2 e, -D) from the scratch bwd16_dq_masked wrote.  head_dim 256: two passes of 4 d-blocks each.
template <typename T, bool CAUSAL, int DP, int MK>
__global__ __launch_bounds__(256, DP == 64 ? 2 : 1) void bwd16_dkdv_masked_kernel(BwdParams p) {
    BWD16_GEO(DP);
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int QT = 0, DOT = QT + 4 * TILE_BYTES, VEC = DOT + 4 * TILE_BYTES;  // [Q 2 x 64 rows][dO 2 x 64 rows][L2 2x64][D 2x64]
    constexpr int QROWS = 64, QTILE_B = QROWS * ROW_B;
    const int tid = threadIdx.x, lane = tid & 63, kl = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t nkb = (p.Skv + 127) / 128;
    const uint32_t n_items = nkb * p.B * p.H;
    const uint32_t vid = xcd_remap(blockIdx.x, n_items);
    uint32_t bh = vid / nkb, kb = vid % nkb;
    if (CAUSAL) kb = causal_rank(vid, nkb, bh, DP == 64);
    const uint32_t key = kb * 128 + wave * 32 + kl;
    const uint32_t wave_k0 = __builtin_amdgcn_readfirstlane(kb * 128 + (uint32_t)uw * 32);
    const bool kok = key < p.Skv;
    const T* qp = (const T*)p.q + (int64_t)bh * p.Sq * DP;
    const T* dop = (const T*)p.dout + (int64_t)bh * p.Sq * DP;
    const T* kp = (const T*)p.k + (int64_t)bh * p.Skv * DP;
    const T* vp = (const T*)p.v + (int64_t)bh * p.Skv * DP;
    const i32x4 q_srd = make_srd(qp, p.Sq * (uint32_t)ROW_B), do_srd = make_srd(dop, p.Sq * (uint32_t)ROW_B);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
    float* const vec = (float*)(smem + VEC);
#pragma unroll
    for (int i = 0; i < VEC / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();
    V8 kf[NKS], vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (kok) {
            kf[ks] = *(const V8*)(kp + (int64_t)key * DP + 16 * ks + 8 * hi);
            vf[ks] = *(const V8*)(vp + (int64_t)key * DP + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { kf[ks][j] = (T)0.0f; vf[ks][j] = (T)0.0f; }
        }
    }
    const float c = p.scale * UMFA_LOG2E;
    uint32_t t_lo = CAUSAL ? (kb * 128) / QROWS : 0u, t_hi = (p.Sq + QROWS - 1) / QROWS;
    if constexpr (MK == MKW) {  // rows that see keys [kb 128, kb 128 + 127]: [key - right, key + left]
        const int64_t rlo = (int64_t)kb * 128 - p.win_right, rhi = (int64_t)kb * 128 + 127 + p.win_left;
        const uint32_t lo = rlo > 0 ? (uint32_t)(rlo / QROWS) : 0u;
        t_lo = t_lo > lo ? t_lo : lo;
        const int64_t lim = rhi / QROWS + 1;
        t_hi = (int64_t)t_hi < lim ? t_hi : (uint32_t)lim;
    }
    auto sub_class = [&](uint32_t w, uint32_t t, int u) -> int {
        const uint32_t r0 = t * QROWS + 32 * u, k0 = kb * 128 + 32 * w;
        if (CAUSAL && r0 + 31 < k0) return TC_SKIP;  // every query of the sub-tile precedes these keys
        return block_class<MK>(p, bh, r0, k0);
    };
    auto next_tile = [&](uint32_t t) -> uint32_t {
        for (; t < t_hi; ++t) {
            bool any = false;
#pragma unroll
            for (int w = 0; w < 4; ++w) any = any || sub_class(w, t, 0) != TC_SKIP || sub_class(w, t, 1) != TC_SKIP;
            if (any) break;
        }
        return __builtin_amdgcn_readfirstlane(t);
    };
    auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
        dma_rows<2 * TILE_PIECES, DP>(q_srd, lds0 + QT + par * QTILE_B, t * QROWS, uw, lane);
        dma_rows<2 * TILE_PIECES, DP>(do_srd, lds0 + DOT + par * QTILE_B, t * QROWS, uw, lane);
    };
    // row constants of a tile by LDS-DMA (wave 0: -LSE log2 e, wave 1: -D; rows past Sq read 0 -- their Q / dO rows are 0 too)
    const i32x4 lse_srd = make_srd(p.rowc + (int64_t)bh * p.Sq, p.Sq * 4u), dv_srd = make_srd(p.rowc + ((int64_t)p.B * p.H + bh) * p.Sq, p.Sq * 4u);
    auto stage_consts = [&](uint32_t t, int par) __attribute__((always_inline)) {
        const int voff = (int)(t * QROWS + (uint32_t)lane) * 4;
        if (uw == 0)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds"
                         ::"s"(lds0 + VEC + par * QROWS * 4), "v"(voff), "s"(lse_srd) : "memory");
        else if (uw == 1)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds"
                         ::"s"(lds0 + VEC + 2 * QROWS * 4 + par * QROWS * 4), "v"(voff), "s"(dv_srd) : "memory");
    };
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;
    const int64_t mcol = (int64_t)(bh / p.H) * p.ms[0] + (int64_t)(bh % p.H) * p.ms[1] + (int64_t)key * p.ms[3];

#pragma unroll 1
    for (int hpass = 0; hpass < NH; ++hpass) {
        f32x16 dk[NDBH], dv[NDBH];
#pragma unroll
        for (int i = 0; i < NDBH; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[i][r] = 0.0f; dv[i][r] = 0.0f; }
        // one 32-row sub-tile u of the tile in buffer `par`
        // ONE body for every class (see bwd16_dq_masked_kernel); `term`, `edge` wave-uniform
        auto sub_body = [&](uint32_t t, int par, int u, bool term, bool edge) __attribute__((always_inline)) {
            const char* Qt = smem + QT + par * QTILE_B + u * TILE_BYTES;
            const char* dOt = smem + DOT + par * QTILE_B + u * TILE_BYTES;
            const float* L2v = vec + par * QROWS + 32 * u;
            const float* Dv = vec + 2 * QROWS + par * QROWS + 32 * u;
            const uint32_t qb0 = t * QROWS + 32 * u;
            float tm[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) tm[r] = 0.0f;
            if (term) {  // registers 4g .. 4g+3: queries qb0 + 8g + 4hi + 0..3
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t row = qb0 + 8 * (r >> 2) + 4 * hi + (r & 3);
                    if constexpr (MK == MKW) tm[r] = window_term(row, key, p.win_left, p.win_right);
                    else tm[r] = (kok && row < p.Sq) ? mask_term(p.mask, mcol + (int64_t)row * p.ms[2], p.mask_kind) : 0.0f;
                }
            }
            f32x16 s, dp;
            V8 aq[NKS], ado[NKS];
#pragma unroll
            for (int j = 0; j < PD; ++j) {
                aq[j] = *(const V8*)(Qt + d_off<DP>(kl, 2 * j + hi));
                ado[j] = *(const V8*)(dOt + d_off<DP>(kl, 2 * j + hi));
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * PD, 0);
#pragma unroll
            for (int j = 0; j < NKS; ++j) {
                if (j + PD < NKS) {
                    aq[j + PD] = *(const V8*)(Qt + d_off<DP>(kl, 2 * (j + PD) + hi));
                    ado[j + PD] = *(const V8*)(dOt + d_off<DP>(kl, 2 * (j + PD) + hi));
                }
                s = M::mma(aq[j], kf[j], j ? s : f32x16{});
                dp = M::mma(ado[j], vf[j], j ? dp : f32x16{});
                if (j + PD < NKS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            }
            V8 pb[2], sb[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l2 = *(const f32x4*)(L2v + 8 * g + 4 * hi);  // -LSE log2(e)
                const f32x4 dl = *(const f32x4*)(Dv + 8 * g + 4 * hi);   // -D
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, l2[e]) + tm[r]);
                    if (CAUSAL && edge && key > qb0 + 8 * g + 4 * hi + e) pr = 0.0f;
                    pb[r >> 3][r & 7] = (T)pr;
                    sb[r >> 3][r & 7] = (T)(pr * (dp[r] + dl[e]));
                }
            }
#pragma unroll
            for (int i = 0; i < NDBH; ++i)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    dv[i] = M::mma(tr_frag<M, DP>(dOt, i + hpass * NDBH, s2, hi, tr_qq, tr_pp, tr_g1), pb[s2], dv[i]);
                    dk[i] = M::mma(tr_frag<M, DP>(Qt, i + hpass * NDBH, s2, hi, tr_qq, tr_pp, tr_g1), sb[s2], dk[i]);
                }
        };
        uint32_t t = next_tile(t_lo);
        int par = 0;
        if (t < t_hi) { stage(t, 0); stage_consts(t, 0); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        while (t < t_hi) {
            const uint32_t tn = next_tile(t + 1);
            if (tn < t_hi) { stage(tn, par ^ 1); stage_consts(tn, par ^ 1); }
#pragma unroll 1
            for (int u = 0; u < 2; ++u) {
                const int cls = sub_class((uint32_t)uw, t, u);
                // (edge: the sub-tile straddles the causal diagonal of this wave's keys)
                if (cls != TC_SKIP) sub_body(t, par, u, cls == TC_MIXED, t * QROWS + 32 * u < wave_k0 + 31);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            t = tn;
            par ^= 1;
        }
        if (kok) {
            const int64_t krow = ((int64_t)bh * p.Skv + key) * DP;
#pragma unroll
            for (int i = 0; i < NDBH; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d0 = 32 * (i + hpass * NDBH) + 8 * g + 4 * hi;
                    f32x4 kv = {dk[i][4 * g] * p.scale, dk[i][4 * g + 1] * p.scale, dk[i][4 * g + 2] * p.scale, dk[i][4 * g + 3] * p.scale};
                    f32x4 vv = {dv[i][4 * g], dv[i][4 * g + 1], dv[i][4 * g + 2], dv[i][4 * g + 3]};
                    store_grad4<T>(p.dk, krow + d0, kv, p.grad_in_type != 0);
                    store_grad4<T>(p.dv, krow + d0, vv, p.grad_in_type != 0);
                }
        }
    }  // hpass
}

bool bwd_16_mask_supported(const BwdParams& p) {
    if (p.mask_kind == MK_NONE || (p.mask_kind != MK_WINDOW && !p.mask)) return false;
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if (p.dout_prec != p.in_prec || (p.D != 256 && p.D != 128 && p.D != 64)) return false;
    if ((p.Hkv && p.Hkv != p.H) || p.units || p.ds || p.phases || p.dkdv_fp32) return false;  // (dense K / V heads, one call, no scaled operands)
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    if (!al16(p.q) || !al16(p.k) || !al16(p.v) || !al16(p.dout) || !al16(p.dq) || !al16(p.dk) || !al16(p.dv)) return false;
    return (uint64_t)p.Sq * 2 * p.D < (1ull << 31) && (uint64_t)p.Skv * 2 * p.D < (1ull << 31);
}

template <typename T, bool CAUSAL, int DP, int MK>
static hipError_t launch_bwd16_masked_t(const BwdParams& p, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds_dq = 4 * TILE_BYTES, lds_kv = 8 * TILE_BYTES + 1024;
    if (hipError_t e = ensure_dynamic_lds((const void*)bwd16_dq_masked_kernel<T, CAUSAL, DP, MK>, lds_dq); e != hipSuccess) return e;
    if (hipError_t e = ensure_dynamic_lds((const void*)bwd16_dkdv_masked_kernel<T, CAUSAL, DP, MK>, lds_kv); e != hipSuccess) return e;
    const uint32_t nqb = (p.Sq + 127) / 128, nkb = (p.Skv + 127) / 128;
    hipLaunchKernelGGL((bwd16_dq_masked_kernel<T, CAUSAL, DP, MK>), dim3(nqb * p.B * p.H), dim3(256), lds_dq, stream, p);
    hipLaunchKernelGGL((bwd16_dkdv_masked_kernel<T, CAUSAL, DP, MK>), dim3(nkb * p.B * p.H), dim3(256), lds_kv, stream, p);
    return hipGetLastError();
}

template <typename T, int DP>
static hipError_t launch_bwd16_masked_d(const BwdParams& p, hipStream_t stream) {
    const bool w = p.mask_kind == MK_WINDOW;
    if (p.causal) return w ? launch_bwd16_masked_t<T, true, DP, MKW>(p, stream) : launch_bwd16_masked_t<T, true, DP, MKT>(p, stream);
    return w ? launch_bwd16_masked_t<T, false, DP, MKW>(p, stream) : launch_bwd16_masked_t<T, false, DP, MKT>(p, stream);
}

hipError_t launch_bwd_16_masked(const BwdParams& p, hipStream_t stream, const char** name) {
    if (!bwd_16_mask_supported(p)) return hipErrorNotSupported;
    static const char* const names[2][3][2] = {
        {{"fa_bwd16<fp16,64,mask>", "fa_bwd16<fp16,64,window>"}, {"fa_bwd16<fp16,128,mask>", "fa_bwd16<fp16,128,window>"},
         {"fa_bwd16<fp16,256,mask>", "fa_bwd16<fp16,256,window>"}},
        {{"fa_bwd16<bf16,64,mask>", "fa_bwd16<bf16,64,window>"}, {"fa_bwd16<bf16,128,mask>", "fa_bwd16<bf16,128,window>"},
         {"fa_bwd16<bf16,256,mask>", "fa_bwd16<bf16,256,window>"}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 64 ? 0 : p.D == 128 ? 1 : 2][p.mask_kind == MK_WINDOW];
    if (p.D == 64) return bf ? launch_bwd16_masked_d<__bf16, 64>(p, stream) : launch_bwd16_masked_d<_Float16, 64>(p, stream);
    if (p.D == 128) return bf ? launch_bwd16_masked_d<__bf16, 128>(p, stream) : launch_bwd16_masked_d<_Float16, 128>(p, stream);
    return bf ? launch_bwd16_masked_d<__bf16, 256>(p, stream) : launch_bwd16_masked_d<_Float16, 256>(p, stream);
}

}  // namespace umfa
