// fa_bwd_16_drop.hip -- bf16 / fp16 MFMA backward with attention dropout, head_dim 64 / 128, causal or not, no mask.
//
// The structure of the masked backward (fa_bwd_16_mask.hip): P recomputed from the forward's (undropped) LSE per tile, no atomics
// (bitwise repeatable), the causal tile classes (a block entirely above the diagonal is skipped, one crossing it masks per score).
// The keep bits are fa_dropout.h's, the forward's bit for bit; with s = 1 / (1 - p) as realised (DropBwdParams::dscale):
//   dV_j  = s sum_i keep_ij P_ij dO_i          keep * P rounded once to the operand type, s in the fp32 epilogue
//   dP_ij = s keep_ij (dO_i . V_j)             in fp32, before dS is formed
//   D_i   = dO_i . O_i                         (O is the dropped output the forward returned: still exact)
//   dS    = P o (dP - D),  dQ = scale dS K,  dK = scale dS^T Q
//   dQ    lane <-> query, registers <-> keys in runs of 4: one Philox call per run, as in the forward.
//   dK dV lane <-> key, registers <-> 4 consecutive queries per run.  The four lanes of a quad hold keys 4g .. 4g+3: lane m computes the
//         call of row m of the run (all four keys' bits), and two xor-shuffles inside the quad hand every lane its own key's bit of all
//         four rows (a 4 x 4 bit transpose) -- one call per 4 scores again.
#include "fa_bwd_16_common.h"
#include "fa_dropout.h"
#include "fa_fwd_16_kernel.h"  // Mma16<T>, xcd_remap
#include "kernels.h"

namespace umfa {

// ------------------------------------------------------------------------------------------------ dQ
template <typename T, bool CAUSAL, int DP>
__global__ __launch_bounds__(256, 2) void bwd16_dq_drop_kernel(DropBwdParams p) {
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
    if (CAUSAL) qb = nqb - 1 - causal_rank(vid, nqb, bh, true);
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
    if (L2 == -INFINITY) L2 = INFINITY;
    float delta = 0.0f;  // D[q] = rowsum(dO o O)
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
        p.rowc[ri] = -L2;  // row constants of bwd16_dkdv_drop
        p.rowc[(int64_t)p.B * p.H * p.Sq + ri] = -delta;
    }
    const uint64_t seed = (uint64_t)p.rng[0], offset = (uint64_t)p.rng[1];
    const uint32_t thresh = p.thresh;
    const float sd = p.dscale;

    const i32x4 k_srd = make_srd(kp, p.Skv * (uint32_t)ROW_B), v_srd = make_srd(vp, p.Skv * (uint32_t)ROW_B);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
#pragma unroll
    for (int i = 0; i < 4 * TILE_BYTES / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();

    uint32_t t_hi = (p.Skv + 31) / 32;
    if (CAUSAL) {
        const uint32_t lim = (qb * 128 + 128 + 31) / 32;
        t_hi = t_hi < lim ? t_hi : lim;
    }
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
    auto tile_body = [&](uint32_t t, int par, bool edge) __attribute__((always_inline)) {
        const char* Kt = smem + par * TILE_BYTES;
        const char* Vt = smem + 2 * TILE_BYTES + par * TILE_BYTES;
        const uint32_t key_base = t * 32;
        f32x16 s, dp;
        V8 ak[NKS], av[NKS];
#pragma unroll
        for (int ks = 0; ks < PD; ++ks) {
            ak[ks] = *(const V8*)(Kt + d_off<DP>(ql, 2 * ks + hi));
            av[ks] = *(const V8*)(Vt + d_off<DP>(ql, 2 * ks + hi));
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * PD, 0);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            if (ks + PD < NKS) {
                ak[ks + PD] = *(const V8*)(Kt + d_off<DP>(ql, 2 * (ks + PD) + hi));
                av[ks + PD] = *(const V8*)(Vt + d_off<DP>(ql, 2 * (ks + PD) + hi));
            }
            s = M::mma(ak[ks], qf[ks], ks ? s : f32x16{});
            dp = M::mma(av[ks], dof[ks], ks ? dp : f32x16{});
            if (ks + PD < NKS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        }
        uint32_t keep[4];  // registers 4g .. 4g+3: keys key_base + 8g + 4hi + 0..3
#pragma unroll
        for (int g = 0; g < 4; ++g) keep[g] = drop_keep4((key_base + 8 * g + 4 * hi) >> 2, q_row, bh, seed, offset, thresh);
        V8 ds[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t key = key_base + acc_row(r, hi);
            float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -L2));
            if (edge && (key >= p.Skv || (CAUSAL && key > q_row))) pr = 0.0f;
            const float dpk = ((keep[r >> 2] >> (r & 3)) & 1u) ? dp[r] * sd : 0.0f;
            ds[r >> 3][r & 7] = (T)(pr * (dpk - delta));
        }
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[i] = M::mma(tr_frag<M, DP>(Kt, i, s2, hi, tr_qq, tr_pp, tr_g1), ds[s2], acc[i]);
    };

    const uint32_t wq0 = __builtin_amdgcn_readfirstlane(qb * 128 + (uint32_t)uw * 32);
    if (t_hi > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int par = 0;
    for (uint32_t t = 0; t < t_hi; ++t) {
        if (t + 1 < t_hi) stage(t + 1, par ^ 1);
        if (!CAUSAL || t * 32 <= wq0 + 31) tile_body(t, par, t * 32 + 31 >= p.Skv || (CAUSAL && t * 32 + 31 > wq0));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
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
// workgroup = 4 waves x 32 keys, K / V fragments in registers, 64-row tiles of Q and dO through LDS (two 32-row sub-tiles), row
// constants (-LSE log2 e, -D) from the scratch bwd16_dq_drop wrote.
template <typename T, bool CAUSAL, int DP>
__global__ __launch_bounds__(256, DP == 64 ? 2 : 1) void bwd16_dkdv_drop_kernel(DropBwdParams p) {
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
    uint64_t seed = (uint64_t)p.rng[0], offset = (uint64_t)p.rng[1];
    asm volatile("" : "+v"(seed));  // the Philox key in vector registers: held in scalar ones, the head_dim 128 causal form spilled SGPRs
    const uint32_t thresh = p.thresh;
    const float sd = p.dscale;
    const uint32_t jq = key >> 2;
    const int qm = kl & 3;  // this lane's position in its quad: the row of each run whose Philox call it computes
    const uint32_t t_lo = CAUSAL ? (kb * 128) / QROWS : 0u, t_hi = (p.Sq + QROWS - 1) / QROWS;
    auto sub_skip = [&](uint32_t w, uint32_t t, int u) -> bool {
        const uint32_t r0 = t * QROWS + 32 * u, k0 = kb * 128 + 32 * w;
        if (r0 >= p.Sq || k0 >= p.Skv) return true;
        return CAUSAL && r0 + 31 < k0;  // every query of the sub-tile precedes these keys
    };
    auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
        dma_rows<2 * TILE_PIECES, DP>(q_srd, lds0 + QT + par * QTILE_B, t * QROWS, uw, lane);
        dma_rows<2 * TILE_PIECES, DP>(do_srd, lds0 + DOT + par * QTILE_B, t * QROWS, uw, lane);
    };
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

    f32x16 dk[NDB], dv[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[i][r] = 0.0f; dv[i][r] = 0.0f; }
    auto sub_body = [&](uint32_t t, int par, int u, bool edge) __attribute__((always_inline)) {
        const char* Qt = smem + QT + par * QTILE_B + u * TILE_BYTES;
        const char* dOt = smem + DOT + par * QTILE_B + u * TILE_BYTES;
        const float* L2v = vec + par * QROWS + 32 * u;
        const float* Dv = vec + 2 * QROWS + par * QROWS + 32 * u;
        const uint32_t qb0 = t * QROWS + 32 * u;
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
            // rows qb0 + 8g + 4hi + 0..3: this lane computes row qm's call (keys 4 jq .. 4 jq + 3), the quad exchanges the nibbles:
            // bit 4e + m of `w` = keep(row e of the run, key 4 jq + m)
            const uint32_t row0 = qb0 + 8 * g + 4 * hi;
            uint32_t w = drop_keep4(jq, row0 + qm, bh, seed, offset, thresh) << (4 * qm);
            w |= (uint32_t)__shfl_xor((int)w, 1, 64);
            w |= (uint32_t)__shfl_xor((int)w, 2, 64);
            const f32x4 l2 = *(const f32x4*)(L2v + 8 * g + 4 * hi);  // -LSE log2(e)
            const f32x4 dl = *(const f32x4*)(Dv + 8 * g + 4 * hi);   // -D
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, l2[e]));
                if (CAUSAL && edge && key > row0 + e) pr = 0.0f;
                const bool kept = (w >> (4 * e + qm)) & 1u;
                pb[r >> 3][r & 7] = (T)(kept ? pr : 0.0f);
                sb[r >> 3][r & 7] = (T)(pr * ((kept ? dp[r] * sd : 0.0f) + dl[e]));
            }
        }
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                dv[i] = M::mma(tr_frag<M, DP>(dOt, i, s2, hi, tr_qq, tr_pp, tr_g1), pb[s2], dv[i]);
                dk[i] = M::mma(tr_frag<M, DP>(Qt, i, s2, hi, tr_qq, tr_pp, tr_g1), sb[s2], dk[i]);
            }
    };
    if (t_lo < t_hi) { stage(t_lo, 0); stage_consts(t_lo, 0); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int par = 0;
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        if (t + 1 < t_hi) { stage(t + 1, par ^ 1); stage_consts(t + 1, par ^ 1); }
#pragma unroll 1
        for (int u = 0; u < 2; ++u)
            if (!sub_skip((uint32_t)uw, t, u)) sub_body(t, par, u, t * QROWS + 32 * u < wave_k0 + 31);  // (edge: straddles the diagonal)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        par ^= 1;
    }
    if (kok) {
        const int64_t krow = ((int64_t)bh * p.Skv + key) * DP;
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = 32 * i + 8 * g + 4 * hi;
                f32x4 kv = {dk[i][4 * g] * p.scale, dk[i][4 * g + 1] * p.scale, dk[i][4 * g + 2] * p.scale, dk[i][4 * g + 3] * p.scale};
                f32x4 vv = {dv[i][4 * g] * sd, dv[i][4 * g + 1] * sd, dv[i][4 * g + 2] * sd, dv[i][4 * g + 3] * sd};
                store_grad4<T>(p.dk, krow + d0, kv, p.grad_in_type != 0);
                store_grad4<T>(p.dv, krow + d0, vv, p.grad_in_type != 0);
            }
    }
}

bool bwd_16_dropout_supported(const BwdParams& p) {
    if (p.mask_kind != MK_NONE || p.mask) return false;
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if (p.dout_prec != p.in_prec || (p.D != 128 && p.D != 64)) return false;
    if ((p.Hkv && p.Hkv != p.H) || p.units || p.ds || p.phases || p.dkdv_fp32) return false;
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    if (!al16(p.q) || !al16(p.k) || !al16(p.v) || !al16(p.dout) || !al16(p.dq) || !al16(p.dk) || !al16(p.dv) || !al16(p.o)) return false;
    return (uint64_t)p.Sq * 2 * p.D < (1ull << 31) && (uint64_t)p.Skv * 2 * p.D < (1ull << 31);
}

template <typename T, bool CAUSAL, int DP>
static hipError_t launch_bwd16_drop_t(const DropBwdParams& p, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds_dq = 4 * TILE_BYTES, lds_kv = 8 * TILE_BYTES + 1024;
    if (hipError_t e = ensure_dynamic_lds((const void*)bwd16_dq_drop_kernel<T, CAUSAL, DP>, lds_dq); e != hipSuccess) return e;
    if (hipError_t e = ensure_dynamic_lds((const void*)bwd16_dkdv_drop_kernel<T, CAUSAL, DP>, lds_kv); e != hipSuccess) return e;
    const uint32_t nqb = (p.Sq + 127) / 128, nkb = (p.Skv + 127) / 128;
    hipLaunchKernelGGL((bwd16_dq_drop_kernel<T, CAUSAL, DP>), dim3(nqb * p.B * p.H), dim3(256), lds_dq, stream, p);
    hipLaunchKernelGGL((bwd16_dkdv_drop_kernel<T, CAUSAL, DP>), dim3(nkb * p.B * p.H), dim3(256), lds_kv, stream, p);
    return hipGetLastError();
}

template <typename T, int DP>
static hipError_t launch_bwd16_drop_d(const DropBwdParams& p, hipStream_t stream) {
    return p.causal ? launch_bwd16_drop_t<T, true, DP>(p, stream) : launch_bwd16_drop_t<T, false, DP>(p, stream);
}

// p.rowc: 2 * B * H * Sq floats of scratch (the row constants bwd16_dq_drop leaves for bwd16_dkdv_drop)
hipError_t launch_bwd_16_dropout(const DropBwdParams& p, hipStream_t stream, const char** name) {
    if (!bwd_16_dropout_supported(p) || !p.rng || !p.rowc) return hipErrorInvalidValue;
    static const char* const names[2][2][2] = {
        {{"bwd16_dq_drop+dkdv_drop<fp16,64>", "bwd16_dq_drop+dkdv_drop<fp16,64,causal>"},
         {"bwd16_dq_drop+dkdv_drop<fp16,128>", "bwd16_dq_drop+dkdv_drop<fp16,128,causal>"}},
        {{"bwd16_dq_drop+dkdv_drop<bf16,64>", "bwd16_dq_drop+dkdv_drop<bf16,64,causal>"},
         {"bwd16_dq_drop+dkdv_drop<bf16,128>", "bwd16_dq_drop+dkdv_drop<bf16,128,causal>"}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.causal != 0];
    if (p.D == 64) return bf ? launch_bwd16_drop_d<__bf16, 64>(p, stream) : launch_bwd16_drop_d<_Float16, 64>(p, stream);
    return bf ? launch_bwd16_drop_d<__bf16, 128>(p, stream) : launch_bwd16_drop_d<_Float16, 128>(p, stream);
}

}  // namespace umfa
