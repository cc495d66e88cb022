// fa_bwd_16_varlen_window.hip -- the packed variable-length backward with a sliding window (flash-attention's window_size), bf16 / fp16,
// head_dim 64 / 128, GQA.  Semantics and layout: fa_varlen.h; the forward: fa_fwd_16_varlen_window.hip.
//
// bwd16_dq_varlen_kernel and bwd16_dkdv_varlen_kernel (fa_bwd_16_varlen.hip) with the band of the windowed forward: row i sees keys
// [i + lo_off, i + hi_off], lo_off = off - left, hi_off = off + right (off = L_k - L_q; bounds from VarlenParams).
//   dQ     key tiles of the workgroup's rows as the forward takes them; per wave skip / mask per score / open.
//   dK dV  key block [k0, k0 + 128) is seen by query rows [k0 - hi_off, k0 + 127 - lo_off], clamped to [0, L_q): only those 64-row
//          tiles are staged (the first one is t_lo); per wave and 32-row sub-tile skip / mask per score / open.  Grouped query heads are
//          summed inside the workgroup in head order: no atomics, bitwise repeatable.
#include "fa_varlen.h"
#include "fa_fwd_16_kernel.h"
#include "kernels.h"

namespace umfa {

// ------------------------------------------------------------------------------------------------ dQ
template <typename T, int DP>
__global__ __launch_bounds__(256, 2) void bwd16_dq_varlen_window_kernel(VarlenParams p) {
    BWD16_GEO(DP);
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t nh = p.N * p.H, nqb = gridDim.x / nh;
    const uint32_t qb = nqb - 1 - blockIdx.x / nh, n = (blockIdx.x % nh) / p.H, h = blockIdx.x % p.H;
    uint32_t qs0, Lq, ks0, Lk;
    varlen_range(p.cu_q, n, p.Tq, p.max_q, qs0, Lq);
    varlen_range(p.cu_k, n, p.Tk, p.max_k, ks0, Lk);
    const uint32_t q0 = qb * 128;
    if (q0 >= Lq) return;
    const int off = (int)Lk - (int)Lq;
    const int lo_off = off - p.win_left, hi_off = off + p.win_right;
    const uint32_t hk = h / (p.H / p.Hkv);
    const uint32_t q_row = q0 + wave * 32 + ql;
    const bool qok = q_row < Lq;
    const int64_t tok = (int64_t)qs0 + q_row;
    const T* qp = (const T*)p.q + (int64_t)qs0 * p.qst + (int64_t)h * p.qsh;
    const T* kp = (const T*)p.k + (int64_t)ks0 * p.kst + (int64_t)hk * p.ksh;
    const T* vp = (const T*)p.v + (int64_t)ks0 * p.vst + (int64_t)hk * p.vsh;
    const uint32_t kst_b = (uint32_t)p.kst * 2, vst_b = (uint32_t)p.vst * 2;
    const int64_t orow = (tok * p.H + h) * DP;  // dense [T_q, H, D]: dO, O, dQ

    V8 qf[NKS], dof[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (qok) {
            qf[ks] = *(const V8*)(qp + (int64_t)q_row * p.qst + 16 * ks + 8 * hi);
            dof[ks] = *(const V8*)((const T*)p.dout + orow + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { qf[ks][j] = (T)0.0f; dof[ks][j] = (T)0.0f; }
        }
    }
    const float c = p.scale * UMFA_LOG2E;
    float L2 = qok ? p.lse[(int64_t)h * p.Tq + tok] * UMFA_LOG2E : INFINITY;  // +inf -> P = 0
    if (L2 == -INFINITY) L2 = INFINITY;  // a row that saw no key: P = 0, never exp(+inf)
    float delta = 0.0f;  // D[q] = rowsum(dO o O)
    if (qok) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int64_t at = orow + 16 * ks + 8 * hi;
            if (p.o_in_type) {
                const V8 ov = *(const V8*)((const T*)p.o + at);
#pragma unroll
                for (int j = 0; j < 8; ++j) delta = __builtin_fmaf((float)dof[ks][j], (float)ov[j], delta);
            } else {
                const f32x4 o0 = *(const f32x4*)((const float*)p.o + at), o1 = *(const f32x4*)((const float*)p.o + at + 4);
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
        const int64_t ri = (int64_t)h * p.Tq + tok;
        p.rowc[ri] = -L2;  // row constants of bwd16_dkdv_varlen_window
        p.rowc[(int64_t)p.H * p.Tq + ri] = -delta;
    }

    const i32x4 k_srd = make_srd(kp, varlen_bytes(Lk, kst_b, ROW_B)), v_srd = make_srd(vp, varlen_bytes(Lk, vst_b, ROW_B));
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
#pragma unroll
    for (int i = 0; i < 4 * TILE_BYTES / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();

    // the block's keys, as the forward takes them
    const int last_row = (int)(q0 + 127 < Lq ? q0 + 127 : Lq - 1);
    const int k_first = (int)q0 + lo_off > 0 ? (int)q0 + lo_off : 0;
    const int k_last = last_row + hi_off < (int)Lk - 1 ? last_row + hi_off : (int)Lk - 1;
    const uint32_t t_lo = (uint32_t)k_first / 32, t_hi = k_last >= k_first ? (uint32_t)k_last / 32 + 1 : t_lo;
    f32x16 acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;
    auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
        dma_rows_strided<TILE_PIECES, DP>(k_srd, lds0 + par * TILE_BYTES, t * 32, kst_b, uw, lane);
        dma_rows_strided<TILE_PIECES, DP>(v_srd, lds0 + 2 * TILE_BYTES + par * TILE_BYTES, t * 32, vst_b, uw, lane);
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
        V8 ds[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = (int)(key_base + acc_row(r, hi));
            float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -L2));
            if (edge && (key >= (int)Lk || key < (int)q_row + lo_off || key > (int)q_row + hi_off)) pr = 0.0f;
            ds[r >> 3][r & 7] = (T)(pr * (dp[r] - delta));
        }
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[i] = M::mma(tr_frag<M, DP>(Kt, i, s2, hi, tr_qq, tr_pp, tr_g1), ds[s2], acc[i]);
    };

    const int wq0 = __builtin_amdgcn_readfirstlane((int)q0 + uw * 32);
    if (t_lo < t_hi) stage(t_lo, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int par = 0;
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        if (t + 1 < t_hi) stage(t + 1, par ^ 1);
        const int kb = (int)(t * 32);  // (the forward's skip and edge tests)
        if (wq0 < (int)Lq && kb + 31 >= wq0 + lo_off && kb <= wq0 + 31 + hi_off)
            tile_body(t, par, kb + 31 >= (int)Lk || kb < wq0 + 31 + lo_off || kb + 31 > wq0 + hi_off);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        par ^= 1;
    }
    if (qok) {
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
template <typename T, int DP>
__global__ __launch_bounds__(256, DP == 64 ? 2 : 1) void bwd16_dkdv_varlen_window_kernel(VarlenParams p) {
    BWD16_GEO(DP);
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int QT = 0, DOT = QT + 4 * TILE_BYTES, VEC = DOT + 4 * TILE_BYTES;  // [Q 2 x 64 rows][dO 2 x 64 rows][L2 2x64][D 2x64]
    constexpr int QROWS = 64, QTILE_B = QROWS * ROW_B;
    const int tid = threadIdx.x, lane = tid & 63, kl = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t nh = p.N * p.Hkv;
    const uint32_t kb = blockIdx.x / nh, n = (blockIdx.x % nh) / p.Hkv, hk = blockIdx.x % p.Hkv;
    uint32_t qs0, Lq, ks0, Lk;
    varlen_range(p.cu_q, n, p.Tq, p.max_q, qs0, Lq);
    varlen_range(p.cu_k, n, p.Tk, p.max_k, ks0, Lk);
    const uint32_t k0 = kb * 128;
    if (k0 >= Lk) return;
    const int off = (int)Lk - (int)Lq;
    const int lo_off = off - p.win_left, hi_off = off + p.win_right;  // key j is seen by rows [j - hi_off, j - lo_off]
    const uint32_t G = p.H / p.Hkv;
    const uint32_t key = k0 + wave * 32 + kl;
    const int wave_k0 = __builtin_amdgcn_readfirstlane((int)k0 + uw * 32);
    const bool kok = key < Lk;
    const T* kp = (const T*)p.k + (int64_t)ks0 * p.kst + (int64_t)hk * p.ksh;
    const T* vp = (const T*)p.v + (int64_t)ks0 * p.vst + (int64_t)hk * p.vsh;
    const uint32_t qst_b = (uint32_t)p.qst * 2, dost_b = p.H * (uint32_t)ROW_B;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
    float* const vec = (float*)(smem + VEC);
#pragma unroll
    for (int i = 0; i < VEC / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();
    V8 kf[NKS], vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (kok) {
            kf[ks] = *(const V8*)(kp + (int64_t)key * p.kst + 16 * ks + 8 * hi);
            vf[ks] = *(const V8*)(vp + (int64_t)key * p.vst + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { kf[ks][j] = (T)0.0f; vf[ks][j] = (T)0.0f; }
        }
    }
    float c = p.scale * UMFA_LOG2E;
    uint32_t qst_v = qst_b, dost_v = dost_b;
    // (in vector registers, as in the causal form: the per-score band test's copies)
    int lo_v = lo_off, hi_v = hi_off;
    asm volatile("" : "+v"(c), "+v"(qst_v), "+v"(dost_v), "+v"(lo_v), "+v"(hi_v));
    // the block's query rows: from the one that sees key k0 first to the one that sees its last key last, inside [0, L_q)
    const int last_key = (int)(k0 + 127 < Lk ? k0 + 127 : Lk - 1);
    const int r_first = (int)k0 - hi_off > 0 ? (int)k0 - hi_off : 0;
    const int r_last = last_key - lo_off < (int)Lq - 1 ? last_key - lo_off : (int)Lq - 1;
    const uint32_t t_lo = (uint32_t)r_first / QROWS, t_hi = r_last >= r_first ? (uint32_t)r_last / QROWS + 1 : t_lo;
    auto sub_skip = [&](uint32_t t, int u) -> bool {
        const int r0 = (int)(t * QROWS + 32 * u);
        if (r0 >= (int)Lq || wave_k0 >= (int)Lk) return true;
        // the sub-tile's last row's band ends before the wave's first key, or its first row's band starts after the wave's last key
        return r0 + 31 + hi_off < wave_k0 || r0 + lo_off > wave_k0 + 31;
    };
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;

    f32x16 dk[NDB], dv[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[i][r] = 0.0f; dv[i][r] = 0.0f; }
#pragma unroll 1
    for (uint32_t g = 0; g < G; ++g) {  // the group's query heads, in order, into the same accumulators
        const uint32_t h = hk * G + g;
        const T* qp = (const T*)p.q + (int64_t)qs0 * p.qst + (int64_t)h * p.qsh;
        const T* dop = (const T*)p.dout + ((int64_t)qs0 * p.H + h) * DP;
        const i32x4 q_srd = make_srd(qp, varlen_bytes(Lq, qst_b, ROW_B)), do_srd = make_srd(dop, varlen_bytes(Lq, dost_b, ROW_B));
        const i32x4 lse_srd = make_srd(p.rowc + (int64_t)h * p.Tq + qs0, Lq * 4u),
                    dv_srd = make_srd(p.rowc + ((int64_t)p.H + h) * p.Tq + qs0, Lq * 4u);
        auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
            dma_rows_strided<2 * TILE_PIECES, DP>(q_srd, lds0 + QT + par * QTILE_B, t * QROWS, qst_v, uw, lane);
            dma_rows_strided<2 * TILE_PIECES, DP>(do_srd, lds0 + DOT + par * QTILE_B, t * QROWS, dost_v, uw, lane);
        };
        auto stage_consts = [&](uint32_t t, int par) __attribute__((always_inline)) {
            const int voff = (int)(t * QROWS + (uint32_t)lane) * 4;
            if (uw == 0)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds"
                             ::"s"(lds0 + VEC + par * QROWS * 4), "v"(voff), "s"(lse_srd) : "memory");
            else if (uw == 1)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds"
                             ::"s"(lds0 + VEC + 2 * QROWS * 4 + par * QROWS * 4), "v"(voff), "s"(dv_srd) : "memory");
        };
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
            for (int g4 = 0; g4 < 4; ++g4) {
                const uint32_t row0 = qb0 + 8 * g4 + 4 * hi;  // registers 4 g4 .. 4 g4 + 3: rows row0 .. row0 + 3
                const f32x4 l2 = *(const f32x4*)(L2v + 8 * g4 + 4 * hi);  // -LSE log2(e)
                const f32x4 dl = *(const f32x4*)(Dv + 8 * g4 + 4 * hi);   // -D
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g4 + e, row = (int)row0 + e;
                    float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, l2[e]));
                    if (edge && ((int)key > row + hi_v || (int)key < row + lo_v)) pr = 0.0f;
                    pb[r >> 3][r & 7] = (T)pr;
                    sb[r >> 3][r & 7] = (T)(pr * (dp[r] + dl[e]));
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
            for (int u = 0; u < 2; ++u) {
                // edge: the sub-tile's first row's upper bound falls before the wave's last key, or its last row's lower bound after
                // the wave's first key (keys past L_k are dropped at the store)
                const int r0 = (int)(t * QROWS + 32 * u);
                if (!sub_skip(t, u)) sub_body(t, par, u, r0 + hi_off < wave_k0 + 31 || r0 + 31 + lo_off > wave_k0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // (also frees both buffers for the next query head's first tile)
            par ^= 1;
        }
    }
    if (kok) {
        const int64_t krow = (((int64_t)ks0 + key) * p.Hkv + hk) * DP;  // dense [T_k, H_kv, D]
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 32 * i + 8 * g4 + 4 * hi;
                f32x4 kv = {dk[i][4 * g4] * p.scale, dk[i][4 * g4 + 1] * p.scale, dk[i][4 * g4 + 2] * p.scale, dk[i][4 * g4 + 3] * p.scale};
                f32x4 vv = {dv[i][4 * g4], dv[i][4 * g4 + 1], dv[i][4 * g4 + 2], dv[i][4 * g4 + 3]};
                store_grad4<T>(p.dk, krow + d0, kv, p.grad_in_type != 0);
                store_grad4<T>(p.dv, krow + d0, vv, p.grad_in_type != 0);
            }
    }
}

template <typename T, int DP>
static hipError_t launch_bwd16_varlen_window_t(const VarlenParams& p, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds_dq = 4 * TILE_BYTES, lds_kv = 8 * TILE_BYTES + 1024;
    if (hipError_t e = ensure_dynamic_lds((const void*)bwd16_dq_varlen_window_kernel<T, DP>, lds_dq); e != hipSuccess) return e;
    if (hipError_t e = ensure_dynamic_lds((const void*)bwd16_dkdv_varlen_window_kernel<T, DP>, lds_kv); e != hipSuccess) return e;
    const uint32_t nqb = (p.max_q + 127) / 128, nkb = (p.max_k + 127) / 128;
    if (nqb) hipLaunchKernelGGL((bwd16_dq_varlen_window_kernel<T, DP>), dim3(nqb * p.N * p.H), dim3(256), lds_dq, stream, p);
    if (nkb) hipLaunchKernelGGL((bwd16_dkdv_varlen_window_kernel<T, DP>), dim3(nkb * p.N * p.Hkv), dim3(256), lds_kv, stream, p);
    return hipGetLastError();
}

// p.rowc as for launch_bwd_16_varlen; p.win_left / p.win_right normalised (varlen_window_ok)
hipError_t launch_bwd_16_varlen_window(const VarlenParams& p, hipStream_t stream, const char** name) {
    if (!varlen_supported(p) || !varlen_window_ok(p) || !p.cu_q || !p.cu_k || !p.rowc || !p.dout || !p.o || !p.lse || !p.dq || !p.dk ||
        !p.dv)
        return hipErrorInvalidValue;
    auto al16 = [](const void* x) { return ((uintptr_t)x & 15) == 0; };
    if (!al16(p.dout) || !al16(p.o) || !al16(p.dq) || !al16(p.dk) || !al16(p.dv) || !al16(p.rowc)) return hipErrorInvalidValue;
    static const char* const names[2][2] = {{"bwd16_dq+dkdv_varlen_window<fp16,64>", "bwd16_dq+dkdv_varlen_window<fp16,128>"},
                                            {"bwd16_dq+dkdv_varlen_window<bf16,64>", "bwd16_dq+dkdv_varlen_window<bf16,128>"}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128];
    if (p.N == 0) return hipSuccess;
    if (p.D == 64) return bf ? launch_bwd16_varlen_window_t<__bf16, 64>(p, stream) : launch_bwd16_varlen_window_t<_Float16, 64>(p, stream);
    return bf ? launch_bwd16_varlen_window_t<__bf16, 128>(p, stream) : launch_bwd16_varlen_window_t<_Float16, 128>(p, stream);
}

}  // namespace umfa
