// fa_fwd_16_varlen_window.hip -- the packed variable-length forward with a sliding window (flash-attention's window_size), bf16 / fp16,
// head_dim 64 / 128, GQA.  Semantics and layout: fa_varlen.h.
//
// fa_fwd16_varlen_kernel (fa_fwd_16_varlen.hip) with a second bound: row i of a sequence sees keys [i + off - left, i + off + right],
// off = L_k - L_q, the bounds runtime values of VarlenParams (win_left / win_right, VARLEN_WIN_OPEN for an unbounded side; causal is
// right = 0).  The workgroup's 128 rows take key tiles from the one holding key max(0, q0 + off - left) to the one holding
// min(L_k - 1, last row + off + right); a wave skips a tile wholly outside the band of its 32 rows, masks per score a tile that crosses
// either bound of any of them (or the sequence's end), and runs the open body on a tile wholly inside.  A workgroup whose range is empty
// loads no K or V and writes O = 0, LSE = -inf.  The tile body, the online softmax and the epilogue are the unwindowed kernel's.
#include <type_traits>

#include "fa_varlen.h"
#include "fa_fwd_16_kernel.h"
#include "kernels.h"

namespace umfa {

template <typename T, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_varlen_window_kernel(VarlenParams p) {
    BWD16_GEO(DP);
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    typedef Mma16<_Float16> MP;  // the P V product: fp16 P, fp16 V
    typedef typename MP::V8 PV8;
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
    const int lo_off = off - p.win_left, hi_off = off + p.win_right;  // row i sees keys [i + lo_off, i + hi_off] (and < L_k)
    const uint32_t hk = h / (p.H / p.Hkv);
    const uint32_t q_row = q0 + wave * 32 + ql;
    const bool qok = q_row < Lq;
    const T* qp = (const T*)p.q + (int64_t)qs0 * p.qst + (int64_t)h * p.qsh;
    const T* kp = (const T*)p.k + (int64_t)ks0 * p.kst + (int64_t)hk * p.ksh;
    const _Float16* vp = (const _Float16*)p.v + (int64_t)ks0 * p.vst + (int64_t)hk * p.vsh;
    const uint32_t kst_b = (uint32_t)p.kst * 2, vst_b = (uint32_t)p.vst * 2;

    V8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (qok) {
            qf[ks] = *(const V8*)(qp + (int64_t)q_row * p.qst + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (T)0.0f;
        }
    }
    const float c = p.scale * UMFA_LOG2E;

    const i32x4 k_srd = make_srd(kp, varlen_bytes(Lk, kst_b, ROW_B)), v_srd = make_srd(vp, varlen_bytes(Lk, vst_b, ROW_B));
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
#pragma unroll
    for (int i = 0; i < 4 * TILE_BYTES / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();

    // the block's keys: from its first row's lower bound to its last row's upper bound, inside [0, L_k)
    const int last_row = (int)(q0 + 127 < Lq ? q0 + 127 : Lq - 1);
    const int k_first = (int)q0 + lo_off > 0 ? (int)q0 + lo_off : 0;
    const int k_last = last_row + hi_off < (int)Lk - 1 ? last_row + hi_off : (int)Lk - 1;
    const uint32_t t_lo = (uint32_t)k_first / 32, t_hi = k_last >= k_first ? (uint32_t)k_last / 32 + 1 : t_lo;
    f32x16 acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;  // running max of c S (log2 domain, shared by the halves), this half's sum of P
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;
    auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
        dma_rows_strided<TILE_PIECES, DP>(k_srd, lds0 + par * TILE_BYTES, t * 32, kst_b, uw, lane);
        dma_rows_strided<TILE_PIECES, DP>(v_srd, lds0 + 2 * TILE_BYTES + par * TILE_BYTES, t * 32, vst_b, uw, lane);
    };
    auto tile_body = [&](uint32_t t, int par, bool edge) __attribute__((always_inline)) {
        const char* Kt = smem + par * TILE_BYTES;
        const char* Vt = smem + 2 * TILE_BYTES + par * TILE_BYTES;
        const uint32_t key_base = t * 32;
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
        for (int r = 0; r < 16; ++r) {
            const int key = (int)(key_base + acc_row(r, hi));
            x[r] = s[r] * c;
            if (edge && (key >= (int)Lk || key < (int)q_row + lo_off || key > (int)q_row + hi_off)) x[r] = -INFINITY;
            mx = fmaxf(mx, x[r]);
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
            for (int r = 0; r < 16; ++r) acc[i][r] *= alpha;
        PV8 pb[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pr = __builtin_amdgcn_exp2f(x[r] - base);
            l += pr;
            pb[r >> 3][r & 7] = (_Float16)pr;
        }
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[i] = MP::mma(tr_frag<MP, DP>(Vt, i, s2, hi, tr_qq, tr_pp, tr_g1), pb[s2], acc[i]);
    };

    const int wq0 = __builtin_amdgcn_readfirstlane((int)q0 + uw * 32);
    if (t_lo < t_hi) stage(t_lo, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int par = 0;
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        if (t + 1 < t_hi) stage(t + 1, par ^ 1);  // other buffer: its last readers passed the previous barrier
        // skip: the wave's rows are past the sequence, or the tile ends before its first row's band / starts after its last row's.
        // edge: the tile crosses the sequence's end, its last row's lower bound or its first row's upper bound.
        const int kb = (int)(t * 32);
        if (wq0 < (int)Lq && kb + 31 >= wq0 + lo_off && kb <= wq0 + 31 + hi_off)
            tile_body(t, par, kb + 31 >= (int)Lk || kb < wq0 + 31 + lo_off || kb + 31 > wq0 + hi_off);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        par ^= 1;
    }
    l += xor32(l);
    const float back = p.vsc ? p.vsc[VSC_HDR_WORDS * (size_t)hk + VSC_HDR_SCALE] : 1.0f;  // bf16: the cast pass shifted this head's V by 2^-e
    const float f = l > 0.0f ? back / l : 0.0f;
    if (qok) {
        const int64_t tok = (int64_t)qs0 + q_row;
        const int64_t orow = (tok * p.H + h) * DP;
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t at = orow + 32 * i + 8 * g + 4 * hi;
                const f32x4 val = {acc[i][4 * g] * f, acc[i][4 * g + 1] * f, acc[i][4 * g + 2] * f, acc[i][4 * g + 3] * f};
                if constexpr (std::is_same<OUT, float>::value) {
                    *(f32x4*)((float*)p.out + at) = val;
                } else {
                    typedef OUT O4 __attribute__((ext_vector_type(4)));
                    *(O4*)((OUT*)p.out + at) = O4{(OUT)val[0], (OUT)val[1], (OUT)val[2], (OUT)val[3]};
                }
            }
        if (hi == 0 && p.lse) p.lse[(int64_t)h * p.Tq + tok] = l > 0.0f ? (m + __builtin_log2f(l)) * UMFA_LN2 : -INFINITY;
    }
}

template <typename T, int DP, typename OUT>
static hipError_t launch_fwd16_varlen_window_t(const VarlenParams& p, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds = 4 * TILE_BYTES;
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_varlen_window_kernel<T, DP, OUT>, lds); e != hipSuccess) return e;
    const uint32_t nqb = (p.max_q + 127) / 128;
    hipLaunchKernelGGL((fa_fwd16_varlen_window_kernel<T, DP, OUT>), dim3(nqb * p.N * p.H), dim3(256), lds, stream, p);
    return hipGetLastError();
}

template <typename T, int DP>
static hipError_t launch_fwd16_varlen_window_d(const VarlenParams& p, hipStream_t stream) {
    return p.out_prec == P_FP32 ? launch_fwd16_varlen_window_t<T, DP, float>(p, stream) : launch_fwd16_varlen_window_t<T, DP, T>(p, stream);
}

// p.v as for launch_fwd_16_varlen; p.win_left / p.win_right normalised (varlen_window_ok)
hipError_t launch_fwd_16_varlen_window(const VarlenParams& p, hipStream_t stream, const char** name) {
    if (!varlen_supported(p) || !varlen_window_ok(p) || !p.cu_q || !p.cu_k || !p.out || ((uintptr_t)p.out & 15)) return hipErrorInvalidValue;
    if (p.out_prec != P_FP32 && p.out_prec != p.in_prec) return hipErrorInvalidValue;
    if (p.in_prec == P_BF16 && !p.vsc) return hipErrorInvalidValue;
    static const char* const names[2][2] = {{"fa_fwd16_varlen_window<fp16,64>", "fa_fwd16_varlen_window<fp16,128>"},
                                            {"fa_fwd16_varlen_window<bf16,64,pv16>", "fa_fwd16_varlen_window<bf16,128,pv16>"}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128];
    if ((uint64_t)p.N * p.H * p.max_q == 0) return hipSuccess;
    if (p.D == 64) return bf ? launch_fwd16_varlen_window_d<__bf16, 64>(p, stream) : launch_fwd16_varlen_window_d<_Float16, 64>(p, stream);
    return bf ? launch_fwd16_varlen_window_d<__bf16, 128>(p, stream) : launch_fwd16_varlen_window_d<_Float16, 128>(p, stream);
}

}  // namespace umfa
