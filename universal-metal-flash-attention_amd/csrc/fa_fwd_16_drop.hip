// fa_fwd_16_drop.hip -- bf16 / fp16 MFMA forward with attention dropout (head_dim 64 / 128, causal or not, no mask), and the keep-mask
// materialiser.  The mask is fa_dropout.h's: a pure function of (query row, key, b*H + h, rng_state), so this kernel, the backward
// (fa_bwd_16_drop.hip) and the materialiser agree bit for bit whatever their tiling.
//
// Structure: the 128-row workgroup of the other 128-row kernels (4 waves x 32 query rows), 32-key tiles of K and V through LDS
// (LDS-DMA, double-buffered), S^T = K Q^T so that a lane owns one query and its registers hold keys in runs of 4 consecutive keys:
// ONE Philox4x32-10 call per run gives the run's four keep bits.  Online softmax per query (the wave halves share the row max through
// v_permlane32_swap); the row sum l accumulates the UNDROPPED P, only the P V operand is masked.  The P V product runs in fp16 as on
// the no-dropout 128-row launch: P rounded to fp16, V the fp16 image (bf16 operands: the runtime's cast pre-pass shifted by one power of
// two per slab, FwdParams::vsc, which the epilogue takes back).  Epilogue: O = acc * (s * 2^e / l) in fp32; LSE is the undropped one.
#include <type_traits>

#include "fa_bwd_16_common.h"
#include "fa_dropout.h"
#include "fa_fwd_16_kernel.h"
#include "kernels.h"

namespace umfa {

template <typename T, bool CAUSAL, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_drop_kernel(DropFwdParams p) {
    BWD16_GEO(DP);
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    typedef Mma16<_Float16> MP;  // the P V product: fp16 P, fp16 V (image)
    typedef typename MP::V8 PV8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t nqb = (p.Sq + 127) / 128;
    const uint32_t vid = xcd_remap(blockIdx.x, nqb * p.B * p.H);
    uint32_t bh = vid / nqb;
    uint32_t qb = vid % nqb;
    if (CAUSAL) qb = nqb - 1 - causal_rank(vid, nqb, bh, true);  // longest blocks first
    const uint32_t b = bh / p.H, h = bh % p.H;
    const uint32_t q0 = qb * 128, q_row = q0 + wave * 32 + ql;
    const bool qok = q_row < p.Sq;
    const T* qp = (const T*)p.q + (int64_t)b * p.qs[0] + (int64_t)h * p.qs[1];
    const T* kp = (const T*)p.k + (int64_t)b * p.ks[0] + (int64_t)h * p.ks[1];
    const _Float16* vp = (const _Float16*)p.v + (int64_t)b * p.vs[0] + (int64_t)h * p.vs[1];

    V8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        if (qok) {
            qf[ks] = *(const V8*)(qp + (int64_t)q_row * p.qs[2] + 16 * ks + 8 * hi);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (T)0.0f;
        }
    }
    const uint64_t seed = (uint64_t)p.rng[0], offset = (uint64_t)p.rng[1];
    const uint32_t thresh = p.thresh;
    const float c = p.scale * UMFA_LOG2E;

    const i32x4 k_srd = make_srd(kp, p.Skv * (uint32_t)ROW_B), v_srd = make_srd(vp, p.Skv * (uint32_t)ROW_B);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
#pragma unroll
    for (int i = 0; i < 4 * TILE_BYTES / 4096; ++i) *(i32x4*)(smem + i * 4096 + tid * 16) = i32x4{0, 0, 0, 0};
    __syncthreads();

    uint32_t t_hi = (p.Skv + 31) / 32;
    if (CAUSAL) {
        const uint32_t lim = (q0 + 128 + 31) / 32;
        t_hi = t_hi < lim ? t_hi : lim;
    }
    f32x16 acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;  // running max of c S (log2 domain, shared by the halves), this half's sum of undropped P
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;
    auto stage = [&](uint32_t t, int par) __attribute__((always_inline)) {
        dma_rows<TILE_PIECES, DP>(k_srd, lds0 + par * TILE_BYTES, t * 32, uw, lane);
        dma_rows<TILE_PIECES, DP>(v_srd, lds0 + 2 * TILE_BYTES + par * TILE_BYTES, t * 32, uw, lane);
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
        // keep bits: registers 4g .. 4g+3 hold keys k0 .. k0+3, k0 = key_base + 8g + 4hi -- one Philox call per run (under the MFMAs)
        uint32_t keep[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) keep[g] = drop_keep4((key_base + 8 * g + 4 * hi) >> 2, q_row, bh, seed, offset, thresh);
        float x[16], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t key = key_base + acc_row(r, hi);
            x[r] = s[r] * c;
            if (edge && (key >= p.Skv || (CAUSAL && key > q_row))) x[r] = -INFINITY;
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
            pb[r >> 3][r & 7] = (_Float16)(((keep[r >> 2] >> (r & 3)) & 1u) ? pr : 0.0f);
        }
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[i] = MP::mma(tr_frag<MP, DP>(Vt, i, s2, hi, tr_qq, tr_pp, tr_g1), pb[s2], acc[i]);
    };

    const uint32_t wq0 = __builtin_amdgcn_readfirstlane(q0 + (uint32_t)uw * 32);
    if (t_hi > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int par = 0;
    for (uint32_t t = 0; t < t_hi; ++t) {
        if (t + 1 < t_hi) stage(t + 1, par ^ 1);  // other buffer: its last readers passed the previous barrier
        if (!CAUSAL || t * 32 <= wq0 + 31) tile_body(t, par, t * 32 + 31 >= p.Skv || (CAUSAL && t * 32 + 31 > wq0));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        par ^= 1;
    }
    l += xor32(l);
    float back = 1.0f;  // bf16: the cast pre-pass shifted this slab's V by 2^-e
    if (p.vsc) back = p.vsc[VSC_HDR_WORDS * ((size_t)b * p.vsc_bs + (size_t)h * p.vsc_hs) + VSC_HDR_SCALE];
    const float f = l > 0.0f ? p.dscale * back / l : 0.0f;
    if (qok) {
        const int64_t orow = ((int64_t)bh * p.Sq + q_row) * DP;
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t at = orow + 32 * i + 8 * g + 4 * hi;
                const f32x4 val = {acc[i][4 * g] * f, acc[i][4 * g + 1] * f, acc[i][4 * g + 2] * f, acc[i][4 * g + 3] * f};
                if constexpr (std::is_same<OUT, float>::value) {
                    *(f32x4*)((float*)p.o + at) = val;
                } else {
                    typedef OUT O4 __attribute__((ext_vector_type(4)));
                    *(O4*)((OUT*)p.o + at) = O4{(OUT)val[0], (OUT)val[1], (OUT)val[2], (OUT)val[3]};
                }
            }
        if (hi == 0 && p.lse) p.lse[(int64_t)bh * p.Sq + q_row] = l > 0.0f ? (m + __builtin_log2f(l)) * UMFA_LN2 : -INFINITY;
    }
}

// keep[b, h, i, j] as 0 / 1 bytes, dense [B, H, Sq, Skv]: one thread per run of four keys of one row
__global__ __launch_bounds__(256) void fa_dropout_keep_kernel(uint8_t* keep, uint32_t BH, uint32_t Sq, uint32_t Skv, const int64_t* rng,
                                                              uint32_t thresh) {
    const uint32_t nq = (Skv + 3) / 4;
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (uint64_t)BH * Sq * nq) return;
    const uint32_t jq = (uint32_t)(idx % nq);
    const uint64_t row = idx / nq;  // bh * Sq + i
    const uint32_t i = (uint32_t)(row % Sq), bh = (uint32_t)(row / Sq);
    const uint32_t bits = drop_keep4(jq, i, bh, (uint64_t)rng[0], (uint64_t)rng[1], thresh);
    uint8_t* dst = keep + row * Skv + 4ull * jq;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * jq + e < Skv) dst[e] = (uint8_t)((bits >> e) & 1u);
}

bool fwd_16_dropout_supported(const FwdParams& p) {
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if (p.D != 64 && p.D != 128) return false;
    if (p.out_prec != P_FP32 && p.out_prec != p.in_prec) return false;
    if (p.mask || p.mask_kind != MK_NONE) return false;
    if (p.qs[3] != 1 || p.ks[3] != 1 || p.vs[3] != 1 || p.ks[2] != (int64_t)p.D || p.vs[2] != (int64_t)p.D) return false;  // K / V rows dense
    if (((uintptr_t)p.q & 15) || ((uintptr_t)p.k & 15) || ((uintptr_t)p.v & 15) || ((uintptr_t)p.o & 15)) return false;
    for (int i = 0; i < 3; ++i)
        if (p.qs[i] % 8 || p.ks[i] % 8 || p.vs[i] % 8) return false;  // 16-byte aligned rows / slabs
    return (uint64_t)p.Skv * 2 * p.D < (1ull << 31);  // a K / V slab through a 32-bit buffer descriptor
}

template <typename T, bool CAUSAL, int DP, typename OUT>
static hipError_t launch_fwd16_drop_t(const DropFwdParams& p, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds = 4 * TILE_BYTES;
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_drop_kernel<T, CAUSAL, DP, OUT>, lds); e != hipSuccess) return e;
    const uint32_t nqb = (p.Sq + 127) / 128;
    hipLaunchKernelGGL((fa_fwd16_drop_kernel<T, CAUSAL, DP, OUT>), dim3(nqb * p.B * p.H), dim3(256), lds, stream, p);
    return hipGetLastError();
}

template <typename T, int DP>
static hipError_t launch_fwd16_drop_d(const DropFwdParams& p, hipStream_t stream) {
    const bool f32 = p.out_prec == P_FP32;
    if (p.causal) return f32 ? launch_fwd16_drop_t<T, true, DP, float>(p, stream) : launch_fwd16_drop_t<T, true, DP, T>(p, stream);
    return f32 ? launch_fwd16_drop_t<T, false, DP, float>(p, stream) : launch_fwd16_drop_t<T, false, DP, T>(p, stream);
}

// p.v: bf16 operands -> the fp16 image of the cast pre-pass with p.vsc set; fp16 -> the caller's V
hipError_t launch_fwd_16_dropout(const DropFwdParams& p, hipStream_t stream, const char** name) {
    if (!fwd_16_dropout_supported(p) || !p.rng || (p.in_prec == P_BF16 && !p.vsc)) return hipErrorInvalidValue;
    static const char* const names[2][2][2] = {
        {{"fa_fwd16_drop<fp16,64>", "fa_fwd16_drop<fp16,64,causal>"}, {"fa_fwd16_drop<fp16,128>", "fa_fwd16_drop<fp16,128,causal>"}},
        {{"fa_fwd16_drop<bf16,64,pv16>", "fa_fwd16_drop<bf16,64,causal,pv16>"}, {"fa_fwd16_drop<bf16,128,pv16>", "fa_fwd16_drop<bf16,128,causal,pv16>"}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.causal != 0];
    if (p.D == 64) return bf ? launch_fwd16_drop_d<__bf16, 64>(p, stream) : launch_fwd16_drop_d<_Float16, 64>(p, stream);
    return bf ? launch_fwd16_drop_d<__bf16, 128>(p, stream) : launch_fwd16_drop_d<_Float16, 128>(p, stream);
}

hipError_t launch_dropout_keep_mask(uint8_t* keep, uint32_t B, uint32_t H, uint32_t Sq, uint32_t Skv, const int64_t* rng, uint32_t thresh,
                                    hipStream_t stream) {
    const uint64_t n = (uint64_t)B * H * Sq * ((Skv + 3) / 4);
    if (n == 0) return hipSuccess;
    if ((n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fa_dropout_keep_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, keep, B * H, Sq, Skv, rng, thresh);
    return hipGetLastError();
}

}  // namespace umfa
