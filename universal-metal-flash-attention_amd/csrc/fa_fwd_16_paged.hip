// fa_fwd_16_paged.hip -- bf16 / fp16 MFMA forward over a paged or static KV cache (head_dim 64 / 128, causal or not, GQA), with the
// in-place append of new tokens and the split-KV fold.  Semantics, layout and memory safety: fa_paged.h.
//
// Structure: the 128-row workgroup of fa_fwd_16_varlen.hip with the rows of one (batch, KV head) packed: row r is query token r / g of
// query head hk g + r % g (g = H / H_kv), so a KV head's keys are staged once for its whole group.  A step stages 128 keys of K and V
// (double-buffered LDS-DMA); with R = g Sq <= 32 rows ("ks4") the four waves split each step's keys, otherwise wave w owns rows 32 w ..
// of the workgroup's 128-row block and sweeps all four subtiles.  The tile step, the page indirection, the bf16 V conversion with its
// range rule, the ks4 exchange and the stores are the shared device pieces of fa_paged_device.h, described there.
//
// Split-KV (OUT = void): part s of nsplit covers its share of the 128-key steps below the workgroup's last visible key and writes its
// normalised partial O with (m, l) to scratch; an empty part writes m = -inf, l = 0.  fa_paged_fold_kernel combines the parts in order.
#include <type_traits>

#include "fa_paged_device.h"
#include "kernels.h"

namespace umfa {

template <typename T, bool CAUSAL, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_kernel(PagedParams p) {
    BWD16_GEO(DP);
    (void)TILE_PIECES, (void)PD;
    constexpr int STAGE_B = 4 * TILE_BYTES;  // one step (128 keys) of K or of V
    constexpr bool VCONV = std::is_same<T, __bf16>::value;
    constexpr bool SPLIT = std::is_same<OUT, void>::value;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t part = blockIdx.x % p.nsplit, item = blockIdx.x / p.nsplit;
    const uint32_t rb = item % p.nrb, bk = item / p.nrb, hk = bk % p.Hkv, b = bk / p.Hkv;
    const uint32_t g = p.H / p.Hkv;
    const bool ks4 = p.ks4 != 0;
    uint32_t L0u, Lku;
    paged_lens(p, b, L0u, Lku);
    const uint32_t Lk = (uint32_t)__builtin_amdgcn_readfirstlane((int)Lku);
    const int off = (int)Lk - (int)p.Sq;  // bottom-right causal: token i sees keys j <= i + off
    const uint32_t wr0 = ks4 ? 0u : rb * 128 + (uint32_t)uw * 32;  // this wave's first row
    const uint32_t r = wr0 + ql;
    const bool rok = r < p.R;
    const uint32_t qi = r / g, h = hk * g + r % g;
    const bool wlive = wr0 < p.R;
    const uint32_t wlast = wlive ? (wr0 + 32 < p.R ? wr0 + 31 : p.R - 1) : 0u;
    const int kl_first = (int)(wr0 / g) + off, kl_last = (int)(wlast / g) + off;  // causal limits of the wave's first / last rows
    uint32_t Le = Lk;  // keys the workgroup sees: [0, Le)
    if (CAUSAL) {
        const uint32_t rend = ks4 ? p.R : (rb * 128 + 128 < p.R ? rb * 128 + 128 : p.R);
        const int last = (int)((rend - 1) / g) + off;
        Le = last < 0 ? 0u : ((uint32_t)last + 1 < Lk ? (uint32_t)last + 1 : Lk);
    }
    const uint32_t nst = (Le + 127) / 128, per = (nst + p.nsplit - 1) / p.nsplit;
    const uint32_t s0 = part * per, s1 = s0 + per < nst ? s0 + per : nst;

    typename Mma16<T>::V8 qf[NKS];
    paged_load_q<T, DP>(qf, (const T*)p.q + (int64_t)b * p.qsb + (int64_t)qi * p.qst + (int64_t)h * p.qsh, rok, hi);
    const float c = p.scale * UMFA_LOG2E;
    const int lim = (int)qi + off;
    const uint32_t tst_k = (uint32_t)p.kst * 2, tst_v = (uint32_t)p.vst * 2;
    const int64_t kpage_b = p.kpg * 2, vpage_b = p.vpg * 2, khead_b = (int64_t)hk * p.ksh * 2, vhead_b = (int64_t)hk * p.vsh * 2;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;

    // every key below L_k is staged: [0, L_k)
    auto stage = [&](uint32_t s, int par, int pgv) __attribute__((always_inline)) {
        paged_dma_step<DP>(p, (const char*)p.kc, kpage_b, khead_b, tst_k, pgv, 0u, Lk, s, lds0 + par * STAGE_B, uw, lane);
        paged_dma_step<DP>(p, (const char*)p.vc, vpage_b, vhead_b, tst_v, pgv, 0u, Lk, s, lds0 + 2 * STAGE_B + par * STAGE_B, uw, lane);
    };
    unsigned vamax = 0;  // bf16: the largest |v| (bits) this thread converted
    auto convert = [&](int par, float vmul) __attribute__((always_inline)) {
        if constexpr (VCONV) paged_convert_v<DP>(smem + 2 * STAGE_B + par * STAGE_B, vmul, vamax, uw, lane);
    };

    int vexp = 0;
    for (int pass = 0;; ++pass) {
        const float vmul = __uint_as_float((unsigned)(127 - vexp) << 23);
        f32x16 acc[NDB];
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[i][rr] = 0.0f;
        float m = -INFINITY, l = 0.0f;  // running max of c S (log2 domain, shared by the halves), this half's sum of P

        int pg_a = paged_table(p, b, 0u, Lk, s0, lane), pg_b = paged_table(p, b, 0u, Lk, s0 + 1, lane);  // steps st, st + 1
        if (s0 < s1) stage(s0, 0, pg_a);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if (s0 < s1) convert(0, vmul);
        __syncthreads();
        int par = 0;
        for (uint32_t st = s0; st < s1; ++st) {
            const int pg_c = paged_table(p, b, 0u, Lk, st + 2, lane);  // (its load is waited for with this step's tiles)
            if (st + 1 < s1) stage(st + 1, par ^ 1, pg_b);  // other buffer: its last readers passed the previous barrier
            if (ks4 || wlive) {
                const int sub_end = ks4 ? uw + 1 : 4;
                for (int sub = ks4 ? uw : 0; sub < sub_end; ++sub) {
                    const uint32_t kb = st * 128 + (uint32_t)sub * 32;
                    if (kb >= Le || (CAUSAL && (int)kb > kl_last)) break;
                    // 16-key groups in pages the table does not hold are masked (their rows landed as zeros)
                    const bool v0 = __builtin_amdgcn_readlane(pg_a, 2 * sub) >= 0;
                    const bool v1 = kb + 16 >= Lk || __builtin_amdgcn_readlane(pg_a, 2 * sub + 1) >= 0;
                    const bool edge = kb + 31 >= Lk || !v0 || !v1 || (CAUSAL && (int)kb + 31 > kl_first);
                    paged_tile<T, DP>(smem + par * STAGE_B + sub * TILE_BYTES, smem + 2 * STAGE_B + par * STAGE_B + sub * TILE_BYTES, qf, c, acc, m,
                                      l, ql, hi, tr_qq, tr_pp, tr_g1, edge, [&](int kr) __attribute__((always_inline)) {
                                          const uint32_t key = kb + kr;
                                          return key >= Lk || !(kr < 16 ? v0 : v1) || (CAUSAL && (int)key > lim);
                                      });
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_waitcnt(0x0F70);
            if (st + 1 < s1) convert(par ^ 1, vmul);
            __syncthreads();
            par ^= 1;
            pg_a = pg_b;
            pg_b = pg_c;
        }
        float L = l + xor32(l);
        const bool owner = !ks4 || uw == 0;
        if (ks4) {  // the four key quarters meet in the free tile area (fa_paged_device.h)
            if (uw > 0) paged_ks4_publish<DP, 4 * STAGE_B>(smem, acc, m, L, uw, lane);
            __syncthreads();
            if (uw == 0) paged_ks4_fold<DP>(smem, acc, m, L, lane);
        }
        if constexpr (VCONV) {
            if (pass == 0) {
                // the range rule (fa_fwd_16_kernel.h v_range_check) on this workgroup's own outputs; the words FWD16_EPI_RED .. + 7 lie in
                // front of the exchange area, and a barrier follows their reads before anything may overwrite them (the second sweep)
                const float inv = L > 0.0f ? 1.0f / L : 0.0f;
                float chk_nan = 0.0f, chk_max = 0.0f;
#pragma unroll
                for (int i = 0; i < NDB; ++i)
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const float val = acc[i][rr] * inv;
                        chk_nan = __builtin_fmaf(val, 0.0f, chk_nan);
                        chk_max = fmaxf(chk_max, __builtin_fabsf(val));
                    }
                const bool live = owner && rok;
                const unsigned bits = (__builtin_amdgcn_ballot_w64(live && chk_nan != chk_nan) != 0 ? 1u : 0u) |
                                      (__builtin_amdgcn_ballot_w64(live && chk_max >= 0x1p-11f) != 0 ? 2u : 0u) |
                                      (__builtin_amdgcn_ballot_w64(live && L > 0.0f) != 0 ? 4u : 0u);
                unsigned am = vamax;
#pragma unroll
                for (int o2 = 32; o2 > 0; o2 >>= 1) {
                    const unsigned t2 = (unsigned)__shfl_xor((int)am, o2, 64);
                    am = am > t2 ? am : t2;
                }
                volatile uint32_t* const red = (volatile uint32_t*)smem + FWD16_EPI_RED;
                if (lane == 0) {
                    red[uw] = bits;
                    red[4 + uw] = am;
                }
                __syncthreads();
                unsigned all = 0, amax = 0;
#pragma unroll
                for (int w2 = 0; w2 < 4; ++w2) {
                    all |= red[w2];
                    const unsigned rv = red[4 + w2];
                    amax = amax > rv ? amax : rv;
                }
                all = __builtin_amdgcn_readfirstlane(all);
                amax = __builtin_amdgcn_readfirstlane(amax);
                if (__builtin_expect((all & 1u) || ((all & 4u) && !(all & 2u)), 0)) {
                    const int e2 = vscale_exponent_of(amax);
                    if (amax != 0 && amax < 0x7f80u && e2 != 0) {
                        __syncthreads();  // every wave has read the words: the second sweep's DMA may overwrite them
                        vexp = e2;
                        continue;
                    }
                }
            }
        }
        const float back = __uint_as_float((unsigned)(127 + vexp) << 23);  // the shift comes back (exact)
        if (owner && rok) {
            const float f = L > 0.0f ? back / L : 0.0f;
            if constexpr (SPLIT) {
                const int64_t rows_all = (int64_t)p.B * p.Hkv * p.R;
                paged_store_part<DP>(p.part, (int64_t)p.nsplit * rows_all, (int64_t)part * rows_all + (int64_t)bk * p.R + r, acc, f, m, L, hi);
            } else {
                paged_store_out<DP, OUT>(p.out, (((int64_t)b * p.Sq + qi) * p.H + h) * DP, p.lse, ((int64_t)b * p.H + h) * p.Sq + qi, acc, f, m,
                                         L, hi);
            }
        }
        return;
    }
}

// the split-KV fold: row (b, hk, r) of every part, in part order (bitwise repeatable), into O and LSE.  D / 4 lanes per row.
template <typename OUT>
__global__ __launch_bounds__(256) void fa_paged_fold_kernel(PagedParams p) {
    const uint32_t nl = p.D / 4, rpb = 256 / nl;
    const uint32_t row = blockIdx.x * rpb + threadIdx.x / nl, d4 = threadIdx.x % nl;
    const uint32_t rows_all = p.B * p.Hkv * p.R;
    if (row >= rows_all) return;
    const float* const ml = p.part + (size_t)p.nsplit * rows_all * p.D;
    float Mx = -INFINITY;
    for (uint32_t s = 0; s < p.nsplit; ++s) Mx = fmaxf(Mx, ml[((size_t)s * rows_all + row) * 2]);
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    float L = 0.0f;
    for (uint32_t s = 0; s < p.nsplit; ++s) {
        const size_t pr = (size_t)s * rows_all + row;
        const float ms = ml[pr * 2], ls = ml[pr * 2 + 1];
        const float w = ms == -INFINITY ? 0.0f : ls * __builtin_amdgcn_exp2f(ms - Mx);
        if (w != 0.0f) {
            const f32x4 os = *(const f32x4*)(p.part + pr * p.D + 4 * d4);
            o += w * os;
            L += w;
        }
    }
    const float f = L > 0.0f ? 1.0f / L : 0.0f;
    const uint32_t g = p.H / p.Hkv, bk = row / p.R, r = row % p.R, b = bk / p.Hkv, hk = bk % p.Hkv;
    const uint32_t qi = r / g, h = hk * g + r % g;
    const int64_t at = (((int64_t)b * p.Sq + qi) * p.H + h) * p.D + 4 * d4;
    if constexpr (std::is_same<OUT, float>::value) {
        *(f32x4*)((float*)p.out + at) = o * f;
    } else {
        typedef OUT O4 __attribute__((ext_vector_type(4)));
        *(O4*)((OUT*)p.out + at) = O4{(OUT)(o[0] * f), (OUT)(o[1] * f), (OUT)(o[2] * f), (OUT)(o[3] * f)};
    }
    if (d4 == 0 && p.lse) p.lse[((int64_t)b * p.H + h) * p.Sq + qi] = L > 0.0f ? (Mx + __builtin_log2f(L)) * UMFA_LN2 : -INFINITY;
}

// the append: row i of k_new / v_new of sequence b goes to cache position clamp(cache_seqlens[b]) + i through the block table.  Rows
// past the capacity and rows of pages the table does not hold are dropped.  One thread per 16 bytes.
__global__ __launch_bounds__(256) void fa_paged_append_kernel(PagedParams p) {
    const uint32_t nch = p.D / 8;
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = (uint64_t)p.B * p.Snew * p.Hkv * nch * 2;
    if (idx >= total) return;
    uint64_t t = idx;
    const uint32_t c = (uint32_t)(t % nch); t /= nch;
    const uint32_t hk = (uint32_t)(t % p.Hkv); t /= p.Hkv;
    const uint32_t i = (uint32_t)(t % p.Snew); t /= p.Snew;
    const uint32_t b = (uint32_t)(t % p.B);
    const bool isv = t / p.B != 0;
    uint32_t L0, Lk;
    paged_lens(p, b, L0, Lk);
    const uint32_t pos = L0 + i;
    if (pos >= p.max_pages * p.page_size) return;
    const uint32_t lp = paged_lpage(p, pos);
    const int pg = paged_page(p, b, lp);
    if (pg < 0) return;
    const uint32_t rip = pos - lp * p.page_size;
    typedef unsigned U4 __attribute__((ext_vector_type(4)));
    const uint16_t* src = (const uint16_t*)(isv ? p.vn : p.kn) +
                          (isv ? (int64_t)b * p.vnb + (int64_t)i * p.vnt + (int64_t)hk * p.vnh : (int64_t)b * p.knb + (int64_t)i * p.knt + (int64_t)hk * p.knh);
    uint16_t* dst = (uint16_t*)(isv ? p.vc : p.kc) +
                    (isv ? (int64_t)pg * p.vpg + (int64_t)rip * p.vst + (int64_t)hk * p.vsh : (int64_t)pg * p.kpg + (int64_t)rip * p.kst + (int64_t)hk * p.ksh);
    *(U4*)(dst + 8 * c) = *(const U4*)(src + 8 * c);
}

// Scope: bf16 / fp16, head_dim 64 / 128, H a multiple of H_kv, strides multiples of 8 elements and rows that do not overlap inside a
// head, 16-byte aligned bases, page_size a multiple of 16 with a block table, and one page (+ the 8 rows a piece may run past a static
// row) inside a 32-bit buffer offset.
bool paged_supported(const PagedParams& p) {
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if (p.D != 64 && p.D != 128) return false;
    if (p.H == 0 || p.Hkv == 0 || p.H % p.Hkv || p.B == 0) return false;
    if (p.page_size == 0 || (p.bt && p.page_size % 16) || p.num_pages == 0 || p.max_pages == 0) return false;
    if (!p.bt && (p.max_pages != 1 || p.num_pages < p.B)) return false;
    if ((uint64_t)p.max_pages * p.page_size >= (1ull << 31) || p.num_pages >= (1u << 31)) return false;
    const int64_t st[9] = {p.qsb, p.qst, p.qsh, p.kpg, p.kst, p.ksh, p.vpg, p.vst, p.vsh};
    for (int64_t s : st)
        if (s < 0 || s % 8) return false;
    if (p.kst < (int64_t)p.D || p.vst < (int64_t)p.D) return false;
    if (p.Snew) {
        const int64_t sn[6] = {p.knb, p.knt, p.knh, p.vnb, p.vnt, p.vnh};
        for (int64_t s : sn)
            if (s < 0 || s % 8) return false;
        if (!p.kn || !p.vn || ((uintptr_t)p.kn & 15) || ((uintptr_t)p.vn & 15)) return false;
        if ((uint64_t)p.B * p.Snew * p.Hkv * (p.D / 8) * 2 >= (1ull << 40)) return false;
    }
    auto al16 = [](const void* x) { return ((uintptr_t)x & 15) == 0; };
    if (!p.q || !p.kc || !p.vc || !p.seqlens || !al16(p.q) || !al16(p.kc) || !al16(p.vc)) return false;
    const uint64_t lim = 1ull << 31;
    if (((uint64_t)p.page_size + 8) * (uint64_t)p.kst * 2 >= lim || ((uint64_t)p.page_size + 8) * (uint64_t)p.vst * 2 >= lim) return false;
    return (uint64_t)p.B * p.Hkv * p.nrb * (p.nsplit ? p.nsplit : 1) < lim;
}

hipError_t launch_paged_append(const PagedParams& p, hipStream_t stream) {
    if (!paged_supported(p)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)p.B * p.Snew * p.Hkv * (p.D / 8) * 2;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(fa_paged_append_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// the fold of p.nsplit parts in p.part into p.out (fp32 or the 16-bit p.in_prec) and p.lse; the partials are fp32 whatever the cache
// holds, so fa_fwd_16_paged_fp8.hip launches it too
hipError_t launch_paged_fold(const PagedParams& p, hipStream_t stream) {
    const uint32_t rows = p.B * p.Hkv * p.R, rpb = 256 / (p.D / 4);
    const dim3 grid((rows + rpb - 1) / rpb);
    if (p.out_prec == P_FP32)
        hipLaunchKernelGGL(fa_paged_fold_kernel<float>, grid, dim3(256), 0, stream, p);
    else if (p.in_prec == P_BF16)
        hipLaunchKernelGGL(fa_paged_fold_kernel<__bf16>, grid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL(fa_paged_fold_kernel<_Float16>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

template <typename T, bool CAUSAL, int DP, typename OUT>
static hipError_t launch_fwd16_paged_t(const PagedParams& p, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds = 4 * 4 * TILE_BYTES;
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_paged_kernel<T, CAUSAL, DP, OUT>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((fa_fwd16_paged_kernel<T, CAUSAL, DP, OUT>), dim3(p.B * p.Hkv * p.nrb * p.nsplit), dim3(256), lds, stream, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (std::is_same<OUT, void>::value) return launch_paged_fold(p, stream);
    return hipSuccess;
}

template <typename T, int DP>
static hipError_t launch_fwd16_paged_d(const PagedParams& p, hipStream_t stream) {
    const bool f32 = p.out_prec == P_FP32;
    if (p.nsplit > 1)
        return p.causal ? launch_fwd16_paged_t<T, true, DP, void>(p, stream) : launch_fwd16_paged_t<T, false, DP, void>(p, stream);
    if (p.causal) return f32 ? launch_fwd16_paged_t<T, true, DP, float>(p, stream) : launch_fwd16_paged_t<T, true, DP, T>(p, stream);
    return f32 ? launch_fwd16_paged_t<T, false, DP, float>(p, stream) : launch_fwd16_paged_t<T, false, DP, T>(p, stream);
}

// the forward launchers' checks behind *_supported (p.H / p.Hkv is safe there): an aligned output, an optional aligned LSE, the output
// type fp32 or the operands', and R / nrb / ks4 consistent with the shape
bool paged_fwd_args_ok(const PagedParams& p) {
    if (!p.out || ((uintptr_t)p.out & 15) || ((uintptr_t)p.lse & 3) || p.nsplit == 0) return false;
    if (p.out_prec != P_FP32 && p.out_prec != p.in_prec) return false;
    return p.R == (p.H / p.Hkv) * p.Sq && p.nrb == (p.ks4 ? 1u : (p.R + 127) / 128) && !(p.ks4 && p.R > 32);
}

// p.nsplit > 1: p.part holds nsplit B H_kv R (D + 2) floats
hipError_t launch_fwd_16_paged(const PagedParams& p, hipStream_t stream, const char** name) {
    if (!paged_supported(p) || !paged_fwd_args_ok(p)) return hipErrorInvalidValue;
    if (p.nsplit > 1 && !p.part) return hipErrorInvalidValue;
    static const char* const names[2][2][2][2] = {
        {{{"fa_fwd16_paged<fp16,64>", "fa_fwd16_paged<fp16,64,split>"}, {"fa_fwd16_paged<fp16,64,causal>", "fa_fwd16_paged<fp16,64,causal,split>"}},
         {{"fa_fwd16_paged<fp16,128>", "fa_fwd16_paged<fp16,128,split>"}, {"fa_fwd16_paged<fp16,128,causal>", "fa_fwd16_paged<fp16,128,causal,split>"}}},
        {{{"fa_fwd16_paged<bf16,64,pv16>", "fa_fwd16_paged<bf16,64,pv16,split>"},
          {"fa_fwd16_paged<bf16,64,causal,pv16>", "fa_fwd16_paged<bf16,64,causal,pv16,split>"}},
         {{"fa_fwd16_paged<bf16,128,pv16>", "fa_fwd16_paged<bf16,128,pv16,split>"},
          {"fa_fwd16_paged<bf16,128,causal,pv16>", "fa_fwd16_paged<bf16,128,causal,pv16,split>"}}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.causal != 0][p.nsplit > 1];
    if ((uint64_t)p.B * p.H * p.Sq == 0) return hipSuccess;
    if (p.D == 64) return bf ? launch_fwd16_paged_d<__bf16, 64>(p, stream) : launch_fwd16_paged_d<_Float16, 64>(p, stream);
    return bf ? launch_fwd16_paged_d<__bf16, 128>(p, stream) : launch_fwd16_paged_d<_Float16, 128>(p, stream);
}

}  // namespace umfa
