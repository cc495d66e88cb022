// fa_fwd_16_paged_fp8.hip -- the bf16 / fp16 MFMA forward of fa_fwd_16_paged.hip over an OCP fp8 (e4m3fn) paged or static KV cache with a
// dequantisation scale per (batch, KV head), and the quantising in-place append.  Semantics: fa_paged_fp8.h (layout, clamps, masking and
// memory safety: fa_paged.h).  runtime_paged.hip drives it.
//
// Arithmetic: the 16-bit kernel's.  Every finite e4m3fn value is exact in fp16 and in bf16, so K8 is expanded to T and V8 to fp16 without
// rounding; k_descale folds into the workgroup's scale log2(e) constant, v_descale into the epilogue's 1 / l (both products in fp32), P is
// rounded to fp16 once as in every pv16 kernel.  The bf16-V range machinery of fa_fwd_16_paged.hip (v 2^-e, v_range_check, the second
// sweep) is not here because nothing can leave fp16's range: P <= 1, |V8| <= 448 and the accumulation is fp32, and v_descale (which may be
// any size) multiplies the fp32 result behind the product.
//
// Structure: fa_fwd16_paged_kernel's (rows of one (batch, KV head) packed into the workgroup, 128-key steps, "ks4" for R <= 32 rows, zero
// -byte descriptors for table entries outside the pool, split-KV parts) with the bytes landing as fp8:
//   * a ring of NS = 2 fp8 stages (one step of K8 and of V8 each: 2 x 128 x D bytes).  A 1-KiB LDS-DMA piece is 8 rows (D = 128) or 16
//     (D = 64), so it never straddles a page whose size is a multiple of 16.  Pieces are PRIVATE to the wave that requested them: it
//     waits for its own (counted vmcnt: the younger stage stays in flight), expands them, and requests the step NS ahead into the same
//     pieces -- no barrier guards the ring, and the stream is never drained at a barrier as the 16-bit kernel's is.
//   * one 16-bit image of the step (K in T, V in fp16; 128 rows in fa_bwd_16_common.h d_off<DP>'s layout), written by the expansion and
//     read by exactly the 16-bit kernel's fragment reads.  Two barriers a step: image complete / image free.
//   * the block table is read 64 16-key groups (8 steps) at a time, one vector load per 8 steps, consumed at once: that one load drains
//     the wave's DMA queue (the compiler's wait cannot be counted past requests it does not see), once per 8 steps.
//
// Measured: 0.79 - 0.85 of the 16-bit kernel's time on the HBM-bound shapes.  The stream is not the limit any
// more -- the expansion and the tiles, in series between the two barriers, each cost about 30 % of a step; converting K at fragment load
// and a second image are the next steps.
//
// LDS images and banks.  The fp8 stage is linear (lane l of a piece owns bytes 16 l ..): the expansion's ds_read_b128 reads 1 KiB
// contiguously, conflict-free.  The 16-bit image is d_off<DP>'s, so the K row reads and the transposed V reads are the ones
// fa_fwd_16_paged.hip makes on the same image (fa_bwd_16_common.h: one swizzle for row and transposed reads).  The expansion's
// writes: a lane holds 16 elements = chunks 2 c, 2 c + 1 of row r (c = 16-element chunk of the fp8 row); ds_write_b128 is served in
// groups of 8 contiguous lanes over 32 banks (128 bytes = 8 chunk slots, slots s and s + 8 of a 256-byte row collide).  D = 128: the 8
// lanes of a group are one row; lanes c < 4 write chunk 2 c first and lanes c >= 4 chunk 2 c + 1, so the group's slots mod 8 are
// {0, 2, 4, 6, 1, 3, 5, 7} ^ (f & 7) -- all different.  D = 64: a group is rows r, r + 1 (128-byte rows, the same swizzle parity);
// even rows write the even chunk first and odd rows the odd one.  LDS: 128 KiB (D = 128, one workgroup per CU), 64 KiB (D = 64, two).
#include <type_traits>

#include "fa_paged_fp8.h"
#include "fa_paged_device.h"
#include "kernels.h"

namespace umfa {

namespace {

// lab switches of the ablation in DESIGN.md section 3.1j (tools/build_paged_fp8_variant.sh); the product builds with neither
#ifndef UMFA_FP8_NS
#define UMFA_FP8_NS 2
#endif
#ifndef UMFA_FP8_ABLATE
#define UMFA_FP8_ABLATE 0  // 1: no expansion, 2: no tiles -- the results are then wrong, only the time means something
#endif
constexpr int FP8_NS = UMFA_FP8_NS;  // fp8 stages in the ring (3 at head_dim 128 is all 160 KiB of a CU's LDS)

}  // namespace

template <typename T, bool CAUSAL, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_fp8_kernel(PagedFp8Params pp) {
    BWD16_GEO(DP);
    (void)TILE_PIECES, (void)PD;
    const PagedParams& p = pp.p;
    constexpr int NS = FP8_NS;
    constexpr int IMG_B = 4 * TILE_BYTES;    // the 16-bit image of one step (128 keys) of K or of V
    constexpr int ST8_B = 128 * DP;          // one step of K8 or of V8
    constexpr int NP = 128 / (1024 / DP);    // fp8 pieces per step and tensor
    constexpr int PER = 2 * NP / 4;          // LDS-DMA requests per wave and step
    constexpr bool SPLIT = std::is_same<OUT, void>::value;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ring = smem + 2 * IMG_B;
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
    const float kd = pp.kd[(int64_t)b * pp.kdb + (int64_t)hk * pp.kdh], vd = pp.vd[(int64_t)b * pp.vdb + (int64_t)hk * pp.vdh];

    typename Mma16<T>::V8 qf[NKS];
    paged_load_q<T, DP>(qf, (const T*)p.q + (int64_t)b * p.qsb + (int64_t)qi * p.qst + (int64_t)h * p.qsh, rok, hi);
    const float c = p.scale * UMFA_LOG2E * kd;  // scores of the dequantised keys, log2 domain
    const int lim = (int)qi + off;
    const uint32_t tst_k = (uint32_t)p.kst, tst_v = (uint32_t)p.vst;  // fp8: elements are bytes
    const int64_t kpage_b = p.kpg, vpage_b = p.vpg, khead_b = (int64_t)hk * p.ksh, vhead_b = (int64_t)hk * p.vsh;
    const unsigned lds_ring = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem)) + 2 * IMG_B;
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;

    auto stage = [&](uint32_t s, int slot, int tab) __attribute__((always_inline)) {
        paged8_dma_step<DP>(p, (const char*)p.kc, kpage_b, khead_b, tst_k, tab, Lk, s, lds_ring + slot * 2 * ST8_B, uw, lane);
        paged8_dma_step<DP>(p, (const char*)p.vc, vpage_b, vhead_b, tst_v, tab, Lk, s, lds_ring + slot * 2 * ST8_B + ST8_B, uw, lane);
    };
    // this wave's own pieces of the stage -> the 16-bit image (K in T, V in fp16)
    auto expand = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int n0 = 0; n0 < NP; n0 += 4) {
            fp8_expand_piece<T, DP>(ring + slot * 2 * ST8_B, smem, n0 + uw, lane);
            fp8_expand_piece<_Float16, DP>(ring + slot * 2 * ST8_B + ST8_B, smem + IMG_B, n0 + uw, lane);
        }
    };

    f32x16 acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[i][rr] = 0.0f;
    float m = -INFINITY, l = 0.0f;  // running max of c S (log2 domain, shared by the halves), this half's sum of P

    // the block table of super-steps S_cur (tab_c) and S_cur + 1 (tab_n): a step's requests run NS steps ahead of its tiles
    uint32_t S_cur = s0 >> 3;
    int tab_c = paged8_table(p, b, Lk, S_cur, lane), tab_n = paged8_table(p, b, Lk, S_cur + 1, lane);
    // every load the compiler knows of is waited for HERE, in front of the first request: a wait it placed inside the loop (for q, on
    // a path where no table entry was loaded) would be vmcnt(0) and drain the ring at every tile
    asm volatile("" : "+v"(tab_c), "+v"(tab_n));
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qf[ks]));
    auto tab_of = [&](uint32_t s) __attribute__((always_inline)) { return (s >> 3) == S_cur ? tab_c : tab_n; };
#pragma unroll
    for (int j = 0; j < NS; ++j)
        if (s0 + j < s1) stage(s0 + j, j, tab_of(s0 + j));
    int slot = 0;
    for (uint32_t st = s0; st < s1; ++st) {
        // this wave's pieces of step st have landed; the stages requested behind them (NS - 1 steps, when the range still holds them)
        // stay in flight
        if (st + NS <= s1)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 1) * PER) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((st >> 3) != S_cur) {
            S_cur = st >> 3;
            tab_c = tab_n;
            tab_n = paged8_table(p, b, Lk, S_cur + 1, lane);
            asm volatile("" : "+v"(tab_n));  // (consumed at once: file header)
        }
        if (UMFA_FP8_ABLATE != 1) expand(slot);  // (the image is free: every wave passed the previous step's second barrier)
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the stage's bytes are in registers before its pieces are requested again
        if (st + NS < s1) stage(st + NS, slot, tab_of(st + NS));
        __syncthreads();
        if (UMFA_FP8_ABLATE != 2 && (ks4 || wlive)) {
            const int sub_end = ks4 ? uw + 1 : 4;
            for (int sub = ks4 ? uw : 0; sub < sub_end; ++sub) {
                const uint32_t kb = st * 128 + (uint32_t)sub * 32;
                if (kb >= Le || (CAUSAL && (int)kb > kl_last)) break;
                // 16-key groups in pages the table does not hold are masked (their rows landed as zeros)
                const int g0 = (int)(8 * (st & 7)) + 2 * sub;
                const bool v0 = __builtin_amdgcn_readlane(tab_c, g0) >= 0;
                const bool v1 = kb + 16 >= Lk || __builtin_amdgcn_readlane(tab_c, g0 + 1) >= 0;
                const bool edge = kb + 31 >= Lk || !v0 || !v1 || (CAUSAL && (int)kb + 31 > kl_first);
                paged_tile<T, DP>(smem + sub * TILE_BYTES, smem + IMG_B + sub * TILE_BYTES, qf, c, acc, m, l, ql, hi, tr_qq, tr_pp, tr_g1, edge,
                                  [&](int kr) __attribute__((always_inline)) {
                                      const uint32_t key = kb + kr;
                                      return key >= Lk || !(kr < 16 ? v0 : v1) || (CAUSAL && (int)key > lim);
                                  });
            }
        }
        __syncthreads();
        slot = slot + 1 == NS ? 0 : slot + 1;
    }
    float L = l + xor32(l);
    const bool owner = !ks4 || uw == 0;
    if (ks4) {  // the four key quarters meet in the free image area (fa_paged_device.h)
        if (uw > 0) paged_ks4_publish<DP, 2 * IMG_B>(smem, acc, m, L, uw, lane);
        __syncthreads();
        if (uw == 0) paged_ks4_fold<DP>(smem, acc, m, L, lane);
    }
    if (owner && rok) {
        const float f = L > 0.0f ? vd / L : 0.0f;  // v_descale: fp32, behind the product
        if constexpr (SPLIT) {
            const int64_t rows_all = (int64_t)p.B * p.Hkv * p.R;
            paged_store_part<DP>(p.part, (int64_t)p.nsplit * rows_all, (int64_t)part * rows_all + (int64_t)bk * p.R + r, acc, f, m, L, hi);
        } else {
            paged_store_out<DP, OUT>(p.out, (((int64_t)b * p.Sq + qi) * p.H + h) * DP, p.lse, ((int64_t)b * p.H + h) * p.Sq + qi, acc, f, m, L,
                                     hi);
        }
    }
}

// the quantising append: row i of k_new / v_new of sequence b goes to cache position clamp(cache_seqlens[b]) + i through the block table
// as e4m3fn_rne(clamp(x / descale, -448, 448)).  Rows past the capacity and rows of pages the table does not hold are dropped.  One thread
// per 16 output bytes (32 input bytes), vector stores only.
template <typename T>
__global__ __launch_bounds__(256) void fa_paged_fp8_append_kernel(PagedFp8Params pp) {
    const PagedParams& p = pp.p;
    const uint32_t nch = p.D / 16;
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
    const T* src = (const T*)(isv ? p.vn : p.kn) +
                   (isv ? (int64_t)b * p.vnb + (int64_t)i * p.vnt + (int64_t)hk * p.vnh : (int64_t)b * p.knb + (int64_t)i * p.knt + (int64_t)hk * p.knh);
    uint8_t* dst = (uint8_t*)(isv ? p.vc : p.kc) +
                   (isv ? (int64_t)pg * p.vpg + (int64_t)rip * p.vst + (int64_t)hk * p.vsh : (int64_t)pg * p.kpg + (int64_t)rip * p.kst + (int64_t)hk * p.ksh);
    const float d = isv ? pp.vd[(int64_t)b * pp.vdb + (int64_t)hk * pp.vdh] : pp.kd[(int64_t)b * pp.kdb + (int64_t)hk * pp.kdh];
    typedef T T8 __attribute__((ext_vector_type(8)));
    const T8 x0 = *(const T8*)(src + 16 * c), x1 = *(const T8*)(src + 16 * c + 8);
    float y[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        y[j] = fminf(fmaxf(__fdiv_rn((float)x0[j], d), -448.0f), 448.0f);
        y[8 + j] = fminf(fmaxf(__fdiv_rn((float)x1[j], d), -448.0f), 448.0f);
    }
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        int v = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w], y[4 * w + 1], 0, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w + 2], y[4 * w + 3], v, true);
        o[w] = (unsigned)v;
    }
    *(u32x4*)(dst + 16 * c) = o;
}

// Scope: bf16 / fp16 q and new tokens, head_dim 64 / 128, H a multiple of H_kv, q / k_new / v_new strides multiples of 8 elements, cache
// strides multiples of 16 bytes and rows that do not overlap inside a head, 16-byte aligned bases, 4-byte aligned descales with
// non-negative strides, page_size a multiple of 16 with a block table, and one page (+ the 16 rows a piece may run past a static row)
// inside a 32-bit buffer offset.
bool paged_fp8_supported(const PagedFp8Params& q) {
    const PagedParams& p = q.p;
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if (p.D != 64 && p.D != 128) return false;
    if (p.H == 0 || p.Hkv == 0 || p.H % p.Hkv || p.B == 0) return false;
    if (p.page_size == 0 || (p.bt && p.page_size % 16) || p.num_pages == 0 || p.max_pages == 0) return false;
    if (!p.bt && (p.max_pages != 1 || p.num_pages < p.B)) return false;
    if ((uint64_t)p.max_pages * p.page_size >= (1ull << 31) || p.num_pages >= (1u << 31)) return false;
    const int64_t sq[3] = {p.qsb, p.qst, p.qsh};
    for (int64_t s : sq)
        if (s < 0 || s % 8) return false;
    const int64_t sc[6] = {p.kpg, p.kst, p.ksh, p.vpg, p.vst, p.vsh};
    for (int64_t s : sc)
        if (s < 0 || s % 16) return false;
    if (p.kst < (int64_t)p.D || p.vst < (int64_t)p.D) return false;
    if (p.Snew) {
        const int64_t sn[6] = {p.knb, p.knt, p.knh, p.vnb, p.vnt, p.vnh};
        for (int64_t s : sn)
            if (s < 0 || s % 8) return false;
        if (!p.kn || !p.vn || ((uintptr_t)p.kn & 15) || ((uintptr_t)p.vn & 15)) return false;
        if ((uint64_t)p.B * p.Snew * p.Hkv * (p.D / 16) * 2 >= (1ull << 40)) return false;
    }
    auto al16 = [](const void* x) { return ((uintptr_t)x & 15) == 0; };
    if (!p.q || !p.kc || !p.vc || !p.seqlens || !al16(p.q) || !al16(p.kc) || !al16(p.vc)) return false;
    if (!q.kd || !q.vd || ((uintptr_t)q.kd & 3) || ((uintptr_t)q.vd & 3) || q.kdb < 0 || q.kdh < 0 || q.vdb < 0 || q.vdh < 0) return false;
    const uint64_t lim = 1ull << 31;
    if (((uint64_t)p.page_size + 16) * (uint64_t)p.kst >= lim || ((uint64_t)p.page_size + 16) * (uint64_t)p.vst >= lim) return false;
    return (uint64_t)p.B * p.Hkv * p.nrb * (p.nsplit ? p.nsplit : 1) < lim;
}

hipError_t launch_paged_fp8_append(const PagedFp8Params& q, hipStream_t stream) {
    if (!paged_fp8_supported(q)) return hipErrorInvalidValue;
    const PagedParams& p = q.p;
    const uint64_t total = (uint64_t)p.B * p.Snew * p.Hkv * (p.D / 16) * 2;
    if (total == 0) return hipSuccess;
    const dim3 grid((uint32_t)((total + 255) / 256));
    if (p.in_prec == P_BF16)
        hipLaunchKernelGGL(fa_paged_fp8_append_kernel<__bf16>, grid, dim3(256), 0, stream, q);
    else
        hipLaunchKernelGGL(fa_paged_fp8_append_kernel<_Float16>, grid, dim3(256), 0, stream, q);
    return hipGetLastError();
}

template <typename T, bool CAUSAL, int DP, typename OUT>
static hipError_t launch_fwd16_paged_fp8_t(const PagedFp8Params& q, hipStream_t stream) {
    const PagedParams& p = q.p;
    const size_t lds = (size_t)DP * (512 + 256 * FP8_NS);  // the 16-bit image of K and V + the fp8 ring
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_paged_fp8_kernel<T, CAUSAL, DP, OUT>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((fa_fwd16_paged_fp8_kernel<T, CAUSAL, DP, OUT>), dim3(p.B * p.Hkv * p.nrb * p.nsplit), dim3(256), lds, stream, q);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (std::is_same<OUT, void>::value) return launch_paged_fold(p, stream);
    return hipSuccess;
}

template <typename T, int DP>
static hipError_t launch_fwd16_paged_fp8_d(const PagedFp8Params& q, hipStream_t stream) {
    const PagedParams& p = q.p;
    const bool f32 = p.out_prec == P_FP32;
    if (p.nsplit > 1)
        return p.causal ? launch_fwd16_paged_fp8_t<T, true, DP, void>(q, stream) : launch_fwd16_paged_fp8_t<T, false, DP, void>(q, stream);
    if (p.causal) return f32 ? launch_fwd16_paged_fp8_t<T, true, DP, float>(q, stream) : launch_fwd16_paged_fp8_t<T, true, DP, T>(q, stream);
    return f32 ? launch_fwd16_paged_fp8_t<T, false, DP, float>(q, stream) : launch_fwd16_paged_fp8_t<T, false, DP, T>(q, stream);
}

// p.nsplit > 1: p.part holds nsplit B H_kv R (D + 2) floats
hipError_t launch_fwd_16_paged_fp8(const PagedFp8Params& q, hipStream_t stream, const char** name) {
    const PagedParams& p = q.p;
    if (!paged_fp8_supported(q) || !paged_fwd_args_ok(p)) return hipErrorInvalidValue;
    if (p.nsplit > 1 && !p.part) return hipErrorInvalidValue;
    static const char* const names[2][2][2][2] = {
        {{{"fa_fwd16_paged_fp8<fp16,64>", "fa_fwd16_paged_fp8<fp16,64,split>"},
          {"fa_fwd16_paged_fp8<fp16,64,causal>", "fa_fwd16_paged_fp8<fp16,64,causal,split>"}},
         {{"fa_fwd16_paged_fp8<fp16,128>", "fa_fwd16_paged_fp8<fp16,128,split>"},
          {"fa_fwd16_paged_fp8<fp16,128,causal>", "fa_fwd16_paged_fp8<fp16,128,causal,split>"}}},
        {{{"fa_fwd16_paged_fp8<bf16,64,pv16>", "fa_fwd16_paged_fp8<bf16,64,pv16,split>"},
          {"fa_fwd16_paged_fp8<bf16,64,causal,pv16>", "fa_fwd16_paged_fp8<bf16,64,causal,pv16,split>"}},
         {{"fa_fwd16_paged_fp8<bf16,128,pv16>", "fa_fwd16_paged_fp8<bf16,128,pv16,split>"},
          {"fa_fwd16_paged_fp8<bf16,128,causal,pv16>", "fa_fwd16_paged_fp8<bf16,128,causal,pv16,split>"}}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.causal != 0][p.nsplit > 1];
    if ((uint64_t)p.B * p.H * p.Sq == 0) return hipSuccess;
    if (p.D == 64) return bf ? launch_fwd16_paged_fp8_d<__bf16, 64>(q, stream) : launch_fwd16_paged_fp8_d<_Float16, 64>(q, stream);
    return bf ? launch_fwd16_paged_fp8_d<__bf16, 128>(q, stream) : launch_fwd16_paged_fp8_d<_Float16, 128>(q, stream);
}

}  // namespace umfa
