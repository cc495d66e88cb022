// fa_fwd_16_paged_varlen_fp8.hip -- packed variable-length queries (cu_seqlens_q) over an OCP fp8 (e4m3fn) paged or static KV cache:
// the forward, the packed quantising append and the packed fp8 rotary pre-pass.  Semantics: fa_paged_varlen_fp8.h (layout, clamps,
// work items and memory safety: fa_paged_varlen.h; bytes and arithmetic: fa_paged_fp8.h; rotary: fa_paged_rope.h).
// runtime_paged_varlen.hip drives it.
//
// The forward is fa_fwd16_paged_fp8_kernel's body (fa_fwd_16_paged_fp8.hip: the ring of two fp8 stages filled by LDS-DMA in pieces
// private to the requesting wave and awaited with a counted vmcnt, the exact expansion into d_off<DP>'s 16-bit image, two barriers a
// step, the block table read 64 groups per vector load, k_descale folded into scale log2(e) and v_descale into 1 / l) under
// fa_fwd16_paged_varlen_kernel's coordinates (fa_fwd_16_paged_varlen.hip: one scalar load of the item {sequence, hk * blocks + row
// block}, varlen_range, paged_varlen_lens, the form chosen per item from R = g L_q -- decode form ks4 for R <= 32, else 128 rows --
// rows at start + token, the packed split partials, the decode / 128-row tally in `counts`).  The stage ring's device pieces are the
// fp8 unit's own (fa_paged_fp8.h); the item-list pre-pass and the packed fold are the 16-bit packed unit's kernels, launched through
// its host launchers (the partials are fp32 rows in the same packed order whatever the cache's format).  With every L_q equal the
// arithmetic, and its order, is fa_fwd16_paged_fp8_kernel's: the results are bitwise the same.
//
// LDS: 128 KiB (D = 128, one workgroup per CU), 64 KiB (D = 64, two) -- the fp8 kernel's.  No bf16-V range machinery: nothing can leave
// fp16's range (fa_fwd_16_paged_fp8.hip's header).
#include <type_traits>

#include "fa_paged_varlen_fp8.h"
#include "fa_paged_rope_device.h"
#include "fa_paged_device.h"
#include "kernels.h"

namespace umfa {

template <typename T, bool CAUSAL, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_varlen_fp8_kernel(PagedVarlenFp8Params f) {
    BWD16_GEO(DP);
    (void)TILE_PIECES, (void)PD;
    const PagedVarlenParams& v = f.v;
    const PagedParams& p = v.p;
    constexpr int NS = 2;                    // fp8 stages in the ring
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
    // this workgroup's item (fa_paged_varlen_items_kernel): {sequence or -1, hk * blocks + row block}; one scalar load
    const int it_b = __builtin_amdgcn_readfirstlane(v.items[2 * (size_t)item]);
    const uint32_t it_j = (uint32_t)__builtin_amdgcn_readfirstlane(v.items[2 * (size_t)item + 1]);
    if (it_b < 0 || (uint32_t)it_b >= p.B) return;  // past the end of the list
    const uint32_t b = (uint32_t)it_b;
    const uint32_t g = p.H / p.Hkv;
    uint32_t q0, Lq;
    varlen_range(v.cu, b, v.Tq, p.Sq, q0, Lq);
    const uint32_t R = g * Lq;  // rows per KV head of this sequence
    if (R == 0) return;
    const bool ks4 = R <= 32;  // the decode form, from the item's own L_q
    const uint32_t nrb = ks4 ? 1u : (R + 127) / 128;
    const uint32_t hk = it_j / nrb, rb = it_j % nrb;
    if (hk >= p.Hkv) return;  // (cu rewritten between the pre-pass and this launch: nothing to do safely)
    // debug tally of the forms this launch ran (umfa_varlen_kvcache_item_counts): one atomic per item
    if (part == 0 && threadIdx.x == 0) atomicAdd(v.counts + (ks4 ? 0 : 1), 1u);
    uint32_t L0u, Lku;
    paged_varlen_lens(v, b, Lq, L0u, Lku);
    const uint32_t Lk = (uint32_t)__builtin_amdgcn_readfirstlane((int)Lku);
    const int off = (int)Lk - (int)Lq;  // bottom-right causal: token i sees keys j <= i + off
    const uint32_t wr0 = ks4 ? 0u : rb * 128 + (uint32_t)uw * 32;  // this wave's first row
    const uint32_t r = wr0 + ql;
    const bool rok = r < R;
    const uint32_t qi = r / g, h = hk * g + r % g;
    const bool wlive = wr0 < R;
    const uint32_t wlast = wlive ? (wr0 + 32 < R ? wr0 + 31 : R - 1) : 0u;
    const int kl_first = (int)(wr0 / g) + off, kl_last = (int)(wlast / g) + off;  // causal limits of the wave's first / last rows
    uint32_t Le = Lk;  // keys the workgroup sees: [0, Le)
    if (CAUSAL) {
        const uint32_t rend = ks4 ? R : (rb * 128 + 128 < R ? rb * 128 + 128 : R);
        const int last = (int)((rend - 1) / g) + off;
        Le = last < 0 ? 0u : ((uint32_t)last + 1 < Lk ? (uint32_t)last + 1 : Lk);
    }
    const uint32_t nst = (Le + 127) / 128, per = (nst + p.nsplit - 1) / p.nsplit;
    const uint32_t s0 = part * per, s1 = s0 + per < nst ? s0 + per : nst;
    const float kd = f.kd[(int64_t)b * f.kdb + (int64_t)hk * f.kdh], vd = f.vd[(int64_t)b * f.vdb + (int64_t)hk * f.vdh];

    typename Mma16<T>::V8 qf[NKS];
    paged_load_q<T, DP>(qf, (const T*)p.q + (int64_t)(q0 + qi) * p.qst + (int64_t)h * p.qsh, rok, hi);
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
        expand(slot);  // (the image is free: every wave passed the previous step's second barrier)
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the stage's bytes are in registers before its pieces are requested again
        if (st + NS < s1) stage(st + NS, slot, tab_of(st + NS));
        __syncthreads();
        if (ks4 || wlive) {
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
        const float fo = L > 0.0f ? vd / L : 0.0f;  // v_descale: fp32, behind the product
        if constexpr (SPLIT) {
            const int64_t rows_all = (int64_t)v.Tq * p.H;  // the packed partial layout (fa_paged_varlen.h)
            paged_store_part<DP>(p.part, (int64_t)p.nsplit * rows_all, (int64_t)part * rows_all + (int64_t)q0 * p.H + (int64_t)hk * R + r, acc, fo,
                                 m, L, hi);
        } else {
            paged_store_out<DP, OUT>(p.out, ((int64_t)(q0 + qi) * p.H + h) * DP, p.lse, (int64_t)h * v.Tq + q0 + qi, acc, fo, m, L, hi);
        }
    }
}

// the packed quantising append: row t of k_new / v_new belongs to the sequence b whose query range holds it and goes to cache position
// clamp(cache_seqlens[b]) + (t - cu[b]) through the block table as e4m3fn_rne(clamp(x / descale[b, h_kv], -448, 448)).  Rows no sequence
// covers, rows past the capacity and rows of pages the table does not hold are dropped (fa_paged_varlen_append_kernel's rules).  One
// thread per 16 output bytes (32 input bytes), vector stores only.
template <typename T>
__global__ __launch_bounds__(256) void fa_paged_varlen_fp8_append_kernel(PagedVarlenFp8Params f) {
    const PagedVarlenParams& v = f.v;
    const PagedParams& p = v.p;
    typedef T T8 __attribute__((ext_vector_type(8)));
    const uint32_t nch = p.D / 16;
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = (uint64_t)v.Tq * p.Hkv * nch * 2;
    if (idx >= total) return;
    uint64_t x = idx;
    const uint32_t c = (uint32_t)(x % nch); x /= nch;
    const uint32_t hk = (uint32_t)(x % p.Hkv); x /= p.Hkv;
    const uint32_t t = (uint32_t)(x % v.Tq);
    const bool isv = x / v.Tq != 0;
    uint32_t b, q0, Lq;
    if (!paged_varlen_find(v, t, b, q0, Lq)) return;
    uint32_t L0, Lk;
    paged_varlen_lens(v, b, Lq, L0, Lk);
    const uint32_t pos = L0 + (t - q0);
    if (pos >= p.max_pages * p.page_size) return;
    const uint32_t lp = paged_lpage(p, pos);
    const int pg = paged_page(p, b, lp);
    if (pg < 0) return;
    const uint32_t rip = pos - lp * p.page_size;
    const T* src = (const T*)(isv ? p.vn : p.kn) + (isv ? (int64_t)t * p.vnt + (int64_t)hk * p.vnh : (int64_t)t * p.knt + (int64_t)hk * p.knh);
    uint8_t* dst = (uint8_t*)(isv ? p.vc : p.kc) +
                   (isv ? (int64_t)pg * p.vpg + (int64_t)rip * p.vst + (int64_t)hk * p.vsh : (int64_t)pg * p.kpg + (int64_t)rip * p.kst + (int64_t)hk * p.ksh);
    const float d = isv ? f.vd[(int64_t)b * f.vdb + (int64_t)hk * f.vdh] : f.kd[(int64_t)b * f.kdb + (int64_t)hk * f.kdh];
    *(U4*)(dst + 16 * c) = quant16(*(const T8*)(src + 16 * c), *(const T8*)(src + 16 * c + 8), d);
}

// the packed fp8 rotary pre-pass (fa_paged_rope_kernel's packed form over an fp8 cache): one launch rotates q into the dense image,
// rotates k_new, rounds it once to T and quantises it into the cache, and quantises v_new unrotated.  One thread per 16 bytes written:
// 8 elements of the q image, 16 of a cache row.  T: operand type; TT: table type (float or T); interleaved / rotary_dim / causal at run
// time.
template <typename T, typename TT>
__global__ __launch_bounds__(256) void fa_paged_varlen_fp8_rope_kernel(PagedVarlenFp8RopeParams r) {
    const PagedVarlenFp8Params& f = r.f;
    const PagedVarlenParams& v = f.v;
    const PagedParams& p = v.p;
    typedef T T8 __attribute__((ext_vector_type(8)));
    const uint32_t nch = p.D / 8, nkv = p.D / 16;
    const uint64_t nq = (uint64_t)v.Tq * p.H * nch, nk = (uint64_t)v.Tq * p.Hkv * nkv;
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nq + 2 * nk) return;
    if (idx < nq) {
        // Q: rotate into the dense image; a row no sequence covers is copied (the attention never uses it)
        uint64_t x = idx;
        const uint32_t c = (uint32_t)(x % nch); x /= nch;
        const uint32_t h = (uint32_t)(x % p.H); x /= p.H;
        const uint32_t t = (uint32_t)x;
        uint32_t b, q0, Lq, L0 = 0, Lk;
        const bool rotate = paged_varlen_find(v, t, b, q0, Lq);
        if (rotate) paged_varlen_lens(v, b, Lq, L0, Lk);
        const uint32_t pos = L0 + (p.causal && rotate ? t - q0 : 0u);
        const T* src = (const T*)p.q + (int64_t)t * p.qst + (int64_t)h * p.qsh;
        T* dst = (T*)r.qimg + ((int64_t)t * p.H + h) * p.D + 8 * c;
        *(T8*)dst = rotate ? rope_chunk<T, TT>(r, src, 8 * c, pos) : *(const T8*)(src + 8 * c);
        return;
    }
    // K (rotated) and V: the quantising append's work
    uint64_t x = idx - nq;
    const uint32_t c = (uint32_t)(x % nkv); x /= nkv;
    const uint32_t hk = (uint32_t)(x % p.Hkv); x /= p.Hkv;
    const bool isv = x >= v.Tq;
    const uint32_t t = (uint32_t)(isv ? x - v.Tq : x);
    uint32_t b, q0, Lq, L0, Lk;
    if (!paged_varlen_find(v, t, b, q0, Lq)) return;
    paged_varlen_lens(v, b, Lq, L0, Lk);
    const uint32_t pos = L0 + (t - q0);
    if (pos >= p.max_pages * p.page_size) return;
    const uint32_t lp = paged_lpage(p, pos);
    const int pg = paged_page(p, b, lp);
    if (pg < 0) return;
    const uint32_t rip = pos - lp * p.page_size;
    const T* src = (const T*)(isv ? p.vn : p.kn) + (isv ? (int64_t)t * p.vnt + (int64_t)hk * p.vnh : (int64_t)t * p.knt + (int64_t)hk * p.knh);
    uint8_t* dst = (uint8_t*)(isv ? p.vc : p.kc) +
                   (isv ? (int64_t)pg * p.vpg + (int64_t)rip * p.vst + (int64_t)hk * p.vsh : (int64_t)pg * p.kpg + (int64_t)rip * p.kst + (int64_t)hk * p.ksh);
    const float d = isv ? f.vd[(int64_t)b * f.vdb + (int64_t)hk * f.vdh] : f.kd[(int64_t)b * f.kdb + (int64_t)hk * f.kdh];
    T8 x0, x1;
    if (isv) {
        x0 = *(const T8*)(src + 16 * c);
        x1 = *(const T8*)(src + 16 * c + 8);
    } else {
        x0 = rope_chunk<T, TT>(r, src, 16 * c, pos);
        x1 = rope_chunk<T, TT>(r, src, 16 * c + 8, pos);
    }
    *(U4*)(dst + 16 * c) = quant16(x0, x1, d);
}

// Scope: paged_fp8_supported's (fa_fwd_16_paged_fp8.hip) for the operands, the caches (byte strides, multiples of 16), the table and the
// descales, plus paged_varlen_supported's packed rules: 32-bit row counts, no batch strides, has_new 0 / 1 and an item list of
// paged_varlen_item_bound entries.
bool paged_varlen_fp8_supported(const PagedVarlenFp8Params& f) {
    const PagedVarlenParams& v = f.v;
    const PagedParams& p = v.p;
    PagedFp8Params d;
    d.p = p;
    d.p.nrb = 1;  // (the grid is checked below, from the item bound)
    d.kd = f.kd; d.vd = f.vd; d.kdb = f.kdb; d.kdh = f.kdh; d.vdb = f.vdb; d.vdh = f.vdh;
    if (!paged_fp8_supported(d) || !v.cu || ((uintptr_t)v.cu & 3)) return false;
    if (p.Snew > 1 || p.qsb || p.knb || p.vnb) return false;
    const uint64_t g = p.H / p.Hkv;
    if (g * p.Sq >= (1ull << 31) || (uint64_t)v.Tq * p.H >= (1ull << 31) || v.Tq >= (1u << 30) || p.Sq > v.Tq) return false;
    if ((uint64_t)v.Tq * p.Hkv * (p.D / 16) * 2 >= (1ull << 40)) return false;
    if (v.n_items != paged_varlen_item_bound(v)) return false;
    return (uint64_t)v.n_items * (p.nsplit ? p.nsplit : 1) < (1ull << 31);
}

hipError_t launch_paged_varlen_fp8_append(const PagedVarlenFp8Params& f, hipStream_t stream) {
    if (!paged_varlen_fp8_supported(f) || !f.v.p.Snew) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)f.v.Tq * f.v.p.Hkv * (f.v.p.D / 16) * 2;
    if (total == 0) return hipSuccess;
    const dim3 grid((uint32_t)((total + 255) / 256));
    if (f.v.p.in_prec == P_BF16)
        hipLaunchKernelGGL(fa_paged_varlen_fp8_append_kernel<__bf16>, grid, dim3(256), 0, stream, f);
    else
        hipLaunchKernelGGL(fa_paged_varlen_fp8_append_kernel<_Float16>, grid, dim3(256), 0, stream, f);
    return hipGetLastError();
}

static uint64_t rope8_threads(const PagedVarlenFp8RopeParams& r) {
    const PagedParams& p = r.f.v.p;
    return (uint64_t)r.f.v.Tq * p.H * (p.D / 8) + 2 * (uint64_t)r.f.v.Tq * p.Hkv * (p.D / 16);
}

// Scope (on top of paged_varlen_fp8_supported, which the runtime has checked): paged_rope_supported's rules for the tables, the q image
// and the grid, in the packed form over an fp8 cache.
bool paged_varlen_fp8_rope_supported(const PagedVarlenFp8RopeParams& r) {
    const PagedParams& p = r.f.v.p;
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if ((p.D != 64 && p.D != 128) || p.Hkv == 0 || p.H % p.Hkv) return false;
    if (!p.Snew || !p.kn || !p.vn || !p.q) return false;
    if (r.rdim < 16 || r.rdim > p.D || r.rdim % 16) return false;
    if (r.seqlen_ro == 0 || r.seqlen_ro >= (1u << 31)) return false;
    const int64_t tb = r.table_f32 ? 4 : 2;
    if (!r.cos || !r.sin || ((uintptr_t)r.cos & 15) || ((uintptr_t)r.sin & 15)) return false;
    if (r.rstride < (int64_t)(r.rdim / 2) || (r.rstride * tb) % 16) return false;
    if (!r.qimg || ((uintptr_t)r.qimg & 15)) return false;
    if (!r.f.kd || !r.f.vd || !r.f.v.cu || p.qsb || p.knb || p.vnb) return false;
    return rope8_threads(r) < (1ull << 39);
}

hipError_t launch_paged_varlen_fp8_rope(const PagedVarlenFp8RopeParams& r, hipStream_t stream) {
    if (!paged_varlen_fp8_rope_supported(r)) return hipErrorInvalidValue;
    const uint64_t total = rope8_threads(r);
    if (total == 0) return hipSuccess;
    const dim3 grid((uint32_t)((total + 255) / 256));
    if (r.f.v.p.in_prec == P_BF16) {
        if (r.table_f32)
            hipLaunchKernelGGL((fa_paged_varlen_fp8_rope_kernel<__bf16, float>), grid, dim3(256), 0, stream, r);
        else
            hipLaunchKernelGGL((fa_paged_varlen_fp8_rope_kernel<__bf16, __bf16>), grid, dim3(256), 0, stream, r);
    } else {
        if (r.table_f32)
            hipLaunchKernelGGL((fa_paged_varlen_fp8_rope_kernel<_Float16, float>), grid, dim3(256), 0, stream, r);
        else
            hipLaunchKernelGGL((fa_paged_varlen_fp8_rope_kernel<_Float16, _Float16>), grid, dim3(256), 0, stream, r);
    }
    return hipGetLastError();
}

template <typename T, bool CAUSAL, int DP, typename OUT>
static hipError_t launch_fwd16_paged_varlen_fp8_t(const PagedVarlenFp8Params& f, hipStream_t stream) {
    const size_t lds = (size_t)DP * (512 + 256 * 2);  // the 16-bit image of K and V + the ring of two fp8 stages
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_paged_varlen_fp8_kernel<T, CAUSAL, DP, OUT>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((fa_fwd16_paged_varlen_fp8_kernel<T, CAUSAL, DP, OUT>), dim3(f.v.n_items * f.v.p.nsplit), dim3(256), lds, stream, f);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (std::is_same<OUT, void>::value) return launch_paged_varlen_fold(f.v, stream);
    return hipSuccess;
}

template <typename T, int DP>
static hipError_t launch_fwd16_paged_varlen_fp8_d(const PagedVarlenFp8Params& f, hipStream_t stream) {
    const PagedParams& p = f.v.p;
    const bool f32 = p.out_prec == P_FP32;
    if (p.nsplit > 1)
        return p.causal ? launch_fwd16_paged_varlen_fp8_t<T, true, DP, void>(f, stream) : launch_fwd16_paged_varlen_fp8_t<T, false, DP, void>(f, stream);
    if (p.causal) return f32 ? launch_fwd16_paged_varlen_fp8_t<T, true, DP, float>(f, stream) : launch_fwd16_paged_varlen_fp8_t<T, true, DP, T>(f, stream);
    return f32 ? launch_fwd16_paged_varlen_fp8_t<T, false, DP, float>(f, stream) : launch_fwd16_paged_varlen_fp8_t<T, false, DP, T>(f, stream);
}

// the item-list pre-pass, the forward and (p.nsplit > 1: p.part holds nsplit T_q H (D + 2) floats) the fold
hipError_t launch_fwd_16_paged_varlen_fp8(const PagedVarlenFp8Params& f, hipStream_t stream, const char** name) {
    const PagedVarlenParams& v = f.v;
    const PagedParams& p = v.p;
    if (!paged_varlen_fp8_supported(f) || !p.out || ((uintptr_t)p.out & 15) || ((uintptr_t)p.lse & 3) || p.nsplit == 0) return hipErrorInvalidValue;
    if (p.out_prec != P_FP32 && p.out_prec != p.in_prec) return hipErrorInvalidValue;
    if (p.nsplit > 1 && !p.part) return hipErrorInvalidValue;
    if (v.n_items && (!v.items || ((uintptr_t)v.items & 7) || !v.counts || ((uintptr_t)v.counts & 15))) return hipErrorInvalidValue;
    static const char* const names[2][2][2][2] = {
        {{{"fa_fwd16_paged_varlen_fp8<fp16,64>", "fa_fwd16_paged_varlen_fp8<fp16,64,split>"},
          {"fa_fwd16_paged_varlen_fp8<fp16,64,causal>", "fa_fwd16_paged_varlen_fp8<fp16,64,causal,split>"}},
         {{"fa_fwd16_paged_varlen_fp8<fp16,128>", "fa_fwd16_paged_varlen_fp8<fp16,128,split>"},
          {"fa_fwd16_paged_varlen_fp8<fp16,128,causal>", "fa_fwd16_paged_varlen_fp8<fp16,128,causal,split>"}}},
        {{{"fa_fwd16_paged_varlen_fp8<bf16,64,pv16>", "fa_fwd16_paged_varlen_fp8<bf16,64,pv16,split>"},
          {"fa_fwd16_paged_varlen_fp8<bf16,64,causal,pv16>", "fa_fwd16_paged_varlen_fp8<bf16,64,causal,pv16,split>"}},
         {{"fa_fwd16_paged_varlen_fp8<bf16,128,pv16>", "fa_fwd16_paged_varlen_fp8<bf16,128,pv16,split>"},
          {"fa_fwd16_paged_varlen_fp8<bf16,128,causal,pv16>", "fa_fwd16_paged_varlen_fp8<bf16,128,causal,pv16,split>"}}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.causal != 0][p.nsplit > 1];
    if (v.n_items == 0) return hipSuccess;  // (T_q = 0 or max_seqlen_q = 0: no row exists)
    if (hipError_t e = launch_paged_varlen_items(v, stream); e != hipSuccess) return e;
    if (p.D == 64) return bf ? launch_fwd16_paged_varlen_fp8_d<__bf16, 64>(f, stream) : launch_fwd16_paged_varlen_fp8_d<_Float16, 64>(f, stream);
    return bf ? launch_fwd16_paged_varlen_fp8_d<__bf16, 128>(f, stream) : launch_fwd16_paged_varlen_fp8_d<_Float16, 128>(f, stream);
}

}  // namespace umfa
