// fa_fwd_16_paged_varlen_window.hip -- bf16 / fp16 MFMA forward of packed variable-length queries (cu_seqlens_q) over a paged or static
// KV cache with a sliding window (flash-attention's window_size), head_dim 64 / 128, GQA.  Semantics: fa_paged_varlen_window.h; layout,
// memory safety and the work distribution: fa_paged_varlen.h.
//
// fa_fwd16_paged_varlen_kernel's shell (fa_fwd_16_paged_varlen.hip: the item read from the list with one scalar load, the sequence's
// query range from cu_seqlens_q, the decode form (ks4: R = g L_q <= 32) or the 128-row form decided from the item's own L_q, rows
// cu[b] + token, the packed split partials, the tally of the forms) over the shared device pieces of fa_paged_device.h, with the banded
// sweep of fa_fwd_16_paged_window.hip: token i of sequence b sees keys [i + off - left, i + off + right], off = L_k,b - L_q,b, the
// bounds runtime values (no causal instantiation).
//
// Step range, per item: with first_tok / last_tok the query tokens of the item's first and last live rows, k_first = max(0, first_tok +
// off - left) and k_last = min(L_k - 1, last_tok + off + right); the item visits the steps [k_first / 128, k_last / 128 + 1), none when
// k_last < k_first.  Split-KV parts divide THAT range (one part count per launch), so the cost of a call follows the band, not the
// context.  An item or part whose range is empty stages nothing and writes O = 0, LSE = -inf (a part: m = -inf, l = 0).
//
// Per wave, the zero landing of keys outside [k_first, k_last] and the block-table entries that are never read:
// fa_fwd_16_paged_window.hip, word for word.  With every L_q equal the arithmetic, and its order, is that of
// fa_fwd16_paged_window_kernel: the results are bitwise the same.
#include <type_traits>

#include "fa_paged_varlen_window.h"
#include "fa_paged_device.h"
#include "kernels.h"

namespace umfa {

template <typename T, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_varlen_window_kernel(PagedVarlenWindowParams vw) {
    const PagedVarlenParams& v = vw.v;
    const PagedParams& p = v.p;
    BWD16_GEO(DP);
    (void)TILE_PIECES, (void)PD;
    constexpr int STAGE_B = 4 * TILE_BYTES;  // one step (128 keys) of K or of V
    constexpr bool VCONV = std::is_same<T, __bf16>::value;
    constexpr bool SPLIT = std::is_same<OUT, void>::value;
    extern __shared__ __attribute__((aligned(16))) char smem[];
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
    const int off = (int)Lk - (int)Lq;
    const int lo_off = off - vw.win_left, hi_off = off + vw.win_right;  // token i sees keys [i + lo_off, i + hi_off] (and < L_k)
    const uint32_t wr0 = ks4 ? 0u : rb * 128 + (uint32_t)uw * 32;  // this wave's first row
    const uint32_t r = wr0 + ql;
    const bool rok = r < R;
    const uint32_t qi = r / g, h = hk * g + r % g;
    const bool wlive = wr0 < R;
    const uint32_t wlast = wlive ? (wr0 + 32 < R ? wr0 + 31 : R - 1) : 0u;
    // the band of the wave's first row [wlo_first, whi_first] and of its last row [wlo_last, whi_last]
    const int wlo_first = (int)(wr0 / g) + lo_off, whi_first = (int)(wr0 / g) + hi_off;
    const int wlo_last = (int)(wlast / g) + lo_off, whi_last = (int)(wlast / g) + hi_off;
    // the item's keys [kfirst, Le) = [k_first, k_last + 1), and its steps [ws_lo, ws_hi); all zero when it sees no key
    const uint32_t row0 = ks4 ? 0u : rb * 128, rend = ks4 ? R : (rb * 128 + 128 < R ? rb * 128 + 128 : R);
    const int k_first = (int)(row0 / g) + lo_off > 0 ? (int)(row0 / g) + lo_off : 0;
    const int k_last = (int)((rend - 1) / g) + hi_off < (int)Lk - 1 ? (int)((rend - 1) / g) + hi_off : (int)Lk - 1;
    const bool any = k_last >= k_first;
    const uint32_t kfirst = any ? (uint32_t)k_first : 0u, Le = any ? (uint32_t)k_last + 1 : 0u;
    const uint32_t ws_lo = kfirst / 128, ws_hi = any ? (uint32_t)k_last / 128 + 1 : ws_lo;
    const uint32_t per = (ws_hi - ws_lo + p.nsplit - 1) / p.nsplit;  // the parts divide the band's steps
    const uint32_t s0r = ws_lo + part * per, s0 = s0r < ws_hi ? s0r : ws_hi, s1 = s0 + per < ws_hi ? s0 + per : ws_hi;

    typename Mma16<T>::V8 qf[NKS];
    paged_load_q<T, DP>(qf, (const T*)p.q + (int64_t)(q0 + qi) * p.qst + (int64_t)h * p.qsh, rok, hi);
    const float c = p.scale * UMFA_LOG2E;
    const int lim_lo = (int)qi + lo_off, lim_hi = (int)qi + hi_off;
    const uint32_t tst_k = (uint32_t)p.kst * 2, tst_v = (uint32_t)p.vst * 2;
    const int64_t kpage_b = p.kpg * 2, vpage_b = p.vpg * 2, khead_b = (int64_t)hk * p.ksh * 2, vhead_b = (int64_t)hk * p.vsh * 2;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((LDS_AS char*)smem));
    const int tr_qq = (lane >> 2) & 3, tr_pp = lane & 3, tr_g1 = (lane >> 4) & 1;

    auto stage = [&](uint32_t s, int par, int pgv) __attribute__((always_inline)) {
        paged_dma_step<DP>(p, (const char*)p.kc, kpage_b, khead_b, tst_k, pgv, kfirst, Le, s, lds0 + par * STAGE_B, uw, lane);
        paged_dma_step<DP>(p, (const char*)p.vc, vpage_b, vhead_b, tst_v, pgv, kfirst, Le, s, lds0 + 2 * STAGE_B + par * STAGE_B, uw, lane);
    };
    unsigned vamax = 0;  // bf16: the largest |v| (bits) this thread converted
    auto convert = [&](int par, float vmul) __attribute__((always_inline)) {
        if constexpr (VCONV) paged_convert_v<DP>(smem + 2 * STAGE_B + par * STAGE_B, vmul, vamax, uw, lane);
    };

    int vexp = 0;
    for (int pass = 0;; ++pass) {  // (bf16: the range rule's second sweep restarts at the item's first band step, s0)
        const float vmul = __uint_as_float((unsigned)(127 - vexp) << 23);
        f32x16 acc[NDB];
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[i][rr] = 0.0f;
        float m = -INFINITY, l = 0.0f;  // running max of c S (log2 domain, shared by the halves), this half's sum of P

        int pg_a = paged_table(p, b, kfirst, Le, s0, lane), pg_b = paged_table(p, b, kfirst, Le, s0 + 1, lane);  // steps st, st + 1
        if (s0 < s1) stage(s0, 0, pg_a);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if (s0 < s1) convert(0, vmul);
        __syncthreads();
        int par = 0;
        for (uint32_t st = s0; st < s1; ++st) {
            const int pg_c = paged_table(p, b, kfirst, Le, st + 2, lane);  // (its load is waited for with this step's tiles)
            if (st + 1 < s1) stage(st + 1, par ^ 1, pg_b);  // other buffer: its last readers passed the previous barrier
            if (ks4 || wlive) {
                const int sub_end = ks4 ? uw + 1 : 4;
                for (int sub = ks4 ? uw : 0; sub < sub_end; ++sub) {
                    const uint32_t kb = st * 128 + (uint32_t)sub * 32;
                    if (kb >= Le || (int)kb > whi_last) break;  // wholly above the band of the wave's last row
                    if ((int)kb + 31 < wlo_first) continue;     // wholly below the band of its first row: later subtiles may be visible
                    // 16-key groups in pages the table does not hold are masked (their rows landed as zeros)
                    const bool v0 = __builtin_amdgcn_readlane(pg_a, 2 * sub) >= 0;
                    const bool v1 = kb + 16 >= Le || __builtin_amdgcn_readlane(pg_a, 2 * sub + 1) >= 0;
                    const bool edge = kb + 31 >= Lk || !v0 || !v1 || (int)kb < wlo_last || (int)kb + 31 > whi_first;
                    paged_tile<T, DP>(smem + par * STAGE_B + sub * TILE_BYTES, smem + 2 * STAGE_B + par * STAGE_B + sub * TILE_BYTES, qf, c, acc, m,
                                      l, ql, hi, tr_qq, tr_pp, tr_g1, edge, [&](int kr) __attribute__((always_inline)) {
                                          const int key = (int)kb + kr;
                                          return key >= (int)Lk || !(kr < 16 ? v0 : v1) || key < lim_lo || key > lim_hi;
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
                const int64_t rows_all = (int64_t)v.Tq * p.H;  // the packed partial layout (fa_paged_varlen.h)
                paged_store_part<DP>(p.part, (int64_t)p.nsplit * rows_all, (int64_t)part * rows_all + (int64_t)q0 * p.H + (int64_t)hk * R + r, acc,
                                     f, m, L, hi);
            } else {
                paged_store_out<DP, OUT>(p.out, ((int64_t)(q0 + qi) * p.H + h) * DP, p.lse, (int64_t)h * v.Tq + q0 + qi, acc, f, m, L, hi);
            }
        }
        return;
    }
}

// fa_paged_varlen.h's scope, a capacity and a max_seqlen_q below 2^30 (the open-side sentinel stays inside int32), and normalised bounds
bool paged_varlen_window_supported(const PagedVarlenWindowParams& w) {
    const PagedParams& p = w.v.p;
    if (!paged_varlen_supported(w.v)) return false;
    const uint64_t cap = (uint64_t)p.max_pages * p.page_size;
    if (cap >= (1ull << 30) || p.Sq >= (1u << 30)) return false;
    if (w.win_left < 0 || w.win_right < 0) return false;
    return (w.win_left == PAGED_WIN_OPEN || (uint64_t)w.win_left < cap) && (w.win_right == PAGED_WIN_OPEN || (uint32_t)w.win_right < (p.Sq ? p.Sq : 1u));
}

template <typename T, int DP, typename OUT>
static hipError_t launch_fwd16_paged_varlen_window_t(const PagedVarlenWindowParams& w, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds = 4 * 4 * TILE_BYTES;
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_paged_varlen_window_kernel<T, DP, OUT>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((fa_fwd16_paged_varlen_window_kernel<T, DP, OUT>), dim3(w.v.n_items * w.v.p.nsplit), dim3(256), lds, stream, w);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (std::is_same<OUT, void>::value) return launch_paged_varlen_fold(w.v, stream);
    return hipSuccess;
}

template <typename T, int DP>
static hipError_t launch_fwd16_paged_varlen_window_d(const PagedVarlenWindowParams& w, hipStream_t stream) {
    if (w.v.p.nsplit > 1) return launch_fwd16_paged_varlen_window_t<T, DP, void>(w, stream);
    return w.v.p.out_prec == P_FP32 ? launch_fwd16_paged_varlen_window_t<T, DP, float>(w, stream)
                                    : launch_fwd16_paged_varlen_window_t<T, DP, T>(w, stream);
}

// the item-list pre-pass, the banded forward and (p.nsplit > 1: p.part holds nsplit T_q H (D + 2) floats) the fold
hipError_t launch_fwd_16_paged_varlen_window(const PagedVarlenWindowParams& w, hipStream_t stream, const char** name) {
    const PagedVarlenParams& v = w.v;
    const PagedParams& p = v.p;
    if (!paged_varlen_window_supported(w) || !p.out || ((uintptr_t)p.out & 15) || ((uintptr_t)p.lse & 3) || p.nsplit == 0) return hipErrorInvalidValue;
    if (p.out_prec != P_FP32 && p.out_prec != p.in_prec) return hipErrorInvalidValue;
    if (p.nsplit > 1 && !p.part) return hipErrorInvalidValue;
    if (v.n_items && (!v.items || ((uintptr_t)v.items & 7) || !v.counts || ((uintptr_t)v.counts & 15))) return hipErrorInvalidValue;
    static const char* const names[2][2][2] = {
        {{"fa_fwd16_paged_varlen_window<fp16,64>", "fa_fwd16_paged_varlen_window<fp16,64,split>"},
         {"fa_fwd16_paged_varlen_window<fp16,128>", "fa_fwd16_paged_varlen_window<fp16,128,split>"}},
        {{"fa_fwd16_paged_varlen_window<bf16,64,pv16>", "fa_fwd16_paged_varlen_window<bf16,64,pv16,split>"},
         {"fa_fwd16_paged_varlen_window<bf16,128,pv16>", "fa_fwd16_paged_varlen_window<bf16,128,pv16,split>"}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.nsplit > 1];
    if (v.n_items == 0) return hipSuccess;  // (T_q = 0 or max_seqlen_q = 0: no row exists)
    if (hipError_t e = launch_paged_varlen_items(v, stream); e != hipSuccess) return e;
    if (p.D == 64) return bf ? launch_fwd16_paged_varlen_window_d<__bf16, 64>(w, stream) : launch_fwd16_paged_varlen_window_d<_Float16, 64>(w, stream);
    return bf ? launch_fwd16_paged_varlen_window_d<__bf16, 128>(w, stream) : launch_fwd16_paged_varlen_window_d<_Float16, 128>(w, stream);
}

}  // namespace umfa
