// fa_paged_window_body.h -- the body of the sliding-window KV-cache forward, written once for fa_fwd16_paged_window_kernel
// (fa_fwd_16_paged_window.hip) and its packed twin fa_fwd16_paged_varlen_window_kernel (fa_fwd_16_paged_varlen_window.hip).  A kernel
// declares its LDS, decodes its item (fa_paged_item.h: the coordinates and the destination rows, the only thing the twins differ in)
// and calls the body with the item's L_k.  The packed kernel's bitwise agreement with the dense one at equal lengths
// (tests/test_gpu_varlen_paged_window.py) follows from the one text.
//
// The plain and the fp8 pairs keep one kernel text per unit: as shared bodies their kernels kept the parent's registers and loop but
// measured 0.5 - 2.5 % slower on the HBM-bound shapes (profiles/paged_body/summary.md).
//
// The workgroup, the page indirection, the bf16 V conversion and the leaves this body calls: fa_paged_device.h.  The bf16 range rule
// is written out here: as a function of its own it cost each bf16 kernel 4 to 10 scalar registers, up to a spill
// (profiles/paged_shared/resources.md).
#pragma once
#include "fa_paged_device.h"
#include "fa_paged_item.h"

namespace umfa {

namespace {

// fa_fwd16_paged_kernel's workgroup (fa_fwd_16_paged.hip: its row packing, its 128-key steps, its decode form and its split-KV parts)
// with a sliding window (flash-attention's window_size): token i sees keys [i + off - left, i + off + right],
// off = L_k - L_q, the bounds runtime values (no causal instantiation).
//
// Step range: with first_tok / last_tok the query tokens of the item's first and last live rows, k_first = max(0, first_tok + off -
// left) and k_last = min(L_k - 1, last_tok + off + right); the item visits the steps [k_first / 128, k_last / 128 + 1), none when
// k_last < k_first.  Split-KV parts divide THAT range, so the cost of a call follows the band, not the context.  An item or part whose
// range is empty stages nothing and writes O = 0, LSE = -inf (a part: m = -inf, l = 0).
//
// Per wave: a subtile wholly below the band of the wave's first row is skipped, one wholly above the band of its last row ends the
// step's subtiles for the wave; a subtile that crosses either bound of any of the wave's rows, L_k, or a 16-key group whose page entry is
// invalid masks per score, every other subtile runs the open body.
//
// Keys outside [k_first, k_last] that share a visited step land in LDS as zeros: above, the descriptors' range stops at k_last + 1; below,
// their lanes get an offset at the end of their piece's descriptor range (the out-of-range load the zero-byte descriptor of an invalid
// page already relies on).  A masked P = 0 then never meets a stale page's NaN or Inf in the P V product, and such rows never steer the
// bf16 path's largest |v|.  Block-table entries of 16-key groups wholly outside [k_first, k_last] are never read.
template <typename T, int DP, typename OUT, typename ITEM>
__device__ __forceinline__ void paged_window_body(char* smem, const PagedParams& p, const ITEM& it, const uint32_t Lk, const int win_left,
                                                  const int win_right) {
    BWD16_GEO(DP);
    (void)TILE_PIECES, (void)PD;
    constexpr int STAGE_B = 4 * TILE_BYTES;  // one step (128 keys) of K or of V
    constexpr bool VCONV = std::is_same<T, __bf16>::value;
    const int tid = threadIdx.x, lane = tid & 63, ql = lane & 31, hi = lane >> 5;
    const int wave = tid >> 6, uw = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t part = it.part, b = it.b, hk = it.hk, rb = it.rb, R = it.R;
    const bool ks4 = it.ks4;
    const uint32_t g = p.H / p.Hkv;
    const int off = (int)Lk - (int)it.Lq;
    const int lo_off = off - win_left, hi_off = off + win_right;  // token i sees keys [i + lo_off, i + hi_off] (and < L_k)
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
    paged_load_q<T, DP>(qf, it.template q_row<T>(qi, h), rok, hi);
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
    for (int pass = 0;; ++pass) {  // (bf16: the range rule's second sweep restarts at the band's first step, s0)
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
        if (owner && rok) paged_store_row<DP, OUT>(p, it, r, qi, h, acc, L > 0.0f ? back / L : 0.0f, m, L, hi);
        return;
    }
}

}  // namespace

}  // namespace umfa
