// fa_fwd_16_paged_varlen.hip -- bf16 / fp16 MFMA forward of packed variable-length queries (cu_seqlens_q) over a paged or static KV
// cache (head_dim 64 / 128, causal or not, GQA), with the packed in-place append, the item-list pre-pass and the split-KV fold.
// Semantics, layout, memory safety and the work distribution: fa_paged_varlen.h.
//
// The workgroup is fa_fwd_16_paged.hip's (the rows of one (sequence, KV head) packed, row r query token r / g of query head hk g + r % g;
// double-buffered 128-key steps; the same split partial format) over the shared device pieces of fa_paged_device.h.  What differs: a
// workgroup reads its (sequence, KV head, row block) from the item list instead of deriving it from blockIdx, takes the sequence's
// query range from cu_seqlens_q, and decides between the decode form (ks4: R = g L_q <= 32) and the 128-row form from its own L_q --
// both forms run in one launch.  q / O / LSE rows are cu[b] + token; the causal offset and the last visible key come from the item's
// L_q and L_k.  With every L_q equal the arithmetic, and its order, is that of fa_fwd16_paged_kernel: the results are bitwise the same.
#include <type_traits>

#include "fa_paged_varlen.h"
#include "fa_paged_device.h"
#include "kernels.h"

namespace umfa {

namespace {

// row blocks of a sequence with R rows per KV head: one in the decode form, else 128 rows each
__device__ __forceinline__ uint32_t varlen_blocks(uint32_t R) { return R == 0 ? 0u : (R <= 32 ? 1u : (R + 127) / 128); }

}  // namespace

template <typename T, bool CAUSAL, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_varlen_kernel(PagedVarlenParams v) {
    const PagedParams& p = v.p;
    BWD16_GEO(DP);
    (void)TILE_PIECES;
    constexpr int STAGE_B = 4 * TILE_BYTES;  // one step (128 keys) of K or of V
    constexpr bool VCONV = std::is_same<T, __bf16>::value;
    constexpr bool SPLIT = std::is_same<OUT, void>::value;
    typedef Mma16<T> M;
    typedef typename M::V8 V8;
    typedef Mma16<_Float16> MP;  // the P V product: fp16 P, fp16 V
    typedef typename MP::V8 PV8;
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

    typename Mma16<T>::V8 qf[NKS];
    paged_load_q<T, DP>(qf, (const T*)p.q + (int64_t)(q0 + qi) * p.qst + (int64_t)h * p.qsh, rok, hi);
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

        // the tile step of fa_paged_device.h (paged_tile), kept in place: as the shared function it cost this kernel alone 1.5 % of its
        // time on the HBM-bound shapes (profiles/paged_shared/summary.md).  The arithmetic and its order are paged_tile's and must stay
        // so: a change to either goes into both (test_gpu_varlen_paged.py holds this kernel bitwise to the plain one at equal lengths)
        auto tile_body = [&](const char* Kt, const char* Vt, uint32_t kb, bool v0, bool v1, bool edge) __attribute__((always_inline)) {
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
            for (int rr = 0; rr < 16; ++rr) {
                const int kr = acc_row(rr, hi);
                const uint32_t key = kb + kr;
                x[rr] = s[rr] * c;
                if (edge && (key >= Lk || !(kr < 16 ? v0 : v1) || (CAUSAL && (int)key > lim))) x[rr] = -INFINITY;
                mx = fmaxf(mx, x[rr]);
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
                for (int rr = 0; rr < 16; ++rr) acc[i][rr] *= alpha;
            PV8 pb[2];
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float pr = __builtin_amdgcn_exp2f(x[rr] - base);
                l += pr;
                pb[rr >> 3][rr & 7] = (_Float16)pr;
            }
#pragma unroll
            for (int i = 0; i < NDB; ++i)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                    acc[i] = MP::mma(tr_frag<MP, DP>(Vt, i, s2, hi, tr_qq, tr_pp, tr_g1), pb[s2], acc[i]);
        };

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
                    tile_body(smem + par * STAGE_B + sub * TILE_BYTES, smem + 2 * STAGE_B + par * STAGE_B + sub * TILE_BYTES, kb, v0, v1, edge);
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

// the item list: entry i of v.n_items is {sequence, hk * blocks + row block} of the i-th (sequence, KV head, row block) in sequence
// order, {-1, 0} past the last one.  One workgroup: 256 sequences at a time, a saturating scan of their entry counts in LDS, then
// every thread fills entries by binary search in the scan.  Counts saturate at n_items, so no contents of cu overflow anything.
__global__ __launch_bounds__(256) void fa_paged_varlen_items_kernel(PagedVarlenParams v) {
    __shared__ uint32_t pre[2][257];
    const uint32_t tid = threadIdx.x, cap = v.n_items, g = v.p.H / v.p.Hkv;
    if (tid < 4) v.counts[tid] = 0;  // the forward's tally of the forms it ran
    uint32_t done = 0;  // entries written so far (saturated at cap)
    for (uint32_t base = 0; base < v.p.B && done < cap; base += 256) {
        const uint32_t b = base + tid;
        uint32_t n = 0;
        if (b < v.p.B) {
            int a = v.cu[b], e = v.cu[b + 1];
            a = a < 0 ? 0 : (a > (int)v.Tq ? (int)v.Tq : a);
            e = e < a ? a : (e > (int)v.Tq ? (int)v.Tq : e);
            uint32_t l = (uint32_t)(e - a);
            l = l < v.p.Sq ? l : v.p.Sq;
            const uint64_t nn = (uint64_t)varlen_blocks(g * l) * v.p.Hkv;
            n = nn < cap ? (uint32_t)nn : cap;
        }
        int cur = 0;
        pre[0][tid + 1] = n;
        if (tid == 0) pre[0][0] = pre[1][0] = 0;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan of pre[.][1 .. 256], saturating at cap
            const uint32_t x = pre[cur][tid + 1], y = tid >= d ? pre[cur][tid + 1 - d] : 0u;
            pre[cur ^ 1][tid + 1] = x + y < cap ? x + y : cap;
            cur ^= 1;
            __syncthreads();
        }
        const uint32_t* const ps = pre[cur];
        const uint32_t total = ps[256], room = cap - done, cnt = total < room ? total : room;
        for (uint32_t i = tid; i < cnt; i += 256) {
            uint32_t lo = 0, hi = 256;  // the sequence with ps[lo] <= i < ps[lo + 1]
            while (lo + 1 < hi) {
                const uint32_t m = (lo + hi) >> 1;
                if (ps[m] <= i) lo = m; else hi = m;
            }
            v.items[2 * (size_t)(done + i)] = (int32_t)(base + lo);
            v.items[2 * (size_t)(done + i) + 1] = (int32_t)(i - ps[lo]);
        }
        done += cnt;
        __syncthreads();
    }
    for (uint32_t i = done + tid; i < cap; i += 256) {
        v.items[2 * (size_t)i] = -1;
        v.items[2 * (size_t)i + 1] = 0;
    }
}

// the split-KV fold: packed row (t, h) of every part, in part order (bitwise repeatable), into O and LSE.  D / 4 lanes per row; a row no
// sequence covers is left alone.
template <typename OUT>
__global__ __launch_bounds__(256) void fa_paged_varlen_fold_kernel(PagedVarlenParams v) {
    const PagedParams& p = v.p;
    const uint32_t nl = p.D / 4, rpb = 256 / nl;
    const uint64_t row = (uint64_t)blockIdx.x * rpb + threadIdx.x / nl;
    const uint32_t d4 = threadIdx.x % nl;
    const uint64_t rows_all = (uint64_t)v.Tq * p.H;
    if (row >= rows_all) return;
    const uint32_t t = (uint32_t)(row / p.H), h = (uint32_t)(row % p.H), g = p.H / p.Hkv, hk = h / g;
    uint32_t b, q0, Lq;
    if (!paged_varlen_find(v, t, b, q0, Lq)) return;
    const uint64_t prow0 = (uint64_t)q0 * p.H + (uint64_t)hk * g * Lq + (uint64_t)(t - q0) * g + h % g;
    const float* const ml = p.part + (size_t)p.nsplit * rows_all * p.D;
    float Mx = -INFINITY;
    for (uint32_t s = 0; s < p.nsplit; ++s) Mx = fmaxf(Mx, ml[((size_t)s * rows_all + prow0) * 2]);
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    float L = 0.0f;
    for (uint32_t s = 0; s < p.nsplit; ++s) {
        const size_t pr = (size_t)s * rows_all + prow0;
        const float ms = ml[pr * 2], ls = ml[pr * 2 + 1];
        const float w = ms == -INFINITY ? 0.0f : ls * __builtin_amdgcn_exp2f(ms - Mx);
        if (w != 0.0f) {
            const f32x4 os = *(const f32x4*)(p.part + pr * p.D + 4 * d4);
            o += w * os;
            L += w;
        }
    }
    const float f = L > 0.0f ? 1.0f / L : 0.0f;
    const int64_t at = (int64_t)row * p.D + 4 * d4;
    if constexpr (std::is_same<OUT, float>::value) {
        *(f32x4*)((float*)p.out + at) = o * f;
    } else {
        typedef OUT O4 __attribute__((ext_vector_type(4)));
        *(O4*)((OUT*)p.out + at) = O4{(OUT)(o[0] * f), (OUT)(o[1] * f), (OUT)(o[2] * f), (OUT)(o[3] * f)};
    }
    if (d4 == 0 && p.lse) p.lse[(int64_t)h * v.Tq + t] = L > 0.0f ? (Mx + __builtin_log2f(L)) * UMFA_LN2 : -INFINITY;
}

// the packed append: row t of k_new / v_new belongs to the sequence b whose query range holds it and goes to cache position
// clamp(cache_seqlens[b]) + (t - cu[b]) through the block table.  Rows no sequence covers, rows past the capacity and rows of pages the
// table does not hold are dropped (fa_paged_append_kernel's rules).  One thread per 16 bytes.
__global__ __launch_bounds__(256) void fa_paged_varlen_append_kernel(PagedVarlenParams v) {
    const PagedParams& p = v.p;
    const uint32_t nch = p.D / 8;
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
    typedef unsigned U4 __attribute__((ext_vector_type(4)));
    const uint16_t* src = (const uint16_t*)(isv ? p.vn : p.kn) + (isv ? (int64_t)t * p.vnt + (int64_t)hk * p.vnh : (int64_t)t * p.knt + (int64_t)hk * p.knh);
    uint16_t* dst = (uint16_t*)(isv ? p.vc : p.kc) +
                    (isv ? (int64_t)pg * p.vpg + (int64_t)rip * p.vst + (int64_t)hk * p.vsh : (int64_t)pg * p.kpg + (int64_t)rip * p.kst + (int64_t)hk * p.ksh);
    *(U4*)(dst + 8 * c) = *(const U4*)(src + 8 * c);
}

uint32_t paged_varlen_item_bound(const PagedVarlenParams& v) {
    if (v.p.Hkv == 0 || v.p.H % v.p.Hkv) return 0;
    const uint64_t g = v.p.H / v.p.Hkv;
    const uint64_t by_rows = g * v.Tq / 128 + v.p.B;  // a sequence costs at most one partly filled block
    const uint64_t by_max = (uint64_t)v.p.B * ((g * v.p.Sq + 127) / 128);
    const uint64_t n = (by_rows < by_max ? by_rows : by_max) * v.p.Hkv;
    return n < (1ull << 31) ? (uint32_t)n : 0u;
}

// Scope: paged_supported's (fa_fwd_16_paged.hip) for the operands, the caches and the table, plus: 32-bit row counts, the new tokens'
// strides, and an item list of paged_varlen_item_bound entries.
bool paged_varlen_supported(const PagedVarlenParams& v) {
    const PagedParams& p = v.p;
    if (!paged_supported(p) || !v.cu || ((uintptr_t)v.cu & 3)) return false;
    if (p.Snew > 1 || p.qsb || p.knb || p.vnb) return false;
    const uint64_t g = p.H / p.Hkv;
    if (g * p.Sq >= (1ull << 31) || (uint64_t)v.Tq * p.H >= (1ull << 31) || v.Tq >= (1u << 30) || p.Sq > v.Tq) return false;
    if ((uint64_t)v.Tq * p.Hkv * (p.D / 8) * 2 >= (1ull << 40)) return false;
    if (v.n_items != paged_varlen_item_bound(v)) return false;
    return (uint64_t)v.n_items * (p.nsplit ? p.nsplit : 1) < (1ull << 31);
}

hipError_t launch_paged_varlen_append(const PagedVarlenParams& v, hipStream_t stream) {
    if (!paged_varlen_supported(v) || !v.p.Snew) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)v.Tq * v.p.Hkv * (v.p.D / 8) * 2;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(fa_paged_varlen_append_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, v);
    return hipGetLastError();
}

// the item-list pre-pass alone (fa_fwd_16_paged_varlen_fp8.hip launches it in front of its own forward)
hipError_t launch_paged_varlen_items(const PagedVarlenParams& v, hipStream_t stream) {
    hipLaunchKernelGGL(fa_paged_varlen_items_kernel, dim3(1), dim3(256), 0, stream, v);
    return hipGetLastError();
}

// the split-KV fold alone (v.p.nsplit parts in v.p.part)
hipError_t launch_paged_varlen_fold(const PagedVarlenParams& v, hipStream_t stream) {
    const uint64_t rows = (uint64_t)v.Tq * v.p.H, rpb = 256 / (v.p.D / 4);
    const dim3 grid((uint32_t)((rows + rpb - 1) / rpb));
    if (v.p.out_prec == P_FP32)
        hipLaunchKernelGGL(fa_paged_varlen_fold_kernel<float>, grid, dim3(256), 0, stream, v);
    else if (v.p.in_prec == P_BF16)
        hipLaunchKernelGGL(fa_paged_varlen_fold_kernel<__bf16>, grid, dim3(256), 0, stream, v);
    else
        hipLaunchKernelGGL(fa_paged_varlen_fold_kernel<_Float16>, grid, dim3(256), 0, stream, v);
    return hipGetLastError();
}

template <typename T, bool CAUSAL, int DP, typename OUT>
static hipError_t launch_fwd16_paged_varlen_t(const PagedVarlenParams& v, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds = 4 * 4 * TILE_BYTES;
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_paged_varlen_kernel<T, CAUSAL, DP, OUT>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((fa_fwd16_paged_varlen_kernel<T, CAUSAL, DP, OUT>), dim3(v.n_items * v.p.nsplit), dim3(256), lds, stream, v);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (std::is_same<OUT, void>::value) return launch_paged_varlen_fold(v, stream);
    return hipSuccess;
}

template <typename T, int DP>
static hipError_t launch_fwd16_paged_varlen_d(const PagedVarlenParams& v, hipStream_t stream) {
    const bool f32 = v.p.out_prec == P_FP32;
    if (v.p.nsplit > 1)
        return v.p.causal ? launch_fwd16_paged_varlen_t<T, true, DP, void>(v, stream) : launch_fwd16_paged_varlen_t<T, false, DP, void>(v, stream);
    if (v.p.causal) return f32 ? launch_fwd16_paged_varlen_t<T, true, DP, float>(v, stream) : launch_fwd16_paged_varlen_t<T, true, DP, T>(v, stream);
    return f32 ? launch_fwd16_paged_varlen_t<T, false, DP, float>(v, stream) : launch_fwd16_paged_varlen_t<T, false, DP, T>(v, stream);
}

// the item-list pre-pass, the forward and (p.nsplit > 1: p.part holds nsplit T_q H (D + 2) floats) the fold
hipError_t launch_fwd_16_paged_varlen(const PagedVarlenParams& v, hipStream_t stream, const char** name) {
    const PagedParams& p = v.p;
    if (!paged_varlen_supported(v) || !p.out || ((uintptr_t)p.out & 15) || ((uintptr_t)p.lse & 3) || p.nsplit == 0) return hipErrorInvalidValue;
    if (p.out_prec != P_FP32 && p.out_prec != p.in_prec) return hipErrorInvalidValue;
    if (p.nsplit > 1 && !p.part) return hipErrorInvalidValue;
    if (v.n_items && (!v.items || ((uintptr_t)v.items & 7) || !v.counts || ((uintptr_t)v.counts & 15))) return hipErrorInvalidValue;
    static const char* const names[2][2][2][2] = {
        {{{"fa_fwd16_paged_varlen<fp16,64>", "fa_fwd16_paged_varlen<fp16,64,split>"},
          {"fa_fwd16_paged_varlen<fp16,64,causal>", "fa_fwd16_paged_varlen<fp16,64,causal,split>"}},
         {{"fa_fwd16_paged_varlen<fp16,128>", "fa_fwd16_paged_varlen<fp16,128,split>"},
          {"fa_fwd16_paged_varlen<fp16,128,causal>", "fa_fwd16_paged_varlen<fp16,128,causal,split>"}}},
        {{{"fa_fwd16_paged_varlen<bf16,64,pv16>", "fa_fwd16_paged_varlen<bf16,64,pv16,split>"},
          {"fa_fwd16_paged_varlen<bf16,64,causal,pv16>", "fa_fwd16_paged_varlen<bf16,64,causal,pv16,split>"}},
         {{"fa_fwd16_paged_varlen<bf16,128,pv16>", "fa_fwd16_paged_varlen<bf16,128,pv16,split>"},
          {"fa_fwd16_paged_varlen<bf16,128,causal,pv16>", "fa_fwd16_paged_varlen<bf16,128,causal,pv16,split>"}}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.causal != 0][p.nsplit > 1];
    if (v.n_items == 0) return hipSuccess;  // (T_q = 0 or max_seqlen_q = 0: no row exists)
    if (hipError_t e = launch_paged_varlen_items(v, stream); e != hipSuccess) return e;
    if (p.D == 64) return bf ? launch_fwd16_paged_varlen_d<__bf16, 64>(v, stream) : launch_fwd16_paged_varlen_d<_Float16, 64>(v, stream);
    return bf ? launch_fwd16_paged_varlen_d<__bf16, 128>(v, stream) : launch_fwd16_paged_varlen_d<_Float16, 128>(v, stream);
}

}  // namespace umfa
