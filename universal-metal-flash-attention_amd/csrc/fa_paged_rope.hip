// fa_paged_rope.hip -- the fused pre-pass of a rotary KV-cache attention call: one launch rotates k_new into the paged / static cache
// (16-bit or quantised fp8), appends v_new, and rotates q into a dense operand-type image for the unchanged attention kernels.  It
// replaces the append launch, so a rotary call launches as many kernels as the same call without rotary.  Semantics, positions, table
// layout and arithmetic: fa_paged_rope.h; layout, clamps, dropped rows and memory safety: fa_paged.h / fa_paged_varlen.h.
//
// One thread per 16 bytes written: 8 elements of the q image or of a 16-bit cache row, 16 elements of an fp8 cache row.  The interleaved
// form rotates inside a thread's 8-element chunk; the non-interleaved form pairs the chunk with the one rotary_dim / 2 elements away,
// which the thread loads as well (rotary_dim is a multiple of 16, so a chunk lies wholly in one half or wholly in the pass-through
// tail).  Plain vector loads and stores, no LDS, no scratch.  HBM-bound and small: it reads q, k_new, v_new once (k_new's rotary part
// twice, from L2) and writes as much.
#include "fa_paged_rope.h"
#include "fa_paged_rope_device.h"

namespace umfa {

enum : int { ROPE_DENSE16 = 0, ROPE_DENSE_FP8 = 1, ROPE_PACKED16 = 2 };

// T: operand type; TT: table type (float or T); MODE: [B, S, ..] operands over a 16-bit cache / over an fp8 cache / packed operands
template <typename T, typename TT, int MODE>
__global__ __launch_bounds__(256) void fa_paged_rope_kernel(PagedRopeParams r) {
    const PagedVarlenParams& v = r.v;
    const PagedParams& p = v.p;
    typedef T T8 __attribute__((ext_vector_type(8)));
    constexpr bool PACKED = MODE == ROPE_PACKED16, FP8 = MODE == ROPE_DENSE_FP8;
    constexpr uint32_t KVE = FP8 ? 16 : 8;  // elements per K / V thread: 16 bytes of the cache
    const uint32_t nch = p.D / 8, nkv = p.D / KVE;
    const uint64_t rows_q = PACKED ? (uint64_t)v.Tq : (uint64_t)p.B * p.Sq;
    const uint64_t rows_n = PACKED ? (uint64_t)v.Tq : (uint64_t)p.B * p.Snew;
    const uint64_t nq = rows_q * p.H * nch, nk = rows_n * p.Hkv * nkv;
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nq + 2 * nk) return;
    if (idx < nq) {
        // Q: rotate into the dense image
        uint64_t x = idx;
        const uint32_t c = (uint32_t)(x % nch); x /= nch;
        const uint32_t h = (uint32_t)(x % p.H); x /= p.H;  // x: the row, b * Sq + i or the packed t
        const T* src;
        uint32_t pos;
        bool rotate = true;
        if constexpr (PACKED) {
            const uint32_t t = (uint32_t)x;
            uint32_t b, q0, Lq, L0 = 0, Lk;
            rotate = paged_varlen_find(v, t, b, q0, Lq);
            if (rotate) paged_varlen_lens(v, b, Lq, L0, Lk);
            pos = L0 + (p.causal && rotate ? t - q0 : 0u);
            src = (const T*)p.q + (int64_t)t * p.qst + (int64_t)h * p.qsh;
        } else {
            const uint32_t i = (uint32_t)(x % p.Sq), b = (uint32_t)(x / p.Sq);
            uint32_t L0, Lk;
            paged_lens(p, b, L0, Lk);
            pos = L0 + (p.causal ? i : 0u);
            src = (const T*)p.q + (int64_t)b * p.qsb + (int64_t)i * p.qst + (int64_t)h * p.qsh;
        }
        T* dst = (T*)r.qimg + ((int64_t)x * p.H + h) * p.D + 8 * c;
        *(T8*)dst = rotate ? rope_chunk<T, TT>(r, src, 8 * c, pos) : *(const T8*)(src + 8 * c);
        return;
    }
    // K (rotated) and V: the append's work, fa_paged_append_kernel's / fa_paged_varlen_append_kernel's rules
    uint64_t x = idx - nq;
    const uint32_t c = (uint32_t)(x % nkv); x /= nkv;
    const uint32_t hk = (uint32_t)(x % p.Hkv); x /= p.Hkv;
    const bool isv = x >= rows_n;
    if (isv) x -= rows_n;
    uint32_t b, i, L0, Lk;
    int64_t srow;  // the row's element offset in k_new / v_new
    if constexpr (PACKED) {
        const uint32_t t = (uint32_t)x;
        uint32_t q0, Lq;
        if (!paged_varlen_find(v, t, b, q0, Lq)) return;
        paged_varlen_lens(v, b, Lq, L0, Lk);
        i = t - q0;
        srow = isv ? (int64_t)t * p.vnt : (int64_t)t * p.knt;
    } else {
        i = (uint32_t)(x % p.Snew);
        b = (uint32_t)(x / p.Snew);
        paged_lens(p, b, L0, Lk);
        srow = isv ? (int64_t)b * p.vnb + (int64_t)i * p.vnt : (int64_t)b * p.knb + (int64_t)i * p.knt;
    }
    const uint32_t pos = L0 + i;
    if (pos >= p.max_pages * p.page_size) return;
    const uint32_t lp = paged_lpage(p, pos);
    const int pg = paged_page(p, b, lp);
    if (pg < 0) return;
    const uint32_t rip = pos - lp * p.page_size;
    const T* src = (const T*)(isv ? p.vn : p.kn) + srow + (isv ? (int64_t)hk * p.vnh : (int64_t)hk * p.knh);
    const int64_t drow = isv ? (int64_t)pg * p.vpg + (int64_t)rip * p.vst + (int64_t)hk * p.vsh
                             : (int64_t)pg * p.kpg + (int64_t)rip * p.kst + (int64_t)hk * p.ksh;
    if constexpr (FP8) {
        uint8_t* dst = (uint8_t*)(isv ? p.vc : p.kc) + drow;
        const float d = isv ? r.vd[(int64_t)b * r.vdb + (int64_t)hk * r.vdh] : r.kd[(int64_t)b * r.kdb + (int64_t)hk * r.kdh];
        T8 x0, x1;
        if (isv) {
            x0 = *(const T8*)(src + 16 * c);
            x1 = *(const T8*)(src + 16 * c + 8);
        } else {
            x0 = rope_chunk<T, TT>(r, src, 16 * c, pos);
            x1 = rope_chunk<T, TT>(r, src, 16 * c + 8, pos);
        }
        *(U4*)(dst + 16 * c) = quant16(x0, x1, d);
    } else {
        T* dst = (T*)(isv ? p.vc : p.kc) + drow;
        *(T8*)(dst + 8 * c) = isv ? *(const T8*)(src + 8 * c) : rope_chunk<T, TT>(r, src, 8 * c, pos);
    }
}

static uint64_t rope_threads(const PagedRopeParams& r) {
    const PagedParams& p = r.v.p;
    const uint64_t rows_q = r.packed ? (uint64_t)r.v.Tq : (uint64_t)p.B * p.Sq;
    const uint64_t rows_n = r.packed ? (uint64_t)r.v.Tq : (uint64_t)p.B * p.Snew;
    return rows_q * p.H * (p.D / 8) + 2 * rows_n * p.Hkv * (p.D / (r.fp8 ? 16 : 8));
}

size_t paged_rope_qimg_bytes(const PagedRopeParams& r) {
    const PagedParams& p = r.v.p;
    return (size_t)(r.packed ? (uint64_t)r.v.Tq : (uint64_t)p.B * p.Sq) * p.H * p.D * 2;
}

// Scope (on top of the call's own paged_supported / paged_fp8_supported / paged_varlen_supported, which the runtime has checked): new
// tokens, rotary_dim a multiple of 16 in [16, D], 1 <= seqlen_ro < 2^31, 16-byte aligned table rows that hold rotary_dim / 2 columns,
// a 16-byte aligned q image, no fp8 cache in the packed form, and a grid inside 31 bits.
bool paged_rope_supported(const PagedRopeParams& r) {
    const PagedParams& p = r.v.p;
    if (p.in_prec != P_FP16 && p.in_prec != P_BF16) return false;
    if ((p.D != 64 && p.D != 128) || p.Hkv == 0 || p.H % p.Hkv) return false;
    if (!p.Snew || !p.kn || !p.vn || !p.q) return false;
    if (r.rdim < 16 || r.rdim > p.D || r.rdim % 16) return false;
    if (r.seqlen_ro == 0 || r.seqlen_ro >= (1u << 31)) return false;
    const int64_t tb = r.table_f32 ? 4 : 2;
    if (!r.cos || !r.sin || ((uintptr_t)r.cos & 15) || ((uintptr_t)r.sin & 15)) return false;
    if (r.rstride < (int64_t)(r.rdim / 2) || (r.rstride * tb) % 16) return false;
    if (!r.qimg || ((uintptr_t)r.qimg & 15)) return false;
    if (r.fp8 && (r.packed || !r.kd || !r.vd)) return false;
    if (r.packed && (!r.v.cu || p.qsb || p.knb || p.vnb)) return false;
    return rope_threads(r) < (1ull << 39);
}

template <typename T, typename TT>
static void launch_rope_m(const PagedRopeParams& r, dim3 grid, hipStream_t stream) {
    if (r.packed)
        hipLaunchKernelGGL((fa_paged_rope_kernel<T, TT, ROPE_PACKED16>), grid, dim3(256), 0, stream, r);
    else if (r.fp8)
        hipLaunchKernelGGL((fa_paged_rope_kernel<T, TT, ROPE_DENSE_FP8>), grid, dim3(256), 0, stream, r);
    else
        hipLaunchKernelGGL((fa_paged_rope_kernel<T, TT, ROPE_DENSE16>), grid, dim3(256), 0, stream, r);
}

hipError_t launch_paged_rope(const PagedRopeParams& r, hipStream_t stream) {
    if (!paged_rope_supported(r)) return hipErrorInvalidValue;
    const uint64_t total = rope_threads(r);
    if (total == 0) return hipSuccess;
    const dim3 grid((uint32_t)((total + 255) / 256));
    if (r.v.p.in_prec == P_BF16) {
        if (r.table_f32) launch_rope_m<__bf16, float>(r, grid, stream); else launch_rope_m<__bf16, __bf16>(r, grid, stream);
    } else {
        if (r.table_f32) launch_rope_m<_Float16, float>(r, grid, stream); else launch_rope_m<_Float16, _Float16>(r, grid, stream);
    }
    return hipGetLastError();
}

}  // namespace umfa
