// fa_fwd_16_paged_varlen_window.hip -- bf16 / fp16 MFMA forward of packed variable-length queries (cu_seqlens_q) over a paged or static
// KV cache with a sliding window (flash-attention's window_size), head_dim 64 / 128, GQA.  Semantics: fa_paged_varlen_window.h; layout,
// memory safety and the work distribution: fa_paged_varlen.h.
//
// The forward is fa_paged_window_body.h's paged_window_body -- the body of fa_fwd16_paged_window_kernel (fa_fwd_16_paged_window.hip) --
// over the packed item of fa_paged_item.h (the item read from the list with one scalar load, the sequence's query range from
// cu_seqlens_q, the form decided from the item's own L_q, rows cu[b] + token, the packed split partials, the tally of the forms): token
// i of sequence b sees keys [i + off - left, i + off + right], off = L_k,b - L_q,b.  One body: with every L_q equal the results are
// bitwise those of fa_fwd16_paged_window_kernel.
#include <type_traits>

#include "fa_paged_varlen_window.h"
#include "fa_paged_window_body.h"
#include "kernels.h"

namespace umfa {

template <typename T, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_varlen_window_kernel(PagedVarlenWindowParams vw) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    PagedPackedItem it;
    if (!it.decode(vw.v)) return;
    paged_window_body<T, DP, OUT>(smem, vw.v.p, it, it.key_count(), vw.win_left, vw.win_right);
}

// fa_paged_varlen.h's scope and fa_paged_window.h's rule for the bounds (max_seqlen_q in Sq's place)
bool paged_varlen_window_supported(const PagedVarlenWindowParams& w) {
    return paged_varlen_supported(w.v) && paged_window_bounds_ok(w.v.p, w.win_left, w.win_right);
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
