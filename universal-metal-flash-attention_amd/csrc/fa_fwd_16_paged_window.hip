// fa_fwd_16_paged_window.hip -- bf16 / fp16 MFMA forward over a paged or static KV cache with a sliding window (flash-attention's
// window_size), head_dim 64 / 128, GQA.  Semantics: fa_paged_window.h; layout and memory safety: fa_paged.h.
//
// The forward is fa_paged_window_body.h's paged_window_body (the banded step range, the subtile skipping and the zero landing are
// described there) over the dense item of fa_paged_item.h; the packed twin, fa_fwd_16_paged_varlen_window.hip, runs the same body over
// its own item.  This unit keeps the kernel's name and instantiations, its launcher and the scope check both twins share.
#include <type_traits>

#include "fa_paged_window.h"
#include "fa_paged_window_body.h"
#include "kernels.h"

namespace umfa {

template <typename T, int DP, typename OUT>
__global__ __launch_bounds__(256, 2) void fa_fwd16_paged_window_kernel(PagedWindowParams pw) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    PagedDenseItem it;
    it.decode(pw.p);
    paged_window_body<T, DP, OUT>(smem, pw.p, it, it.key_count(), pw.win_left, pw.win_right);
}

// a capacity and a query count (packed: max_seqlen_q) below 2^30 (the open-side sentinel stays inside int32), and normalised bounds
bool paged_window_bounds_ok(const PagedParams& p, int left, int right) {
    const uint64_t cap = (uint64_t)p.max_pages * p.page_size;
    if (cap >= (1ull << 30) || p.Sq >= (1u << 30)) return false;
    if (left < 0 || right < 0) return false;
    return (left == PAGED_WIN_OPEN || (uint64_t)left < cap) && (right == PAGED_WIN_OPEN || (uint32_t)right < (p.Sq ? p.Sq : 1u));
}

// fa_paged.h's scope and the bounds' rule
bool paged_window_supported(const PagedWindowParams& w) { return paged_supported(w.p) && paged_window_bounds_ok(w.p, w.win_left, w.win_right); }

template <typename T, int DP, typename OUT>
static hipError_t launch_fwd16_paged_window_t(const PagedWindowParams& w, hipStream_t stream) {
    constexpr int TILE_BYTES = 32 * 2 * DP;
    const size_t lds = 4 * 4 * TILE_BYTES;
    const PagedParams& p = w.p;
    if (hipError_t e = ensure_dynamic_lds((const void*)fa_fwd16_paged_window_kernel<T, DP, OUT>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((fa_fwd16_paged_window_kernel<T, DP, OUT>), dim3(p.B * p.Hkv * p.nrb * p.nsplit), dim3(256), lds, stream, w);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (std::is_same<OUT, void>::value) return launch_paged_fold(p, stream);
    return hipSuccess;
}

template <typename T, int DP>
static hipError_t launch_fwd16_paged_window_d(const PagedWindowParams& w, hipStream_t stream) {
    if (w.p.nsplit > 1) return launch_fwd16_paged_window_t<T, DP, void>(w, stream);
    return w.p.out_prec == P_FP32 ? launch_fwd16_paged_window_t<T, DP, float>(w, stream) : launch_fwd16_paged_window_t<T, DP, T>(w, stream);
}

// w.p.nsplit > 1: w.p.part holds nsplit B H_kv R (D + 2) floats
hipError_t launch_fwd_16_paged_window(const PagedWindowParams& w, hipStream_t stream, const char** name) {
    const PagedParams& p = w.p;
    if (!paged_window_supported(w) || !paged_fwd_args_ok(p)) return hipErrorInvalidValue;
    static const char* const names[2][2][2] = {
        {{"fa_fwd16_paged_window<fp16,64>", "fa_fwd16_paged_window<fp16,64,split>"},
         {"fa_fwd16_paged_window<fp16,128>", "fa_fwd16_paged_window<fp16,128,split>"}},
        {{"fa_fwd16_paged_window<bf16,64,pv16>", "fa_fwd16_paged_window<bf16,64,pv16,split>"},
         {"fa_fwd16_paged_window<bf16,128,pv16>", "fa_fwd16_paged_window<bf16,128,pv16,split>"}}};
    const bool bf = p.in_prec == P_BF16;
    *name = names[bf][p.D == 128][p.nsplit > 1];
    if ((uint64_t)p.B * p.H * p.Sq == 0) return hipSuccess;  // (an empty call needs no partials: before the check of p.part)
    if (p.nsplit > 1 && !p.part) return hipErrorInvalidValue;
    if (p.D == 64) return bf ? launch_fwd16_paged_window_d<__bf16, 64>(w, stream) : launch_fwd16_paged_window_d<_Float16, 64>(w, stream);
    return bf ? launch_fwd16_paged_window_d<__bf16, 128>(w, stream) : launch_fwd16_paged_window_d<_Float16, 128>(w, stream);
}

}  // namespace umfa
