// fa_paged_window.h -- sliding-window attention over a 16-bit paged or static KV cache (fa_fwd_16_paged_window.hip, runtime_paged.hip):
// the parameters of fa_paged.h with the band's two sides.  PagedParams is a kernel argument of the existing kernels and does not grow:
// this struct wraps it.
//
// flash-attention's window_size = (left, right), bottom-right per sequence: with L_k as fa_paged.h clamps it and off = L_k - Sq, query
// token i of sequence b sees key j iff j < L_k, j's page entry lies in [0, num_pages) and i + off - win_left <= j <= i + off + win_right
// (PAGED_WIN_OPEN: that side is unbounded; causal is win_right = 0, set by the runtime -- the kernels do not look at p.causal).  A row
// that sees no key gives O = 0 and LSE = -inf.  Layout, append, clamps, masking and memory safety: fa_paged.h, word for word.
#pragma once
#include "fa_paged.h"

namespace umfa {

// an unbounded side: i + off +- PAGED_WIN_OPEN stays inside int32 and past every key (capacity and Sq < 2^30)
constexpr int PAGED_WIN_OPEN = 1 << 30;

struct PagedWindowParams {
    PagedParams p;
    int win_left, win_right;  // each in [0, capacity) / [0, Sq) or PAGED_WIN_OPEN
};

bool paged_window_supported(const PagedWindowParams& w);
// the bounds' part of it, which the packed form (fa_paged_varlen_window.h) shares: capacity and p.Sq below 2^30, each side normalised
bool paged_window_bounds_ok(const PagedParams& p, int left, int right);
// the append and (split) the fold are fa_paged.h's launch_paged_append / launch_paged_fold; this launches the attention and the fold
hipError_t launch_fwd_16_paged_window(const PagedWindowParams& w, hipStream_t stream, const char** name);

}  // namespace umfa
