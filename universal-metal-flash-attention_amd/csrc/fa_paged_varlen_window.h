// fa_paged_varlen_window.h -- packed variable-length queries over a 16-bit paged / static KV cache with a sliding window
// (fa_fwd_16_paged_varlen_window.hip, runtime_paged_varlen.hip): fa_paged_varlen.h's parameters with the band's two sides.
// PagedVarlenParams is a kernel argument of the existing kernels and does not grow: this struct wraps it.
//
// The contract is fa_paged_varlen.h's with fa_paged_window.h's bound applied per sequence.  For sequence b, L_q,b, L0 and L_k,b are
// varlen_range's / paged_varlen_lens' values and off_b = L_k,b - L_q,b.  Query token i of sequence b sees key j iff j < L_k,b, j's page
// entry lies in [0, num_pages) and i + off_b - win_left <= j <= i + off_b + win_right (flash-attention's window_size = (left, right);
// PAGED_WIN_OPEN: that side is unbounded; causal is win_right = 0, set by the runtime -- the kernel does not look at p.causal).  A row
// that sees no key gives O = 0 exactly and LSE = -inf.  Rows no sequence covers are not written.  Layout, the append, the clamps, the
// dropped rows, memory safety for any contents of cu_seqlens_q, cache_seqlens and the block table, the item list, the packed partials
// and the fused rotary pre-pass (whose positions come from cache_seqlens and `causal`, never from the window): fa_paged_varlen.h and
// fa_paged_rope.h, word for word.
//
// The C entry normalises once: a left bound >= capacity and a right bound >= max_seqlen_q cannot bind and become PAGED_WIN_OPEN; a
// window with both sides open -- or the left open, the right 0 and causal set -- launches the unwindowed packed kernels, unchanged.
// Capacity and max_seqlen_q stay below 2^30, so i + off +- PAGED_WIN_OPEN stays inside int32.
#pragma once
#include "fa_paged_varlen.h"
#include "fa_paged_window.h"  // PAGED_WIN_OPEN

namespace umfa {

struct PagedVarlenWindowParams {
    PagedVarlenParams v;
    int win_left, win_right;  // each in [0, capacity) / [0, max_seqlen_q) or PAGED_WIN_OPEN
};

bool paged_varlen_window_supported(const PagedVarlenWindowParams& w);
// the item-list pre-pass, the banded forward and (split) the fold; the append, the item list and the fold are fa_paged_varlen.h's
// launch_paged_varlen_append / launch_paged_varlen_items / launch_paged_varlen_fold
hipError_t launch_fwd_16_paged_varlen_window(const PagedVarlenWindowParams& w, hipStream_t stream, const char** name);

}  // namespace umfa
