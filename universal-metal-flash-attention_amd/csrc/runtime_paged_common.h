// runtime_paged_common.h -- what the two KV-cache entry units (runtime_paged.hip: dense queries, runtime_paged_varlen.hip: packed
// queries) decide the same way: the error map, the CU count, the automatic split-KV part count, the window's normalisation and the
// descales of an fp8 call.  Host code only; internal to those two units.
#pragma once
#include "runtime_internal.h"
#include "fa_paged_window.h"  // PAGED_WIN_OPEN

namespace umfa_rt {

namespace {

mfa_error_t rc_paged(hipError_t e) {
    return e == hipSuccess ? MFA_SUCCESS : e == hipErrorInvalidValue ? MFA_ERROR_INVALID_ARGS
                                         : e == hipErrorOutOfMemory ? MFA_ERROR_MEMORY_ALLOCATION : MFA_ERROR_EXECUTION_FAILED;
}

int paged_cu_count(int dev) {
    static int cached[64] = {0};
    if (dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            n = 256;
        }
        cached[dev] = n;
    }
    return cached[dev];
}

// the band of a window call, normalised by the entry: each side a bound that binds or PAGED_WIN_OPEN
struct WindowArgs {
    int left, right;
};

// the window, normalised once: causal is right = 0; a side that cannot bind (left >= capacity, right >= the query count -- packed:
// max_seqlen_q) is open.  plain: the window bounds nothing (or only as causal does), so the unwindowed kernels run, unchanged
inline WindowArgs paged_window_normalise(int32_t window_left, int32_t window_right, bool causal, uint64_t cap, uint32_t seqlen_q, bool& plain) {
    if (causal) window_right = 0;
    WindowArgs w;
    w.left = window_left < 0 || (uint64_t)window_left >= cap ? umfa::PAGED_WIN_OPEN : window_left;
    w.right = window_right < 0 || (uint32_t)window_right >= seqlen_q ? umfa::PAGED_WIN_OPEN : window_right;
    plain = w.left == umfa::PAGED_WIN_OPEN && (w.right == umfa::PAGED_WIN_OPEN || (causal && w.right == 0));
    return w;
}

// split-KV parts when the caller leaves it to the library: enough workgroups for every CU's slots (one workgroup per CU at head_dim 128,
// two at 64), each part at least two 128-key steps, at most 64 parts.  items: the launch's work items (dense: B H_kv row blocks; packed:
// the item bound -- with every L_q equal the two are the same number, so both entries choose the same).  The steps are the capacity's,
// or with a window (win != NULL) the band's: a workgroup visits the steps of at most left + right + Sq keys (an open side: the
// capacity), plus one step for a band that straddles a step boundary.
inline uint32_t paged_auto_splits(const umfa::PagedParams& p, uint64_t items, const WindowArgs* win, int ncu) {
    const uint64_t slots = (uint64_t)ncu * (p.D == 128 ? 1 : 2);
    if (items == 0 || items >= slots) return 1;
    uint64_t n = (slots + items - 1) / items;
    const uint64_t cap = (uint64_t)p.max_pages * p.page_size;
    uint64_t steps = (cap + 127) / 128;
    if (win) {
        const uint64_t band = (win->left == umfa::PAGED_WIN_OPEN ? cap : (uint64_t)win->left) +
                              (win->right == umfa::PAGED_WIN_OPEN ? cap : (uint64_t)win->right) + p.Sq;
        steps = ((band < cap ? band : cap) + 127) / 128 + 1;
    }
    const uint64_t by_len = steps / 2 ? steps / 2 : 1;
    n = n < by_len ? n : by_len;
    return (uint32_t)(n < 64 ? n : 64);
}

// the descales of an fp8 call into F (PagedFp8Params or PagedVarlenFp8Params); false: one of the four is missing
template <typename F>
bool paged_fill_descales(F& f, const float* k_descale, const int64_t* k_descale_strides, const float* v_descale, const int64_t* v_descale_strides) {
    if (!k_descale || !v_descale || !k_descale_strides || !v_descale_strides) return false;
    f.kd = k_descale; f.kdb = k_descale_strides[0]; f.kdh = k_descale_strides[1];
    f.vd = v_descale; f.vdb = v_descale_strides[0]; f.vdh = v_descale_strides[1];
    return true;
}

}  // namespace

}  // namespace umfa_rt
