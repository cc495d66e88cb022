// fa_paged_fp8.h -- KV-cache attention over an OCP fp8 (e4m3fn) cache (fa_fwd_16_paged_fp8.hip, runtime_paged.hip): the parameters of
// fa_paged.h with a dequantisation scale per (batch, KV head).  PagedParams is a kernel argument of the 16-bit kernels and does not grow:
// this struct wraps it.
//
// A cache byte stands for e4m3fn(byte) * descale[b, h_kv]; q, k_new / v_new and the output are 16-bit as in fa_paged.h.  Cache strides
// (PagedParams::kpg .. vsh) are in ELEMENTS, which are bytes here: multiples of 16 (the LDS-DMA's 16-byte granule), head_dim contiguous.
// The descales are device fp32, addressed as d[b * db + h_kv * dh] with element strides that may be 0 (a scalar, [H_kv], [B, 1],
// [B, H_kv]); the kernels read them, the host never does.  Layout, clamps, masking and memory safety: fa_paged.h, word for word.
//
// Append: element x of k_new / v_new is stored as e4m3fn_rne(clamp(fp32(x) / descale, -448, +448)) -- IEEE fp32 division, the clamp in
// front of the conversion (its result then does not depend on the conversion's overflow mode), round to nearest even.
#pragma once
#include "fa_paged.h"

namespace umfa {

struct PagedFp8Params {
    PagedParams p;
    const float* kd;  // k_descale
    const float* vd;  // v_descale
    int64_t kdb, kdh, vdb, vdh;  // (batch, KV head) element strides, >= 0
};

bool paged_fp8_supported(const PagedFp8Params& q);
hipError_t launch_paged_fp8_append(const PagedFp8Params& q, hipStream_t stream);
hipError_t launch_fwd_16_paged_fp8(const PagedFp8Params& q, hipStream_t stream, const char** name);

}  // namespace umfa
