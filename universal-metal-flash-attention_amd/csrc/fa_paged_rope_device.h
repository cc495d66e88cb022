// fa_paged_rope_device.h -- the device pieces of the fused rotary pre-pass that fa_paged_rope.hip and the packed fp8 pre-pass of
// fa_fwd_16_paged_varlen_fp8.hip share: the rotation of one 8-element chunk (fa_paged_rope.h's rule and arithmetic) and the fp8
// quantiser (fa_paged_fp8.h's rule).  RP: the pre-pass's parameters -- cos, sin, rstride, seqlen_ro, rdim, interleaved.
#pragma once
#include "fa_common.h"  // rope_rotate8, f32x4

namespace umfa {

namespace {

typedef unsigned U4 __attribute__((ext_vector_type(4)));

// 8 consecutive elements e0 .. e0 + 7 of one head's row, rotated at table row `pos` (clamped) and rounded to T
template <typename T, typename TT, typename RP>
__device__ __forceinline__ auto rope_chunk(const RP& r, const T* __restrict__ row, uint32_t e0, uint32_t pos) {
    typedef T T8 __attribute__((ext_vector_type(8)));
    typedef TT TT4 __attribute__((ext_vector_type(4)));
    const T8 x = *(const T8*)(row + e0);
    if (e0 >= r.rdim) return x;
    const uint32_t tr = pos < r.seqlen_ro ? pos : r.seqlen_ro - 1;
    const TT* ct = (const TT*)r.cos + (int64_t)tr * r.rstride;
    const TT* st = (const TT*)r.sin + (int64_t)tr * r.rstride;
    float xf[8], yf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) xf[j] = (float)x[j];
    if (r.interleaved) {
        const TT4 c = *(const TT4*)(ct + e0 / 2), s = *(const TT4*)(st + e0 / 2);
        const f32x4 c0 = {(float)c[0], 0.0f, (float)c[1], 0.0f}, c1 = {(float)c[2], 0.0f, (float)c[3], 0.0f};
        const f32x4 s0 = {(float)s[0], 0.0f, (float)s[1], 0.0f}, s1 = {(float)s[2], 0.0f, (float)s[3], 0.0f};
        rope_rotate8(xf, c0, c1, s0, s1, false, yf);
    } else {
        const uint32_t half = r.rdim / 2;
        const bool lo = e0 < half;
        const uint32_t col = lo ? e0 : e0 - half;
        const T8 px = *(const T8*)(row + (lo ? e0 + half : e0 - half));
        const TT4 ca = *(const TT4*)(ct + col), cb = *(const TT4*)(ct + col + 4);
        const TT4 sa = *(const TT4*)(st + col), sb = *(const TT4*)(st + col + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float c = (float)(j < 4 ? ca[j & 3] : cb[j & 3]), s = (float)(j < 4 ? sa[j & 3] : sb[j & 3]);
            const float o = (float)px[j];
            // rope_rotate8's pair arithmetic (fa_common.h): this element is the pair's a (lower half) or its b (upper half)
            yf[j] = lo ? __builtin_fmaf(xf[j], c, -__fmul_rn(o, s)) : __builtin_fmaf(xf[j], c, __fmul_rn(o, s));
        }
        // the fp32 results are final here, as in rope_rotate8: no folding of the FMA into the conversion
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(yf[j]));
    }
    T8 y;
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = (T)yf[j];
    return y;
}

// fa_paged_fp8_append_kernel's quantiser: 16 operand-type values -> 16 e4m3fn bytes, e4m3fn_rne(clamp(fp32(x) / d, -448, 448))
template <typename T8>
__device__ __forceinline__ U4 quant16(const T8& x0, const T8& x1, float d) {
    float y[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        y[j] = fminf(fmaxf(__fdiv_rn((float)x0[j], d), -448.0f), 448.0f);
        y[8 + j] = fminf(fmaxf(__fdiv_rn((float)x1[j], d), -448.0f), 448.0f);
    }
    U4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        int v = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w], y[4 * w + 1], 0, false);
        v = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w + 2], y[4 * w + 3], v, true);
        o[w] = (unsigned)v;
    }
    return o;
}

}  // namespace


}  // namespace umfa
