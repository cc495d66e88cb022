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

// the device pieces of the fp8 stage ring, shared by fa_fwd_16_paged_fp8.hip and fa_fwd_16_paged_varlen_fp8.hip
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// lane l: the physical page of 16-key group l of super-step S (keys 1024 S + 16 l ..), -1 for an entry outside the pool or a group at or
// past L_k
__device__ __forceinline__ int paged8_table(const PagedParams& p, uint32_t b, uint32_t Lk, uint32_t S, int lane) {
    const uint64_t key = (uint64_t)S * 1024 + 16 * (uint32_t)lane;
    return key < Lk ? paged_page(p, b, paged_lpage(p, (uint32_t)key)) : -1;
}

// LDS-DMA of step s of one fp8 cache tensor (KV head at head_b bytes) into the linear stage at lds_dst: piece n (RPP rows of DP bytes)
// goes to lds_dst + n KiB, wave uw requests pieces uw, uw + 4, ...  tab: paged8_table of super-step s / 8.
template <int DP>
__device__ __forceinline__ void paged8_dma_step(const PagedParams& p, const char* pool, int64_t page_b, int64_t head_b, uint32_t tst_b,
                                                int tab, uint32_t Lk, uint32_t s, unsigned lds_dst, int uw, int lane) {
    constexpr int NCH = DP / 16, RPP = 1024 / DP, NP = 128 / RPP;
    const int r = lane / NCH, c = lane % NCH;
#pragma nounroll
    for (int n0 = 0; n0 < NP; n0 += 4) {
        const int n = n0 + uw;
        const uint32_t key0 = s * 128 + (uint32_t)(RPP * n);
        const uint32_t lp = paged_lpage(p, key0);
        const int pg = __builtin_amdgcn_readlane(tab, (int)(8 * (s & 7)) + (RPP * n) / 16);
        const uint32_t pstart = lp * p.page_size;
        uint32_t nv = Lk > pstart ? Lk - pstart : 0u;
        nv = nv < p.page_size ? nv : p.page_size;
        const uint32_t bytes = pg >= 0 && nv ? (nv - 1) * tst_b + DP : 0u;
        const i32x4 srd = make_srd(pool + (int64_t)(pg >= 0 ? pg : 0) * page_b + head_b, bytes);
        const int voff = (int)((key0 - pstart + (uint32_t)r) * tst_b) + 16 * c;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                     ::"s"(lds_dst + n * 1024), "v"(voff), "s"(srd) : "memory");
    }
}

// four e4m3fn bytes -> four T (exact)
template <typename T>
__device__ __forceinline__ void fp8x4_expand(unsigned w, unsigned& lo, unsigned& hi) {
    if constexpr (std::is_same<T, __bf16>::value) {
        lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
        hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
    } else {
        lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
        hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
    }
}

// piece n of a stage (this wave's own) -> rows RPP n .. of the 16-bit image
template <typename T, int DP>
__device__ __forceinline__ void fp8_expand_piece(const char* stage, char* img, int n, int lane) {
    constexpr int NCH = DP / 16, RPP = 1024 / DP;
    const int r = lane / NCH, c = lane % NCH, row = RPP * n + r;
    const u32x4 x = *(const u32x4*)(stage + n * 1024 + lane * 16);
    unsigned e[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) fp8x4_expand<T>(x[j], e[2 * j], e[2 * j + 1]);
    const u32x4 a = {e[0], e[1], e[2], e[3]}, b2 = {e[4], e[5], e[6], e[7]};
    const bool sw = DP == 128 ? (c >> 2) & 1 : r & 1;  // which chunk goes first (banks: file header)
    const u32x4 first = sw ? b2 : a, second = sw ? a : b2;
    *(u32x4*)(img + d_off<DP>(row, 2 * c + (sw ? 1 : 0))) = first;
    *(u32x4*)(img + d_off<DP>(row, 2 * c + (sw ? 0 : 1))) = second;
}

}  // namespace

}  // namespace umfa
