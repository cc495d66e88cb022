// fa_bwd_16_common.h -- pieces of the bf16 / fp16 MFMA backward shared by fa_bwd_16.hip (the unmasked kernels) and
// fa_bwd_16_mask.hip (their masked / sliding-window counterparts): the dual-use LDS image geometry, LDS-DMA staging,
// transposed-read fragments, gradient stores, causal work order.  Each translation unit gets its own copy (internal linkage).
#pragma once
#include <hip/hip_runtime.h>

#include "fa_common.h"
#include "fa_fwd_16_kernel.h"  // Mma16<T>, LDS_AS

namespace umfa {

namespace {

// geometry of one head_dim: 16-key MFMA steps, 32-column d-blocks, 32-row tiles of 2*DP-byte rows
#define BWD16_GEO(DP)                                                                    \
    constexpr int ROW_B = 2 * DP, NKS = DP / 16, NDB = DP / 32, TILE_BYTES = 32 * ROW_B; \
    constexpr int TILE_PIECES = TILE_BYTES / 1024;                                       \
    constexpr int PD = DP >= 128 ? 4 : 2; /* k-steps of LDS row fragments in flight ahead of their MFMAs */ \
    constexpr int NH = DP == 256 ? 2 : 1; /* dkdv: passes over the query range, each owning NDB / NH d-blocks of dK, dV */ \
    [[maybe_unused]] constexpr int NDBH = NDB / NH

template <int DP>
__device__ __forceinline__ constexpr int d_off(int row, int ch) {
    static_assert(DP == 256 || DP == 128 || DP == 64, "swizzles exist for 512-, 256- and 128-byte rows");
    // rows of 256 and 512 bytes all start at bank 0, so they share one swizzle (on the low four chunk-index bits)
    const int f = DP >= 128 ? (((row & 3) << 2) | ((row >> 2) & 3)) : (((row >> 2) & 3) | (((row >> 1) & 1) << 2));
    return 2 * DP * row + 16 * (ch ^ f);
}

__device__ __forceinline__ i32x4 make_srd(const void* base, uint32_t bytes) {
    const unsigned long long a = (unsigned long long)base;
    i32x4 d;
    d[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
    d[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu));
    d[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    d[3] = 0x00020000;
    return d;
}

// LDS-DMA of `npieces` 1-KiB pieces (4 or 8 rows each) of a [rows][2*DP B] slab image starting at global row `row0`.
// Piece n goes to lds_dst + n KiB; wave w issues pieces w, w+4, ...  Rows past the slab are range-checked away.
template <int NPIECES, int DP>
__device__ __forceinline__ void dma_rows(const i32x4& srd, unsigned lds_dst, uint32_t row0, int uw, int lane) {
    constexpr int ROW_B = 2 * DP, NCH = DP / 8, RPP = 1024 / ROW_B;  // chunks per row, rows per piece
    const int r = lane / NCH, c = lane % NCH;
#pragma unroll
    for (int n0 = 0; n0 < NPIECES; n0 += 4) {
        const int n = n0 + uw;
        if (n < NPIECES) {
            const int row = RPP * n + r;
            const int voff = (int)(row0 + row) * ROW_B + (d_off<DP>(row, c) - row * ROW_B);
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                         ::"s"(lds_dst + n * 1024), "v"(voff), "s"(srd) : "memory");
        }
    }
}

// The same with the lane-dependent part of every piece's source offset computed ONCE (dma_lane_offsets, before the tile
// loop): per tile one scalar multiply and one vector add per piece are left.  As dma_rows inside the loop the row / chunk /
// swizzle arithmetic of all pieces was redone for every tile: ~540 of ~3600 cycles per tile of bwd16_dkdv (phase stamps,
// tools/lab/bwd_stamps.py).
template <int NPIECES, int DP>
__device__ __forceinline__ void dma_lane_offsets(int (&off)[(NPIECES + 3) / 4], int uw, int lane) {
    constexpr int NCH = DP / 8, RPP = 1024 / (2 * DP);
    const int r = lane / NCH, c = lane % NCH;
#pragma unroll
    for (int i = 0; i < (NPIECES + 3) / 4; ++i) {
        const int row = RPP * (4 * i + uw) + r;
        off[i] = d_off<DP>(row, c);  // = row * ROW_B + 16 * (c ^ swizzle(row))
    }
}
template <int NPIECES, int DP>
__device__ __forceinline__ void dma_rows_pre(const i32x4& srd, unsigned lds_dst, uint32_t row0, int uw, const int (&off)[(NPIECES + 3) / 4]) {
    constexpr int ROW_B = 2 * DP;
    const int base = (int)row0 * ROW_B;
#pragma unroll
    for (int i = 0; i < (NPIECES + 3) / 4; ++i) {
        const int n = 4 * i + uw;
        if (n < NPIECES) {
            const int voff = base + off[i];
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                         ::"s"(lds_dst + n * 1024), "v"(voff), "s"(srd) : "memory");
        }
    }
}

// one 1-KiB piece of an LDS-DMA tile (see dma_rows_pre)
__device__ __forceinline__ void dma_piece(const i32x4& srd, unsigned lds_dst, int voff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_dst), "v"(voff), "s"(srd) : "memory");
}

// transposed-read fragment: rows (row0 .. +3) and (row0+8 .. +11) x 16 columns of d-block i, as the A operand whose
// element j is image row 16 s + 8 (j>>2) + 4 hi + (j&3) (the k order of an accumulator used as B operand)
template <typename M, int DP>
__device__ __forceinline__ typename M::V8 tr_frag(const char* img, int i, int s, int hi, int tr_qq, int tr_pp, int tr_g1) {
    const int ch = 4 * i + 2 * tr_g1 + (tr_pp >> 1);
    const int r0 = 16 * s + 4 * hi + tr_qq;
    const typename M::V4 lo = M::tr_read(img + d_off<DP>(r0, ch) + 8 * (tr_pp & 1));
    const typename M::V4 hi4 = M::tr_read(img + d_off<DP>(r0 + 8, ch) + 8 * (tr_pp & 1));
    return __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
}

// four consecutive gradient elements: fp32 (ABI contract) or rounded once to the input type T
template <typename T>
__device__ __forceinline__ void store_grad4(void* base, int64_t elem, f32x4 val, bool in_type) {
    if (in_type) {
        typedef T T4 __attribute__((ext_vector_type(4)));
        *(T4*)((T*)base + elem) = T4{(T)val[0], (T)val[1], (T)val[2], (T)val[3]};
    } else {
        *(f32x4*)((float*)base + elem) = val;
    }
}

// Causal work items differ in length; with two workgroups per CU they finish together only if the lengths on a CU add
// up alike.  Same order as the forward (fa_fwd_16_kernel.h, where it was measured): consecutive items are a mirrored
// pair of blocks, and the pair 32 items (= CUs per XCD) further on has its long and short member swapped.
// Returns the block's rank by length (0 = longest) and its (batch, head).  Only when every workgroup of the launch is
// resident at once (two per CU): with more workgroups than slots the dispatcher refills slots as they free up and
// plain longest-first order is the better schedule (B1 H16 S8192 causal backward: 1.52 ms vs 1.92 ms paired).
__device__ __forceinline__ uint32_t causal_rank(uint32_t item, uint32_t nblk, uint32_t& bh, bool two_per_cu) {
    if ((nblk & 1) || !two_per_cu || gridDim.x > 512) { bh = item / nblk; return item % nblk; }
    const uint32_t pi = item >> 1, h2 = nblk >> 1, j = pi % h2;
    bh = pi / h2;
    return (((item & 1) ^ (item >> 5)) & 1) ? nblk - 1 - j : j;
}

}  // namespace

// (batch, key/value head) slab that query head `bh` attends to: grouped-query attention without expanded K / V copies
__device__ __forceinline__ uint32_t bwd16_kv_slab(const BwdParams& p, uint32_t bh) {
    if (p.Hkv == 0 || p.Hkv == p.H) return bh;
    return (bh / p.H) * p.Hkv + (bh % p.H) / (p.H / p.Hkv);
}

}  // namespace umfa
