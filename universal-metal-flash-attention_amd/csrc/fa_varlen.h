// fa_varlen.h -- packed variable-length attention (fa_fwd_16_varlen.hip, fa_bwd_16_varlen.hip, runtime_varlen.hip): the launch
// parameters, the per-sequence range every kernel reads from cu_seq_* on the device, and the LDS-DMA of rows with a token stride.
// Included only by the varlen translation units: no existing unit's device code depends on it.
//
// Layout: q [T_q, H, D], k / v [T_k, H_kv, D] with element strides (token, head; head_dim contiguous); out / dO / dQ dense [T_q, H, D],
// dK / dV dense [T_k, H_kv, D], lse fp32 [H, T_q].  Sequence n owns rows cu[n] .. cu[n+1]-1.  Causal is bottom-right per sequence:
// query i sees key j iff j <= i + (L_k - L_q).  The window form (fa_fwd_16_varlen_window.hip, fa_bwd_16_varlen_window.hip) bounds both
// sides: query i sees key j iff i + (L_k - L_q) - win_left <= j <= i + (L_k - L_q) + win_right (VARLEN_WIN_OPEN: unbounded).
#pragma once
#include <hip/hip_runtime.h>

#include "fa_bwd_16_common.h"  // d_off, make_srd, i32x4
#include "fa_common.h"

namespace umfa {

struct VarlenParams {
    const void* q;
    const void* k;
    const void* v;        // forward: bf16 operands -> the fp16 image of the cast pass (dense [H_kv, T_k, D], vst = D, vsh = T_k D)
    const void* dout;     // backward: dense [T_q, H, D], operand type
    const void* o;        // backward: the forward's O, dense [T_q, H, D], operand type (o_in_type) or fp32
    void* out;            // forward: dense [T_q, H, D], out_prec
    float* lse;           // forward: optional output; backward: input.  [H, T_q], natural log
    void* dq;             // backward: dense outputs, operand type (grad_in_type) or fp32
    void* dk;
    void* dv;
    float* rowc;          // backward scratch: 2 H T_q floats (-LSE log2 e, then -D), written by the dQ kernel for the dK / dV kernel
    const int32_t* cu_q;  // device int32 [N + 1]
    const int32_t* cu_k;
    const float* vsc;     // forward, bf16: the cast pass's slab headers (2^e of KV head hk in word VSC_HDR_WORDS hk + VSC_HDR_SCALE)
    int64_t qst, qsh, kst, ksh, vst, vsh;  // element strides: token, head
    uint32_t N, H, Hkv, D, Tq, Tk, max_q, max_k;
    float scale;
    int causal, in_prec, out_prec, o_in_type, grad_in_type;
    int win_left, win_right;  // window kernels only: the band's sides, each in [0, max_k] / [0, max_q] or VARLEN_WIN_OPEN
};

// an unbounded side of the window kernels' band: i + off +- VARLEN_WIN_OPEN stays inside int32 and past every key (lengths < 2^30)
constexpr int VARLEN_WIN_OPEN = 1 << 30;

bool varlen_supported(const VarlenParams& p);
hipError_t launch_fwd_16_varlen(const VarlenParams& p, hipStream_t stream, const char** name);
hipError_t launch_bwd_16_varlen(const VarlenParams& p, hipStream_t stream, const char** name);
hipError_t launch_fwd_16_varlen_window(const VarlenParams& p, hipStream_t stream, const char** name);
hipError_t launch_bwd_16_varlen_window(const VarlenParams& p, hipStream_t stream, const char** name);

// the window bounds the window kernels take (runtime_varlen.hip normalises them so)
inline bool varlen_window_ok(const VarlenParams& p) {
    return p.win_left >= 0 && p.win_right >= 0 && (p.win_left == VARLEN_WIN_OPEN || (uint32_t)p.win_left <= p.max_k) &&
           (p.win_right == VARLEN_WIN_OPEN || (uint32_t)p.win_right <= p.max_q);
}

namespace {

// rows [start, start + len) of sequence n: cu[n] and cu[n+1] clamped on the device into [0, T], the length to at most `cap` (max_q /
// max_k, the part the grid covers and the host's 32-bit offset check holds for).  Whatever cu holds, start + len <= T.  n is a
// workgroup-uniform index, so the two loads are scalar; readfirstlane makes the results provably uniform for the buffer descriptors.
__device__ __forceinline__ void varlen_range(const int32_t* cu, uint32_t n, uint32_t T, uint32_t cap, uint32_t& start, uint32_t& len) {
    int a = cu[n], b = cu[n + 1];
    a = a < 0 ? 0 : (a > (int)T ? (int)T : a);
    b = b < a ? a : (b > (int)T ? (int)T : b);
    const uint32_t l = (uint32_t)(b - a);
    start = (uint32_t)__builtin_amdgcn_readfirstlane(a);
    len = (uint32_t)__builtin_amdgcn_readfirstlane((int)(l < cap ? l : cap));
}

// bytes a buffer descriptor over `len` rows of `stride_b` bytes (the last one 2 D bytes long) may reach: every row < len is inside,
// every row >= len is range-checked away (stride_b >= 2 D)
__device__ __forceinline__ uint32_t varlen_bytes(uint32_t len, uint32_t stride_b, uint32_t row_b) {
    return len ? (len - 1) * stride_b + row_b : 0u;
}

// dma_rows (fa_bwd_16_common.h) for rows `stride_b` bytes apart in global memory: the LDS image is the same swizzled [rows][2 DP B]
// tile, only the source offset of row r is r * stride_b.  Rows past the descriptor's range land as zeros.
template <int NPIECES, int DP>
__device__ __forceinline__ void dma_rows_strided(const i32x4& srd, unsigned lds_dst, uint32_t row0, uint32_t stride_b, int uw, int lane) {
    constexpr int ROW_B = 2 * DP, NCH = DP / 8, RPP = 1024 / ROW_B;  // chunks per row, rows per piece
    const int r = lane / NCH, c = lane % NCH;
#pragma unroll
    for (int n0 = 0; n0 < NPIECES; n0 += 4) {
        const int n = n0 + uw;
        if (n < NPIECES) {
            const int row = RPP * n + r;
            const int voff = (int)((row0 + (uint32_t)row) * stride_b) + (d_off<DP>(row, c) - row * ROW_B);
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
                         ::"s"(lds_dst + n * 1024), "v"(voff), "s"(srd) : "memory");
        }
    }
}

}  // namespace

}  // namespace umfa
