// fa_dropout.h -- the attention-dropout keep mask: ONE definition, shared by the forward (fa_fwd_16_drop.hip), both backward kernels
// (fa_bwd_16_drop.hip), the materialiser and the host (tests/test_dropout_rng_cpu.py compiles this header for the CPU).
//
// The mask is a pure function of logical coordinates, so every kernel produces identical bits whatever its tiling:
//   rng_state : device int64[2] = {seed, offset}, read by the kernels on the device
//   key  = (lo32(seed), hi32(seed))
//   ctr  = (j >> 2, i, b*H + h, lo32(offset))        i = query row, j = key, h = query head (absolute indices)
//   w    = Philox4x32-10(ctr, key)[j & 3]
//   t    = min(round(p * 2^32), 2^32 - 1)             0 < p < 1
//   keep = (w >= t)
//   s    = 2^32 / (2^32 - t)                          the exact inverse of the realised keep probability, rounded once to fp32
// One Philox call gives the words of the four keys 4 (j >> 2) ... + 3 of one row.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define UMFA_DROP_HD __host__ __device__ __forceinline__
#else
#define UMFA_DROP_HD inline
#endif

namespace umfa {

struct DropWords {
    uint32_t w[4];
};

UMFA_DROP_HD void drop_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
    const uint64_t r = (uint64_t)a * b;
    hi = (uint32_t)(r >> 32);
    lo = (uint32_t)r;
}

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
UMFA_DROP_HD DropWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        drop_mulhilo(0xD2511F53u, c0, hi0, lo0);
        drop_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return DropWords{{c0, c1, c2, c3}};
}

// keep bits of keys 4 jq ... 4 jq + 3 of query row i of slab bh (= b * H + h): bit e set = key 4 jq + e is kept
UMFA_DROP_HD uint32_t drop_keep4(uint32_t jq, uint32_t i, uint32_t bh, uint64_t seed, uint64_t offset, uint32_t thresh) {
    const DropWords w = philox4x32_10(jq, i, bh, (uint32_t)offset, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (uint32_t)(w.w[0] >= thresh) | ((uint32_t)(w.w[1] >= thresh) << 1) | ((uint32_t)(w.w[2] >= thresh) << 2) |
           ((uint32_t)(w.w[3] >= thresh) << 3);
}

// host: the threshold and the scale of probability p (0 < p < 1)
inline uint32_t drop_threshold(double p) {
    const double t = p * 4294967296.0;
    const double r = t - (double)(uint64_t)t >= 0.5 ? (double)(uint64_t)t + 1.0 : (double)(uint64_t)t;  // round half up
    return r >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)r;
}
inline float drop_scale(uint32_t thresh) { return (float)(4294967296.0 / (4294967296.0 - (double)thresh)); }

}  // namespace umfa
