"""numpy restatement of the attention-dropout definition (csrc/fa_dropout.h) and an fp64 dropout SDPA, forward and backward.

keep[b, h, i, j] = Philox4x32-10(ctr = (j >> 2, i, b*H + h, lo32(offset)), key = (lo32(seed), hi32(seed)))[j & 3] >= t,
t = min(round(p 2^32), 2^32 - 1), s = 2^32 / (2^32 - t) rounded once to fp32.  O = s (keep o P) V, LSE undropped.
The backward also returns a dropout-aware FORMAT FLOOR: an ideal 16-bit backward that rounds keep o P once before dV and dS once before
dK / dQ (the roundings the kernels make), everything else fp64 -- oracle.flash_backward_format_floor's idea with the mask in it.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counters as uint32-valued arrays (broadcast), key words as Python ints."""
    c = [np.asarray(x, np.uint64) & MASK32 for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(p: float) -> int:
    t = int(np.floor(float(p) * 4294967296.0 + 0.5))
    return min(t, 0xFFFFFFFF)


def keep_scale(p: float) -> float:
    return float(np.float32(4294967296.0 / (4294967296.0 - threshold(p))))


def _u64(x: int) -> int:
    return int(x) & 0xFFFFFFFFFFFFFFFF


def keep_bits(i, j, bh, seed: int, offset: int, thresh: int):
    """keep decisions at broadcast coordinates (query row i, key j, slab bh = b*H + h)."""
    seed, offset = _u64(seed), _u64(offset)
    i, j, bh = (np.asarray(x, np.uint64) for x in (i, j, bh))
    w = philox4x32_10(j >> np.uint64(2), i, bh, np.uint64(offset & 0xFFFFFFFF), seed & 0xFFFFFFFF, seed >> 32)
    jj = np.broadcast_to(j & np.uint64(3), w[0].shape)
    word = np.choose(jj.astype(np.int64), w)
    return word >= np.uint32(thresh)


def keep_mask(B, H, Sq, Skv, p, seed, offset):
    """dense keep [B, H, Sq, Skv] (bool)"""
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    i = np.arange(Sq, dtype=np.uint64).reshape(1, 1, Sq, 1)
    j = np.arange(Skv, dtype=np.uint64).reshape(1, 1, 1, Skv)
    return keep_bits(i, j, bh, seed, offset, threshold(p))


def _f64(a):
    a = np.asarray(a)
    if a.dtype == np.uint16:  # bf16 bits
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def _exp(Q, K, scale, causal):
    """(exp(S - row max), its row sums [.., 1], the row max [.., 1])"""
    s = np.einsum("bhid,bhjd->bhij", Q, K) * scale
    if causal:
        Sq, Skv = s.shape[-2:]
        s = np.where(np.arange(Skv)[None, :] <= np.arange(Sq)[:, None], s, -np.inf)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    return e, e.sum(-1, keepdims=True), m


def _softmax(Q, K, scale, causal):
    e, l, m = _exp(Q, K, scale, causal)
    return e / l, (m + np.log(l))[..., 0]


def forward(q, k, v, keep, p, *, scale, causal=False, kind=None):
    """fp64 O = s (keep o P) V and the undropped LSE [B, H, Sq].

    kind ('bf16' / 'fp16'): the FORMAT FLOOR instead of the exact O: keep o exp(S - the row's exact max) rounded once to `kind` in the
    numerator only; the scores, the (undropped) denominator, s and V stay fp64.  V is taken as exact: a bf16 V enters the kernels' fp16
    product as V 2^-e, exact except for values that fall into fp16's subnormals.  kind None: the exact values, unchanged."""
    Q, K, V = _f64(q), _f64(k), _f64(v)
    if kind is not None:
        e, l, m = _exp(Q, K, scale, causal)
        return keep_scale(p) * np.einsum("bhij,bhjd->bhid", _round(e * keep, kind), V) / l, (m + np.log(l))[..., 0]
    P, lse = _softmax(Q, K, scale, causal)
    return keep_scale(p) * np.einsum("bhij,bhjd->bhid", P * keep, V), lse


def _round(x, kind):
    if kind == "fp16":
        return x.astype(np.float16).astype(np.float64)
    f = x.astype(np.float32)  # bf16: round to nearest even on the fp32 bits
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def backward(dout, q, k, v, out, keep, p, *, scale, causal=False, kind=None):
    """fp64 (dq, dk, dv) of the dropout SDPA, given the O the forward returned; with kind ('bf16' / 'fp16') the format floor instead:
    keep o P rounded once before dV, dS once before dK / dQ."""
    Q, K, V, dO, O = (_f64(a) for a in (q, k, v, dout, out))
    P, _ = _softmax(Q, K, scale, causal)
    s = keep_scale(p)
    Pk = P * keep
    dP = s * keep * np.einsum("bhid,bhjd->bhij", dO, V)
    D = (dO * O).sum(-1, keepdims=True)
    dS = P * (dP - D)
    if kind is not None:
        Pk, dS = _round(Pk, kind), _round(dS, kind)
    dv = s * np.einsum("bhij,bhid->bhjd", Pk, dO)
    dq = scale * np.einsum("bhij,bhjd->bhid", dS, K)
    dk = scale * np.einsum("bhij,bhid->bhjd", dS, Q)
    return dq, dk, dv
