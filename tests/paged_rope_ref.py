"""fp64 reference of the rotary embedding fused into the KV-cache attention calls (kvcache_attention / varlen_kvcache_attention with
rotary_cos / rotary_sin): the rotation, the position rules, the rounding to the operand type, and the whole call
composed with tests/paged_ref.py, tests/paged_fp8_ref.py and tests/varlen_paged_ref.py.

Tables cos / sin [seqlen_ro, rotary_dim / 2].  Non-interleaved (GPT-NeoX): element i pairs with i + rotary_dim / 2; interleaved: element
2i with 2i + 1; table column i either way; elements at rotary_dim and above pass through.  The pair (a, b) at column i, position p:
    a' = a cos[p, i] - b sin[p, i]        b' = b cos[p, i] + a sin[p, i]
Positions: new-key row t of sequence b at L0_b + t, L0_b = clamp(cache_seqlens[b], 0, cap); query row i at L0_b + i when causal, every
query row at L0_b when not.  A position >= seqlen_ro takes table row seqlen_ro - 1.  V is not rotated.  The call is then the plain call on
the rotated operands ROUNDED to the operand type ("bf16" / "fp16"): everything else is the plain references'.
"""
from __future__ import annotations

import numpy as np

import paged_fp8_ref
import paged_ref
import varlen_paged_ref

SIG_BITS = {"bf16": 8, "fp16": 11}  # significand bits, the hidden one included
MIN_ULP = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}  # the subnormal spacing


def ulp(x, operand):
    """spacing of the operand type at |x| (fp64 array)"""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))  # |x| = m 2^e, m in [0.5, 1)
    return np.maximum(np.ldexp(1.0, e - SIG_BITS[operand]), MIN_ULP[operand])


def round_operand(x, operand):
    """fp64 values rounded once, to nearest even, to the operand type (kept as fp64; no overflow handling: test values are small)"""
    x = np.asarray(x, np.float64)
    u = ulp(x, operand)
    return np.rint(x / u) * u


def pair_index(D, rotary_dim, interleaved):
    """(ia, ib): element indices of the a and b of pair i, i < rotary_dim / 2"""
    i = np.arange(rotary_dim // 2)
    return (2 * i, 2 * i + 1) if interleaved else (i, i + rotary_dim // 2)


def rotate(x, cos, sin, pos, interleaved=False, dtype=np.float64):
    """x [..., D] rotated row by row at positions pos (broadcastable to x.shape[:-1]); dtype: the working precision (fp64: the reference)"""
    x = np.asarray(x, dtype)
    cos, sin = np.asarray(cos, dtype), np.asarray(sin, dtype)
    seqlen_ro, half = cos.shape
    p = np.minimum(np.broadcast_to(np.asarray(pos, np.int64), x.shape[:-1]), seqlen_ro - 1)
    c, s = cos[p], sin[p]  # [..., half]
    ia, ib = pair_index(x.shape[-1], 2 * half, interleaved)
    a, b = x[..., ia], x[..., ib]
    y = x.copy()
    y[..., ia] = a * c - b * s
    y[..., ib] = b * c + a * s
    return y


def pair_magnitude(x, rotary_dim, interleaved):
    """|a| + |b| of the pair each element belongs to ([..., D]; 0 on the pass-through tail): the scale of the rotation's rounding bound"""
    x = np.abs(np.asarray(x, np.float64))
    ia, ib = pair_index(x.shape[-1], rotary_dim, interleaved)
    m = np.zeros_like(x)
    m[..., ia] = m[..., ib] = x[..., ia] + x[..., ib]
    return m


def positions(cache_seqlens, rows, cap, advance=True):
    """[B, rows]: clamp(cache_seqlens[b], 0, cap) + i (advance) or + 0 (the queries of a non-causal call)"""
    L0 = np.clip(np.asarray(cache_seqlens, np.int64), 0, cap)
    return L0[:, None] + (np.arange(rows)[None, :] if advance else np.zeros((1, rows), np.int64))


def packed_positions(cu, Tq, max_q, cache_seqlens, cap, advance=True):
    """(pos [T_q], covered [T_q]): row t of sequence b at L0_b + (t - start_b); rows no sequence covers are not rotated"""
    pos, cov = np.zeros(Tq, np.int64), np.zeros(Tq, bool)
    L0 = np.clip(np.asarray(cache_seqlens, np.int64), 0, cap)
    for b, (q0, Lq) in enumerate(varlen_paged_ref.ranges(cu, Tq, max_q)):
        pos[q0:q0 + Lq] = L0[b] + (np.arange(Lq) if advance else 0)
        cov[q0:q0 + Lq] = True
    return pos, cov


def operands(q, k_new, k_cache, cache_seqlens, cos, sin, block_table, causal, interleaved):
    """(R_q(q), R_k(k_new)) in fp64, not rounded: q [B, Sq, H, D], k_new [B, S_new, H_kv, D]"""
    B = q.shape[0]
    cap = paged_ref.geometry(k_cache, block_table, B)[3]
    pq = positions(cache_seqlens, q.shape[1], cap, causal)[:, :, None]
    pk = positions(cache_seqlens, k_new.shape[1], cap, True)[:, :, None]
    return rotate(q, cos, sin, pq, interleaved), rotate(k_new, cos, sin, pk, interleaved)


def packed_operands(q, k_new, k_cache, cu, max_q, cache_seqlens, cos, sin, block_table, causal, interleaved):
    """(R_q(q), R_k(k_new)) in fp64, not rounded: q [T_q, H, D], k_new [T_q, H_kv, D]; uncovered rows unchanged"""
    B = len(np.asarray(cu)) - 1
    cap = paged_ref.geometry(k_cache, block_table, B)[3]
    res = []
    for x, adv in ((q, causal), (k_new, True)):
        pos, cov = packed_positions(cu, x.shape[0], max_q, cache_seqlens, cap, adv)
        y = rotate(x, cos, sin, pos[:, None], interleaved)
        y[~cov] = np.asarray(x, np.float64)[~cov]
        res.append(y)
    return res


def forward(q, k_cache, v_cache, cache_seqlens, cos, sin, block_table=None, k_new=None, v_new=None, causal=False, scale=None,
            interleaved=False, operand="bf16"):
    """paged_ref.forward on the rotated operands rounded to the operand type: (O, LSE, k_cache', v_cache')"""
    rq, rk = operands(q, k_new, k_cache, cache_seqlens, cos, sin, block_table, causal, interleaved)
    return paged_ref.forward(round_operand(rq, operand), k_cache, v_cache, cache_seqlens, block_table, round_operand(rk, operand), v_new,
                             causal, scale)


def forward_fp8(q, k8, v8, cache_seqlens, k_descale, v_descale, cos, sin, block_table=None, k_new=None, v_new=None, causal=False, scale=None,
                interleaved=False, operand="bf16"):
    """paged_fp8_ref.forward on the rotated operands rounded to the operand type (the rounded key is what the quantiser sees)"""
    rq, rk = operands(q, k_new, k8, cache_seqlens, cos, sin, block_table, causal, interleaved)
    return paged_fp8_ref.forward(round_operand(rq, operand), k8, v8, cache_seqlens, k_descale, v_descale, block_table,
                                 round_operand(rk, operand), np.asarray(v_new, np.float64), causal, scale)


def forward_packed(q, k_cache, v_cache, cu, max_q, cache_seqlens, cos, sin, block_table=None, k_new=None, v_new=None, causal=False,
                   scale=None, interleaved=False, operand="bf16"):
    """varlen_paged_ref.forward on the rotated operands rounded to the operand type"""
    rq, rk = packed_operands(q, k_new, k_cache, cu, max_q, cache_seqlens, cos, sin, block_table, causal, interleaved)
    return varlen_paged_ref.forward(round_operand(rq, operand), k_cache, v_cache, cu, max_q, cache_seqlens, block_table,
                                    round_operand(rk, operand), v_new, causal, scale)
