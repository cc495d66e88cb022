"""fp64 reference of packed variable-length attention (umfa_torch.varlen_attention), per sequence.

q [T_q, H, D], k / v [T_k, H_kv, D] (any float arrays), cu_q / cu_k the N + 1 cumulative offsets.  Causal is BOTTOM-RIGHT aligned per
sequence: query i sees key j iff j <= i + (L_k - L_q) -- torch.nn.attention.bias.causal_lower_right, flash-attention's varlen
convention (tests/test_varlen_ref_cpu.py pins it to torch's own definition).  Query head h reads KV head h // (H // H_kv).  A row that
sees no key (L_k = 0, or causal with L_q > L_k) gives O = 0 and LSE = -inf.
"""
from __future__ import annotations

import numpy as np

from paged_ref import round_p


def visible(Lq: int, Lk: int, causal: bool) -> np.ndarray:
    """bool [Lq, Lk]: which keys each query of one sequence sees"""
    if not causal:
        return np.ones((Lq, Lk), bool)
    return np.arange(Lk)[None, :] <= np.arange(Lq)[:, None] + (Lk - Lq)


def seqs(cu_q, cu_k):
    """[(q0, Lq, k0, Lk)] per sequence"""
    cu_q, cu_k = np.asarray(cu_q, np.int64), np.asarray(cu_k, np.int64)
    return [(int(cu_q[n]), int(cu_q[n + 1] - cu_q[n]), int(cu_k[n]), int(cu_k[n + 1] - cu_k[n])) for n in range(len(cu_q) - 1)]


def forward(q, k, v, cu_q, cu_k, causal: bool = False, scale=None, kind=None):
    """(O [T_q, H, D], LSE [H, T_q]) in fp64; rows no sequence covers stay 0 / -inf.  kind ("fp16" / "bf16"): the format floor instead --
    P relative to the row's exact max, rounded once to `kind`, in the numerator only (scores, denominator and V in fp64; V is taken as
    exact); kind None: the exact values, unchanged."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Tq, H, D = q.shape
    G = H // k.shape[1]
    scale = D ** -0.5 if scale is None else scale
    out = np.zeros((Tq, H, D))
    lse = np.full((H, Tq), -np.inf)
    for q0, Lq, k0, Lk in seqs(cu_q, cu_k):
        if Lq == 0 or Lk == 0:
            continue
        vis = visible(Lq, Lk, causal)
        live = vis.any(1)
        for h in range(H):
            s = q[q0:q0 + Lq, h] @ k[k0:k0 + Lk, h // G].T * scale
            s = np.where(vis, s, -np.inf)
            m = np.where(live, s.max(1), 0.0)[:, None]
            p = np.exp(s - m)
            l = p.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                o = (round_p(p, kind) @ v[k0:k0 + Lk, h // G]) / l[:, None]
                lse[h, q0:q0 + Lq] = np.where(live, np.log(l) + m[:, 0], -np.inf)
            out[q0:q0 + Lq, h] = np.where(live[:, None], o, 0.0)
    return out, lse


def backward(dout, q, k, v, cu_q, cu_k, causal: bool = False, scale=None):
    """(dQ [T_q, H, D], dK / dV [T_k, H_kv, D]) in fp64, the grouped heads' dK / dV summed"""
    dout, q, k, v = (np.asarray(a, np.float64) for a in (dout, q, k, v))
    Tq, H, D = q.shape
    G = H // k.shape[1]
    scale = D ** -0.5 if scale is None else scale
    o, lse = forward(q, k, v, cu_q, cu_k, causal, scale)
    dq, dk, dv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    for q0, Lq, k0, Lk in seqs(cu_q, cu_k):
        if Lq == 0 or Lk == 0:
            continue
        vis = visible(Lq, Lk, causal)
        for h in range(H):
            kh = h // G
            rq, rk = slice(q0, q0 + Lq), slice(k0, k0 + Lk)
            s = q[rq, h] @ k[rk, kh].T * scale
            L = lse[h, rq][:, None]
            p = np.where(vis & np.isfinite(L), np.exp(np.where(vis, s, 0.0) - np.where(np.isfinite(L), L, 0.0)), 0.0)
            dp = dout[rq, h] @ v[rk, kh].T
            ds = p * (dp - (dout[rq, h] * o[rq, h]).sum(1)[:, None])
            dq[rq, h] += scale * ds @ k[rk, kh]
            dk[rk, kh] += scale * ds.T @ q[rq, h]
            dv[rk, kh] += p.T @ dout[rq, h]
    return dq, dk, dv
