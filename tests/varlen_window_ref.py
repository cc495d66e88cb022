"""fp64 reference of packed variable-length attention with a sliding window (umfa_torch.varlen_attention(window_size=...), DESIGN.md
section 3.1h), per sequence.

flash-attention's window_size = (left, right), bottom-right per sequence: with off = L_k - L_q, query i sees key j iff 0 <= j < L_k,
(left < 0 or j >= i + off - left) and (right < 0 or j <= i + off + right); -1 is unbounded, causal sets right = 0.  With L_q == L_k it
is the dense sliding window i - left <= j <= i + right.  Layout, grouping and the conventions for rows that see no key are those of
tests/varlen_ref.py (tests/test_varlen_window_ref_cpu.py pins this module to torch SDPA with an explicit mask).
"""
from __future__ import annotations

import numpy as np

import varlen_ref
from varlen_ref import seqs  # noqa: F401  (re-exported: [(q0, Lq, k0, Lk)] per sequence)


def visible(Lq: int, Lk: int, causal: bool = False, window=(-1, -1)) -> np.ndarray:
    """bool [Lq, Lk]: which keys each query of one sequence sees"""
    left, right = window
    if causal:
        right = 0
    i = np.arange(Lq)[:, None] + (Lk - Lq)
    j = np.arange(Lk)[None, :]
    vis = np.ones((Lq, Lk), bool)
    if left >= 0:
        vis &= j >= i - left
    if right >= 0:
        vis &= j <= i + right
    return vis


def _with_window(fn, causal, window):
    """run varlen_ref's per-sequence loop with this module's visibility"""
    saved = varlen_ref.visible
    varlen_ref.visible = lambda Lq, Lk, _causal: visible(Lq, Lk, causal, window)
    try:
        return fn()
    finally:
        varlen_ref.visible = saved


def forward(q, k, v, cu_q, cu_k, causal: bool = False, window=(-1, -1), scale=None, kind=None):
    """(O [T_q, H, D], LSE [H, T_q]) in fp64; rows that see no key: O = 0, LSE = -inf.

    kind ("fp16" / "bf16"): the FORMAT FLOOR on the band's visibility instead of the exact O: P = exp(S - the row's exact max over the keys
    it sees), rounded once to `kind`, in the numerator only; scores, denominator and V stay fp64.  V is taken as exact: a bf16 V enters the
    kernels' fp16 product as V 2^-e, exact except for values that fall into fp16's subnormals.  kind None: the exact values, unchanged."""
    return _with_window(lambda: varlen_ref.forward(q, k, v, cu_q, cu_k, True, scale, kind), causal, window)


def backward(dout, q, k, v, cu_q, cu_k, causal: bool = False, window=(-1, -1), scale=None):
    """(dQ [T_q, H, D], dK / dV [T_k, H_kv, D]) in fp64, the grouped heads' dK / dV summed"""
    return _with_window(lambda: varlen_ref.backward(dout, q, k, v, cu_q, cu_k, True, scale), causal, window)
