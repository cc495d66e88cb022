"""fp64 reference of KV-cache attention over an fp8 (OCP e4m3fn) cache (umfa_torch.kvcache_attention with k_descale / v_descale; DESIGN.md
section 3.1j): the decode table, the append's quantiser, and forward() = paged_ref.forward on the dequantised caches.

A cache byte stands for E4M3FN[byte] * descale[b, h_kv].  New tokens are stored as e4m3fn_rne(clamp(fp32(x) / fp32(descale), -448, 448))
and attended as what was stored (quantised, then dequantised).  Everything else -- pages, clamps, masking, bottom-right causal -- is
tests/paged_ref.py's.
"""
from __future__ import annotations

import numpy as np

import paged_ref


def _decode(byte: int) -> float:
    s, e, m = byte >> 7, (byte >> 3) & 15, byte & 7
    if e == 15 and m == 7:
        return float("nan")  # e4m3fn: no infinities, one NaN per sign
    v = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


E4M3FN = np.array([_decode(b) for b in range(256)], np.float64)  # value of each byte
_POS = E4M3FN[:127]  # the finite non-negative values, ascending: byte = index


def dequantise(bytes_, descale=1.0):
    """fp64 values of uint8 e4m3fn bytes times a (broadcastable) descale: exact, both factors are short"""
    return E4M3FN[np.asarray(bytes_, np.uint8)] * np.asarray(descale, np.float64)


def quantise(x, descale):
    """uint8 e4m3fn bytes of x (any float array) under a broadcastable descale: fp32 IEEE division, clamp to +-448, round to nearest even"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        y = (np.asarray(x, np.float32) / np.asarray(descale, np.float32)).astype(np.float32)
    y = np.clip(y, np.float32(-448), np.float32(448)).astype(np.float64)
    a = np.abs(y)
    hi = np.clip(np.searchsorted(_POS, a, side="left"), 0, 126)  # first value >= a
    lo = np.clip(hi - 1, 0, 126)
    dlo, dhi = a - _POS[lo], _POS[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))  # a tie goes to the even mantissa = the even byte
    byte = np.where(pick_hi, hi, lo).astype(np.uint8)
    return (byte | (np.signbit(y).astype(np.uint8) << 7)).astype(np.uint8)


def _bh(d, B, Hkv):
    return np.broadcast_to(np.asarray(d, np.float32), (B, Hkv))


def append(k8, v8, k_new, v_new, cache_seqlens, k_descale, v_descale, block_table=None):
    """the byte caches after the quantising in-place append (copies)"""
    if k_new is None:
        return np.array(k8, copy=True), np.array(v8, copy=True)
    B, Hkv = k_new.shape[0], k_new.shape[2]
    kq = quantise(k_new, _bh(k_descale, B, Hkv)[:, None, :, None])
    vq = quantise(v_new, _bh(v_descale, B, Hkv)[:, None, :, None])
    return paged_ref.append(np.asarray(k8, np.uint8), np.asarray(v8, np.uint8), kq, vq, cache_seqlens, block_table)


def forward(q, k8, v8, cache_seqlens, k_descale, v_descale, block_table=None, k_new=None, v_new=None, causal=False, scale=None, kind=None):
    """(O [B, Sq, H, D], LSE [B, H, Sq], k8', v8'): paged_ref.forward, one sequence at a time, on the cache dequantised with that
    sequence's descales (a page shared by two sequences decodes under each one's own) and the quantised-then-dequantised new tokens.

    kind ("fp16" / "bf16"): paged_ref.forward's format floor on the same dequantised post-append bytes (the append quantises, so the new
    tokens enter as what was stored).  K8 and V8 are exact in both operand types, so only P rounds; V is taken as exact.  kind None: the
    exact values, unchanged."""
    q = np.asarray(q, np.float64)
    k8, v8 = np.asarray(k8, np.uint8), np.asarray(v8, np.uint8)
    B, Sq, H, D = q.shape
    Hkv = k8.shape[2]
    kd, vd = _bh(k_descale, B, Hkv).astype(np.float64), _bh(v_descale, B, Hkv).astype(np.float64)
    out, lse = np.zeros((B, Sq, H, D)), np.full((B, H, Sq), -np.inf)
    sl = np.asarray(cache_seqlens)
    for b in range(B):
        dk, dv = kd[b][None, None, :, None], vd[b][None, None, :, None]
        kn = vn = None
        if k_new is not None:
            kn = dequantise(quantise(k_new[b:b + 1], dk), dk)
            vn = dequantise(quantise(v_new[b:b + 1], dv), dv)
        if block_table is None:  # static: page b is sequence b's row
            kc, vc, bt = dequantise(k8[b:b + 1], dk), dequantise(v8[b:b + 1], dv), None
        else:
            kc, vc, bt = dequantise(k8, dk), dequantise(v8, dv), np.asarray(block_table)[b:b + 1]
        o, l, _, _ = paged_ref.forward(q[b:b + 1], kc, vc, sl[b:b + 1], bt, kn, vn, causal, scale, kind)
        out[b], lse[b] = o[0], l[0]
    k8n, v8n = append(k8, v8, k_new, v_new, cache_seqlens, k_descale, v_descale, block_table)
    return out, lse, k8n, v8n
