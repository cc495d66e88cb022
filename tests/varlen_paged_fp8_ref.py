"""fp64 reference of packed variable-length queries over an fp8 (OCP e4m3fn) KV cache (umfa_torch.varlen_kvcache_attention with
k_descale / v_descale): per sequence, varlen_paged_ref.forward on the pool dequantised with that sequence's
descales.

A cache byte stands for E4M3FN[byte] * descale[b, h_kv] with b the SEQUENCE: a page shared by two sequences decodes under each one's own
descale.  Packed row t of sequence b is stored as e4m3fn_rne(clamp(fp32(x) / fp32(descale[b, h_kv]), -448, 448)) (paged_fp8_ref.quantise)
and attended as what was stored.  Ranges, lengths, clamps, dropped rows, masking and bottom-right causal: tests/varlen_paged_ref.py's.
"""
from __future__ import annotations

import numpy as np

import varlen_paged_ref
from paged_fp8_ref import dequantise, quantise  # noqa: F401  (re-exported: the tests quantise with the same functions)


def _bh(d, B, Hkv):
    return np.broadcast_to(np.asarray(d, np.float32), (B, Hkv))


def _one(cu, b):
    """cu_seqlens_q of sequence b alone (varlen_paged_ref.ranges clamps it exactly as it clamps the whole vector's entries)"""
    cu = np.asarray(cu, np.int64)
    return cu[b:b + 2]


def append(k8, v8, k_new, v_new, cu, max_q, cache_seqlens, k_descale, v_descale, block_table=None):
    """the byte caches after the packed quantising in-place append (copies): sequence by sequence, each row under its sequence's descales"""
    k8, v8 = np.array(k8, dtype=np.uint8, copy=True), np.array(v8, dtype=np.uint8, copy=True)
    if k_new is None:
        return k8, v8
    B, Hkv = len(np.asarray(cu)) - 1, k_new.shape[1]
    kd, vd = _bh(k_descale, B, Hkv), _bh(v_descale, B, Hkv)
    sl = np.asarray(cache_seqlens)
    for b in range(B):
        kq, vq = quantise(k_new, kd[b][None, :, None]), quantise(v_new, vd[b][None, :, None])
        if block_table is None:  # static: page b is sequence b's row
            k8[b:b + 1], v8[b:b + 1] = varlen_paged_ref.append(k8[b:b + 1], v8[b:b + 1], kq, vq, _one(cu, b), max_q, sl[b:b + 1], None)
        else:
            k8, v8 = varlen_paged_ref.append(k8, v8, kq, vq, _one(cu, b), max_q, sl[b:b + 1], np.asarray(block_table)[b:b + 1])
    return k8, v8


def forward(q, k8, v8, cu, max_q, cache_seqlens, k_descale, v_descale, block_table=None, k_new=None, v_new=None, causal=False, scale=None,
            kind=None):
    """(O [T_q, H, D], LSE [H, T_q], k8', v8'): varlen_paged_ref.forward, one sequence at a time, on the cache dequantised with that
    sequence's descales and the quantised-then-dequantised new tokens; rows no sequence covers stay 0 / -inf.

    kind ("fp16" / "bf16"): varlen_paged_ref.forward's format floor on the same dequantised post-append bytes.  K8 and V8 are exact in
    both operand types, so only P rounds.  kind None: the exact values, unchanged."""
    q = np.asarray(q, np.float64)
    k8, v8 = np.asarray(k8, np.uint8), np.asarray(v8, np.uint8)
    Tq, H, D = q.shape
    B, Hkv = len(np.asarray(cu)) - 1, k8.shape[2]
    kd, vd = _bh(k_descale, B, Hkv).astype(np.float64), _bh(v_descale, B, Hkv).astype(np.float64)
    out, lse = np.zeros((Tq, H, D)), np.full((H, Tq), -np.inf)
    sl = np.asarray(cache_seqlens)
    for b, (q0, Lq) in enumerate(varlen_paged_ref.ranges(cu, Tq, max_q)):
        if Lq == 0:
            continue
        dk, dv = kd[b][None, None, :, None], vd[b][None, None, :, None]
        kn = vn = None
        if k_new is not None:
            kn = dequantise(quantise(k_new, dk[0]), dk[0])
            vn = dequantise(quantise(v_new, dv[0]), dv[0])
        if block_table is None:
            kc, vc, bt = dequantise(k8[b:b + 1], dk), dequantise(v8[b:b + 1], dv), None
        else:
            kc, vc, bt = dequantise(k8, dk), dequantise(v8, dv), np.asarray(block_table)[b:b + 1]
        o, l, _, _ = varlen_paged_ref.forward(q, kc, vc, _one(cu, b), max_q, sl[b:b + 1], bt, kn, vn, causal, scale, kind)
        out[q0:q0 + Lq], lse[:, q0:q0 + Lq] = o[q0:q0 + Lq], l[:, q0:q0 + Lq]
    k8n, v8n = append(k8, v8, k_new, v_new, cu, max_q, cache_seqlens, k_descale, v_descale, block_table)
    return out, lse, k8n, v8n

