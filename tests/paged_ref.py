"""fp64 reference of KV-cache attention (umfa_torch.kvcache_attention): pages resolved through the block table,
the in-place append, the device-side clamps and bottom-right causal.

q [B, Sq, H, D]; paged: k_cache / v_cache [num_pages, page_size, H_kv, D] with block_table [B, max_pages]; static (block_table None):
k_cache / v_cache [B, S_max, H_kv, D] (page b = sequence b's row).  cache_seqlens [B].  k_new / v_new [B, S_new, H_kv, D].

Semantics (the kernels' contract):
  * L0 = clamp(cache_seqlens[b], 0, cap) with cap = max_pages * page_size (static: S_max); L_k = min(L0 + S_new, cap).
  * append: row i of k_new / v_new goes to position L0 + i if that is below cap and its page entry lies in [0, num_pages); else dropped.
  * key j < L_k is visible iff its page entry lies in [0, num_pages) (and, causal, j <= i + L_k - Sq for query i).
  * a row that sees no key: O = 0, LSE = -inf.
"""
from __future__ import annotations

import numpy as np


def _page(block_table, b, lp, num_pages, max_pages):
    if lp >= max_pages:
        return -1
    pg = b if block_table is None else int(block_table[b][lp])
    return pg if 0 <= pg < num_pages else -1


def geometry(k_cache, block_table, B):
    """(page_size, num_pages, max_pages, cap)"""
    if block_table is None:
        return k_cache.shape[1], B, 1, k_cache.shape[1]
    bt = np.asarray(block_table)
    return k_cache.shape[1], k_cache.shape[0], bt.shape[1], k_cache.shape[1] * bt.shape[1]


def lengths(cache_seqlens, S_new, cap):
    """[(L0, L_k)] per sequence, clamped as the kernels clamp them"""
    res = []
    for s in np.asarray(cache_seqlens, np.int64):
        L0 = int(min(max(s, 0), cap))
        res.append((L0, min(L0 + S_new, cap)))
    return res


def append(k_cache, v_cache, k_new, v_new, cache_seqlens, block_table=None):
    """the caches after the in-place append (copies; any array type with numpy indexing)"""
    k_cache, v_cache = np.array(k_cache, copy=True), np.array(v_cache, copy=True)
    if k_new is None:
        return k_cache, v_cache
    B, S_new = k_new.shape[0], k_new.shape[1]
    ps, num_pages, max_pages, cap = geometry(k_cache, block_table, B)
    for b, (L0, _) in enumerate(lengths(cache_seqlens, S_new, cap)):
        for i in range(S_new):
            pos = L0 + i
            if pos >= cap:
                continue
            pg = _page(block_table, b, pos // ps, num_pages, max_pages)
            if pg < 0:
                continue
            k_cache[pg, pos % ps] = k_new[b, i]
            v_cache[pg, pos % ps] = v_new[b, i]
    return k_cache, v_cache


def gather(k_cache, v_cache, cache_seqlens, S_new, block_table=None):
    """per sequence: (K [L_k, H_kv, D], V, valid [L_k] bool) of the (already appended) cache"""
    B = len(np.asarray(cache_seqlens))
    ps, num_pages, max_pages, cap = geometry(k_cache, block_table, B)
    res = []
    for b, (_, Lk) in enumerate(lengths(cache_seqlens, S_new, cap)):
        ks, vs, ok = [], [], []
        for j in range(Lk):
            pg = _page(block_table, b, j // ps, num_pages, max_pages)
            ok.append(pg >= 0)
            ks.append(k_cache[max(pg, 0), j % ps])
            vs.append(v_cache[max(pg, 0), j % ps])
        shape = (0,) + tuple(k_cache.shape[2:])
        res.append((np.array(ks, np.float64).reshape((-1,) + shape[1:]) if ks else np.zeros(shape),
                    np.array(vs, np.float64).reshape((-1,) + shape[1:]) if vs else np.zeros(shape), np.array(ok, bool)))
    return res


def round_p(p, kind):
    """the unnormalised P of the format floor: unchanged for kind None, else rounded once to `kind` ("fp16" / "bf16"), as fp64"""
    if kind is None:
        return p
    from dropout_ref import _round  # (the one numpy restatement of the two 16-bit roundings the test references share)
    return _round(np.asarray(p, np.float64), kind)


def forward(q, k_cache, v_cache, cache_seqlens, block_table=None, k_new=None, v_new=None, causal=False, scale=None, kind=None):
    """(O [B, Sq, H, D], LSE [B, H, Sq], k_cache', v_cache') in fp64, the caches after the append.

    kind ("fp16" / "bf16"): the FORMAT FLOOR instead of the exact O -- what an ideal flash kernel gives (oracle.flash_format_floor's idea
    on this module's visibility): P = exp(S - the row's exact max), rounded once to `kind`, in the numerator only; the scores, the
    denominator and V stay fp64.  V is taken as exact: a bf16 V enters the kernels' fp16 product as V 2^-e, exact except for values that
    fall into fp16's subnormals.  kind None returns the exact values, bit for bit what this function returned before it had the argument."""
    q = np.asarray(q, np.float64)
    B, Sq, H, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    kc, vc = append(np.asarray(k_cache, np.float64), np.asarray(v_cache, np.float64),
                    None if k_new is None else np.asarray(k_new, np.float64), None if v_new is None else np.asarray(v_new, np.float64),
                    cache_seqlens, block_table)
    S_new = 0 if k_new is None else k_new.shape[1]
    G = H // kc.shape[2]
    out = np.zeros((B, Sq, H, D))
    lse = np.full((B, H, Sq), -np.inf)
    for b, (K, V, ok) in enumerate(gather(kc, vc, cache_seqlens, S_new, block_table)):
        Lk = len(ok)
        vis = np.broadcast_to(ok[None, :], (Sq, Lk)).copy()
        if causal:
            vis &= np.arange(Lk)[None, :] <= np.arange(Sq)[:, None] + (Lk - Sq)
        live = vis.any(1)
        for h in range(H):
            s = q[b, :, h] @ K[:, h // G].T * scale if Lk else np.zeros((Sq, 0))
            s = np.where(vis, s, -np.inf)
            m = np.where(live, s.max(1, initial=-np.inf), 0.0)[:, None]
            p = np.where(vis, np.exp(s - m), 0.0)
            l = p.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                o = (round_p(p, kind) @ V[:, h // G]) / l[:, None] if Lk else np.zeros((Sq, D))
                lse[b, h] = np.where(live, np.log(l) + m[:, 0], -np.inf)
            out[b, :, h] = np.where(live[:, None], o, 0.0)
    return out, lse, kc, vc
