"""fp64 reference of packed variable-length queries over a paged / static KV cache (umfa_torch.varlen_kvcache_attention, DESIGN.md
section 3.1k), built on tests/paged_ref.py's page, geometry and clamp helpers.

q [T_q, H, D], cu_seqlens_q [B + 1], max_seqlen_q; the caches, block_table and cache_seqlens as paged_ref takes them; k_new / v_new
[T_q, H_kv, D], packed by the same cu_seqlens_q.

Semantics (the kernels' contract):
  * sequence b's rows: start = clamp(cu[b], 0, T_q), end = clamp(cu[b+1], start, T_q), L_q = min(end - start, max_seqlen_q).
  * L0 = clamp(cache_seqlens[b], 0, cap); L_k = min(L0 + L_q, cap) with new tokens, L0 without.
  * append: row i of sequence b goes to position L0 + i if that is below cap and its page entry lies in [0, num_pages); else dropped.
  * key j < L_k is visible iff its page entry lies in [0, num_pages) and (causal) j <= i + L_k - L_q for query i of the sequence.
  * a row that sees no key: O = 0, LSE = -inf.  Rows no sequence covers are not written (`covered` tells which are).
Results are defined for non-decreasing cu with cu[B] <= T_q; the clamps above are what the kernels do with anything else.
"""
from __future__ import annotations

import numpy as np

import paged_ref


def ranges(cu, Tq, max_q):
    """[(start, L_q)] per sequence, clamped as the kernels clamp them"""
    cu = np.asarray(cu, np.int64)
    res = []
    for b in range(len(cu) - 1):
        a = int(min(max(cu[b], 0), Tq))
        e = int(min(max(cu[b + 1], a), Tq))
        res.append((a, min(e - a, int(max_q))))
    return res


def lengths(cache_seqlens, lq, cap, has_new):
    """[(L0, L_k)] per sequence (lq: each sequence's L_q)"""
    return [paged_ref.lengths([s], l if has_new else 0, cap)[0] for s, l in zip(np.asarray(cache_seqlens, np.int64), lq)]


def append(k_cache, v_cache, k_new, v_new, cu, max_q, cache_seqlens, block_table=None):
    """the caches after the packed in-place append (copies; any array type with numpy indexing)"""
    k_cache, v_cache = np.array(k_cache, copy=True), np.array(v_cache, copy=True)
    if k_new is None:
        return k_cache, v_cache
    B = len(np.asarray(cu)) - 1
    ps, num_pages, max_pages, cap = paged_ref.geometry(k_cache, block_table, B)
    rg = ranges(cu, k_new.shape[0], max_q)
    for b, ((q0, Lq), (L0, _)) in enumerate(zip(rg, lengths(cache_seqlens, [r[1] for r in rg], cap, True))):
        for i in range(Lq):
            pos = L0 + i
            if pos >= cap:
                continue
            pg = paged_ref._page(block_table, b, pos // ps, num_pages, max_pages)
            if pg < 0:
                continue
            k_cache[pg, pos % ps] = k_new[q0 + i]
            v_cache[pg, pos % ps] = v_new[q0 + i]
    return k_cache, v_cache


def covered(cu, Tq, max_q):
    """bool [T_q]: the rows some sequence owns"""
    cov = np.zeros(Tq, bool)
    for q0, Lq in ranges(cu, Tq, max_q):
        cov[q0:q0 + Lq] = True
    return cov


def forward(q, k_cache, v_cache, cu, max_q, cache_seqlens, block_table=None, k_new=None, v_new=None, causal=False, scale=None, kind=None):
    """(O [T_q, H, D], LSE [H, T_q], k_cache', v_cache') in fp64, the caches after the append; rows no sequence covers stay 0 / -inf.

    kind ("fp16" / "bf16"): the format floor (paged_ref.forward): P relative to the row's exact max, rounded once to `kind`, in the
    numerator only; scores, denominator and V in fp64.  V is taken as exact: a bf16 V enters the kernels' fp16 product as V 2^-e, exact
    except for values that fall into fp16's subnormals.  kind None: the exact values, unchanged."""
    q = np.asarray(q, np.float64)
    Tq, H, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    kc, vc = append(f64(k_cache), f64(v_cache), f64(k_new), f64(v_new), cu, max_q, cache_seqlens, block_table)
    B = len(np.asarray(cu)) - 1
    ps, num_pages, max_pages, cap = paged_ref.geometry(kc, block_table, B)
    G = H // kc.shape[2]
    rg = ranges(cu, Tq, max_q)
    lens = lengths(cache_seqlens, [r[1] for r in rg], cap, k_new is not None)
    out = np.zeros((Tq, H, D))
    lse = np.full((H, Tq), -np.inf)
    for b, ((q0, Lq), (_, Lk)) in enumerate(zip(rg, lens)):
        if Lq == 0:
            continue
        # the sequence's keys through paged_ref.gather (S_new = 0 on a length that already holds the appended rows)
        bt_b = None if block_table is None else np.asarray(block_table)[b:b + 1]
        kc_b, vc_b = (kc, vc) if block_table is not None else (kc[b:b + 1], vc[b:b + 1])
        K, V, ok = paged_ref.gather(kc_b, vc_b, [Lk], 0, bt_b)[0]
        vis = np.broadcast_to(ok[None, :], (Lq, Lk)).copy()
        if causal:
            vis &= np.arange(Lk)[None, :] <= np.arange(Lq)[:, None] + (Lk - Lq)
        live = vis.any(1)
        for h in range(H):
            s = q[q0:q0 + Lq, h] @ K[:, h // G].T * scale if Lk else np.zeros((Lq, 0))
            s = np.where(vis, s, -np.inf)
            m = np.where(live, s.max(1, initial=-np.inf), 0.0)[:, None]
            p = np.where(vis, np.exp(s - m), 0.0)
            l = p.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                o = (paged_ref.round_p(p, kind) @ V[:, h // G]) / l[:, None] if Lk else np.zeros((Lq, D))
                lse[h, q0:q0 + Lq] = np.where(live, np.log(l) + m[:, 0], -np.inf)
            out[q0:q0 + Lq, h] = np.where(live[:, None], o, 0.0)
    return out, lse, kc, vc
