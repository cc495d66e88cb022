"""fp64 reference of sliding-window attention for packed variable-length queries over a paged or static KV cache
(umfa_torch.varlen_kvcache_window_attention): tests/varlen_paged_ref.py's ranges, lengths, append and clamps with
tests/paged_window_ref.py's band applied per sequence.

For sequence b, (start, L_q) = varlen_paged_ref.ranges, (L0, L_k) = varlen_paged_ref.lengths and off = L_k - L_q: query token i of the
sequence sees key j iff j < L_k, j's page entry lies in [0, num_pages) and i + off - left <= j <= i + off + right; a side given as -1 is
unbounded, causal sets right = 0.  A row that sees no key: O = 0, LSE = -inf.  Rows no sequence covers are not written.

forward() is the reference and (kind=) the format floor; nkeys() counts the visible keys apart from it (forward_floor_ref.check_pool's
live= cross-check); normalise() restates the C entry's window normalisation; step_range() is the kernel's per-item step range in int32
arithmetic; emulate() is forward_floor_ref.emulate's arithmetic with the per-item step range and the split rule.
"""
from __future__ import annotations

import numpy as np

import forward_floor_ref as ffr
import paged_ref
import paged_window_ref as pwr
import varlen_paged_ref as vpr

OPEN = pwr.OPEN  # the C side's sentinel of an unbounded side (fa_paged_window.h PAGED_WIN_OPEN)
MAX_CAPACITY = 1 << 30  # (exclusive) the C entry's bound on the capacity and on max_seqlen_q


def _sequences(cu, Tq, max_q, cache_seqlens, k_cache, block_table, has_new):
    """[(b, start, L_q, L_k, K, V, ok)] of the sequences with rows: the sequence's keys through paged_ref.gather on caches that already
    hold the appended rows (K / V None when k_cache is only a shape)"""
    B = len(np.asarray(cu)) - 1
    shape_only = not isinstance(k_cache[0], np.ndarray)  # a shape (nkeys) or the pair (kc, vc)
    kc, vc = (None, None) if shape_only else k_cache
    shape = k_cache if shape_only else kc.shape
    ps = shape[1]
    num_pages, max_pages = (B, 1) if block_table is None else (shape[0], np.asarray(block_table).shape[1])
    rg = vpr.ranges(cu, Tq, max_q)
    lens = vpr.lengths(cache_seqlens, [r[1] for r in rg], ps * max_pages, has_new)
    res = []
    for b, ((q0, Lq), (_, Lk)) in enumerate(zip(rg, lens)):
        if Lq == 0:
            continue
        if shape_only:
            K = V = None
            ok = np.array([paged_ref._page(block_table, b, j // ps, num_pages, max_pages) >= 0 for j in range(Lk)], bool)
        else:
            bt_b = None if block_table is None else np.asarray(block_table)[b:b + 1]
            kc_b, vc_b = (kc, vc) if block_table is not None else (kc[b:b + 1], vc[b:b + 1])
            K, V, ok = paged_ref.gather(kc_b, vc_b, [Lk], 0, bt_b)[0]
        res.append((b, q0, Lq, Lk, K, V, ok))
    return res


def forward(q, k_cache, v_cache, cu, max_q, cache_seqlens, block_table=None, k_new=None, v_new=None, causal=False, window=(-1, -1),
            scale=None, kind=None):
    """(O [T_q, H, D], LSE [H, T_q], k_cache', v_cache') in fp64, the caches after the append; rows no sequence covers stay 0 / -inf.
    kind ("fp16" / "bf16"): the format floor, with varlen_paged_ref.forward's meaning.  With a window that bounds nothing this is
    varlen_paged_ref.forward's arithmetic, operation by operation."""
    (out,), lse, kc, vc = forward_kinds(q, k_cache, v_cache, cu, max_q, cache_seqlens, block_table, k_new, v_new, causal, window, scale, (kind,))
    return out, lse, kc, vc


def forward_kinds(q, k_cache, v_cache, cu, max_q, cache_seqlens, block_table=None, k_new=None, v_new=None, causal=False, window=(-1, -1),
                  scale=None, kinds=(None, ffr.KIND)):
    """([O per kind], LSE, k_cache', v_cache'): forward() for several kinds in one pass over the scores -- the exact O and the format
    floor of a case share S, the maxima, P and l; each O is forward(kind=)'s, operation by operation"""
    q = np.asarray(q, np.float64)
    Tq, H, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    kc, vc = vpr.append(f64(k_cache), f64(v_cache), f64(k_new), f64(v_new), cu, max_q, cache_seqlens, block_table)
    G = H // kc.shape[2]
    outs = [np.zeros((Tq, H, D)) for _ in kinds]
    lse = np.full((H, Tq), -np.inf)
    for _, q0, Lq, Lk, K, V, ok in _sequences(cu, Tq, max_q, cache_seqlens, (kc, vc), block_table, k_new is not None):
        vis = ok[None, :] & pwr.band(Lq, Lk, causal, window)
        live = vis.any(1)
        for h in range(H):
            s = q[q0:q0 + Lq, h] @ K[:, h // G].T * scale if Lk else np.zeros((Lq, 0))
            s = np.where(vis, s, -np.inf)
            m = np.where(live, s.max(1, initial=-np.inf), 0.0)[:, None]
            p = np.where(vis, np.exp(s - m), 0.0)
            l = p.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                lse[h, q0:q0 + Lq] = np.where(live, np.log(l) + m[:, 0], -np.inf)
                for out, kind in zip(outs, kinds):
                    o = (paged_ref.round_p(p, kind) @ V[:, h // G]) / l[:, None] if Lk else np.zeros((Lq, D))
                    out[q0:q0 + Lq, h] = np.where(live[:, None], o, 0.0)
    return outs, lse, kc, vc


def nkeys(Tq, cu, max_q, cache_seqlens, k_cache_shape, block_table=None, has_new=False, causal=False, window=(-1, -1)):
    """[T_q] number of keys each packed row sees (0 for rows no sequence covers), counted key by key from the statement of the semantics
    (not through band() or forward())"""
    left, right = window
    if causal:
        right = 0
    out = np.zeros(Tq, np.int64)
    for _, q0, Lq, Lk, _, _, ok in _sequences(cu, Tq, max_q, cache_seqlens, tuple(k_cache_shape), block_table, has_new):
        off = Lk - Lq
        for j in range(Lk):
            if not ok[j]:
                continue
            for i in range(Lq):
                if (left < 0 or j >= i + off - left) and (right < 0 or j <= i + off + right):
                    out[q0 + i] += 1
    return out


def normalise(window, causal: bool, max_q: int, capacity: int):
    """the C entry's normalisation (umfa_varlen_kvcache_attention_window_forward_stream): ((left, right), plain) with -1 for an open
    side, plain = the call launches the unwindowed packed kernels.  Values below -1, anything but a pair, and a capacity or a
    max_seqlen_q of 2^30 or more raise ValueError."""
    if max_q >= MAX_CAPACITY:
        raise ValueError(f"max_seqlen_q must be below 2^30 (got {max_q})")
    return pwr.normalise(window, causal, max_q, capacity)


def _i32(x: int) -> int:
    assert -(1 << 31) <= x < (1 << 31), f"{x} leaves int32"
    return x


def step_range(first_tok: int, last_tok: int, Lq: int, Lk: int, window, causal=False):
    """the item's 128-key steps [lo, hi) by the kernel's rule, every intermediate checked to stay in int32 as the kernel computes it:
    lo_off = off - left, hi_off = off + right (an open side: OPEN), k_first = max(0, first_tok + lo_off), k_last = min(L_k - 1, last_tok +
    hi_off); steps [k_first // 128, k_last // 128 + 1), empty (lo == hi) when k_last < k_first"""
    left, right = window
    if causal:
        right = 0
    off = _i32(Lk - Lq)
    lo_off = _i32(off - (OPEN if left < 0 else left))
    hi_off = _i32(off + (OPEN if right < 0 else right))
    k_first = max(0, _i32(first_tok + lo_off))
    k_last = min(Lk - 1, _i32(last_tok + hi_off))
    lo = k_first // 128
    return (lo, k_last // 128 + 1) if k_last >= k_first else (lo, lo)


def items(lq, g, Hkv):
    """(decode-form items, 128-row items) a launch over these lengths runs"""
    dec = sum(Hkv for l in lq if 0 < g * l <= 32)
    blk = sum(Hkv * ((g * l + 127) // 128) for l in lq if g * l > 32)
    return dec, blk


def emulate(q, kc, vc, cu, max_q, cache_seqlens, causal, window, nsplit=1, scale=None, kind=ffr.KIND, defect=None, block_table=None):
    """O [T_q, H, D] as fa_fwd16_paged_varlen_window computes it, in fp64 but for the rounding of P: per sequence the rows of one KV head
    packed (row r = token r // g of head hk g + r % g), the decode form for R = g L_q <= 32, else 128-row blocks -- decided per sequence;
    each item sweeps step_range() of its first and last rows' tokens, nsplit parts (one count for the launch) dividing that range
    (paged_window_ref._emulate_rows).  New tokens are emulated as already appended: kc / vc hold them and cache_seqlens counts them.
    defect: "parts_from_zero" (the parts divide [0, nst) instead of the band) or "band_from_first_row" (the item's step range taken from
    its first row alone)."""
    Tq, H, D = q.shape
    Hkv = kc.shape[2]
    g = H // Hkv
    scale = D ** -0.5 if scale is None else scale
    out = np.zeros_like(q)
    for _, q0, Lq, Lk, K, V, ok in _sequences(cu, Tq, max_q, cache_seqlens, (kc, vc), block_table, False):
        R = g * Lq
        tok = np.arange(R) // g
        vis = (ok[None, :] & pwr.band(Lq, Lk, causal, window))[tok]
        for hk in range(Hkv):
            qr = q[q0 + tok, hk * g + np.arange(R) % g]
            blocks = [np.arange(R)] if R <= 32 else [np.arange(r0, min(r0 + 128, R)) for r0 in range(0, R, 128)]
            o = np.zeros((R, D))
            for rows in blocks:
                last = rows[0] if defect == "band_from_first_row" else rows[-1]
                lo, hi = step_range(int(tok[rows[0]]), int(tok[last]), Lq, Lk, window, causal)
                o[rows] = pwr._emulate_rows(qr[rows], K[:, hk], V[:, hk], vis[rows], lo, hi, kind, scale, R <= 32, nsplit,
                                            defect if defect == "parts_from_zero" else None)
            out[q0 + tok, hk * g + np.arange(R) % g] = o
    return out
