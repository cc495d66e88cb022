"""fp64 reference of sliding-window attention over a paged or static KV cache (umfa_torch.kvcache_window_attention, DESIGN.md section
3.1m): tests/paged_ref.py's append, page resolution and clamps with flash-attention's window_size = (left, right).

With L_k = clamp(cache_seqlens[b]) + S_new (clamped as paged_ref.lengths clamps it) and off = L_k - Sq, query token i of sequence b sees
key j iff j < L_k, j's page entry lies in [0, num_pages) and i + off - left <= j <= i + off + right; a side given as -1 is unbounded,
causal sets right = 0.  A row that sees no key: O = 0, LSE = -inf.

forward() is the reference and (kind=) the format floor; nkeys() counts the visible keys apart from it (forward_floor_ref.check_pool's
live= cross-check); normalise() restates the C entry's window normalisation; emulate_window() is forward_floor_ref.emulate's arithmetic
with the banded kernel's step range and split rule.
"""
from __future__ import annotations

import numpy as np

import forward_floor_ref as ffr
import paged_ref

OPEN = 1 << 30  # the C side's sentinel of an unbounded side (fa_paged_window.h PAGED_WIN_OPEN)
MAX_CAPACITY = 1 << 30  # (exclusive)


def band(Sq: int, Lk: int, causal: bool = False, window=(-1, -1)) -> np.ndarray:
    """bool [Sq, Lk]: the keys of the band each query token sees (page validity apart)"""
    left, right = window
    if causal:
        right = 0
    i = np.arange(Sq)[:, None] + (Lk - Sq)
    j = np.arange(Lk)[None, :]
    vis = np.ones((Sq, Lk), bool)
    if left >= 0:
        vis &= j >= i - left
    if right >= 0:
        vis &= j <= i + right
    return vis


def forward(q, k_cache, v_cache, cache_seqlens, block_table=None, k_new=None, v_new=None, causal=False, window=(-1, -1), scale=None,
            kind=None):
    """(O [B, Sq, H, D], LSE [B, H, Sq], k_cache', v_cache') in fp64, the caches after the append.  kind ("fp16" / "bf16"): the format
    floor, with paged_ref.forward's meaning -- P = exp(S - the row's exact max over the keys it sees) rounded once to `kind`, in the
    numerator only.  With a window that bounds nothing this is paged_ref.forward's arithmetic, operation by operation."""
    q = np.asarray(q, np.float64)
    B, Sq, H, D = q.shape
    scale = D ** -0.5 if scale is None else scale
    kc, vc = paged_ref.append(np.asarray(k_cache, np.float64), np.asarray(v_cache, np.float64),
                              None if k_new is None else np.asarray(k_new, np.float64),
                              None if v_new is None else np.asarray(v_new, np.float64), cache_seqlens, block_table)
    S_new = 0 if k_new is None else k_new.shape[1]
    G = H // kc.shape[2]
    out = np.zeros((B, Sq, H, D))
    lse = np.full((B, H, Sq), -np.inf)
    for b, (K, V, ok) in enumerate(paged_ref.gather(kc, vc, cache_seqlens, S_new, block_table)):
        Lk = len(ok)
        vis = ok[None, :] & band(Sq, Lk, causal, window)
        live = vis.any(1)
        for h in range(H):
            s = q[b, :, h] @ K[:, h // G].T * scale if Lk else np.zeros((Sq, 0))
            s = np.where(vis, s, -np.inf)
            m = np.where(live, s.max(1, initial=-np.inf), 0.0)[:, None]
            p = np.where(vis, np.exp(s - m), 0.0)
            l = p.sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                o = (paged_ref.round_p(p, kind) @ V[:, h // G]) / l[:, None] if Lk else np.zeros((Sq, D))
                lse[b, h] = np.where(live, np.log(l) + m[:, 0], -np.inf)
            out[b, :, h] = np.where(live[:, None], o, 0.0)
    return out, lse, kc, vc


def nkeys(Sq, cache_seqlens, k_cache_shape, block_table=None, S_new=0, causal=False, window=(-1, -1)):
    """[B, Sq] number of keys each query token sees, counted key by key from the statement of the semantics (not through band() or
    forward())"""
    left, right = window
    if causal:
        right = 0
    B = len(np.asarray(cache_seqlens))
    ps = k_cache_shape[1]
    num_pages, max_pages = (B, 1) if block_table is None else (k_cache_shape[0], np.asarray(block_table).shape[1])
    out = np.zeros((B, Sq), np.int64)
    for b, (_, Lk) in enumerate(paged_ref.lengths(cache_seqlens, S_new, ps * max_pages)):
        off = Lk - Sq
        for j in range(Lk):
            if paged_ref._page(block_table, b, j // ps, num_pages, max_pages) < 0:
                continue
            for i in range(Sq):
                if (left < 0 or j >= i + off - left) and (right < 0 or j <= i + off + right):
                    out[b, i] += 1
    return out


def normalise(window, causal: bool, Sq: int, capacity: int):
    """the C entry's normalisation (umfa_kvcache_attention_window_forward_stream): ((left, right), plain) with -1 for an open side, plain
    = the call launches the unwindowed kernels.  Values below -1, anything but a pair and a capacity of 2^30 or more raise ValueError."""
    try:
        left, right = (int(w) for w in window)
    except (TypeError, ValueError):
        raise ValueError(f"window must be a pair of ints (got {window!r})") from None
    if left < -1 or right < -1:
        raise ValueError(f"window values must be >= -1 (got {(left, right)})")
    if capacity >= MAX_CAPACITY:
        raise ValueError(f"capacity must be below 2^30 (got {capacity})")
    if causal:
        right = 0
    if left >= capacity:
        left = -1
    if right >= Sq:
        right = -1
    return (left, right), left < 0 and (right < 0 or (causal and right == 0))


def step_range(rows_tok_first: int, rows_tok_last: int, Sq: int, Lk: int, window, causal=False):
    """the workgroup's 128-key steps [lo, hi) by the kernel's rule: k_first = max(0, first_tok + off - left), k_last = min(L_k - 1,
    last_tok + off + right), steps [k_first // 128, k_last // 128 + 1), empty (lo == hi) when k_last < k_first"""
    left, right = window
    if causal:
        right = 0
    off = Lk - Sq
    k_first = max(0, rows_tok_first + off - (OPEN if left < 0 else left))
    k_last = min(Lk - 1, rows_tok_last + off + (OPEN if right < 0 else right))
    lo = k_first // 128
    return (lo, k_last // 128 + 1) if k_last >= k_first else (lo, lo)


def _emulate_rows(q, K, V, vis, lo, hi, kind, scale, ks4, nsplit, defect):
    """forward_floor_ref.emulate with the steps [lo, hi) shared among nsplit parts (its _stream and _merge; the fold is emulate's, without
    its planted defects)"""
    R, D = vis.shape[0], V.shape[1]
    S = np.where(vis, q @ K.T * scale, -np.inf) if vis.shape[1] else np.zeros((R, 0))
    if defect == "parts_from_zero":  # the parts divide [0, nst) and end there, while each part's sweep starts at the band
        per = (hi + nsplit - 1) // nsplit
        ranges = [range(lo + part * per, min(part * per + per, hi)) for part in range(nsplit)]
    else:
        per = (hi - lo + nsplit - 1) // nsplit
        ranges = [range(lo + part * per, min(lo + part * per + per, hi)) for part in range(nsplit)]
    parts = []
    for steps in ranges:
        if ks4:
            parts.append(ffr._merge([ffr._stream(S, V, [128 * st + 32 * w for st in steps], kind, None, None, 1.0) for w in range(4)]))
        else:
            parts.append(ffr._stream(S, V, [128 * st + 32 * w for st in steps for w in range(4)], kind, None, None, 1.0))
    os_, ws = [], []
    M = np.max([m for _, m, _ in parts], axis=0)
    Mb = np.where(np.isneginf(M), 0.0, M)
    for acc, m, l in parts:
        with np.errstate(invalid="ignore", divide="ignore"):
            os_.append(np.where(l[:, None] > 0, acc / l[:, None], 0.0))  # a part writes its normalised O with (m, l)
        ws.append(np.where(np.isneginf(m), 0.0, np.exp(m - Mb)) * l)
    if nsplit == 1:
        return os_[0]
    tot = np.sum(ws, axis=0)
    o = np.zeros((R, D))
    for w, po in zip(ws, os_):
        with np.errstate(invalid="ignore", divide="ignore"):
            o += np.where(tot > 0, w / tot, 0.0)[:, None] * po
    return o


def emulate_window(q, kc, vc, cache_seqlens, causal, window, nsplit=1, scale=None, kind=ffr.KIND, defect=None, block_table=None):
    """O [B, Sq, H, D] as fa_fwd16_paged_window computes it, in fp64 but for the rounding of P (forward_floor_ref.emulate_paged with the
    band): the rows of one (batch, KV head) packed (row r = token r // g of head hk g + r % g), the decode form for R = g Sq <= 32, else
    128-row blocks; each workgroup sweeps step_range() of its first and last rows' tokens, the parts dividing that range.  New tokens are
    emulated as already appended.  defect: "lo_plus1" (the lower bound one key too high) or "parts_from_zero" (see _emulate_rows)."""
    B, Sq, H, D = q.shape
    Hkv = kc.shape[2]
    g = H // Hkv
    R = g * Sq
    scale = D ** -0.5 if scale is None else scale
    left, right = window
    vis_window = (left - 1 if left > 0 else left, right) if defect == "lo_plus1" else window
    assert defect != "lo_plus1" or left > 0
    out = np.zeros_like(q)
    for b, (K, V, ok) in enumerate(paged_ref.gather(kc, vc, cache_seqlens, 0, block_table)):
        Lk = len(ok)
        tok = np.arange(R) // g
        vis = (ok[None, :] & band(Sq, Lk, causal, vis_window))[tok]
        for hk in range(Hkv):
            qr = q[b, tok, hk * g + np.arange(R) % g]
            blocks = [np.arange(R)] if R <= 32 else [np.arange(r0, min(r0 + 128, R)) for r0 in range(0, R, 128)]
            o = np.zeros((R, D))
            for rows in blocks:
                lo, hi = step_range(int(tok[rows[0]]), int(tok[rows[-1]]), Sq, Lk, window, causal)
                o[rows] = _emulate_rows(qr[rows], K[:, hk], V[:, hk], vis[rows], lo, hi, kind, scale, R <= 32, nsplit,
                                        None if defect == "lo_plus1" else defect)
            out[b, tok, hk * g + np.arange(R) % g] = o
    return out
