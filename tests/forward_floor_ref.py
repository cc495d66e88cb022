"""Shared by tests/test_forward_floor_cpu.py and tests/test_gpu_forward_floor.py: the shapes at which the KV-cache forwards are held to
the forward format floor, the regime of each kernel form, the pooling of a case's rows into one comparison, and an fp64 emulator of
the paged kernels' arithmetic (fa_fwd16_paged / _paged_fp8 / _paged_varlen: 128-key steps of four 32-key tiles, an exact running max per
tile, P rounded once to the P V operand type, the decode form's four quarters, split parts folded afterwards).

The floor itself is the references' forward(kind=...): exact fp64 scores, exponentials and sums, P relative to the row's exact max
rounded ONCE to `kind` in the numerator.  Every kernel held here multiplies P V in fp16 (fp16 operands, or bf16 operands with "pv16"), so
the floor's kind is KIND for both input types; the input type only decides which values Q, K and V can take.
"""
from __future__ import annotations

import numpy as np

import paged_ref
import tolerances as tol

KIND = "fp16"  # the format of P in every kernel held to this floor
ONE_KEY_REL = 2.0 ** -22  # a row that sees exactly one key: P = 1, l = 1, O = that key's V, to fp32 rounding

# ------------------------------------------------------------------------------------------------------------ the shapes
DECODE_LENS = [0, 1, 21, 127, 128, 129, 333, 640]  # B 8, H_kv 2, g 8, page 16: empty, one key, ragged page, around one 128-key step, several
DECODE = [  # (g, Sq, causal, num_splits)
    (8, 1, False, 1), (8, 1, False, 3),
    (8, 4, True, 1), (8, 4, True, 3),  # R = 32 exactly, the last decode-form count
]
ROWS128 = [(1, 200), (8, 16)]  # (g, Sq): a ragged second 128-row block; R = 128 exactly
ROWS128_PAGES = [16, 64, 256]


def rows128_lens(page):
    return [0, 150, page + 5, 640]


ROWS128_SPLIT = [(3, 1300), (8, 300)]  # (num_splits, L): three real parts; three steps over eight parts leaves five of them empty
APPEND_LENS = [14, 30, 47, 62]  # three new tokens from these positions of 16-key pages: each append crosses into the next page
HOLE_LENS = [100, 40, 70, 128]  # 16-key pages; table entry 1 of every sequence and entry 3 of sequence 2 lie outside the pool
# tests/test_gpu_varlen_window.py's lengths and windows (the GPU test asserts they are the same)
BAND_LENS_Q = (1, 31, 127, 128, 129, 300, 0, 64, 200)
BAND_LENS_K = (1, 40, 100, 128, 300, 129, 5, 0, 200)
WINDOWS = [(0, 0), (1, 0), (31, 0), (32, 0), (100, 17), (-1, 40), (40, -1), (127, 128)]
PACKED_LQ = [1, 1, 5, 130, 200, 0, 32, 33]
PACKED_CACHE = [640, 37, 5, 130, 450, 77, 1000, 64]
PACKED_G, PACKED_HKV = 4, 4  # (H_kv 4: the decode-form items alone -- L_q 1, 1, 5 -- pool 96 rows of two or more keys, 6144 elements at D = 64)


def form_regime(R: int, split: bool):
    """check_forward's regime= of one kernel form.  All forms keep an exact running max, so the rms multiple is FLOOR_MULT["exact"]'s
    throughout.  The unsplit 128-row form rounds P against one reference per row and takes the exact max multiple as well.  The decode
    form (R = g Sq <= 32: each of four quarters has its own running max) and every split kernel (each part its own) round P against
    several references: the MAX of the pooled error differs from the ideal kernel's by sample noise and takes the "stale" multiple."""
    return ("stale", "exact") if R <= 32 or split else "exact"


# ------------------------------------------------------------------------------------------------------------ pooling
def paged_nkeys(Sq, cache_seqlens, k_cache_shape, block_table=None, S_new=0, causal=False):
    """[B, Sq] number of keys each query token sees (paged_ref's visibility: clamped lengths, table entries outside the pool, bottom-right
    causal)"""
    B = len(np.asarray(cache_seqlens))
    if block_table is None:
        ps, num_pages, max_pages, cap = k_cache_shape[1], B, 1, k_cache_shape[1]
    else:
        ps, num_pages, max_pages = k_cache_shape[1], k_cache_shape[0], np.asarray(block_table).shape[1]
        cap = ps * max_pages
    out = np.zeros((B, Sq), np.int64)
    for b, (_, Lk) in enumerate(paged_ref.lengths(cache_seqlens, S_new, cap)):
        ok = np.array([paged_ref._page(block_table, b, j // ps, num_pages, max_pages) >= 0 for j in range(Lk)], bool)
        vis = np.broadcast_to(ok[None, :], (Sq, Lk)).copy()
        if causal:
            vis &= np.arange(Lk)[None, :] <= np.arange(Sq)[:, None] + (Lk - Sq)
        out[b] = vis.sum(1)
    return out


def check_pool(got, want, floor, nkeys, dt, kernel, tag, regime, min_elems=4096, live=None):
    """One comparison of a case: got / want / floor [N, D] rows (any order, already divided by the group's v_descale for fp8), nkeys [N] the
    keys each row sees.  Rows without keys: exact zeros.  Rows with exactly one key: O = that key's V (= want) to ONE_KEY_REL.  All
    others pooled into one [1, 1, R, D] check_forward against the floor; the pool must hold at least min_elems elements, and nothing but
    dead and one-key rows may be left out of it: `live` [N] bool, the rows whose reference LSE is finite, must be exactly the rows the
    count gives a key (the count is computed apart from the reference: a wrong count cannot hide rows from the pool)."""
    got, want, floor, nkeys = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(floor, np.float64), np.asarray(nkeys)
    assert got.shape == want.shape == floor.shape and got.shape[0] == nkeys.shape[0], (got.shape, want.shape, floor.shape, nkeys.shape)
    assert np.isfinite(got).all(), (tag, "non-finite O")
    pool = nkeys >= 2
    if live is not None:
        assert ((nkeys > 0) == np.asarray(live, bool).reshape(-1)).all(), (tag, "the key count disagrees with the reference's live rows")
    dead, one = nkeys == 0, nkeys == 1
    assert (got[dead] == 0).all(), (tag, "a row without keys is not exactly zero")
    if one.any():
        d = np.abs(got[one] - want[one])
        assert (d <= ONE_KEY_REL * np.abs(want[one])).all(), (tag, "a one-key row is not that key's V", float(d.max()))
    assert int(pool.sum()) * got.shape[1] >= min_elems, (tag, "pool too small", int(pool.sum()) * got.shape[1])
    if not pool.any():  # (only with min_elems = 0: a case of one-key rows alone)
        return None
    return tol.check_forward(got[pool][None, None], want[pool][None, None], KIND, kernel, tag=tag, floor=floor[pool][None, None], regime=regime)


# ------------------------------------------------------------------------------------------------------------ the emulator
def _round_p(p, kind, defect):
    """paged_ref.round_p, or one of the planted roundings"""
    if defect == "p_bf16":
        return paged_ref.round_p(p, "bf16")
    r = paged_ref.round_p(p, kind)
    if defect == "p_trunc":  # towards zero instead of to nearest
        assert kind == "fp16"
        r16 = r.astype(np.float16)
        r = np.where(r > p, np.nextafter(r16, np.float16(0)).astype(np.float64), r)
    return r


def _stream(S, V, tiles, kind, defect, keep, keep_s):
    """one wave's sweep over its 32-key tiles: (acc [R, D], m [R], l [R]) with the running max renewed per tile"""
    R = S.shape[0]
    m, l, acc = np.full(R, -np.inf), np.zeros(R), np.zeros((R, V.shape[1]))
    for k0 in tiles:
        x = S[:, k0:k0 + 32]
        if x.shape[1] == 0:
            continue
        mn = np.maximum(m, x.max(1))
        base = np.where(np.isneginf(mn), 0.0, mn)
        alpha = np.exp(m - base)
        p = np.exp(x - base[:, None])
        l = l * alpha + p.sum(1)  # the denominator is undropped and unrounded
        if keep is None:
            pn = _round_p(p, kind, defect)
        elif defect == "keep_after":  # 1 / (1 - p) folded into P before it is rounded, keep applied to the rounded P
            pn = _round_p(p * keep_s, kind, None) * keep[:, k0:k0 + 32]
        else:
            pn = _round_p(p * keep[:, k0:k0 + 32], kind, defect)
        acc = acc * alpha[:, None] + pn @ V[k0:k0 + 32]
        m = mn
    return acc, m, l


def _merge(parts):
    """(acc, m, l) of several streams over disjoint keys -> one, against the common max"""
    M = np.max([m for _, m, _ in parts], axis=0)
    acc, l = 0.0, 0.0
    for a, m, ll in parts:
        w = np.where(np.isneginf(m), 0.0, np.exp(m - np.where(np.isneginf(M), 0.0, M)))
        acc, l = acc + w[:, None] * a, l + w * ll
    return acc, M, l


def emulate(q, K, V, vis, kind=KIND, *, scale, ks4, nsplit=1, defect=None, keep=None, keep_s=1.0):
    """O [R, D] of one workgroup's rows as the paged kernels compute it, in fp64 but for the rounding of P: q [R, D], K / V [L, D], vis
    [R, L] bool.  128-key steps below the last key the workgroup sees, shared among nsplit parts; ks4: the four quarters of the decode
    form take one 32-key tile of every step each and meet behind the loop; the parts' normalised O, m and l are folded afterwards.
    keep [R, L] / keep_s: dropout's mask and 1 / (1 - p) (O = keep_s (keep o P) V / l).  defect: one planted error --
    "p_bf16", "p_trunc", "part_o_fp16", "fold_w_fp16", "keep_after"."""
    R, L = vis.shape
    D = V.shape[1]
    if L == 0 or not vis.any():
        return np.zeros((R, D))
    S = np.where(vis, q @ K.T * scale, -np.inf)
    Le = int(np.nonzero(vis.any(0))[0].max()) + 1
    nst = (Le + 127) // 128
    per = (nst + nsplit - 1) // nsplit
    parts = []
    for part in range(nsplit):
        steps = range(part * per, min(part * per + per, nst))
        if ks4:
            res = _merge([_stream(S, V, [128 * st + 32 * w for st in steps], kind, defect, keep, keep_s) for w in range(4)])
        else:
            res = _stream(S, V, [128 * st + 32 * w for st in steps for w in range(4)], kind, defect, keep, keep_s)
        parts.append(res)
    if nsplit == 1:
        acc, _, l = parts[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            o = np.where(l[:, None] > 0, acc / l[:, None], 0.0)
    else:
        M = np.max([m for _, m, _ in parts], axis=0)
        Mb = np.where(np.isneginf(M), 0.0, M)
        ws, os_ = [], []
        for acc, m, l in parts:
            with np.errstate(invalid="ignore", divide="ignore"):
                po = np.where(l[:, None] > 0, acc / l[:, None], 0.0)  # a part writes its normalised O with (m, l)
            if defect == "part_o_fp16":
                po = paged_ref.round_p(po, "fp16")
            ws.append(np.where(np.isneginf(m), 0.0, np.exp(m - Mb)) * l)
            os_.append(po)
        tot = np.sum(ws, axis=0)
        o = np.zeros((R, D))
        for w, po in zip(ws, os_):
            with np.errstate(invalid="ignore", divide="ignore"):
                wn = np.where(tot > 0, w / tot, 0.0)
            if defect == "fold_w_fp16":
                wn = paged_ref.round_p(wn, "fp16")
            o += wn[:, None] * po
    return o * (1.0 if keep is None or defect == "keep_after" else keep_s)


def emulate_paged(q, kc, vc, cache_seqlens, causal, nsplit, scale=None, kind=KIND, defect=None, page=None, block_table=None):
    """emulate() over a cache as paged_ref takes it (q [B, Sq, H, D], kc / vc in fp64, static or paged with block_table; keys behind a table
    entry outside the pool are invisible): the rows of one (batch, KV head) packed as the kernels pack them (row r = token r // g of head
    hk g + r % g), the decode form for R = g Sq <= 32, else 128-row blocks.  New tokens are emulated as already appended (the lengths
    include them).  defect "ragged_key" drops the last key of a sequence whose length is no multiple of `page`."""
    B, Sq, H, D = q.shape
    Hkv = kc.shape[2]
    g = H // Hkv
    R = g * Sq
    scale = D ** -0.5 if scale is None else scale
    out = np.zeros_like(q)
    for b, (K, V, ok) in enumerate(paged_ref.gather(kc, vc, cache_seqlens, 0, block_table)):
        Lk = len(ok)
        tok = np.arange(R) // g
        vis = np.broadcast_to(ok[None, :], (R, Lk)).copy()
        if causal:
            vis &= np.arange(Lk)[None, :] <= tok[:, None] + (Lk - Sq)
        if defect == "ragged_key" and Lk and Lk % page:
            vis[:, Lk - 1] = False
        for hk in range(Hkv):
            qr = q[b, tok, hk * g + np.arange(R) % g]
            blocks = [np.arange(R)] if R <= 32 else [np.arange(r0, min(r0 + 128, R)) for r0 in range(0, R, 128)]
            o = np.zeros((R, D))
            for rows in blocks:
                o[rows] = emulate(qr[rows], K[:, hk], V[:, hk], vis[rows], kind, scale=scale, ks4=R <= 32, nsplit=nsplit,
                                  defect=None if defect == "ragged_key" else defect)
            out[b, tok, hk * g + np.arange(R) % g] = o
    return out
