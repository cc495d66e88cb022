"""The KV-cache, banded and dropout forwards held to the forward FORMAT FLOOR on the GPU (profiles/fwd_floor):
fa_fwd16_paged, fa_fwd16_paged_fp8, fa_fwd16_paged_varlen, fa_fwd16_varlen_window and fa_fwd16_drop against the ideal flash kernel of the
same operation -- the references' forward(kind=...): fp64 throughout, P relative to the row's exact max rounded once to the P V operand
type -- on the same rows, under tolerances.check_forward(floor=, regime=): rms <= 1.05 x the floor's for every form, max <= 1.15 x (x 1.25
below 2^17 elements) for the unsplit 128-row form and <= 2.5 x for the forms that round P against several references (the decode form
R = g Sq <= 32, and every split kernel).  tests/test_forward_floor_cpu.py shows that an emulation of the kernels' arithmetic stays inside
these bounds at these very shapes and that one planted defect each does not.

Per case all live rows that see two keys or more are pooled into one [1, 1, R, D] comparison (fp8: divided by the group's v_descale
first); the pool holds at least 4096 elements, nothing but rows without keys (exact zeros) and one-key rows (O = that key's V to 2^-22)
is left out.  The one exception is the window (0, 0), where every row sees exactly one key: there is nothing to pool, and every row is
held to the one-key bound.  Seeded inputs, fp32 O."""
import numpy as np
import pytest
import torch

import dropout_ref
import forward_floor_ref as ffr
import paged_fp8_ref
import paged_ref
import test_gpu_dropout as td
import test_gpu_paged as tp
import test_gpu_paged_fp8 as tf
import test_gpu_varlen_paged as tv
import test_gpu_varlen_window as tw
import tolerances as tol
import varlen_paged_ref
import varlen_window_ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TYPES = pytest.mark.parametrize("dt", ["bf16", "fp16"])
DIMS = pytest.mark.parametrize("D", [64, 128])


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _paged_check(dt, q, kc0, vc0, sl, bt, o, kernel, causal, num_splits, tag, kn=None, vn=None, descales=None):
    """one pooled comparison of a kvcache_attention call (the caches as they were before it)"""
    B, Sq, H, D = q.shape
    Hkv = kc0.shape[2]
    if num_splits:
        assert ("split" in kernel) == (num_splits > 1), kernel
    slv, btn = sl.cpu().numpy(), None if bt is None else bt.cpu().numpy()
    knn, vnn = (None if t is None else _np(t) for t in (kn, vn))
    if descales is None:
        assert kernel.startswith("fa_fwd16_paged<"), kernel
        want, lse = paged_ref.forward(_np(q), _np(kc0), _np(vc0), slv, btn, knn, vnn, causal)[:2]
        floor = paged_ref.forward(_np(q), _np(kc0), _np(vc0), slv, btn, knn, vnn, causal, kind=ffr.KIND)[0]
        div = 1.0
    else:
        assert kernel.startswith("fa_fwd16_paged_fp8<"), kernel
        kd, vd = (d.cpu().numpy() for d in descales)
        args = (_np(q), tf._bytes(kc0), tf._bytes(vc0), slv, kd, vd, btn, knn, vnn, causal)
        want, lse = paged_fp8_ref.forward(*args)[:2]
        floor = paged_fp8_ref.forward(*args, kind=ffr.KIND)[0]
        div = np.repeat(vd.astype(np.float64), H // Hkv, axis=1)[:, None, :, None]
    nk = np.repeat(ffr.paged_nkeys(Sq, slv, tuple(kc0.shape), btn, 0 if kn is None else kn.shape[1], causal)[:, :, None], H, axis=2)
    got = _np(o)
    ffr.check_pool((got / div).reshape(-1, D), (want / div).reshape(-1, D), (floor / div).reshape(-1, D), nk.reshape(-1), dt, kernel,
                   f"{tag} {dt}", ffr.form_regime((H // Hkv) * Sq, "split" in kernel), live=np.isfinite(lse).transpose(0, 2, 1))


def _paged_run(dt, D, B, Hkv, g, Sq, ps, lens, causal, num_splits, fp8, tag, seed, S_new=0, table=None):
    max_pages = max(2, -(-(max(lens) + S_new) // ps))
    mod = tf if fp8 else tp
    q, kc, vc, bt, kn, vn = mod._paged(B, Sq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=seed, S_new=S_new, share=S_new == 0)
    if table is not None:
        bt = table(bt, kc.shape[0])
    sl = tp._seqlens(lens)
    kc0, vc0 = kc.clone(), vc.clone()
    if fp8:
        kd, vd = (tf._dev(x) for x in tf._descales(B, Hkv, seed=seed))
        o, _, kernel = tf._run(q, kc, vc, sl, bt, kd, vd, kn, vn, causal=causal, num_splits=num_splits)
        _paged_check(dt, q, kc0, vc0, sl, bt, o, kernel, causal, num_splits, tag, kn, vn, (kd, vd))
    else:
        o, _, kernel = tp._run(q, kc, vc, sl, bt, kn, vn, causal=causal, num_splits=num_splits)
        _paged_check(dt, q, kc0, vc0, sl, bt, o, kernel, causal, num_splits, tag, kn, vn)


# ------------------------------------------------------------------------------------------------ the decode form (ks4), 16-bit and fp8
@TYPES
@DIMS
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("g,Sq,causal,num_splits", ffr.DECODE)
def test_decode_form(dt, D, fp8, g, Sq, causal, num_splits):
    _paged_run(dt, D, 8, 2, g, Sq, 16, ffr.DECODE_LENS, causal, num_splits, fp8, f"decode g{g} Sq{Sq} splits{num_splits}", seed=40 + Sq + num_splits)


# ------------------------------------------------------------------------------------------------ the 128-row form
@TYPES
@DIMS
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("ps", ffr.ROWS128_PAGES)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_128_row_form(dt, D, causal, ps, g, Sq):
    _paged_run(dt, D, 4, 2, g, Sq, ps, ffr.rows128_lens(ps), causal, 1, False, f"128-row g{g} Sq{Sq} page{ps}", seed=50 + ps + Sq)


@TYPES
@DIMS
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_128_row_form_fp8(dt, D, causal, g, Sq):
    _paged_run(dt, D, 4, 2, g, Sq, 16, ffr.rows128_lens(16), causal, 1, True, f"128-row fp8 g{g} Sq{Sq}", seed=60 + Sq)


@TYPES
@DIMS
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
@pytest.mark.parametrize("num_splits,L", ffr.ROWS128_SPLIT)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_128_row_form_split(dt, D, fp8, num_splits, L, g, Sq):
    """3 parts over 1300 keys; 8 parts over 300 keys: three 128-key steps, so five parts are empty (m = -inf, l = 0 in the fold)"""
    _paged_run(dt, D, 2, 2, g, Sq, 64, [L, L - 37], True, num_splits, fp8, f"128-row split{num_splits} L{L} g{g} Sq{Sq}", seed=70 + L + Sq)


# ------------------------------------------------------------------------------------------------ one case each
@TYPES
@DIMS
def test_static_bhsd_view(dt, D):
    B, Smax, Hkv, g, Sq = 3, 300, 2, 4, 4
    gen = torch.Generator(device="cuda").manual_seed(81)
    q = torch.randn(B, Sq, g * Hkv, D, device="cuda", dtype=DT[dt], generator=gen)
    kc = torch.randn(B, Hkv, Smax, D, device="cuda", dtype=DT[dt], generator=gen).transpose(1, 2)  # HF StaticCache's [B, S_max, H_kv, D] view
    vc = torch.randn(B, Hkv, Smax, D, device="cuda", dtype=DT[dt], generator=gen).transpose(1, 2)
    sl = tp._seqlens([17, 300, 129])
    o, _, kernel = tp._run(q, kc, vc, sl, None, causal=True)
    _paged_check(dt, q, kc, vc, sl, None, o, kernel, True, 0, "static bhsd")


@TYPES
@DIMS
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
def test_append_across_a_page_boundary(dt, D, fp8):
    """three new tokens from positions 14, 30, 47 and 62 of 16-key pages: each append crosses into the next page (the fp8 floor runs on the
    dequantised post-append bytes: the append quantises)"""
    _paged_run(dt, D, 4, 2, 8, 3, 16, ffr.APPEND_LENS, True, 0, fp8, "append", seed=82, S_new=3)


@TYPES
@DIMS
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
def test_table_entry_outside_the_pool_in_mid_sequence(dt, D, fp8):
    def table(bt, num_pages):
        b = bt.cpu().numpy().copy()
        b[:, 1] = num_pages  # keys 16 .. 31 of every sequence: one past the pool
        b[2, 3] = -1
        return torch.tensor(b, device="cuda")

    _paged_run(dt, D, 4, 2, 8, 1, 16, ffr.HOLE_LENS, False, 0, fp8, "hole in the table", seed=83, table=table)


# ------------------------------------------------------------------------------------------------ packed queries over the cache
@TYPES
@DIMS
@pytest.mark.parametrize("num_splits", [0, 1, 3], ids=["auto", "unsplit", "splits3"])
def test_packed_queries(dt, D, num_splits):
    """decode-form items (g L_q <= 32: L_q 1, 1, 5) and 128-row items (130, 200, 32, 33) of one launch, pooled separately; automatic
    parts (at these lengths the launch splits), one part (the unsplit kernel: its 128-row items take the exact max multiple) and three"""
    g, Hkv, ps = ffr.PACKED_G, ffr.PACKED_HKV, 16
    lq, cache = ffr.PACKED_LQ, ffr.PACKED_CACHE
    H = g * Hkv
    q, kc, vc, bt, _, _ = tv._setup(lq, H, Hkv, D, ps, -(-max(cache) // ps), DT[dt], seed=90 + D)
    cu, sl = tv._i32(tv._cu(lq)), tv._i32(cache)
    o, _, kernel = tv._run(q, kc, vc, cu, max(lq), sl, bt, causal=True, num_splits=num_splits)
    assert kernel.startswith("fa_fwd16_paged_varlen<"), kernel
    if num_splits:
        assert ("split" in kernel) == (num_splits > 1), kernel
    args = (_np(q), _np(kc), _np(vc), cu.cpu().numpy(), max(lq), sl.cpu().numpy(), bt.cpu().numpy(), None, None, True)
    want, lse = varlen_paged_ref.forward(*args)[:2]
    floor = varlen_paged_ref.forward(*args, kind=ffr.KIND)[0]
    got = _np(o)
    nk = np.zeros(sum(lq), np.int64)
    decode = np.zeros(sum(lq), bool)
    for (q0, Lq), L in zip(varlen_paged_ref.ranges(cu.cpu().numpy(), sum(lq), max(lq)), cache):
        nk[q0:q0 + Lq] = np.clip(np.arange(Lq) + L - Lq + 1, 0, L)  # bottom-right causal, every page in the pool
        decode[q0:q0 + Lq] = g * Lq <= 32
    for dec in (True, False):
        sel = decode == dec
        rows = lambda a: a[sel].reshape(-1, D)  # noqa: E731
        ffr.check_pool(rows(got), rows(want), rows(floor), np.repeat(nk[sel], H), dt, kernel,
                       f"packed {'decode' if dec else '128-row'} items {dt}", ffr.form_regime(32 if dec else 128, "split" in kernel),
                       live=np.isfinite(lse).T[sel])


# ------------------------------------------------------------------------------------------------ the banded packed forward
@TYPES
@DIMS
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("window", tw.WINDOWS)
def test_windowed_varlen(dt, D, causal, window):
    assert (tw.LENS_Q, tw.LENS_K, tw.WINDOWS) == (ffr.BAND_LENS_Q, ffr.BAND_LENS_K, ffr.WINDOWS)  # (what the CPU emulation was accepted at)
    um = tw._umfa()
    q, k, v, cu_q, cu_k = tw._case(tw.LENS_Q, tw.LENS_K, 4, 2, D, DT[dt], seed=7 + causal)
    out, _ = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, max(tw.LENS_Q), max(tw.LENS_K), scale=D ** -0.5, causal=causal,
                                             out_dtype=torch.float32, window=window)
    torch.cuda.synchronize()
    kernel = um.last_kernel()
    banded = not (window[0] == -1 and (causal or window[1] == 0))
    assert kernel.startswith("fa_fwd16_varlen_window<" if banded else "fa_fwd16_varlen<"), kernel
    cq, ck = cu_q.cpu().numpy(), cu_k.cpu().numpy()
    want, lse = varlen_window_ref.forward(_np(q), _np(k), _np(v), cq, ck, causal, window)
    floor = varlen_window_ref.forward(_np(q), _np(k), _np(v), cq, ck, causal, window, kind=ffr.KIND)[0]  # the band's visibility
    nk = np.zeros(q.shape[0], np.int64)
    for q0, Lq, _, Lk in varlen_window_ref.seqs(cq, ck):
        nk[q0:q0 + Lq] = varlen_window_ref.visible(Lq, Lk, causal, window).sum(1)
    one_key_only = window == (0, 0) or (causal and window[0] == 0)  # every row sees its own diagonal key and nothing else
    assert one_key_only == (nk.max() <= 1)
    H = q.shape[1]
    ffr.check_pool(_np(out).reshape(-1, D), want.reshape(-1, D), floor.reshape(-1, D), np.repeat(nk, H), dt, kernel,
                   f"window {window} causal={causal} {dt}", "exact", min_elems=0 if one_key_only else 4096, live=np.isfinite(lse).T)


# ------------------------------------------------------------------------------------------------ the dropout forward
@TYPES
@pytest.mark.parametrize("B,H,Sq,Skv,D,causal,p", td.VALUE_CASES[:3])
def test_dropout_forward(dt, B, H, Sq, Skv, D, causal, p):
    """the floor rounds keep o P; compared on sample_rows (both edges of every 128-row block and seeded interior rows per slab)"""
    um = td._umfa()
    gen = torch.Generator(device="cuda").manual_seed(Sq * 31 + Skv + D)
    q, k, v = (torch.randn(B, H, S, D, generator=gen, device="cuda").to(DT[dt]) for S in (Sq, Skv, Skv))
    rs = td._rs(977 + Sq, 13 * Skv)
    keep = td._keep(B, H, Sq, Skv, p, rs)
    o, _ = um.ops.attention_forward_dropout(q, k, v, p, rs, scale=D ** -0.5, causal=causal, out_dtype=torch.float32)
    torch.cuda.synchronize()
    kernel = um.last_kernel()
    assert kernel.startswith("fa_fwd16_drop<"), kernel
    rows = tol.sample_rows(Sq, B, H, seed=Sq + Skv)
    want = dropout_ref.forward(_np(q), _np(k), _np(v), keep, p, scale=D ** -0.5, causal=causal)[0]
    floor = dropout_ref.forward(_np(q), _np(k), _np(v), keep, p, scale=D ** -0.5, causal=causal, kind=ffr.KIND)[0]
    nk = np.minimum(rows + 1, Skv) if causal else np.full(rows.shape, Skv)  # visible keys (top-left causal), kept or not
    sel = lambda a: tol.gather_rows(a, rows).reshape(-1, D)  # noqa: E731
    ffr.check_pool(sel(_np(o)), sel(want), sel(floor), nk.reshape(-1), dt, kernel, f"dropout p={p} {Sq}x{Skv} {dt}", "exact",
                   live=np.ones(nk.size, bool))  # (top-left causal with Sq <= Skv or row 0 onwards: every row sees its own key)
