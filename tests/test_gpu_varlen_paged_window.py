"""Sliding-window attention for packed variable-length queries over a paged or static KV cache on the GPU
(umfa_torch.varlen_kvcache_window_attention, fa_fwd16_paged_varlen_window), held to the forward FORMAT FLOOR as
tests/test_gpu_paged_window.py holds the dense entry: per case all live rows that see two keys or more are pooled into one comparison
against tests/varlen_paged_window_ref.py's forward(kind=KIND) under forward_floor_ref.check_pool (floor=, form_regime, live= from the
reference's LSE, at least 4096 elements); only rows without keys (exact zeros) and one-key rows (2^-22) are left out.  The window (0, 0) is
the exception: every live row sees one key (min_elems = 0).  A launch that holds a decode-form item (or is split) takes form_regime's
"stale" multiple for the pool's maximum, as every kernel with several running maxima does; the rms multiple is the same for all forms.
tests/test_varlen_paged_window_ref_cpu.py shows that an emulation of the kernel's arithmetic stays inside these bounds at these shapes.

Then: bitwise agreement with kvcache_window_attention at equal L_q and with varlen_kvcache_attention for a window that bounds nothing,
parts that divide the band, NaN-poisoned rows and garbage table entries below the band (bitwise the clean run), table holes inside the
band, bf16 V far from fp16's range, the append (bitwise, nothing else written), static caches, hostile cu / lengths / table entries
(guards and canaries), the fused rotary, graph replay across a step boundary, and the ops' plumbing.  Seeded inputs, fp32 O."""
import numpy as np
import pytest
import torch

import forward_floor_ref as ffr
import paged_rope_ref as rr
import test_gpu_varlen_paged as tv
import tolerances as tol
import varlen_paged_ref as vpr
import varlen_paged_window_ref as vwr
from paged_rope_gpu import rotate_by_ops, tables

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
GUARD = tv.GUARD
NEW = "fa_fwd16_paged_varlen_window<"
_np, _bits, _i32, _cu = tv._np, tv._bits, tv._i32, tv._cu


def _umfa():
    import umfa_torch
    return umfa_torch


def _run(q, kc, vc, cu, max_q, sl, bt, kn=None, vn=None, causal=False, window=(-1, -1), num_splits=0, out=None, lse=None, **rope):
    um = _umfa()
    o, lse = um.ops.varlen_kvcache_attention_window_forward(q, kc, vc, cu, max_q, sl, bt, kn, vn, scale=q.shape[-1] ** -0.5, causal=causal,
                                                            window=window, num_splits=num_splits, out_dtype=torch.float32, out=out, lse=lse,
                                                            **rope)
    torch.cuda.synchronize()
    return o, lse, um.last_kernel()


def _check(dt, q, kc0, vc0, cu, max_q, sl, bt, o, lse, kernel, causal, window, num_splits, tag, kn=None, vn=None):
    """one pooled comparison of a window call (the caches as they were before it) over the rows some sequence covers"""
    Tq, H, D = q.shape
    Hkv = kc0.shape[2]
    g = H // Hkv
    cap = kc0.shape[1] * (bt.shape[1] if bt is not None else 1)
    plain = vwr.normalise(window, causal, max_q, cap)[1]
    assert kernel.startswith("fa_fwd16_paged_varlen<" if plain else NEW) and f"{dt},{D}" in kernel, kernel
    if num_splits:
        assert ("split" in kernel) == (num_splits > 1), kernel
    cuv, slv, btn = cu.cpu().numpy(), sl.cpu().numpy(), None if bt is None else bt.cpu().numpy()
    knn, vnn = (None if t is None else _np(t) for t in (kn, vn))
    (want, floor), lse_ref = vwr.forward_kinds(_np(q), _np(kc0), _np(vc0), cuv, max_q, slv, btn, knn, vnn, causal, window)[:2]
    nk = vwr.nkeys(Tq, cuv, max_q, slv, tuple(kc0.shape), btn, kn is not None, causal, window)
    cov = vpr.covered(cuv, Tq, max_q)
    live = np.isfinite(lse_ref)  # [H, T_q]
    l_ = _np(lse)
    assert np.isneginf(l_[~live & cov[None, :]]).all(), (tag, "a row without keys has a finite LSE")
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)  # (the bound tests/test_gpu_paged.py holds the LSE to)
    decode = any(0 < g * l <= 32 for _, l in vpr.ranges(cuv, Tq, max_q))
    rows = lambda a: a[cov].reshape(-1, D)  # noqa: E731
    res = ffr.check_pool(rows(_np(o)), rows(want), rows(floor), np.repeat(nk[cov], H), dt, kernel, f"{tag} {dt}",
                         ffr.form_regime(32 if decode else 128, "split" in kernel), min_elems=0 if tuple(window) == (0, 0) else 4096,
                         live=live.T[cov])
    print(f"{tag} {dt} D{D}: {kernel} pool {int((nk[cov] >= 2).sum()) * H * D} elements, (max, rms) vs floor {res}")


# ------------------------------------------------------------------------------------------------ the mixed batch
MIXED_WINDOWS = ffr.WINDOWS + [(128, 0), (300, 0)]
# (page_size, g, dtype, head_dim, num_splits): pages 16 and 64, g 1 and 8, both operand types and head dims, automatic / one / three parts
MIXED = [(16, 1, "bf16", 128, 0), (64, 8, "fp16", 64, 1), (16, 8, "bf16", 128, 3), (64, 1, "fp16", 64, 0)]


@pytest.mark.parametrize("window", MIXED_WINDOWS)
def test_mixed_batch(window):
    """prefill chunks beside decode in one launch: L_q 1, 1, 5, 130, 200, 0, 32, 33 over 5 .. 1000 cached keys; per window every
    configuration of MIXED, with and without new tokens"""
    um = _umfa()
    lq, cache, Hkv = ffr.PACKED_LQ, ffr.PACKED_CACHE, 2
    cu, sl = _i32(_cu(lq)), _i32(cache)
    causal = window[1] == 0
    for ps, g, dt, D, num_splits in MIXED:
        for new in (False, True):
            max_pages = -(-(max(cache) + max(lq)) // ps)
            q, kc, vc, bt, kn, vn = tv._setup(lq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=700 + ps + g + window[0], new=new, share=not new)
            kc0, vc0 = kc.clone(), vc.clone()
            o, lse, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, kn, vn, causal=causal, window=window, num_splits=num_splits)
            assert kernel.startswith(NEW), kernel
            assert um.ops.varlen_kvcache_item_counts() == vwr.items(lq, g, Hkv)  # both forms, in this one launch
            _check(dt, q, kc0, vc0, cu, max(lq), sl, bt, o, lse, kernel, causal, window, num_splits, f"mixed g{g} page{ps} {window} new{new}",
                   kn, vn)


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("Sq,new", [(1, False), (1, True), (4, True), (40, False), (40, True)])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("num_splits", [0, 1, 3])
def test_equal_lengths_agree_bitwise_with_kvcache_window_attention(Sq, new, dt, num_splits):
    """every L_q equal: the arithmetic, its order and the automatic part count are kvcache_window_attention's (decode form at Sq 1 and
    4, 128-row blocks at Sq 40)"""
    um = _umfa()
    B, H, Hkv, D, ps, mp = 4, 8, 2, 128, 16, 40
    q, kc, vc, bt, kn, vn = tv._setup([Sq] * B, H, Hkv, D, ps, mp, DT[dt], seed=730 + Sq, new=new, share=False)
    cu, sl = _i32(_cu([Sq] * B)), _i32([0, 150, ps + 5, 600])
    r = lambda t: None if t is None else t.view(B, Sq, *t.shape[1:])  # noqa: E731
    for window, causal in (((100, 0), True), ((30, 2), False), ((-1, Sq - 1), False) if Sq > 1 else ((0, 0), True)):
        kc1, vc1, kc2, vc2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        o, lse, kernel = _run(q, kc1, vc1, cu, Sq, sl, bt, kn, vn, causal=causal, window=window, num_splits=num_splits)
        assert kernel.startswith(NEW), kernel
        o2, lse2 = um.ops.kvcache_attention_window_forward(r(q), kc2, vc2, sl, bt, r(kn), r(vn), scale=D ** -0.5, causal=causal, window=window,
                                                           num_splits=num_splits, out_dtype=torch.float32)
        torch.cuda.synchronize()
        assert um.last_kernel() == kernel.replace("_varlen", ""), (um.last_kernel(), kernel)  # (the same part count when automatic)
        assert torch.equal(o.view(B, Sq, H, D), o2), window
        assert torch.equal(lse.view(H, B, Sq).permute(1, 0, 2), lse2), window
        assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2)


def test_a_window_that_bounds_nothing_is_the_unwindowed_call():
    um = _umfa()
    lq = [1, 40, 4, 9]
    q, kc, vc, bt, _, _ = tv._setup(lq, 8, 2, 128, 16, 8, torch.bfloat16, seed=740)
    cu, sl = _i32(_cu(lq)), _i32([5, 77, 128, 100])
    cap, mq = 16 * 8, 40
    for causal in (False, True):
        want = um.varlen_kvcache_attention(q, kc, vc, cu, mq, sl, block_table=bt, causal=causal, return_softmax_lse=True)
        torch.cuda.synchronize()
        plain = um.last_kernel()
        assert plain.startswith("fa_fwd16_paged_varlen<"), plain
        for w in ((-1, -1), (cap, mq), (cap + 5, -1)) + (((-1, 0), (cap, 0), (-1, 3)) if causal else ()):
            got = um.varlen_kvcache_window_attention(q, kc, vc, cu, mq, sl, block_table=bt, causal=causal, window_size=w, return_softmax_lse=True)
            torch.cuda.synchronize()
            assert um.last_kernel() == plain, (w, um.last_kernel())
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), w
            # ... and the C entry normalises for itself: the same window handed to it unnormalised
            o2, l2 = um.ops.varlen_kvcache_attention_window_forward(q, kc, vc, cu, mq, sl, bt, scale=128 ** -0.5, causal=causal, window=w)
            torch.cuda.synchronize()
            assert um.last_kernel() == plain and torch.equal(o2, want[0]) and torch.equal(l2, want[1]), w
    for causal, w in ((False, (-1, 0)), (True, (cap - 1, 0)), (False, (-1, mq - 1)), (False, (8, 0))):  # binding windows
        um.varlen_kvcache_window_attention(q, kc, vc, cu, mq, sl, block_table=bt, causal=causal, window_size=w)
        torch.cuda.synchronize()
        assert um.last_kernel().startswith(NEW), (w, um.last_kernel())


# ------------------------------------------------------------------------------------------------ split and band
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128)])
@pytest.mark.parametrize("window,num_splits", [((64, 0), 8), ((300, 0), 3), ((300, 0), 0)])
def test_parts_divide_each_items_band(dt, D, window, num_splits):
    """window (64, 0) with 8 forced parts: a decode item's band is one or two steps and a 128-row item's at most three, so most parts are
    empty; sequence 2 has L_k < L_q (its first 50 tokens see nothing); the band of 301 keys is longer than sequences 1 and 2 hold and
    shorter than sequences 0 and 3"""
    lq, cache = [1, 4, 150, 40, 2], [1000, 30, 100, 700, 129]
    q, kc, vc, bt, _, _ = tv._setup(lq, 8, 2, D, 64, 16, DT[dt], seed=750)
    cu, sl = _i32(_cu(lq)), _i32(cache)
    o, lse, kernel = _run(q, kc, vc, cu, 150, sl, bt, causal=True, window=window, num_splits=num_splits)
    _check(dt, q, kc, vc, cu, 150, sl, bt, o, lse, kernel, True, window, num_splits, f"band {window} splits{num_splits}")
    assert torch.equal(o[5:55], torch.zeros_like(o[5:55])) and torch.isneginf(lse[:, 5:55]).all()
    o2, lse2, _ = _run(q, kc, vc, cu, 150, sl, bt, causal=True, window=window, num_splits=num_splits)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)  # the fold takes the parts in order: bitwise repeatable


# ------------------------------------------------------------------------------------------------ one mechanism each
@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 64)])
@pytest.mark.parametrize("num_splits", [0, 2])
def test_poison_below_the_band_is_never_read(dt, D, num_splits):
    """window (40, 0), decode items beside a 40-token chunk: NaN in every cache row below each sequence's first band and garbage in the
    table entries of every logical page wholly below it change no bit of O or LSE; the guard pages come back as they were"""
    B, Hkv, g, ps, left = 4, 2, 4, 16, 40
    lq, lens = [1, 1, 40, 1], [100, 200, 333, 640]
    q, kc, vc, bt, _, _ = tv._setup(lq, g * Hkv, Hkv, D, ps, 40, DT[dt], seed=760, share=False)
    cu, sl = _i32(_cu(lq)), _i32(lens)
    args = dict(causal=True, window=(left, 0), num_splits=num_splits)
    o0, lse0, kernel = _run(q, kc, vc, cu, 40, sl, bt, **args)
    assert kernel.startswith(NEW), kernel
    assert torch.isfinite(o0).all() and torch.isfinite(lse0).all()
    btn = bt.cpu().numpy()
    first = [L - l - left for l, L in zip(lq, lens)]  # the lowest key any row of the sequence sees: token 0's i + off - left
    kp, vp = (torch.full_like(t, float("nan")) for t in (kc, vc))
    for t, src in ((kp, kc), (vp, vc)):
        t[:GUARD], t[-GUARD:] = src[:GUARD], src[-GUARD:]
        for b, L in enumerate(lens):
            for j in range(first[b], L):  # the bands' rows alone hold values
                t[btn[b, j // ps], j % ps] = src[btn[b, j // ps], j % ps]
    kp0, vp0 = kp.clone(), vp.clone()
    for bad in (-1, kc.shape[0], 2 ** 31 - 1, -(2 ** 31), "other"):
        b2 = btn.copy()
        for b, L in enumerate(lens):
            below = first[b] // ps  # logical pages 0 .. below - 1 lie wholly below every band of the sequence
            b2[b, :below] = btn[(b + 1) % B, (lens[(b + 1) % B] - 1) // ps] if bad == "other" else bad
        o1, lse1, _ = _run(q, kp, vp, cu, 40, sl, torch.tensor(b2, device="cuda"), **args)
        assert torch.equal(o0, o1) and torch.equal(lse0, lse1), bad
    assert (_bits(kp) == _bits(kp0)).all() and (_bits(vp) == _bits(vp0)).all()  # (NaN != NaN: the pools are compared as bits)


@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128)])
@pytest.mark.parametrize("window", [(40, 0), (90, 0)])
def test_table_entries_outside_the_pool_inside_the_band(dt, D, window):
    lq = [1, 24, 3, 40]
    q, kc, vc, bt, _, _ = tv._setup(lq, 16, 2, D, 16, 8, DT[dt], seed=770, share=False)
    b = bt.cpu().numpy().copy()
    b[:, 1] = kc.shape[0]  # keys 16 .. 31 of every sequence: one past the pool
    b[2, 3] = -1
    b[3, 6] = 2 ** 31 - 1
    bt = torch.tensor(b, device="cuda")
    cu, sl = _i32(_cu(lq)), _i32(ffr.HOLE_LENS)
    o, lse, kernel = _run(q, kc, vc, cu, 40, sl, bt, causal=True, window=window)
    assert torch.isfinite(o).all()
    _check(dt, q, kc, vc, cu, 40, sl, bt, o, lse, kernel, True, window, 0, f"holes {window}")


@pytest.mark.parametrize("mag", [1e-9, 1e20])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_bf16_v_far_from_fp16_range(mag, num_splits):
    """the range rule's second sweep starts at each item's own band: window (100, 0) at L_k 640 is step 4 alone of five for the decode item"""
    lq = [4, 1, 150]
    q, kc, vc, bt, _, _ = tv._setup(lq, 8, 2, 128, 32, 20, torch.bfloat16, seed=780)
    vc = (vc.float() * mag).to(torch.bfloat16)
    cu, sl = _i32(_cu(lq)), _i32([640, 77, 333])
    o, lse, kernel = _run(q, kc, vc, cu, 150, sl, bt, causal=True, window=(100, 0), num_splits=num_splits)
    assert kernel.startswith(NEW) and ("split" in kernel) == (num_splits > 1), kernel
    assert torch.isfinite(o).all()
    o_ref, lse_ref = vwr.forward(_np(q), _np(kc), _np(vc), _cu(lq), 150, sl.cpu().numpy(), bt.cpu().numpy(), None, None, True, (100, 0))[:2]
    assert np.isfinite(lse_ref).all()
    np.testing.assert_allclose(_np(lse), lse_ref, rtol=0, atol=2e-3)
    tol.check_forward(_np(o).reshape(1, 1, -1, 128), o_ref.reshape(1, 1, -1, 128), torch.bfloat16, kernel, tag="varlen_paged_window far V")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("static", [False, True], ids=["paged", "static"])
def test_append_writes_rows_bitwise_and_nothing_else(dt, static):
    lq, H, Hkv, D = [5, 0, 1, 40, 3], 8, 2, 64
    if static:
        g = torch.Generator(device="cuda").manual_seed(790)
        q = torch.randn(sum(lq), H, D, device="cuda", dtype=DT[dt], generator=g)
        kc, vc, = (torch.randn(len(lq), 48, Hkv, D, device="cuda", dtype=DT[dt], generator=g) for _ in range(2))
        kn, vn = (torch.randn(sum(lq), Hkv, D, device="cuda", dtype=DT[dt], generator=g) for _ in range(2))
        bt = None
    else:
        q, kc, vc, bt, kn, vn = tv._setup(lq, H, Hkv, D, 16, 3, DT[dt], seed=791, new=True, share=False)
    lens = [14, 7, 47, 3, 46]  # page crossings; the last one runs past the capacity of 48: one row dropped
    cu, sl = _i32(_cu(lq)), _i32(lens)
    kc0, vc0 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, cu, 40, sl, bt, kn, vn, causal=True, window=(20, 0))
    btn = None if bt is None else bt.cpu().numpy()
    kw, vw = vpr.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), _cu(lq), 40, np.array(lens), btn)
    assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()  # the rows written, bitwise, and every other byte unchanged
    assert not (kw == _bits(kc0)).all()
    if not static:
        assert (_bits(kc)[:GUARD] == _bits(kc0)[:GUARD]).all() and (_bits(kc)[-GUARD:] == _bits(kc0)[-GUARD:]).all()
    _check(dt, q, kc0, vc0, cu, 40, sl, bt, o, lse, kernel, True, (20, 0), 0, f"append static={static}", kn, vn)
    assert sl.cpu().tolist() == lens  # cache_seqlens is not advanced
    # append + attention = attention on a pre-appended cache with the advanced lengths (clamped at the capacity)
    o2, lse2, _ = _run(q, kc, vc, cu, 40, _i32(np.minimum(np.array(lens) + np.array(lq), 48)), bt, causal=True, window=(20, 0))
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("layout", ["bshd", "bhsd"])
def test_static_cache_mixed_batch(layout):
    lq, H, Hkv, D, Smax = [1, 200, 0, 4, 33], 8, 2, 128, 300
    g = torch.Generator(device="cuda").manual_seed(795)
    q = torch.randn(sum(lq), H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    if layout == "bshd":
        kc, vc = (torch.randn(len(lq), Smax, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    else:  # HF StaticCache: [B, H_kv, S_max, D], handed over as its [B, S_max, H_kv, D] view
        kc, vc = (torch.randn(len(lq), Hkv, Smax, D, device="cuda", dtype=torch.bfloat16, generator=g).transpose(1, 2) for _ in range(2))
    cu, sl = _i32(_cu(lq)), _i32([17, 300, 129, 0, 250])
    for window, causal in (((50, 0), True), ((20, 9), False)):
        o, lse, kernel = _run(q, kc, vc, cu, 200, sl, None, causal=causal, window=window)
        _check("bf16", q, kc, vc, cu, 200, sl, None, o, lse, kernel, causal, window, 0, f"static {layout} {window}")


# ------------------------------------------------------------------------------------------------ the contract's inputs
@pytest.mark.parametrize("num_splits", [0, 3])
@pytest.mark.parametrize("cu_kind", ["good", "non_monotone", "beyond"])
def test_hostile_contents_touch_nothing_else(num_splits, cu_kind):
    """tests/test_gpu_varlen_paged.py's case under a window: table entries -1 / num_pages / 2^31 - 1 / -2^31, lengths negative and 10^9,
    cu non-monotone and beyond T_q -- every index is clamped or range-checked on the device: the guard pages and the canary rows around
    q / k_new / v_new / O / LSE come back bit-identical"""
    H, Hkv, D, ps, mp, C = 8, 2, 128, 16, 4, 8  # C canary rows around q / O / LSE
    lq = [3, 2, 40, 1, 5]
    Tq = sum(lq)
    _, kc, vc, bt, _, _ = tv._setup(lq, H, Hkv, D, ps, mp, torch.bfloat16, seed=800, share=False)
    g = torch.Generator(device="cuda").manual_seed(801)
    q_big = torch.randn(Tq + 2 * C, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kn_big = torch.randn(Tq + 2 * C, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vn_big = torch.randn(Tq + 2 * C, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    o_big = torch.full((Tq + 2 * C, H, D), 7.0, device="cuda", dtype=torch.float32)
    lse_big = torch.full(((H + 2 * C) * Tq,), 7.0, device="cuda", dtype=torch.float32)
    q, kn, vn, out = q_big[C:C + Tq], kn_big[C:C + Tq], vn_big[C:C + Tq], o_big[C:C + Tq]
    lse = lse_big[C * Tq:(C + H) * Tq].view(H, Tq)
    btn = bt.cpu().numpy()
    num_pages = kc.shape[0]
    btn[0, :] = -1
    btn[1, 1], btn[1, 3] = num_pages, 2 ** 31 - 1
    btn[2, 2] = -(2 ** 31)
    bt = torch.tensor(btn, device="cuda")
    sl = _i32([20, 30, -7, 10 ** 9, 60])
    cuv = {"good": _cu(lq), "non_monotone": np.array([0, 40, 3, 45, 20, Tq]), "beyond": np.array([-9, 5, 10 ** 9, 7, 2 ** 31 - 1, Tq + 50])}[cu_kind]
    cu = _i32(cuv)
    kc0, vc0, q0, kn0, vn0 = kc.clone(), vc.clone(), q_big.clone(), kn_big.clone(), vn_big.clone()
    _, _, kernel = _run(q, kc, vc, cu, 40, sl, bt, kn, vn, causal=True, window=(20, 0), num_splits=num_splits, out=out, lse=lse)
    assert kernel.startswith(NEW), kernel  # the call returns; values are checked for the good cu alone
    assert torch.equal(kc[:GUARD], kc0[:GUARD]) and torch.equal(kc[-GUARD:], kc0[-GUARD:])
    assert torch.equal(vc[:GUARD], vc0[:GUARD]) and torch.equal(vc[-GUARD:], vc0[-GUARD:])
    assert torch.equal(q_big, q0) and torch.equal(kn_big, kn0) and torch.equal(vn_big, vn0)
    assert (o_big[:C] == 7.0).all() and (o_big[C + Tq:] == 7.0).all()
    assert (lse_big[:C * Tq] == 7.0).all() and (lse_big[(C + H) * Tq:] == 7.0).all()
    if cu_kind == "good":  # defined results: the pools equal the reference's append, the values its attention
        kw, vw = vpr.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), cuv, 40, sl.cpu().numpy(), btn)
        assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()
        _check("bf16", q, kc0, vc0, cu, 40, sl, bt, out, lse, kernel, True, (20, 0), num_splits, "hostile", kn, vn)


def test_uncovered_rows_are_not_written():
    lq, pad = [3, 50, 1], 6  # max_seqlen_q = 20 caps the 50-token sequence: its rows 20 .. 49 and the 6 pad rows belong to nobody
    q, kc, vc, bt, _, _ = tv._setup(lq, 8, 2, 64, 16, 8, torch.float16, seed=810, pad=pad)
    Tq = q.shape[0]
    cu, sl = _i32(_cu(lq)), _i32([100, 90, 128])
    cov = torch.tensor(vpr.covered(_cu(lq), Tq, 20), device="cuda")
    assert cov.sum().item() == 3 + 20 + 1
    for n in (1, 2):
        out = torch.full((Tq, 8, 64), 7.0, device="cuda", dtype=torch.float32)
        lse = torch.full((8, Tq), 7.0, device="cuda", dtype=torch.float32)
        _, _, kernel = _run(q, kc, vc, cu, 20, sl, bt, causal=False, window=(30, 2), num_splits=n, out=out, lse=lse)
        assert (out[~cov] == 7.0).all() and (lse[:, ~cov] == 7.0).all()
        _check("fp16", q, kc, vc, cu, 20, sl, bt, out, lse, kernel, False, (30, 2), n, "uncovered")


# ------------------------------------------------------------------------------------------------ rotary, graph replay
@pytest.mark.parametrize("dt,D,rd,inter,causal,splits", [("bf16", 128, 128, False, True, 0), ("fp16", 64, 32, True, False, 2)])
def test_fused_rotary_is_the_call_on_rotated_operands(dt, D, rd, inter, causal, splits):
    um = _umfa()
    lq, H, Hkv, ps, maxp = [4, 1, 40, 2], 8, 2, 16, 12
    q, kc, vc, bt, kn, vn = tv._setup(lq, H, Hkv, D, ps, maxp, DT[dt], seed=820, new=True, share=False)
    cos, sin = tables(ps * maxp + 8, rd, torch.float32, 821)
    lens = [14, 60, 100, 150]
    cu, sl = _i32(_cu(lq)), _i32(lens)
    window = (30, 0) if causal else (30, 1)
    kw = dict(block_table=bt, causal=causal, window_size=window, num_splits=splits, return_softmax_lse=True)
    k1, v1 = kc.clone(), vc.clone()
    o1, l1 = um.varlen_kvcache_window_attention(q, k1, v1, cu, 40, sl, k=kn, v=vn, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, **kw)
    torch.cuda.synchronize()
    name = um.last_kernel()
    assert name.startswith(NEW) and ("split" in name) == (splits > 1), name
    pq, cov = rr.packed_positions(_cu(lq), sum(lq), 40, np.array(lens), ps * maxp, causal)
    pk, _ = rr.packed_positions(_cu(lq), sum(lq), 40, np.array(lens), ps * maxp, True)
    assert cov.all()
    rq, rk = rotate_by_ops(um, q, pq, cos, sin, inter), rotate_by_ops(um, kn, pk, cos, sin, inter)
    k2, v2 = kc.clone(), vc.clone()
    o2, l2 = um.varlen_kvcache_window_attention(rq, k2, v2, cu, 40, sl, k=rk, v=vn, **kw)
    torch.cuda.synchronize()
    assert um.last_kernel() == name
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(k1, kc)


def test_graph_replay_follows_cu_lengths_and_table_across_a_step_boundary():
    """append + attention with window (16, 0) captured with a decode sequence at length 140 (k_first = 124, step 0); the lengths advance
    to 150 between replays (k_first = 134, step 1), cu moves the 40-token chunk to another sequence and the table is permuted: every
    replay equals the eager call, bit for bit"""
    um = _umfa()
    H, Hkv, D, ps, Tq, max_q = 8, 2, 128, 16, 42, 40
    first, second = [1, 40, 1], [40, 1, 1]
    q, kc, vc, bt, kn, vn = tv._setup(first, H, Hkv, D, ps, 20, torch.bfloat16, seed=830, new=True, share=False)
    cu, sl = _i32(_cu(first)), _i32([140, 60, 250])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.varlen_kvcache_window_attention(q, kc, vc, cu, max_q, sl, block_table=bt, k=kn, v=vn, causal=True, window_size=(16, 0),
                                                  num_splits=2, return_softmax_lse=True)

    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: scratch grows outside the capture
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = step()
    perm = torch.tensor(np.random.default_rng(0).permutation(bt.cpu().numpy().ravel()).reshape(bt.shape), device="cuda")
    for it in range(4):  # lengths 140, 145, 150, 150
        if it in (1, 2):
            sl.add_(5)
        if it == 2:
            bt.copy_(perm)
        if it == 3:
            cu.copy_(_i32(_cu(second)))
        kc0, vc0 = kc.clone(), vc.clone()
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in res]
        kr, vr = kc.clone(), vc.clone()
        kc.copy_(kc0)
        vc.copy_(vc0)
        want = step()
        torch.cuda.synchronize()
        assert um.last_kernel().startswith(NEW) and "split" in um.last_kernel()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), it
        assert torch.equal(kr, kc) and torch.equal(vr, vc), it
        o_ref, lse_ref = vwr.forward(_np(q), _np(kc0), _np(vc0), cu.cpu().numpy(), max_q, sl.cpu().numpy(), bt.cpu().numpy(), _np(kn), _np(vn),
                                     True, (16, 0))[:2]
        assert np.isfinite(lse_ref).all()
        np.testing.assert_allclose(_np(got[1]), lse_ref, rtol=0, atol=2e-3)
        tol.check_forward(_np(got[0]).reshape(1, 1, -1, D), o_ref.reshape(1, 1, -1, D), torch.bfloat16, um.last_kernel(),
                          tag="varlen_paged_window graph", out_dt=torch.bfloat16)
    assert sl.cpu().tolist() == [150, 70, 260]


# ------------------------------------------------------------------------------------------------ plumbing
def test_opcheck_custom_ops():
    _umfa()
    lq = [2, 40, 1]
    q, kc, vc, bt, kn, vn = tv._setup(lq, 8, 2, 64, 16, 4, torch.bfloat16, seed=840, new=True)
    cos, sin = tables(72, 32, torch.float32, 841)
    cu, sl = _i32(_cu(lq)), _i32([5, 20, 33])
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_window_forward.default, (q, kc, vc, cu, 40, sl, bt, True, 8, 0, 0.125, 0))
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_window_forward_append.default, (q, kc, vc, kn, vn, cu, 40, sl, bt, True, 8, 0, 0.125, 2))
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_window_rope_forward_append.default,
                          (q, kc, vc, kn, vn, cu, 40, sl, cos, sin, False, bt, False, 8, 1, 0.125, 0))


def test_compile_fullgraph_single_node():
    um = _umfa()
    lq = [1, 35, 2]
    q, kc, vc, bt, kn, vn = tv._setup(lq, 8, 2, 128, 16, 8, torch.float16, seed=850, new=True)
    cu, sl = _i32(_cu(lq)), _i32([30, 64, 1])
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.varlen_kvcache_window_attention(q, kc, vc, cu, 35, sl, block_table=bt, k=kn, v=vn, causal=True, window_size=(20, 0))

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.varlen_kvcache_window_forward_append"], calls
    assert torch.equal(oc, oe)
    assert torch.equal(kc, kc_e) and torch.equal(vc, vc_e)  # the compiled call appended in place too


def test_refusals_and_no_backward():
    um = _umfa()
    lq = [1, 20, 3]
    q, kc, vc, bt, kn, vn = tv._setup(lq, 8, 2, 128, 16, 4, torch.bfloat16, seed=860, new=True)
    cu, sl = _i32(_cu(lq)), _i32([10, 20, 30])
    kc0 = kc.clone()
    call = lambda **kw: um.varlen_kvcache_window_attention(q, kw.pop("kc", kc), kw.pop("vc", vc), cu, 20, sl, block_table=bt, k=kn, v=vn,  # noqa: E731
                                                           **{"window_size": (8, 0), **kw})
    f8 = torch.float8_e4m3fn
    with pytest.raises(ValueError, match="fp8"):  # fp8 caches
        call(kc=kc.to(f8), vc=vc.to(f8))
    with pytest.raises(ValueError, match="fp8"):  # ... with descales too
        call(kc=kc.to(f8), vc=vc.to(f8), k_descale=1.0, v_descale=1.0)
    with pytest.raises(ValueError, match="fp8"):  # descales
        call(k_descale=1.0)
    for w in ((-2, 0), (0, -2), (8,), 8, (1, 2, 3)):
        with pytest.raises(ValueError):
            call(window_size=w)
    for kw in (dict(cache_batch_idx=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(softcap=30.0), dict(alibi_slopes=torch.zeros(8)),
               dict(cache_leftpad=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(seqused_k=sl), dict(dropout_p=0.1)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(TypeError):
        call(no_such_argument=1)
    with pytest.raises(ValueError):  # head_dim 96
        um.varlen_kvcache_window_attention(q[..., :96].contiguous(), kc[..., :96].contiguous(), vc[..., :96].contiguous(), cu, 20, sl,
                                           block_table=bt, window_size=(8, 0))
    with pytest.raises(um.ops.MFAError) as e:  # the C entry: a value below -1 is invalid arguments, nothing launched
        um.ops.varlen_kvcache_attention_window_forward(q, kc, vc, cu, 20, sl, bt, kn, vn, scale=0.1, window=(-2, 0))
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0)  # nothing was appended by a refused call
    o = call(softcap=0.0, dropout_p=0.0, cache_leftpad=None)  # the defaults are accepted
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == q.dtype and um.last_kernel().startswith(NEW) and not torch.equal(kc, kc0)
    qg = q.clone().requires_grad_(True)
    o = um.varlen_kvcache_window_attention(qg, kc, vc, cu, 20, sl, block_table=bt, window_size=(8, 0))
    with pytest.raises(RuntimeError):  # inference only: no backward
        o.float().sum().backward()


def test_public_entry_output_dtype_and_lse():
    um = _umfa()
    lq = [3, 1, 50]
    for dt in ("bf16", "fp16"):
        q, kc, vc, bt, _, _ = tv._setup(lq, 8, 2, 128, 64, 4, DT[dt], seed=870)
        cu, sl = _i32(_cu(lq)), _i32([100, 7, 200])
        o = um.varlen_kvcache_window_attention(q, kc, vc, cu, 50, sl, block_table=bt, causal=True, window_size=(50, 0))
        o2, lse = um.varlen_kvcache_window_attention(q, kc, vc, cu, 50, sl, block_table=bt, causal=True, window_size=(50, 0),
                                                     return_softmax_lse=True)
        torch.cuda.synchronize()
        assert o.dtype == DT[dt] and o.shape == q.shape and torch.equal(o, o2)
        assert lse.dtype == torch.float32 and lse.shape == (8, sum(lq))
        o_ref, lse_ref = vwr.forward(_np(q), _np(kc), _np(vc), _cu(lq), 50, sl.cpu().numpy(), bt.cpu().numpy(), None, None, True, (50, 0))[:2]
        assert np.isfinite(lse_ref).all()
        np.testing.assert_allclose(_np(lse), lse_ref, rtol=0, atol=1e-5)
        tol.check_forward(_np(o).reshape(1, 1, -1, 128), o_ref.reshape(1, 1, -1, 128), DT[dt], um.last_kernel(), tag="varlen_paged_window out",
                          out_dt=DT[dt])
