"""Sliding-window attention over a paged or static KV cache on the GPU (umfa_torch.kvcache_window_attention, fa_fwd16_paged_window;
DESIGN.md section 3.1m), held to the forward FORMAT FLOOR as tests/test_gpu_forward_floor.py holds the unwindowed kernels: per case all
live rows that see two keys or more are pooled into one comparison against tests/paged_window_ref.py's forward(kind=KIND) under
forward_floor_ref.check_pool (floor=, form_regime, live= from the reference's LSE, at least 4096 elements); only rows without keys
(exact zeros) and one-key rows (2^-22) are left out.  The window (0, 0) is the exception: every live row sees one key (min_elems = 0).
tests/test_paged_window_ref_cpu.py shows that an emulation of the kernel's arithmetic stays inside these bounds at these shapes.

Then: the append (bitwise, nothing else written), static caches, NaN-poisoned rows and garbage table entries below the band (bitwise
the clean run), bf16 V far from fp16's range, the bit-for-bit routing of a window that bounds nothing, agreement with the gather route,
the fused rotary, graph replay across a step boundary, and the ops' plumbing.  Seeded inputs, fp32 O."""
import numpy as np
import pytest
import torch

import forward_floor_ref as ffr
import paged_ref
import paged_rope_ref as rr
import paged_window_ref as pwr
import test_gpu_paged as tp
import tolerances as tol
from paged_rope_gpu import rotate_by_ops, tables

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TYPES = pytest.mark.parametrize("dt", ["bf16", "fp16"])
DIMS = pytest.mark.parametrize("D", [64, 128])
GUARD = tp.GUARD


def _umfa():
    import umfa_torch
    return umfa_torch


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def _run(q, kc, vc, sl, bt, kn=None, vn=None, causal=False, window=(-1, -1), num_splits=0, out_dtype=torch.float32):
    um = _umfa()
    o, lse = um.ops.kvcache_attention_window_forward(q, kc, vc, sl, bt, kn, vn, scale=q.shape[-1] ** -0.5, causal=causal, window=window,
                                                     num_splits=num_splits, out_dtype=out_dtype)
    torch.cuda.synchronize()
    return o, lse, um.last_kernel()


def _check(dt, q, kc0, vc0, sl, bt, o, lse, kernel, causal, window, num_splits, tag, kn=None, vn=None):
    """one pooled comparison of a window call (the caches as they were before it)"""
    B, Sq, H, D = q.shape
    Hkv = kc0.shape[2]
    cap = kc0.shape[1] * (bt.shape[1] if bt is not None else 1)
    plain = pwr.normalise(window, causal, Sq, cap)[1]  # (a side too wide to bind at this Sq / capacity: the unwindowed kernel, by the rule)
    assert kernel.startswith("fa_fwd16_paged<" if plain else "fa_fwd16_paged_window<") and f"{dt},{D}" in kernel, kernel
    if num_splits:
        assert ("split" in kernel) == (num_splits > 1), kernel
    slv, btn = sl.cpu().numpy(), None if bt is None else bt.cpu().numpy()
    knn, vnn = (None if t is None else _np(t) for t in (kn, vn))
    want, lse_ref = pwr.forward(_np(q), _np(kc0), _np(vc0), slv, btn, knn, vnn, causal, window)[:2]
    floor = pwr.forward(_np(q), _np(kc0), _np(vc0), slv, btn, knn, vnn, causal, window, kind=ffr.KIND)[0]
    nk = np.repeat(pwr.nkeys(Sq, slv, tuple(kc0.shape), btn, 0 if kn is None else kn.shape[1], causal, window)[:, :, None], H, axis=2)
    live = np.isfinite(lse_ref)
    l_ = _np(lse)
    assert np.isneginf(l_[~live]).all(), (tag, "a row without keys has a finite LSE")
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)  # (the bound tests/test_gpu_paged.py holds the LSE to)
    res = ffr.check_pool(_np(o).reshape(-1, D), want.reshape(-1, D), floor.reshape(-1, D), nk.reshape(-1), dt, kernel, f"{tag} {dt}",
                         ffr.form_regime((H // Hkv) * Sq, "split" in kernel), min_elems=0 if tuple(window) == (0, 0) else 4096,
                         live=live.transpose(0, 2, 1))
    print(f"{tag} {dt} D{D}: {kernel} pool {int((nk >= 2).sum()) * D} elements, (max, rms) vs floor {res}")


def _paged_run(dt, D, B, Hkv, g, Sq, ps, lens, causal, window, num_splits, tag, seed, S_new=0, table=None):
    max_pages = max(2, -(-(max(lens) + S_new) // ps))
    q, kc, vc, bt, kn, vn = tp._paged(B, Sq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=seed, S_new=S_new, share=S_new == 0)
    if table is not None:
        bt = table(bt, kc.shape[0])
    sl = tp._seqlens(lens)
    kc0, vc0 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, sl, bt, kn, vn, causal=causal, window=window, num_splits=num_splits)
    _check(dt, q, kc0, vc0, sl, bt, o, lse, kernel, causal, window, num_splits, tag, kn, vn)
    return (kc0, vc0, kc, vc, bt, kn, vn, sl)


# ------------------------------------------------------------------------------------------------ the decode form
# (Sq, window, causal, num_splits): a band inside one subtile; ending on and around the 32, 128 and page boundaries; longer than some
# sequences and shorter than others of one launch; L_k < Sq; more parts than band steps
DECODE = [(1, (0, 0), True, 1), (1, (1, 0), True, 1), (1, (15, 0), True, 1), (1, (16, 0), True, 1), (1, (127, 0), True, 3),
          (1, (128, 0), True, 1), (1, (300, 0), True, 3), (4, (17, 0), True, 1), (4, (130, 0), True, 3), (4, (5, 2), False, 1),
          (4, (-1, 1), False, 1), (4, (40, -1), False, 1)]


@TYPES
@DIMS
@pytest.mark.parametrize("Sq,window,causal,num_splits", DECODE)
def test_decode_form(dt, D, Sq, window, causal, num_splits):
    _paged_run(dt, D, 8, 2, 8, Sq, 16, ffr.DECODE_LENS, causal, window, num_splits, f"decode Sq{Sq} {window} splits{num_splits}",
               seed=200 + Sq + num_splits + window[0])


# ------------------------------------------------------------------------------------------------ the 128-row form
ROWS128_WINDOWS = [(31, 0), (128, 0), (100, 17), (-1, 40), (40, -1), (300, 0)]  # at Sq 200 and left 31 each wave's band is two subtiles


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 64)])
@pytest.mark.parametrize("ps", ffr.ROWS128_PAGES)
@pytest.mark.parametrize("window", ROWS128_WINDOWS)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_128_row_form(dt, D, ps, window, g, Sq):
    _paged_run(dt, D, 4, 2, g, Sq, ps, ffr.rows128_lens(ps), window[1] == 0, window, 1, f"128-row g{g} Sq{Sq} page{ps} {window}",
               seed=300 + ps + Sq)


@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128)])
@pytest.mark.parametrize("num_splits,L", ffr.ROWS128_SPLIT)
@pytest.mark.parametrize("window", [(64, 0), (500, 0)])
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_128_row_form_split(dt, D, num_splits, L, window, g, Sq):
    """the parts divide the band's steps: with window (64, 0) a block's band is at most three steps, so 8 parts leave five or more empty"""
    _paged_run(dt, D, 2, 2, g, Sq, 64, [L, L - 37], True, window, num_splits, f"128-row split{num_splits} L{L} g{g} Sq{Sq} {window}",
               seed=400 + L + Sq)


# ------------------------------------------------------------------------------------------------ one mechanism each
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("fp16", 128)])
@pytest.mark.parametrize("Sq", [1, 24])
@pytest.mark.parametrize("window", [(40, 0), (90, 0)])
def test_table_entries_outside_the_pool_inside_the_band(dt, D, Sq, window):
    def table(bt, num_pages):
        b = bt.cpu().numpy().copy()
        b[:, 1] = num_pages  # keys 16 .. 31 of every sequence: one past the pool
        b[2, 3] = -1
        return torch.tensor(b, device="cuda")

    _paged_run(dt, D, 4, 2, 8, Sq, 16, ffr.HOLE_LENS, True, window, 0, f"holes Sq{Sq} {window}", seed=500 + Sq, table=table)


@TYPES
@DIMS
def test_append_across_a_page_boundary(dt, D):
    """three new tokens from positions 14, 30, 47 and 62 of 16-key pages, window (20, 0): the rows written bitwise, nothing else"""
    kc0, vc0, kc, vc, bt, kn, vn, sl = _paged_run(dt, D, 4, 2, 8, 3, 16, ffr.APPEND_LENS, True, (20, 0), 0, "append", seed=510, S_new=3)
    kw, vw = paged_ref.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), sl.cpu().numpy(), bt.cpu().numpy())
    assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()  # the rows written, bitwise, and every other byte unchanged
    assert not (kw == _bits(kc0)).all()
    assert (sl.cpu().numpy() == ffr.APPEND_LENS).all()  # cache_seqlens is not advanced


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 64)])
@pytest.mark.parametrize("layout", ["bshd", "bhsd"])
def test_static_cache(dt, D, layout):
    B, Smax, Hkv, g, Sq = 3, 300, 2, 4, 4
    gen = torch.Generator(device="cuda").manual_seed(520)
    q = torch.randn(B, Sq, g * Hkv, D, device="cuda", dtype=DT[dt], generator=gen)
    if layout == "bshd":
        kc, vc = (torch.randn(B, Smax, Hkv, D, device="cuda", dtype=DT[dt], generator=gen) for _ in range(2))
    else:  # HF StaticCache's [B, H_kv, S_max, D], handed over as its [B, S_max, H_kv, D] view
        kc, vc = (torch.randn(B, Hkv, Smax, D, device="cuda", dtype=DT[dt], generator=gen).transpose(1, 2) for _ in range(2))
    sl = tp._seqlens([17, 300, 129])
    o, lse, kernel = _run(q, kc, vc, sl, None, causal=True, window=(50, 0))
    _check(dt, q, kc, vc, sl, None, o, lse, kernel, True, (50, 0), 0, f"static {layout}")


@TYPES
@DIMS
def test_poison_below_the_band_is_never_read(dt, D):
    """decode, window (40, 0): NaN in every cache row outside each sequence's band and garbage in the table entries of every logical page
    wholly below it change no bit of O or LSE; the guard pages come back as they were.  Both head dims: a DMA piece holds 4 rows at D 128
    and 8 at D 64, so the rows of one 16-key group that land as zeros are cut differently"""
    B, Hkv, g, ps, left = 4, 2, 4, 16, 40
    lens = [100, 200, 333, 640]
    q, kc, vc, bt, _, _ = tp._paged(B, 1, g * Hkv, Hkv, D, ps, 40, DT[dt], seed=530, share=False)
    sl = tp._seqlens(lens)
    o0, lse0, kernel = _run(q, kc, vc, sl, bt, causal=True, window=(left, 0), num_splits=0)
    assert kernel.startswith("fa_fwd16_paged_window<"), kernel
    assert torch.isfinite(o0).all() and torch.isfinite(lse0).all()
    btn = bt.cpu().numpy()
    kp, vp = (torch.full_like(t, float("nan")) for t in (kc, vc))
    for t, src in ((kp, kc), (vp, vc)):
        t[:GUARD], t[-GUARD:] = src[:GUARD], src[-GUARD:]
        for b, L in enumerate(lens):
            for j in range(L - 1 - left, L):  # the band's rows alone hold values
                t[btn[b, j // ps], j % ps] = src[btn[b, j // ps], j % ps]
    kp0, vp0 = kp.clone(), vp.clone()
    for bad in (-1, kc.shape[0], 2 ** 31 - 1, -(2 ** 31), "other"):
        b2 = btn.copy()
        for b, L in enumerate(lens):
            below = (L - 1 - left) // ps  # logical pages 0 .. below - 1 lie wholly below the band
            b2[b, :below] = btn[(b + 1) % B, (lens[(b + 1) % B] - 1) // ps] if bad == "other" else bad
        o1, lse1, _ = _run(q, kp, vp, sl, torch.tensor(b2, device="cuda"), causal=True, window=(left, 0), num_splits=0)
        assert torch.equal(o0, o1) and torch.equal(lse0, lse1), bad
    # (NaN != NaN: the pools are compared as bits)
    assert (_bits(kp) == _bits(kp0)).all() and (_bits(vp) == _bits(vp0)).all()
    assert (_bits(kp[:GUARD]) == _bits(kc[:GUARD])).all() and (_bits(kp[-GUARD:]) == _bits(kc[-GUARD:])).all()


@pytest.mark.parametrize("mag", [1e-9, 1e20])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_bf16_v_far_from_fp16_range(mag, num_splits):
    """the range rule's second sweep starts at the band: with Sq 4 and window (100, 0) at L 640 the band is keys 536 .. 639, step 4 alone of
    five (under 4 parts one part works and three are empty); the sequence of 77 keys sweeps its one step"""
    q, kc, vc, bt, _, _ = tp._paged(2, 4, 8, 2, 128, 32, 20, torch.bfloat16, seed=540)
    vc = (vc.float() * mag).to(torch.bfloat16)
    sl = tp._seqlens([640, 77])
    o, lse, kernel = _run(q, kc, vc, sl, bt, causal=True, window=(100, 0), num_splits=num_splits)
    assert kernel.startswith("fa_fwd16_paged_window<") and ("split" in kernel) == (num_splits > 1), kernel
    assert torch.isfinite(o).all()
    o_ref, lse_ref = pwr.forward(_np(q), _np(kc), _np(vc), sl.cpu().numpy(), bt.cpu().numpy(), None, None, True, (100, 0))[:2]
    live = np.isfinite(lse_ref)
    assert live.all()
    np.testing.assert_allclose(_np(lse), lse_ref, rtol=0, atol=2e-3)
    tol.check_forward(_np(o).reshape(1, 1, -1, 128), o_ref.reshape(1, 1, -1, 128), torch.bfloat16, kernel, tag="paged_window far V")


# ------------------------------------------------------------------------------------------------ routing, bit for bit
def test_a_window_that_bounds_nothing_is_the_unwindowed_call():
    um = _umfa()
    q, kc, vc, bt, _, _ = tp._paged(3, 4, 8, 2, 128, 16, 8, torch.bfloat16, seed=550)
    sl = tp._seqlens([5, 77, 128])
    cap, Sq = 16 * 8, 4
    for causal in (False, True):
        want = um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=causal, return_softmax_lse=True)
        torch.cuda.synchronize()
        plain = um.last_kernel()
        assert plain.startswith("fa_fwd16_paged<"), plain
        for w in ((-1, -1), (cap, Sq), (cap + 5, -1)) + (((-1, 0), (cap, 0), (-1, 3)) if causal else ()):
            got = um.kvcache_window_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=causal, window_size=w, return_softmax_lse=True)
            torch.cuda.synchronize()
            assert um.last_kernel() == plain, (w, um.last_kernel())
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), w
            # ... and the C entry normalises for itself: the same window handed to it unnormalised
            o2, l2 = um.ops.kvcache_attention_window_forward(q, kc, vc, sl, bt, scale=128 ** -0.5, causal=causal, window=w)
            torch.cuda.synchronize()
            assert um.last_kernel() == plain and torch.equal(o2, want[0]) and torch.equal(l2, want[1]), w
    for causal, w in ((False, (-1, 0)), (True, (cap - 1, 0)), (False, (-1, Sq - 1)), (False, (8, 0))):  # binding windows
        um.kvcache_window_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=causal, window_size=w)
        torch.cuda.synchronize()
        assert um.last_kernel().startswith("fa_fwd16_paged_window<"), (w, um.last_kernel())


def test_agrees_with_the_gather_route():
    """Sq 1: the window call equals kvcache_attention over a contiguous static cache holding only the last left + 1 keys.  The two
    outputs differ by no more than the format ceiling (tolerances.check_forward's: one fp16 ulp at 1 of the largest |O|)."""
    um = _umfa()
    B, H, Hkv, D, ps, left = 2, 16, 4, 128, 16, 255
    q, kc, vc, bt, _, _ = tp._paged(B, 1, H, Hkv, D, ps, 64, torch.float16, seed=560, share=False)
    lens = [1000, 333]
    sl = tp._seqlens(lens)
    o, _, kernel = _run(q, kc, vc, sl, bt, causal=True, window=(left, 0))
    assert kernel.startswith("fa_fwd16_paged_window<"), kernel
    kg, vg = (torch.stack([t[bt[b, :-(-L // ps)].long()].reshape(-1, Hkv, D)[L - left - 1:L] for b, L in enumerate(lens)]) for t in (kc, vc))
    od = um.kvcache_attention(q, kg.contiguous(), vg.contiguous(), cache_seqlens=left + 1, causal=True).float()
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("fa_fwd16_paged<")
    a, b = _np(o), _np(od)
    print(f"gather route: max |a - b| {np.abs(a - b).max():.3e}, ceiling {tol.ULP_AT_ONE['fp16'] * np.abs(b).max():.3e}")
    assert np.abs(a - b).max() <= tol.ULP_AT_ONE["fp16"] * np.abs(b).max(), np.abs(a - b).max()


def _launches(fn):
    """the number of kernels one call of fn launches, counted by torch's profiler (fn has run before: no first-call work is counted)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    print("launches:", names)
    return len(names)


@pytest.mark.parametrize("dt,D,rd,inter,causal,splits", [("bf16", 128, 128, False, True, 0), ("fp16", 64, 32, True, False, 2)])
def test_fused_rotary_is_the_call_on_rotated_operands(dt, D, rd, inter, causal, splits):
    um = _umfa()
    B, Sq, Sn, H, Hkv, ps, maxp = 3, 4, 4, 8, 2, 16, 8
    q, kc, vc, bt, kn, vn = tp._paged(B, Sq, H, Hkv, D, ps, maxp, DT[dt], seed=570, S_new=Sn, share=False)
    cos, sin = tables(ps * maxp + 8, rd, torch.float32, 571)
    lens = [14, 60, 100]
    sl = tp._seqlens(lens)
    window = (30, 0) if causal else (30, 1)
    kw = dict(cache_seqlens=sl, block_table=bt, causal=causal, window_size=window, num_splits=splits, return_softmax_lse=True)
    k1, v1 = kc.clone(), vc.clone()
    o1, l1 = um.kvcache_window_attention(q, k1, v1, kn, vn, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, **kw)
    torch.cuda.synchronize()
    name = um.last_kernel()
    assert name.startswith("fa_fwd16_paged_window<") and ("split" in name) == (splits > 1), name
    s = np.array(lens)
    rq = rotate_by_ops(um, q, rr.positions(s, Sq, ps * maxp, causal), cos, sin, inter)
    rk = rotate_by_ops(um, kn, rr.positions(s, Sn, ps * maxp, True), cos, sin, inter)
    k2, v2 = kc.clone(), vc.clone()
    o2, l2 = um.kvcache_window_attention(rq, k2, v2, rk, vn, **kw)
    torch.cuda.synchronize()
    assert um.last_kernel() == name
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(k1, kc)
    # as many launches with rotary as without: the pre-pass stands in for the append
    n_rot = _launches(lambda: um.kvcache_window_attention(q, k1, v1, kn, vn, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, **kw))
    n_plain = _launches(lambda: um.kvcache_window_attention(rq, k2, v2, rk, vn, **kw))
    assert n_rot == n_plain == (3 if splits > 1 else 2), (n_rot, n_plain)


def test_graph_replay_follows_lengths_and_table_across_a_step_boundary():
    """append + attention with window (16, 0) captured at length 140 (k_first = 124, step 0); the lengths advance to 150 between replays
    (k_first = 134, step 1) and the table is permuted: every replay equals the eager call, bit for bit"""
    um = _umfa()
    B, H, Hkv, D, ps = 2, 8, 2, 128, 16
    q, kc, vc, bt, kn, vn = tp._paged(B, 1, H, Hkv, D, ps, 16, torch.bfloat16, seed=580, S_new=1, share=False)
    sl = tp._seqlens([140, 60])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.kvcache_window_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, window_size=(16, 0),
                                           num_splits=2, return_softmax_lse=True)

    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: scratch grows outside the capture
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = step()
    perm = torch.tensor(np.random.default_rng(0).permutation(bt.cpu().numpy().ravel()).reshape(bt.shape), device="cuda")
    for it in range(3):  # lengths 140, 145, 150
        if it:
            sl.add_(5)
        if it == 2:
            bt.copy_(perm)
        kc0, vc0 = kc.clone(), vc.clone()
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in res]
        kr, vr = kc.clone(), vc.clone()
        kc.copy_(kc0)
        vc.copy_(vc0)
        want = step()
        torch.cuda.synchronize()
        assert um.last_kernel().startswith("fa_fwd16_paged_window<") and "split" in um.last_kernel()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), it
        assert torch.equal(kr, kc) and torch.equal(vr, vc), it
        o_ref, lse_ref = pwr.forward(_np(q), _np(kc0), _np(vc0), sl.cpu().numpy(), bt.cpu().numpy(), _np(kn), _np(vn), True, (16, 0))[:2]
        np.testing.assert_allclose(_np(got[1]), lse_ref, rtol=0, atol=2e-3)
        tol.check_forward(_np(got[0]).reshape(1, 1, -1, D), o_ref.reshape(1, 1, -1, D), torch.bfloat16, um.last_kernel(), tag="paged_window graph",
                          out_dt=torch.bfloat16)
    assert sl.cpu().tolist() == [150, 70]


# ------------------------------------------------------------------------------------------------ plumbing
def test_opcheck_custom_ops():
    _umfa()
    q, kc, vc, bt, kn, vn = tp._paged(2, 2, 8, 2, 64, 16, 4, torch.bfloat16, seed=590, S_new=2)
    cos, sin = tables(72, 32, torch.float32, 591)
    sl = tp._seqlens([5, 33])
    torch.library.opcheck(torch.ops.umfa.kvcache_window_forward.default, (q, kc, vc, sl, bt, True, 8, 0, 0.125, 0))
    torch.library.opcheck(torch.ops.umfa.kvcache_window_forward_append.default, (q, kc, vc, kn, vn, sl, bt, True, 8, 0, 0.125, 2))
    torch.library.opcheck(torch.ops.umfa.kvcache_window_rope_forward_append.default,
                          (q, kc, vc, kn, vn, sl, cos, sin, False, bt, False, 8, 1, 0.125, 0))


def test_compile_fullgraph_single_node():
    um = _umfa()
    q, kc, vc, bt, kn, vn = tp._paged(2, 1, 8, 2, 128, 16, 8, torch.float16, seed=600, S_new=1)
    sl = tp._seqlens([30, 64])
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.kvcache_window_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, window_size=(20, 0))

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.kvcache_window_forward_append"], calls
    assert torch.equal(oc, oe)
    assert torch.equal(kc, kc_e) and torch.equal(vc, vc_e)  # the compiled call appended in place too


def test_refusals_and_no_backward():
    um = _umfa()
    q, kc, vc, bt, _, _ = tp._paged(2, 1, 8, 2, 128, 16, 4, torch.bfloat16, seed=610)
    kw = dict(cache_seqlens=10, block_table=bt, window_size=(8, 0))
    f8 = torch.float8_e4m3fn
    with pytest.raises(ValueError):  # fp8 caches
        um.kvcache_window_attention(q, kc.to(f8), vc.to(f8), **kw)
    with pytest.raises(ValueError):  # descales
        um.kvcache_window_attention(q, kc, vc, k_descale=1.0, **kw)
    for w in ((-2, 0), (0, -2), (8,), 8, (1, 2, 3)):
        with pytest.raises(ValueError):
            um.kvcache_window_attention(q, kc, vc, cache_seqlens=10, block_table=bt, window_size=w)
    with pytest.raises(ValueError):  # head_dim 96
        um.kvcache_window_attention(q[..., :96].contiguous(), kc[..., :96].contiguous(), vc[..., :96].contiguous(), **kw)
    # the C entry: cache_fp8 set, a value below -1 -- invalid arguments, nothing launched
    sl = tp._seqlens([10, 10])
    for bad in (dict(cache_fp8=True), dict(window=(-2, 0))):
        with pytest.raises(um.ops.MFAError) as e:
            um.ops.kvcache_attention_window_forward(q, kc, vc, sl, bt, scale=0.1, **{"window": (8, 0), **bad})
        assert e.value.code == 1
    # a capacity of exactly 2^30 keys (2^26 pages of 16: a real, contiguous 256 MB table of zeros, of which only the first entries are
    # read) is refused by the public function and by the C entry; 2^30 - 16 is accepted and gives what a table of the used width gives
    wide = torch.zeros(1, 1 << 26, dtype=torch.int32, device="cuda")
    wide[0, :4] = bt[0]
    q1, sl1 = q[:1], tp._seqlens([50])
    with pytest.raises(ValueError, match="capacity"):
        um.kvcache_window_attention(q1, kc, vc, cache_seqlens=sl1, block_table=wide, window_size=(8, 0))
    with pytest.raises(um.ops.MFAError) as e:
        um.ops.kvcache_attention_window_forward(q1, kc, vc, sl1, wide, scale=0.1, window=(8, 0), num_splits=1)
    assert e.value.code == 1
    with pytest.raises(um.ops.MFAError) as e:  # ... whatever the window: the entry checks the capacity before it routes
        um.ops.kvcache_attention_window_forward(q1, kc, vc, sl1, wide, scale=0.1, window=(-1, -1), num_splits=1)
    assert e.value.code == 1
    got = um.ops.kvcache_attention_window_forward(q1, kc, vc, sl1, wide[:, :-1], scale=0.1, window=(8, 0), num_splits=1)
    want = um.ops.kvcache_attention_window_forward(q1, kc, vc, sl1, bt[:1], scale=0.1, window=(8, 0), num_splits=1)
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("fa_fwd16_paged_window<")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    del wide
    qg = q.clone().requires_grad_(True)
    o = um.kvcache_window_attention(qg, kc, vc, **kw)
    with pytest.raises(RuntimeError):  # inference only: no backward
        o.float().sum().backward()


def test_public_entry_output_dtype_and_lse():
    um = _umfa()
    for dt in ("bf16", "fp16"):
        q, kc, vc, bt, _, _ = tp._paged(2, 3, 8, 2, 128, 64, 4, DT[dt], seed=620)
        sl = tp._seqlens([100, 7])
        o = um.kvcache_window_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=True, window_size=(50, 0))
        o2, lse = um.kvcache_window_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=True, window_size=(50, 0), return_softmax_lse=True)
        torch.cuda.synchronize()
        assert o.dtype == DT[dt] and o.shape == q.shape and torch.equal(o, o2)
        assert lse.dtype == torch.float32 and lse.shape == (2, 8, 3)
        o_ref, lse_ref = pwr.forward(_np(q), _np(kc), _np(vc), sl.cpu().numpy(), bt.cpu().numpy(), None, None, True, (50, 0))[:2]
        assert np.isfinite(lse_ref).all()
        np.testing.assert_allclose(_np(lse), lse_ref, rtol=0, atol=1e-5)
        tol.check_forward(_np(o).reshape(1, 1, -1, 128), o_ref.reshape(1, 1, -1, 128), DT[dt], um.last_kernel(), tag="paged_window out",
                          out_dt=DT[dt])
