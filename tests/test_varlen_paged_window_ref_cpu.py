"""tests/varlen_paged_window_ref.py without a GPU (sliding-window attention for packed queries over the KV cache).

1. A window that bounds nothing -- (-1, -1), or (-1, 0) with causal -- is varlen_paged_ref.forward, bit for bit.
2. With every L_q equal it is paged_window_ref.forward to 1e-12; on hole-free identity tables it is varlen_window_ref.forward on the
   gathered contiguous keys to 1e-12; nkeys() agrees with the reference's live rows.
3. An fp64 emulation of the kernel (per-item step range, the parts dividing that range) stays inside forward_floor_ref.check_pool's
   bounds at the mixed batch tests/test_gpu_varlen_paged_window.py runs; two planted defects do not: parts that divide [0, nst) while each
   part's sweep starts at the band, and the band taken from the item's first row alone.
4. step_range's arithmetic stays in int32 at the extremes; the C entry's normalisation, restated in normalise, against a table of cases.
"""
import numpy as np
import pytest

import forward_floor_ref as ffr
import paged_ref
import paged_window_ref as pwr
import varlen_paged_ref as vpr
import varlen_paged_window_ref as vwr
import varlen_window_ref
from oracle import oracle as orc

MIXED_WINDOWS = ffr.WINDOWS + [(128, 0), (300, 0)]  # tests/test_gpu_varlen_paged_window.py's


def _rnd(rng, shape, dt):
    return orc.round_to(rng.standard_normal(shape), dt)


def _cu(lq):
    return np.concatenate([[0], np.cumsum(lq)]).astype(np.int64)


def _paged_case(dt, lq, Hkv, g, D, ps, max_pages, seed, holes=False, identity=False):
    rng = np.random.default_rng(seed)
    B, Tq = len(lq), int(sum(lq))
    num_pages = B * max_pages + 3
    q = _rnd(rng, (Tq, Hkv * g, D), dt)
    kc, vc = _rnd(rng, (num_pages, ps, Hkv, D), dt), _rnd(rng, (num_pages, ps, Hkv, D), dt)
    bt = (np.arange(B * max_pages) if identity else rng.permutation(B * max_pages) + 1).reshape(B, max_pages).astype(np.int32)
    if holes:
        bt[:, 1] = num_pages
    return q, kc, vc, bt


# ------------------------------------------------------------------------------------------------ 1. nothing bound: varlen_paged_ref, bitwise
@pytest.mark.parametrize("causal,window", [(False, (-1, -1)), (True, (-1, -1)), (True, (-1, 0))])
@pytest.mark.parametrize("kind", [None, "fp16"])
def test_unbounded_window_is_varlen_paged_ref_bit_for_bit(causal, window, kind):
    lq = [5, 0, 1, 9]
    q, kc, vc, bt = _paged_case("bf16", lq, 2, 2, 64, 16, 4, seed=1, holes=True)
    rng = np.random.default_rng(2)
    kn, vn = _rnd(rng, (sum(lq), 2, 64), "bf16"), _rnd(rng, (sum(lq), 2, 64), "bf16")
    sl = np.array([3, 40, 63, 60])  # L_k < L_q with the append; no rows; one row; the append runs past the capacity of 64
    got = vwr.forward(q, kc, vc, _cu(lq), 9, sl, bt, kn, vn, causal, window, kind=kind)
    want = vpr.forward(q, kc, vc, _cu(lq), 9, sl, bt, kn, vn, causal, kind=kind)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. the band, stated independently
@pytest.mark.parametrize("window", ffr.WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
def test_equal_lengths_are_the_dense_window_reference(window, causal):
    B, Sq, Hkv, g, D, ps, max_pages = 4, 7, 2, 2, 64, 16, 10
    q, kc, vc, bt = _paged_case("fp16", [Sq] * B, Hkv, g, D, ps, max_pages, seed=3, holes=True)
    rng = np.random.default_rng(4)
    kn, vn = _rnd(rng, (B * Sq, Hkv, D), "fp16"), _rnd(rng, (B * Sq, Hkv, D), "fp16")
    sl = np.array([3, 40, 150, 0])
    for new in (False, True):
        a = (kn, vn) if new else (None, None)
        r = lambda t: None if t is None else t.reshape(B, Sq, *t.shape[1:])  # noqa: E731
        for kind in (None, "fp16"):
            o, lse, k2, v2 = vwr.forward(q, kc, vc, _cu([Sq] * B), Sq, sl, bt, *a, causal, window, kind=kind)
            od, ld, kd, vd = pwr.forward(r(q), kc, vc, sl, bt, r(a[0]), r(a[1]), causal, window, kind=kind)
            np.testing.assert_allclose(o.reshape(B, Sq, Hkv * g, D), od, rtol=1e-12, atol=1e-12)
            lp = lse.reshape(Hkv * g, B, Sq).transpose(1, 0, 2)
            assert np.array_equal(np.isfinite(lp), np.isfinite(ld))
            np.testing.assert_allclose(lp[np.isfinite(ld)], ld[np.isfinite(ld)], rtol=1e-12, atol=1e-12)
            assert np.array_equal(k2, kd) and np.array_equal(v2, vd)
        nk = vwr.nkeys(B * Sq, _cu([Sq] * B), Sq, sl, kc.shape, bt, new, causal, window)
        assert np.array_equal(nk.reshape(B, Sq), pwr.nkeys(Sq, sl, kc.shape, bt, Sq if new else 0, causal, window))
        assert np.array_equal(nk > 0, np.isfinite(lse[0]))


@pytest.mark.parametrize("window", ffr.WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
def test_band_equals_the_varlen_window_reference_on_gathered_keys(window, causal):
    lq, sl = [1, 40, 0, 17, 33], np.array([17, 40, 9, 160, 0])  # L_k above, equal to, (no rows), above L_q, and no key at all
    Hkv, g, D, ps, max_pages = 2, 2, 64, 16, 10
    q, kc, vc, bt = _paged_case("fp16", lq, Hkv, g, D, ps, max_pages, seed=5, identity=True)
    o, lse, _, _ = vwr.forward(q, kc, vc, _cu(lq), 40, sl, bt, None, None, causal, window)
    fl = vwr.forward(q, kc, vc, _cu(lq), 40, sl, bt, None, None, causal, window, kind="fp16")[0]
    ks, vs = zip(*[(K, V) for K, V, ok in paged_ref.gather(kc, vc, sl, 0, bt)])
    args = (q, np.concatenate(ks), np.concatenate(vs), _cu(lq), _cu(sl), causal, window)
    ow, lw = varlen_window_ref.forward(*args)
    np.testing.assert_allclose(o, ow, rtol=1e-12, atol=1e-12)
    assert np.array_equal(np.isfinite(lse), np.isfinite(lw))
    np.testing.assert_allclose(lse[np.isfinite(lw)], lw[np.isfinite(lw)], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(fl, varlen_window_ref.forward(*args, kind="fp16")[0], rtol=1e-12, atol=1e-12)
    nk = vwr.nkeys(sum(lq), _cu(lq), 40, sl, kc.shape, bt, False, causal, window)
    assert np.array_equal(nk > 0, np.isfinite(lse[0]))
    vis = np.concatenate([varlen_window_ref.visible(l, int(L), causal, window).sum(1) for l, L in zip(lq, sl)])
    assert np.array_equal(nk, vis)


def test_clamps_holes_and_uncovered_rows():
    """max_seqlen_q caps a sequence (its tail belongs to nobody), a hole inside the band is invisible, the append enters the band"""
    lq = [3, 10, 2]
    q, kc, vc, bt = _paged_case("bf16", lq, 2, 2, 64, 16, 4, seed=6, holes=True)
    rng = np.random.default_rng(7)
    kn, vn = _rnd(rng, (15, 2, 64), "bf16"), _rnd(rng, (15, 2, 64), "bf16")
    sl = np.array([30, 14, 5])  # sequence 0: keys 16 .. 31 behind the hole, its band [28 + i, 30 + i] is hole but for key 32
    o, lse, kc2, vc2 = vwr.forward(q, kc, vc, _cu(lq), 4, sl, bt, kn, vn, True, (2, 0))
    kw, vw = vpr.append(kc, vc, kn, vn, _cu(lq), 4, sl, bt)
    assert np.array_equal(kc2, kw) and np.array_equal(vc2, vw)
    nk = vwr.nkeys(15, _cu(lq), 4, sl, kc.shape, bt, True, True, (2, 0))
    assert nk.tolist() == [0, 0, 1] + [3, 3, 2, 1] + [0] * 6 + [3, 3]  # (sequence 1: L_q 4, keys 12 .. 17 with 16, 17 behind the hole)
    assert np.array_equal(nk > 0, np.isfinite(lse[0]))
    assert (o[7:13] == 0).all() and np.isneginf(lse[:, 7:13]).all()
    assert np.array_equal(vpr.covered(_cu(lq), 15, 4), np.array([1] * 3 + [1] * 4 + [0] * 6 + [1] * 2, bool))


# ------------------------------------------------------------------------------------------------ 3. the emulation, and two defects
def _static_case(dt, lq, Hkv, g, D, lens, seed):
    rng = np.random.default_rng(seed)
    Smax = max(max(lens), 1)
    return _rnd(rng, (sum(lq), Hkv * g, D), dt), _rnd(rng, (len(lq), Smax, Hkv, D), dt), _rnd(rng, (len(lq), Smax, Hkv, D), dt)


def _emulated(dt, D, Hkv, g, lq, lens, causal, window, nsplit, tag, defect=None, seed=0):
    q, kc, vc = _static_case(dt, lq, Hkv, g, D, lens, seed)
    cu, mq, H = _cu(lq), max(lq), Hkv * g
    got = vwr.emulate(q, kc, vc, cu, mq, lens, causal, window, nsplit, defect=defect)
    want, lse = vwr.forward(q, kc, vc, cu, mq, lens, None, causal=causal, window=window)[:2]
    floor = vwr.forward(q, kc, vc, cu, mq, lens, None, causal=causal, window=window, kind=ffr.KIND)[0]
    nk = np.repeat(vwr.nkeys(sum(lq), cu, mq, lens, kc.shape, None, False, causal, window), H)
    decode = any(0 < g * l <= 32 for l in lq)
    return ffr.check_pool(got.reshape(-1, D), want.reshape(-1, D), floor.reshape(-1, D), nk, dt, "emulated", tag,
                          ffr.form_regime(32 if decode else 128, nsplit > 1), min_elems=0 if tuple(window) == (0, 0) else 4096,
                          live=np.isfinite(lse).T)


@pytest.mark.parametrize("new", [False, True])
@pytest.mark.parametrize("g,nsplit", [(1, 1), (8, 3)])
@pytest.mark.parametrize("window", MIXED_WINDOWS)
def test_emulated_mixed_batch_is_accepted(window, g, nsplit, new):
    """the GPU test's lengths (new tokens emulated as already appended: the lengths count them)"""
    lens = [L + (l if new else 0) for l, L in zip(ffr.PACKED_LQ, ffr.PACKED_CACHE)]
    _emulated("bf16" if g == 1 else "fp16", 64, 2, g, ffr.PACKED_LQ, lens, window[1] == 0, window, nsplit, f"mixed g{g} {window} new{new}")


def test_the_mixed_batch_pools_what_the_issue_counted():
    """H 2: every window but (0, 0) leaves 400 .. 402 of the 402 rows with two keys or more, at most 2 with one"""
    lq = ffr.PACKED_LQ
    for new in (False, True):
        lens = [L + (l if new else 0) for l, L in zip(lq, ffr.PACKED_CACHE)]
        for window in MIXED_WINDOWS:
            nk = vwr.nkeys(sum(lq), _cu(lq), max(lq), lens, (len(lq), max(lens), 2, 64), None, False, window[1] == 0, window)
            if tuple(window) == (0, 0):
                assert (nk == 1).all()
            else:
                assert (nk >= 2).sum() >= 400 and (nk == 1).sum() <= 2 and (nk == 0).sum() == 0, (window, new)


def test_parts_dividing_the_context_instead_of_the_band_are_rejected():
    """window (127, 0), 3 parts: at L_k 640 a decode item's band is one step, [4, 5); parts of ceil(5 / 3) = 2 steps that end at 2, 4 and
    5 but start at 4, 6 and 8 visit nothing, and the rows come out as zeros"""
    args = (2, 8, ffr.PACKED_LQ, ffr.PACKED_CACHE, True, (127, 0), 3)
    _emulated("fp16", 64, *args, "parts")
    with pytest.raises(AssertionError):
        _emulated("fp16", 64, *args, "parts", defect="parts_from_zero")
    assert vwr.step_range(0, 0, 1, 640, (127, 0)) == (4, 5)


def test_a_band_taken_from_the_first_row_alone_is_rejected():
    """g 1, window (31, 0): the 128-row item of tokens 0 .. 127 of the sequence with L_q 200 over 450 keys needs keys 219 .. 377, steps
    [1, 3); from its first row alone it is keys 219 .. 250, step [1, 2), and the rows past token 5 lose keys"""
    args = (2, 1, ffr.PACKED_LQ, ffr.PACKED_CACHE, True, (31, 0), 1)
    _emulated("fp16", 64, *args, "first row")
    with pytest.raises(AssertionError):
        _emulated("fp16", 64, *args, "first row", defect="band_from_first_row")
    assert vwr.step_range(0, 127, 200, 450, (31, 0)) == (1, 3) and vwr.step_range(0, 0, 200, 450, (31, 0)) == (1, 2)


# ------------------------------------------------------------------------------------------------ 4. step range and normalisation
def test_step_range():
    assert vwr.step_range(0, 0, 1, 0, (5, 0)) == (0, 0)                 # no key
    assert vwr.step_range(0, 3, 4, 2, (-1, 0), True) == (0, 1)          # L_k < L_q: tokens 0, 1 see nothing, the item keys 0 .. 1
    assert vwr.step_range(0, 1, 4, 2, (0, 0)) == (0, 0)                 # ... and an item of tokens 0, 1 alone is empty
    assert vwr.step_range(0, 0, 1, 129, (1, 0)) == (0, 2)               # straddles the step boundary
    assert vwr.step_range(128, 199, 200, 640, (31, 0)) == (4, 5)
    for a in ((0, 127, 200, 640, (31, 0)), (0, 15, 16, 640, (-1, 40)), (0, 15, 16, 640, (40, -1)), (0, 3, 4, 2, (-1, 0), True)):
        assert vwr.step_range(*a) == pwr.step_range(*a)


def test_step_range_stays_in_int32_at_the_extremes():
    """L_q, the capacity and the bounds just below 2^30, and open sides: step_range asserts every intermediate the kernel forms"""
    big = (1 << 30) - 1
    for Lq, Lk in ((1, big), (big, big), (big, 0), (big, 1), (1, 0), (big, big - 5)):
        for window in ((big - 1, big - 1), (-1, -1), (-1, 0), (0, -1), (0, 0), (big - 1, -1), (-1, big - 1)):
            for first, last in ((0, 0), (0, min(127, Lq - 1)), (Lq - 1, Lq - 1), (max(0, Lq - 128), Lq - 1)):
                lo, hi = vwr.step_range(first, last, Lq, Lk, window)
                assert 0 <= lo <= hi <= (Lk + 127) // 128
    assert vwr.step_range(big - 1, big - 1, big, big, (-1, -1)) == (0, (big + 127) // 128)
    assert vwr.step_range(0, 0, big, 1, (-1, -1)) == (0, 1)  # both sides open: the one key
    assert vwr.step_range(0, 0, big, 1, (-1, 0)) == (0, 0)   # off = 1 - L_q: token 0 sees keys <= off < 0, none
    assert vwr.step_range(big - 1, big - 1, big, 1, (-1, 0)) == (0, 1)
    with pytest.raises(AssertionError):  # (the assertion is live: a length of 2^30 with an open right side leaves int32)
        vwr.step_range(0, 1 << 30, (1 << 30) + 1, 1 << 31, (0, -1))


@pytest.mark.parametrize("window,causal,max_q,cap,want,plain", [
    ((-1, -1), False, 4, 640, (-1, -1), True),
    ((-1, -1), True, 4, 640, (-1, 0), True),
    ((-1, 0), False, 4, 640, (-1, 0), False),
    ((639, -1), False, 4, 640, (639, -1), False),
    ((640, -1), False, 4, 640, (-1, -1), True),
    ((-1, 3), False, 4, 640, (-1, 3), False),
    ((-1, 4), False, 4, 640, (-1, -1), True),      # right = max_seqlen_q becomes open
    ((8, 5), True, 4, 640, (8, 0), False),
    ((640, 5), True, 4, 640, (-1, 0), True),
    ((5, 0), False, (1 << 30) - 1, (1 << 30) - 16, (5, 0), False),
])
def test_window_normalisation(window, causal, max_q, cap, want, plain):
    assert vwr.normalise(window, causal, max_q, cap) == (want, plain)


@pytest.mark.parametrize("window,max_q,cap", [((-2, 0), 4, 640), ((0, -2), 4, 640), ((5,), 4, 640), (7, 4, 640), ((5, 0), 4, 1 << 30),
                                              ((5, 0), 1 << 30, 640), ((-1, -1), 1 << 30, 640)])
def test_window_normalisation_refuses(window, max_q, cap):
    with pytest.raises(ValueError):
        vwr.normalise(window, False, max_q, cap)


def test_item_counts():
    assert vwr.items(ffr.PACKED_LQ, 1, 2) == (2 * 4, 2 * (2 + 2 + 1))  # decode: L_q 1, 1, 5, 32; 128-row: 130, 200 (two blocks each), 33
    assert vwr.items(ffr.PACKED_LQ, 8, 2) == (2 * 2, 2 * (1 + 9 + 13 + 2 + 3))
