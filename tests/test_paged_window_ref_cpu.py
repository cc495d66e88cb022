"""tests/paged_window_ref.py without a GPU (sliding-window KV-cache attention).

1. A window that bounds nothing -- (-1, -1), or (-1, 0) with causal -- is paged_ref.forward, bit for bit.
2. On hole-free tables the band equals varlen_window_ref.forward on the gathered contiguous keys (an independent statement of the
   band), for forward_floor_ref.WINDOWS and L_k below, at and above Sq, to 1e-12; nkeys() agrees with the reference's live rows.
3. An fp64 emulation of the banded kernel (its step range, the parts dividing that range) stays inside forward_floor_ref.check_pool's
   bounds at the decode and 128-row shapes tests/test_gpu_paged_window.py runs; two planted defects do not: a lower bound one key too
   high, and parts that divide [0, nst) while each part's sweep starts at the band.
4. The C entry's window normalisation, restated in paged_window_ref.normalise, against a table of cases.
"""
import numpy as np
import pytest

import forward_floor_ref as ffr
import paged_ref
import paged_window_ref as pwr
import varlen_window_ref
from oracle import oracle as orc


def _rnd(rng, shape, dt):
    return orc.round_to(rng.standard_normal(shape), dt)


def _paged_case(dt, B, Sq, Hkv, g, D, ps, max_pages, seed, holes=False):
    rng = np.random.default_rng(seed)
    num_pages = B * max_pages + 3
    q = _rnd(rng, (B, Sq, Hkv * g, D), dt)
    kc, vc = _rnd(rng, (num_pages, ps, Hkv, D), dt), _rnd(rng, (num_pages, ps, Hkv, D), dt)
    bt = (rng.permutation(B * max_pages) + 1).reshape(B, max_pages).astype(np.int32)
    if holes:
        bt[:, 1] = num_pages
    return q, kc, vc, bt


# ------------------------------------------------------------------------------------------------ 1. nothing bound: paged_ref, bitwise
@pytest.mark.parametrize("causal,window", [(False, (-1, -1)), (True, (-1, -1)), (True, (-1, 0))])
@pytest.mark.parametrize("kind", [None, "fp16"])
def test_unbounded_window_is_paged_ref_bit_for_bit(causal, window, kind):
    q, kc, vc, bt = _paged_case("bf16", 3, 5, 2, 2, 64, 16, 4, seed=1, holes=True)
    rng = np.random.default_rng(2)
    kn, vn = _rnd(rng, (3, 2, 2, 64), "bf16"), _rnd(rng, (3, 2, 2, 64), "bf16")
    sl = np.array([3, 40, 63])  # L_k < Sq with the append; mid; the append runs past the capacity of 64
    got = pwr.forward(q, kc, vc, sl, bt, kn, vn, causal, window, kind=kind)
    want = paged_ref.forward(q, kc, vc, sl, bt, kn, vn, causal, kind=kind)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    nk = pwr.nkeys(5, sl, kc.shape, bt, 2, causal, window)
    assert np.array_equal(nk, ffr.paged_nkeys(5, sl, kc.shape, bt, 2, causal))


# ------------------------------------------------------------------------------------------------ 2. the band, stated independently
@pytest.mark.parametrize("window", ffr.WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
def test_band_equals_the_varlen_window_reference_on_gathered_keys(window, causal):
    B, Sq, Hkv, g, D, ps, max_pages = 4, 40, 2, 2, 64, 16, 10
    q, kc, vc, bt = _paged_case("fp16", B, Sq, Hkv, g, D, ps, max_pages, seed=3)
    sl = np.array([17, 40, 160, 0])  # L_k below Sq, equal to Sq, above Sq, and no key at all
    o, lse, _, _ = pwr.forward(q, kc, vc, sl, bt, None, None, causal, window)
    fl = pwr.forward(q, kc, vc, sl, bt, None, None, causal, window, kind="fp16")[0]
    ks, vs = zip(*[(K, V) for K, V, ok in paged_ref.gather(kc, vc, sl, 0, bt) if ok.all() or not len(ok)])
    assert len(ks) == B
    cu_q, cu_k = np.arange(B + 1) * Sq, np.concatenate([[0], np.cumsum(sl)])
    args = (q.reshape(B * Sq, Hkv * g, D), np.concatenate(ks), np.concatenate(vs), cu_q, cu_k, causal, window)
    ow, lw = varlen_window_ref.forward(*args)
    np.testing.assert_allclose(o.reshape(B * Sq, Hkv * g, D), ow, rtol=1e-12, atol=1e-12)
    lse_p = lse.transpose(1, 0, 2).reshape(Hkv * g, B * Sq)
    assert np.array_equal(np.isfinite(lse_p), np.isfinite(lw))
    np.testing.assert_allclose(lse_p[np.isfinite(lw)], lw[np.isfinite(lw)], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(fl.reshape(B * Sq, Hkv * g, D), varlen_window_ref.forward(*args, kind="fp16")[0], rtol=1e-12, atol=1e-12)
    nk = pwr.nkeys(Sq, sl, kc.shape, bt, 0, causal, window)
    assert np.array_equal(nk > 0, np.isfinite(lse[:, 0]))
    vis = [varlen_window_ref.visible(Sq, int(L), causal, window).sum(1) for L in sl]
    assert np.array_equal(nk, np.array(vis))


def test_holes_and_the_append_enter_the_band():
    """keys behind a table entry outside the pool are invisible inside the band too, and the appended rows are the band's newest keys"""
    q, kc, vc, bt = _paged_case("bf16", 2, 3, 2, 2, 64, 16, 4, seed=4, holes=True)
    rng = np.random.default_rng(5)
    kn, vn = _rnd(rng, (2, 3, 2, 64), "bf16"), _rnd(rng, (2, 3, 2, 64), "bf16")
    sl = np.array([30, 14])  # keys 16 .. 31 are behind the hole: sequence 0's band [28, 32] is all hole but its last key, 32
    o, lse, kc2, vc2 = pwr.forward(q, kc, vc, sl, bt, kn, vn, True, (2, 0))
    kw, vw = paged_ref.append(kc, vc, kn, vn, sl, bt)
    assert np.array_equal(kc2, kw) and np.array_equal(vc2, vw)
    nk = pwr.nkeys(3, sl, kc.shape, bt, 3, True, (2, 0))
    assert nk.tolist() == [[0, 0, 1], [3, 3, 2]]  # (sequence 1: keys 12 .. 16 with 16 behind the hole)
    assert np.array_equal(nk > 0, np.isfinite(lse[:, 0]))
    assert (o[0, :2] == 0).all()
    np.testing.assert_allclose(o[0, 2], vw[bt[0, 2], 0][np.arange(4) // 2], rtol=1e-12)  # one key: that key's V, the appended row


# ------------------------------------------------------------------------------------------------ 3. the emulation, and two defects
def _static_case(dt, B, Sq, Hkv, g, D, lens, seed):
    rng = np.random.default_rng(seed)
    Smax = max(max(lens), 1)
    return _rnd(rng, (B, Sq, Hkv * g, D), dt), _rnd(rng, (B, Smax, Hkv, D), dt), _rnd(rng, (B, Smax, Hkv, D), dt)


def _pool(q, kc, vc, lens, causal, window, got):
    B, Sq, H, D = q.shape
    want, lse = pwr.forward(q, kc, vc, lens, None, causal=causal, window=window)[:2]
    floor = pwr.forward(q, kc, vc, lens, None, causal=causal, window=window, kind=ffr.KIND)[0]
    nk = np.repeat(pwr.nkeys(Sq, lens, kc.shape, None, 0, causal, window)[:, :, None], H, axis=2)
    return (got.reshape(-1, D), want.reshape(-1, D), floor.reshape(-1, D), nk.reshape(-1)), np.isfinite(lse).transpose(0, 2, 1)


def _emulated(dt, D, B, Hkv, g, Sq, lens, causal, window, nsplit, tag, defect=None, seed=0):
    q, kc, vc = _static_case(dt, B, Sq, Hkv, g, D, lens, seed)
    got = pwr.emulate_window(q, kc, vc, lens, causal, window, nsplit, defect=defect)
    rows, live = _pool(q, kc, vc, lens, causal, window, got)
    one_key = tuple(window) == (0, 0)
    return ffr.check_pool(*rows, dt, "emulated", tag, ffr.form_regime(g * Sq, nsplit > 1), min_elems=0 if one_key else 4096, live=live)


# (Sq, window, causal, num_splits): tests/test_gpu_paged_window.py DECODE
DECODE = [(1, (0, 0), True, 1), (1, (1, 0), True, 1), (1, (15, 0), True, 1), (1, (16, 0), True, 1), (1, (127, 0), True, 3),
          (1, (128, 0), True, 1), (1, (300, 0), True, 3), (4, (17, 0), True, 1), (4, (130, 0), True, 3), (4, (5, 2), False, 1),
          (4, (-1, 1), False, 1), (4, (40, -1), False, 1)]
ROWS128_WINDOWS = [(31, 0), (128, 0), (100, 17), (-1, 40), (40, -1), (300, 0)]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("Sq,window,causal,nsplit", DECODE)
def test_emulated_decode_form_is_accepted(dt, Sq, window, causal, nsplit):
    _emulated(dt, 64, 8, 2, 8, Sq, ffr.DECODE_LENS, causal, window, nsplit, f"decode Sq{Sq} {window}")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("window", ROWS128_WINDOWS)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_emulated_128_row_form_is_accepted(dt, window, g, Sq):
    _emulated(dt, 64, 4, 2, g, Sq, ffr.rows128_lens(64), window[1] == 0, window, 1, f"128-row g{g} Sq{Sq} {window}")


@pytest.mark.parametrize("nsplit,L", ffr.ROWS128_SPLIT)
@pytest.mark.parametrize("window", [(64, 0), (500, 0)])
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_emulated_128_row_split_is_accepted(nsplit, L, window, g, Sq):
    _emulated("bf16", 64, 2, 2, g, Sq, [L, L - 37], True, window, nsplit, f"split{nsplit} L{L} g{g} Sq{Sq} {window}")


@pytest.mark.parametrize("case", ["decode", "rows128"])
def test_a_lower_bound_one_key_too_high_is_rejected(case):
    args = (8, 2, 8, 1, ffr.DECODE_LENS, True, (15, 0), 1) if case == "decode" else (4, 2, 1, 200, ffr.rows128_lens(64), True, (31, 0), 1)
    _emulated("fp16", 64, *args, case)
    with pytest.raises(AssertionError):
        _emulated("fp16", 64, *args, case, defect="lo_plus1")


def test_parts_dividing_the_context_instead_of_the_band_are_rejected():
    """The case: decode form, Sq 1, window (127, 0), 3 parts.  At L = 640 the band is keys 512 .. 639, one step, [4, 5); parts of
    ceil(5 / 3) = 2 steps that end at 2, 4 and 5 but start at 4, 6 and 8 visit nothing.  At L = 333 the band's steps are [1, 3): parts
    of one step ending at 1, 2, 3 and starting at 1, 2, 3 visit nothing either.  The rows come out as zeros."""
    args = (8, 2, 8, 1, ffr.DECODE_LENS, True, (127, 0), 3)
    _emulated("fp16", 64, *args, "parts")
    with pytest.raises(AssertionError):
        _emulated("fp16", 64, *args, "parts", defect="parts_from_zero")
    assert pwr.step_range(0, 0, 1, 640, (127, 0)) == (4, 5) and pwr.step_range(0, 0, 1, 333, (127, 0)) == (1, 3)


def test_step_range():
    assert pwr.step_range(0, 0, 1, 0, (5, 0)) == (0, 0)                 # no key
    assert pwr.step_range(0, 3, 4, 2, (-1, 0), True) == (0, 1)          # L_k < Sq: tokens 0, 1 see nothing, the workgroup keys 0 .. 1
    assert pwr.step_range(0, 1, 4, 2, (0, 0)) == (0, 0)                 # ... and a workgroup of tokens 0, 1 alone is empty
    assert pwr.step_range(0, 0, 1, 129, (0, 0)) == (1, 2)               # the last key alone
    assert pwr.step_range(0, 0, 1, 129, (1, 0)) == (0, 2)               # straddles the step boundary
    assert pwr.step_range(0, 127, 200, 640, (31, 0)) == (3, 5)          # rows of tokens 0 .. 127: keys 409 .. 567
    assert pwr.step_range(128, 199, 200, 640, (31, 0)) == (4, 5)
    assert pwr.step_range(0, 15, 16, 640, (-1, 40)) == (0, 5) and pwr.step_range(0, 15, 16, 640, (40, -1)) == (4, 5)


# ------------------------------------------------------------------------------------------------ 4. the normalisation
@pytest.mark.parametrize("window,causal,Sq,cap,want,plain", [
    ((-1, -1), False, 4, 640, (-1, -1), True),
    ((-1, -1), True, 4, 640, (-1, 0), True),
    ((-1, 0), True, 4, 640, (-1, 0), True),
    ((-1, 0), False, 4, 640, (-1, 0), False),     # not causal: the banded kernel (the rotary positions differ)
    ((639, -1), False, 4, 640, (639, -1), False),  # left = capacity - 1 stays
    ((640, -1), False, 4, 640, (-1, -1), True),    # left = capacity becomes open
    ((-1, 3), False, 4, 640, (-1, 3), False),      # right = Sq - 1 stays
    ((-1, 4), False, 4, 640, (-1, -1), True),      # right = Sq becomes open
    ((8, 5), True, 4, 640, (8, 0), False),         # causal with right = 5 gives 0
    ((640, 5), True, 4, 640, (-1, 0), True),
    ((640, 4), False, 4, 640, (-1, -1), True),
    ((0, 0), False, 1, 16, (0, 0), False),
    ((5, 0), False, 1, (1 << 30) - 16, (5, 0), False),
])
def test_window_normalisation(window, causal, Sq, cap, want, plain):
    assert pwr.normalise(window, causal, Sq, cap) == (want, plain)


@pytest.mark.parametrize("window,cap", [((-2, 0), 640), ((0, -2), 640), ((5,), 640), (7, 640), ((5, 0), 1 << 30), ((-1, -1), 1 << 30)])
def test_window_normalisation_refuses(window, cap):
    with pytest.raises(ValueError):
        pwr.normalise(window, False, 4, cap)
