"""The fp64 reference of packed queries over the KV cache (tests/varlen_paged_ref.py) pinned to the two references the project already
trusts (no GPU): with every L_q equal it is tests/paged_ref.py on the reshaped q; with an identity block table holding each sequence's
contiguous keys and no append it is tests/varlen_ref.py; and the contract's clamps and drop rules on hostile table entries, lengths and
cu values."""
import numpy as np
import pytest

import paged_ref
import varlen_paged_ref as ref
import varlen_ref


def _pool(rng, num_pages, ps, Hkv, D):
    return rng.standard_normal((num_pages, ps, Hkv, D)), rng.standard_normal((num_pages, ps, Hkv, D))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("static", [False, True])
@pytest.mark.parametrize("new", [False, True])
def test_equal_lengths_reproduce_paged_ref(causal, static, new):
    rng = np.random.default_rng(1)
    B, Sq, H, Hkv, D, ps, mp = 3, 5, 4, 2, 8, 16, 3
    q = rng.standard_normal((B, Sq, H, D))
    if static:
        kc, vc = _pool(rng, B, 40, Hkv, D)
        bt, sl = None, [0, 14, 37]  # the last one runs past S_max = 40 with the append
    else:
        kc, vc = _pool(rng, B * mp + 2, ps, Hkv, D)
        bt = (rng.permutation(B * mp) + 1).reshape(B, mp).astype(np.int32)
        sl = [0, 14, 46]  # page crossing; past the capacity of 48 with the append
    kn = rng.standard_normal((B, Sq, Hkv, D)) if new else None
    vn = rng.standard_normal((B, Sq, Hkv, D)) if new else None
    o0, l0, k0, v0 = paged_ref.forward(q, kc, vc, sl, bt, kn, vn, causal)
    cu = np.arange(B + 1) * Sq
    o1, l1, k1, v1 = ref.forward(q.reshape(B * Sq, H, D), kc, vc, cu, Sq, sl, bt, None if kn is None else kn.reshape(B * Sq, Hkv, D),
                                 None if vn is None else vn.reshape(B * Sq, Hkv, D), causal)
    np.testing.assert_allclose(o1.reshape(B, Sq, H, D), o0, rtol=0, atol=1e-12)
    a, b = l1.reshape(H, B, Sq).transpose(1, 0, 2), l0
    assert (np.isneginf(a) == np.isneginf(b)).all()
    np.testing.assert_allclose(a[np.isfinite(b)], b[np.isfinite(b)], rtol=0, atol=1e-12)
    assert np.abs(k1 - k0).max() <= 1e-12 and np.abs(v1 - v0).max() <= 1e-12
    if new:
        assert not (k1 == kc).all()


@pytest.mark.parametrize("causal", [False, True])
def test_identity_table_reproduces_varlen_ref(causal):
    rng = np.random.default_rng(2)
    H, Hkv, D, ps, mp = 4, 2, 8, 16, 4
    Lq, Lk = [3, 0, 7, 1, 20], [10, 5, 7, 64, 9]  # (L_q > L_k in the last one: causal rows without keys)
    B = len(Lq)
    cu_q, cu_k = np.concatenate([[0], np.cumsum(Lq)]), np.concatenate([[0], np.cumsum(Lk)])
    q = rng.standard_normal((cu_q[-1], H, D))
    k, v = rng.standard_normal((cu_k[-1], Hkv, D)), rng.standard_normal((cu_k[-1], Hkv, D))
    kc, vc = _pool(rng, B * mp, ps, Hkv, D)
    bt = np.arange(B * mp, dtype=np.int32).reshape(B, mp)  # identity: sequence b's pages are b mp .. b mp + mp - 1
    for b in range(B):
        kc.reshape(B, mp * ps, Hkv, D)[b, :Lk[b]] = k[cu_k[b]:cu_k[b + 1]]
        vc.reshape(B, mp * ps, Hkv, D)[b, :Lk[b]] = v[cu_k[b]:cu_k[b + 1]]
    o0, l0 = varlen_ref.forward(q, k, v, cu_q, cu_k, causal)
    o1, l1, k1, v1 = ref.forward(q, kc, vc, cu_q, max(Lq), Lk, bt, causal=causal)
    np.testing.assert_allclose(o1, o0, rtol=0, atol=1e-12)
    assert (np.isneginf(l1) == np.isneginf(l0)).all()
    np.testing.assert_allclose(l1[np.isfinite(l0)], l0[np.isfinite(l0)], rtol=0, atol=1e-12)
    assert (k1 == kc).all() and (v1 == vc).all()
    if causal:
        assert np.isneginf(l1[:, cu_q[4]:cu_q[4] + 11]).all() and (o1[cu_q[4]:cu_q[4] + 11] == 0).all()


def test_out_of_range_entries_and_lengths():
    rng = np.random.default_rng(3)
    H, Hkv, D, ps, mp, B = 2, 1, 4, 16, 2, 4
    num_pages = 8
    Lq = [3, 2, 4, 5]
    cu = np.concatenate([[0], np.cumsum(Lq)])
    q = rng.standard_normal((cu[-1], H, D))
    kn, vn = rng.standard_normal((cu[-1], Hkv, D)), rng.standard_normal((cu[-1], Hkv, D))
    kc, vc = _pool(rng, num_pages, ps, Hkv, D)
    bt = np.array([[-1, num_pages], [1, 2 ** 31 - 1], [-(2 ** 31), 3], [4, 5]], dtype=np.int64)
    sl = [5, 15, -7, 10 ** 9]
    o, lse, k1, v1 = ref.forward(q, kc, vc, cu, 5, sl, bt, kn, vn, causal=False)
    # sequence 0: no page the pool holds -- nothing appended, no key seen
    assert (o[0:3] == 0).all() and np.isneginf(lse[:, 0:3]).all()
    # sequence 1: L0 = 15: row 0 goes to page 1 slot 15, row 1 would go to the out-of-range page -> dropped; L_k = 17, 16 keys visible
    assert (k1[1, 15] == kn[3]).all() and np.isfinite(lse[:, 3:5]).all()
    # sequence 2: the negative length is 0; positions 0 .. 3 lie in the out-of-range page -> dropped, no key seen
    assert np.isneginf(lse[:, 5:9]).all()
    # sequence 3: the huge length is the capacity: every append row is past it -> dropped; L_k = 32
    assert (k1[4] == kc[4]).all() and (k1[5] == kc[5]).all() and np.isfinite(lse[:, 9:14]).all()
    changed = np.argwhere((k1 != kc).any(axis=(2, 3)))
    assert changed.tolist() == [[1, 15]]


def test_zero_length_capped_and_hostile_cu():
    rng = np.random.default_rng(4)
    H, Hkv, D, ps, mp = 2, 1, 4, 16, 2
    Tq = 12
    q = rng.standard_normal((Tq, H, D))
    kc, vc = _pool(rng, 6, ps, Hkv, D)
    bt = np.arange(6, dtype=np.int32).reshape(3, mp)
    # L_q = 0 in the middle; the last sequence covers 4 .. 9 only: rows 10, 11 belong to nobody
    cu = [0, 4, 4, 10]
    o, lse, _, _ = ref.forward(q, kc, vc, cu, 6, [10, 10, 10], bt, causal=True)
    assert ref.ranges(cu, Tq, 6) == [(0, 4), (4, 0), (4, 6)]
    assert ref.covered(cu, Tq, 6).tolist() == [True] * 10 + [False] * 2
    assert np.isfinite(lse[:, :10]).all() and np.isneginf(lse[:, 10:]).all() and (o[10:] == 0).all()
    # L_q is capped at max_seqlen_q: the rows past it are not covered
    assert ref.ranges(cu, Tq, 3) == [(0, 3), (4, 0), (4, 3)]
    assert ref.covered(cu, Tq, 3).tolist() == [True] * 3 + [False] + [True] * 3 + [False] * 5
    # values beyond T_q and below zero are clamped into [0, T_q]; a decreasing pair is an empty sequence
    assert ref.ranges([-5, 3, 100, 7], Tq, 12) == [(0, 3), (3, 9), (12, 0)]
    o2, lse2, _, _ = ref.forward(q, kc, vc, [-5, 3, 100, 7], 12, [10, 10, 10], bt)
    assert np.isfinite(o2).all() and np.isfinite(lse2).all()
    # bottom-right causal per sequence with an append: query i sees L0 + i + 1 keys
    kn, vn = rng.standard_normal((Tq, Hkv, D)), rng.standard_normal((Tq, Hkv, D))
    o3, lse3, k3, _ = ref.forward(q, kc, vc, cu, 6, [10, 10, 10], bt, kn, vn, causal=True)
    K = np.concatenate([kc[4], kc[5]])[:10, 0]
    K = np.concatenate([K, kn[4:10, 0]])
    s = q[4, 0] @ K[:11].T * D ** -0.5
    assert abs(lse3[0, 4] - (np.log(np.exp(s - s.max()).sum()) + s.max())) < 1e-12
    assert (k3[4, 10:16, 0] == kn[4:10, 0]).all()
