"""The fp64 KV-cache reference (tests/paged_ref.py) pinned on the CPU: against torch's SDPA with causal_lower_right over the gathered
sequences, against the varlen reference on the same data, and its append / clamp / invalid-page semantics."""
import numpy as np
import pytest
import torch
from torch.nn.attention.bias import causal_lower_right

import paged_ref as ref
import varlen_ref


def _case(rng, B=3, Sq=4, H=4, Hkv=2, D=16, ps=16, num_pages=12, max_pages=4, S_new=0):
    q = rng.standard_normal((B, Sq, H, D))
    kc = rng.standard_normal((num_pages, ps, Hkv, D))
    vc = rng.standard_normal((num_pages, ps, Hkv, D))
    bt = rng.permutation(num_pages)[:B * max_pages].reshape(B, max_pages).astype(np.int32)
    kn = rng.standard_normal((B, S_new, Hkv, D)) if S_new else None
    vn = rng.standard_normal((B, S_new, Hkv, D)) if S_new else None
    return q, kc, vc, bt, kn, vn


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S_new", [0, 3])
def test_against_torch_sdpa_lower_right(causal, S_new):
    rng = np.random.default_rng(1)
    q, kc, vc, bt, kn, vn = _case(rng, S_new=S_new)
    seqlens = np.array([5, 40, 17], np.int32)
    o, lse, kc2, vc2 = ref.forward(q, kc, vc, seqlens, bt, kn, vn, causal=causal, scale=0.3)
    G = q.shape[2] // kc.shape[2]
    for b, (K, V, ok) in enumerate(ref.gather(kc2, vc2, seqlens, S_new, bt)):
        assert ok.all()
        qt = torch.tensor(q[b]).transpose(0, 1)[None]
        kt = torch.tensor(K).transpose(0, 1).repeat_interleave(G, 0)[None]
        vt = torch.tensor(V).transpose(0, 1).repeat_interleave(G, 0)[None]
        mask = causal_lower_right(q.shape[1], K.shape[0]) if causal else None
        want = torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, attn_mask=mask, scale=0.3)[0].transpose(0, 1).numpy()
        np.testing.assert_allclose(o[b], want, rtol=1e-10, atol=1e-10)
        s = np.einsum("qhd,khd->hqk", q[b], np.repeat(K, G, 1)) * 0.3
        if causal:
            s = np.where(np.arange(K.shape[0])[None, None] <= np.arange(q.shape[1])[None, :, None] + K.shape[0] - q.shape[1], s, -np.inf)
        np.testing.assert_allclose(lse[b], np.log(np.exp(s).sum(-1)), rtol=1e-10)


@pytest.mark.parametrize("causal", [False, True])
def test_against_varlen_reference(causal):
    rng = np.random.default_rng(2)
    q, kc, vc, bt, _, _ = _case(rng, Sq=5)
    seqlens = np.array([3, 64, 29], np.int32)
    o, lse, _, _ = ref.forward(q, kc, vc, seqlens, bt, causal=causal)
    g = ref.gather(kc, vc, seqlens, 0, bt)
    kp = np.concatenate([K for K, _, _ in g])
    vp = np.concatenate([V for _, V, _ in g])
    cu_k = np.concatenate([[0], np.cumsum([len(ok) for _, _, ok in g])])
    cu_q = np.arange(0, 3 * 5 + 1, 5)
    ov, lv = varlen_ref.forward(q.reshape(15, 4, 16), kp, vp, cu_q, cu_k, causal)
    np.testing.assert_allclose(o.reshape(15, 4, 16), ov, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lse.transpose(1, 0, 2).reshape(4, 15), lv, rtol=1e-12)


def test_static_cache_is_one_page_per_sequence():
    rng = np.random.default_rng(3)
    q = rng.standard_normal((2, 3, 4, 16))
    kc = rng.standard_normal((2, 50, 4, 16))
    vc = rng.standard_normal((2, 50, 4, 16))
    seqlens = np.array([7, 50], np.int32)
    o, _, _, _ = ref.forward(q, kc, vc, seqlens, None)
    for b, L in enumerate(seqlens):
        s = np.einsum("qhd,khd->hqk", q[b], kc[b, :L]) / 4.0
        p = np.exp(s - s.max(-1, keepdims=True))
        want = np.einsum("hqk,khd->qhd", p / p.sum(-1, keepdims=True), vc[b, :L])
        np.testing.assert_allclose(o[b], want, rtol=1e-12, atol=1e-12)


def test_append_writes_through_the_table_and_clamps():
    rng = np.random.default_rng(4)
    q, kc, vc, bt, kn, vn = _case(rng, S_new=5, max_pages=2, num_pages=8)  # capacity 32
    bt[1, 1] = 99  # an entry outside the pool: its rows are dropped and its keys masked
    seqlens = np.array([14, 12, 30], np.int32)
    kc2, vc2 = ref.append(kc, vc, kn, vn, seqlens, bt)
    # sequence 0: positions 14 .. 18 cross from logical page 0 into page 1
    for i in range(5):
        pos = 14 + i
        assert (kc2[bt[0, pos // 16], pos % 16] == kn[0, i]).all() and (vc2[bt[0, pos // 16], pos % 16] == vn[0, i]).all()
    # sequence 1: positions 12 .. 15 land, 16 belongs to the invalid page and is dropped
    for i in range(4):
        assert (kc2[bt[1, 0], 12 + i] == kn[1, i]).all()
    # sequence 2: positions 30, 31 land, 32 .. 34 are past the capacity
    assert (kc2[bt[2, 1], 14] == kn[2, 0]).all() and (kc2[bt[2, 1], 15] == kn[2, 1]).all()
    touched = {(bt[0, 0], r) for r in (14, 15)} | {(bt[0, 1], r) for r in (0, 1, 2)} | {(bt[1, 0], r) for r in range(12, 16)} | \
              {(bt[2, 1], 14), (bt[2, 1], 15)}
    for pg in range(kc.shape[0]):
        for r in range(16):
            same = (kc2[pg, r] == kc[pg, r]).all() and (vc2[pg, r] == vc[pg, r]).all()
            assert same != ((pg, r) in touched), (pg, r)
    _, Lk = zip(*ref.lengths(seqlens, 5, 32))
    assert Lk == (19, 17, 32)
    g = ref.gather(kc2, vc2, seqlens, 5, bt)
    assert g[1][2].tolist() == [True] * 16 + [False]


def test_invalid_entries_and_lengths_are_masked():
    rng = np.random.default_rng(5)
    q, kc, vc, bt, _, _ = _case(rng, B=4, Sq=2, max_pages=2, num_pages=8)
    bt[0, :] = -1  # no valid page: every row sees no key
    bt[1, 1] = 8   # == num_pages: outside
    seqlens = np.array([20, 30, -5, 1000], np.int32)  # negative -> 0, past the capacity -> 32
    o, lse, _, _ = ref.forward(q, kc, vc, seqlens, bt, causal=False)
    assert (o[0] == 0).all() and np.isneginf(lse[0]).all()
    assert (o[2] == 0).all() and np.isneginf(lse[2]).all()
    # sequence 1 sees exactly its first page
    o1, l1, _, _ = ref.forward(q[1:2], kc, vc, np.array([16], np.int32), bt[1:2])
    np.testing.assert_allclose(o[1], o1[0], rtol=1e-12)
    np.testing.assert_allclose(lse[1], l1[0], rtol=1e-12)
    # sequence 3 is clamped to the capacity of 32 keys
    o3, _, _, _ = ref.forward(q[3:4], kc, vc, np.array([32], np.int32), bt[3:4])
    np.testing.assert_allclose(o[3], o3[0], rtol=1e-12)


def test_causal_rows_without_keys():
    rng = np.random.default_rng(6)
    q, kc, vc, bt, _, _ = _case(rng, B=1, Sq=6)
    o, lse, _, _ = ref.forward(q, kc, vc, np.array([3], np.int32), bt[:1], causal=True)
    # L_k = 3 < Sq = 6: queries 0 .. 2 see no key
    assert (o[0, :3] == 0).all() and np.isneginf(lse[0, :, :3]).all()
    assert np.isfinite(lse[0, :, 3:]).all()
