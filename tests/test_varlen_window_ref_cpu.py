"""The fp64 sliding-window varlen reference (tests/varlen_window_ref.py) against torch's own definitions, on the CPU: every sequence
through torch SDPA with an explicit bool mask built from flash-attention's window_size rule (bottom-right per sequence), at L_q < L_k,
L_q == L_k and L_q > L_k; the dense top-left rule when the lengths match; causal with (left, -1) equal to (left, 0)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import varlen_window_ref as ref

LENS_Q = [1, 31, 0, 128, 129, 50, 7, 64, 40]
LENS_K = [1, 40, 5, 100, 129, 0, 7, 200, 40]  # L_q > L_k, L_q < L_k, L_q == L_k, empty either side
WINDOWS = [(0, 0), (1, 0), (31, 0), (32, 0), (100, 17), (-1, 40), (40, -1), (127, 128), (-1, -1), (3, 5)]


def _case(lens_q, lens_k, H, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int64)
    cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int64)
    q = torch.randn(int(cu_q[-1]), H, D, generator=g, dtype=torch.float64)
    k = torch.randn(int(cu_k[-1]), Hkv, D, generator=g, dtype=torch.float64)
    v = torch.randn(int(cu_k[-1]), Hkv, D, generator=g, dtype=torch.float64)
    return q, k, v, cu_q, cu_k


def _formula_mask(Lq, Lk, causal, window):
    """flash-attention's rule written out element by element"""
    left, right = window
    if causal:
        right = 0
    off = Lk - Lq
    m = torch.zeros(Lq, Lk, dtype=torch.bool)
    for i in range(Lq):
        for j in range(Lk):
            m[i, j] = (left < 0 or j >= i + off - left) and (right < 0 or j <= i + off + right)
    return m


def _torch_seq(q, k, v, mask, scale, G):
    qh, kh, vh = (t.transpose(0, 1)[None] for t in (q, k, v))
    kh, vh = kh.repeat_interleave(G, 1), vh.repeat_interleave(G, 1)
    return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=scale)[0].transpose(0, 1)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
def test_forward_matches_torch_with_formula_mask(window, causal):
    H, Hkv = 4, 2
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, H, Hkv, 16, seed=7 + causal)
    scale = 0.3
    o, lse = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, causal, window, scale)
    for q0, Lq, k0, Lk in ref.seqs(cu_q, cu_k):
        if Lq == 0:
            continue
        rows = slice(q0, q0 + Lq)
        mask = _formula_mask(Lq, Lk, causal, window)
        assert (ref.visible(Lq, Lk, causal, window) == mask.numpy()).all(), (Lq, Lk)
        live = mask.any(1).numpy()
        if live.any():
            want = _torch_seq(q[rows], k[k0:k0 + Lk], v[k0:k0 + Lk], mask, scale, H // Hkv).numpy()
            np.testing.assert_allclose(o[rows][live], want[live], rtol=1e-10, atol=1e-12)
            s = torch.einsum("ihd,jhd->hij", q[rows], k[k0:k0 + Lk].repeat_interleave(H // Hkv, 1)) * scale
            s = s.masked_fill(~mask[None], float("-inf"))
            np.testing.assert_allclose(lse[:, rows][:, live], torch.logsumexp(s, -1).numpy()[:, live], rtol=1e-12, atol=1e-12)
        # rows that see no key: O = 0 exactly, LSE = -inf
        assert (o[rows][~live] == 0).all() and np.isneginf(lse[:, rows][:, ~live]).all()


@pytest.mark.parametrize("window", [(0, 0), (5, 0), (5, 9), (-1, 3), (3, -1)])
def test_equal_lengths_is_the_dense_top_left_window(window):
    L = 70
    left, right = window
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    dense = ((left < 0) | (j >= i - left)) & ((right < 0) | (j <= i + right))
    assert (ref.visible(L, L, False, window) == dense).all()
    q, k, v, cu_q, cu_k = _case([L], [L], 2, 2, 8, seed=3)
    o, _ = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, False, window)
    want = _torch_seq(q, k, v, torch.from_numpy(dense), 8 ** -0.5, 1).numpy()
    np.testing.assert_allclose(o, want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("left", [0, 1, 17, 300])
def test_causal_left_unbounded_right_equals_right_zero(left):
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 2, 1, 8, seed=left)
    a = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, True, (left, -1))
    b = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, False, (left, 0))
    c = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, True, (left, 0))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("window", [(3, 2), (10, -1), (-1, 4)])
def test_backward_matches_torch_autograd(causal, window):
    lens_q, lens_k = [5, 0, 40, 17, 30], [9, 4, 40, 0, 12]
    H, Hkv = 4, 2
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, H, Hkv, 8, seed=11 + causal)
    do = torch.randn(q.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    dq, dk, dv = ref.backward(do.numpy(), q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, causal, window)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    outs = []
    for q0, Lq, k0, Lk in ref.seqs(cu_q, cu_k):
        if Lq == 0 or Lk == 0:
            continue
        mask = _formula_mask(Lq, Lk, causal, window)
        o = _torch_seq(qg[q0:q0 + Lq], kg[k0:k0 + Lk], vg[k0:k0 + Lk], mask, 8 ** -0.5, H // Hkv)
        outs.append((o.masked_fill(~mask.any(1)[:, None, None], 0.0).nan_to_num() * do[q0:q0 + Lq]).sum())
    torch.stack(outs).sum().backward()
    np.testing.assert_allclose(dq, qg.grad.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(dk, kg.grad.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(dv, vg.grad.numpy(), rtol=1e-9, atol=1e-11)
