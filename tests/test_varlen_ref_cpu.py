"""The fp64 varlen reference (tests/varlen_ref.py) against torch's own definitions, on the CPU: every sequence through
torch SDPA with torch.nn.attention.bias.causal_lower_right (bottom-right causal), grouped heads expanded, empty sequences."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.attention.bias import causal_lower_right

import varlen_ref as ref


def _case(lens_q, lens_k, H, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int64)
    cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int64)
    q = torch.randn(int(cu_q[-1]), H, D, generator=g, dtype=torch.float64)
    k = torch.randn(int(cu_k[-1]), Hkv, D, generator=g, dtype=torch.float64)
    v = torch.randn(int(cu_k[-1]), Hkv, D, generator=g, dtype=torch.float64)
    return q, k, v, cu_q, cu_k


def _torch_seq(q, k, v, causal, scale, G):
    """torch SDPA of one sequence ([L, H, D] -> [L, H, D]); bottom-right causal through causal_lower_right"""
    qh, kh, vh = (t.transpose(0, 1)[None] for t in (q, k, v))
    kh, vh = kh.repeat_interleave(G, 1), vh.repeat_interleave(G, 1)
    mask = causal_lower_right(q.shape[0], k.shape[0]) if causal else None
    return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=scale)[0].transpose(0, 1)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (8, 1)])
def test_forward_matches_torch_per_sequence(causal, H, Hkv):
    lens_q = [1, 31, 0, 128, 129, 50, 7, 64]
    lens_k = [1, 40, 5, 100, 129, 0, 7, 200]  # L_q > L_k, L_q < L_k, L_q == L_k, empty either side
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, H, Hkv, 16, seed=H * 10 + Hkv + causal)
    scale = 0.3
    o, lse = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, causal, scale)
    assert o.shape == tuple(q.shape) and lse.shape == (H, q.shape[0])
    for q0, Lq, k0, Lk in ref.seqs(cu_q, cu_k):
        if Lq == 0:
            continue
        rows = slice(q0, q0 + Lq)
        vis = ref.visible(Lq, Lk, causal)
        live = vis.any(1)
        if Lk > 0:
            want = _torch_seq(q[rows], k[k0:k0 + Lk], v[k0:k0 + Lk], causal, scale, H // Hkv).numpy()
            np.testing.assert_allclose(o[rows][live], want[live], rtol=1e-10, atol=1e-12)
            # LSE: torch.logsumexp of the masked scores
            s = torch.einsum("ihd,jhd->hij", q[rows], k[k0:k0 + Lk].repeat_interleave(H // Hkv, 1)) * scale
            s = s.masked_fill(~torch.from_numpy(vis)[None], float("-inf"))
            np.testing.assert_allclose(lse[:, rows][:, live], torch.logsumexp(s, -1).numpy()[:, live], rtol=1e-12, atol=1e-12)
        # rows that see no key: O = 0 exactly, LSE = -inf
        assert (o[rows][~live] == 0).all() and np.isneginf(lse[:, rows][:, ~live]).all()


def test_bottom_right_equals_top_left_when_lengths_match():
    q, k, v, cu_q, cu_k = _case([96, 33], [96, 33], 2, 2, 8, seed=3)
    o, _ = ref.forward(q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, causal=True)
    for q0, Lq, k0, Lk in ref.seqs(cu_q, cu_k):
        qh, kh, vh = (t[q0:q0 + Lq].transpose(0, 1)[None] for t in (q, k, v))
        want = F.scaled_dot_product_attention(qh, kh, vh, is_causal=True)[0].transpose(0, 1).numpy()
        np.testing.assert_allclose(o[q0:q0 + Lq], want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("causal", [False, True])
def test_backward_matches_torch_autograd(causal):
    lens_q, lens_k = [5, 0, 40, 17, 30], [9, 4, 40, 0, 12]
    H, Hkv = 4, 2
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, H, Hkv, 8, seed=11 + causal)
    do = torch.randn(q.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    dq, dk, dv = ref.backward(do.numpy(), q.numpy(), k.numpy(), v.numpy(), cu_q, cu_k, causal)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    outs = []
    for q0, Lq, k0, Lk in ref.seqs(cu_q, cu_k):
        if Lq == 0 or Lk == 0:
            continue
        vis = torch.from_numpy(ref.visible(Lq, Lk, causal))
        o = _torch_seq(qg[q0:q0 + Lq], kg[k0:k0 + Lk], vg[k0:k0 + Lk], causal, 8 ** -0.5, H // Hkv)
        outs.append((o.masked_fill(~vis.any(1)[:, None, None], 0.0).nan_to_num() * do[q0:q0 + Lq]).sum())
    torch.stack(outs).sum().backward()
    np.testing.assert_allclose(dq, qg.grad.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(dk, kg.grad.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(dv, vg.grad.numpy(), rtol=1e-9, atol=1e-11)
    # empty sides: dQ of a sequence without keys and dK / dV of one without queries are zero
    assert (dq[45:62] == 0).all() and (dk[9:13] == 0).all() and (dv[9:13] == 0).all()
