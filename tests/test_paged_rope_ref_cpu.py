"""The fp64 reference of the rotary KV-cache calls (tests/paged_rope_ref.py) pinned without a GPU: the rotation against the stored
fixtures of the reference's eager rope (tests/golden/rope.npz: interleaved pairs, full rotary_dim, positions 0 .. S - 1), the
non-interleaved form as the interleaved one under the column permutation, the pass-through tail, the position rules (causal or not, the
clamp of cache_seqlens, the clamp to the last table row), the rounding helper against numpy / torch, and the composition with the plain
references.

The fixture's y32 is the eager spec evaluated in fp32 (x cos + rotate_half(x) sin, every product and the sum rounded to fp32).  The
reference's formula evaluated at that working precision reproduces it to 1e-12 (in fact bit for bit); evaluated in fp64 it differs from it
by the fp32 roundings of the fixture alone, bounded here by 3 ulp_fp32 of |a| + |b|."""
import numpy as np
import pytest
import torch

import paged_ref
import paged_rope_ref as rr
import varlen_paged_ref


def _tables(rng, seqlen_ro, half):
    ang = rng.uniform(0, 2 * np.pi, (seqlen_ro, half))
    return np.cos(ang), np.sin(ang)


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_rotation_agrees_with_the_golden_fixture(golden_dir, name):
    g = np.load(golden_dir / "rope.npz")
    x = g[f"x_{name}_sd"]
    if name == "bf16":
        x = (x.astype(np.uint32) << 16).view(np.float32)
    x = x.astype(np.float32)
    cos, sin = g[f"cos_{name}_sd"][:, 0::2], g[f"sin_{name}_sd"][:, 0::2]  # pair-duplicated [S, D] -> [S, D / 2]
    S = x.shape[2]
    want = g[f"y32_{name}_sd"]
    pos = np.arange(S)[None, None, :]
    got32 = rr.rotate(x, cos, sin, pos, interleaved=True, dtype=np.float32)
    assert np.abs(got32.astype(np.float64) - want.astype(np.float64)).max() <= 1e-12
    got64 = rr.rotate(x, cos, sin, pos, interleaved=True)
    assert got64.dtype == np.float64
    bound = 3 * 2.0 ** -24 * rr.pair_magnitude(x, x.shape[-1], True)
    assert (np.abs(got64 - want) <= bound + 1e-30).all()


@pytest.mark.parametrize("rotary_dim", [64, 32, 16])
def test_non_interleaved_is_the_interleaved_form_under_the_column_permutation(rotary_dim):
    rng = np.random.default_rng(rotary_dim)
    D = 64
    x = rng.standard_normal((3, 5, 2, D))
    cos, sin = _tables(rng, 40, rotary_dim // 2)
    pos = rng.integers(0, 40, (3, 5))[:, :, None]
    perm = np.concatenate([np.stack([np.arange(rotary_dim // 2), np.arange(rotary_dim // 2) + rotary_dim // 2], 1).ravel(),
                           np.arange(rotary_dim, D)])  # pairs (i, i + rd / 2) laid side by side
    y_neox = rr.rotate(x, cos, sin, pos, interleaved=False)
    y_perm = rr.rotate(x[..., perm], cos, sin, pos, interleaved=True)
    assert (y_neox[..., perm] == y_perm).all()
    assert (y_neox[..., rotary_dim:] == x[..., rotary_dim:]).all()  # the tail passes through
    if rotary_dim < D:
        assert (y_perm[..., rotary_dim:] == x[..., rotary_dim:]).all()
    # a rotation: pair norms are kept
    ia, ib = rr.pair_index(D, rotary_dim, False)
    np.testing.assert_allclose(y_neox[..., ia] ** 2 + y_neox[..., ib] ** 2, x[..., ia] ** 2 + x[..., ib] ** 2, rtol=1e-12)


def test_single_pair_by_hand():
    cos, sin = np.array([[1.0], [0.0]]), np.array([[0.0], [1.0]])  # position 1: a quarter turn
    x = np.array([[3.0, 4.0]])
    assert (rr.rotate(x, cos, sin, [0]) == x).all()
    assert (rr.rotate(x, cos, sin, [1]) == np.array([[-4.0, 3.0]])).all()  # a' = -b, b' = a
    assert (rr.rotate(x, cos, sin, [7]) == np.array([[-4.0, 3.0]])).all()  # past the table: its last row


def test_position_rules():
    cap = 48
    sl = [0, 14, 47, -5, 10 ** 9]
    assert rr.positions(sl, 3, cap).tolist() == [[0, 1, 2], [14, 15, 16], [47, 48, 49], [0, 1, 2], [48, 49, 50]]
    assert rr.positions(sl, 3, cap, advance=False).tolist() == [[0] * 3, [14] * 3, [47] * 3, [0] * 3, [48] * 3]
    # packed: rows of sequence b at L0_b + (t - start_b); uncovered rows (past max_q, behind cu[B]) are not rotated
    cu = [0, 1, 5, 5, 7]
    pos, cov = rr.packed_positions(cu, 9, 3, [10, 20, 30, -1], cap)
    assert pos.tolist() == [10, 20, 21, 22, 0, 0, 1, 0, 0] and cov.tolist() == [True, True, True, True, False, True, True, False, False]
    pos, _ = rr.packed_positions(cu, 9, 3, [10, 20, 30, -1], cap, advance=False)
    assert pos.tolist() == [10, 20, 20, 20, 0, 0, 0, 0, 0]
    # the clamp to the table: seqlen_ro - 1 exactly, and one past it
    rng = np.random.default_rng(3)
    cos, sin = _tables(rng, 16, 8)
    x = rng.standard_normal((1, 2, 1, 16))
    at15 = rr.rotate(x, cos, sin, np.array([[15, 15]])[:, :, None])
    assert (rr.rotate(x, cos, sin, np.array([[15, 16]])[:, :, None]) == at15).all()
    assert (rr.rotate(x, cos, sin, np.array([[14, 15]])[:, :, None])[0, 0] != at15[0, 0]).any()


def test_operands_follow_causal_and_lengths():
    rng = np.random.default_rng(5)
    B, Sq, Sn, H, Hkv, D, ps = 2, 2, 5, 4, 2, 32, 16
    q, kn = rng.standard_normal((B, Sq, H, D)), rng.standard_normal((B, Sn, Hkv, D))
    kc = np.zeros((6, ps, Hkv, D))
    bt = np.arange(6).reshape(2, 3)
    cos, sin = _tables(rng, 64, 8)
    sl = [14, 60]  # 60 is clamped to the capacity 48
    for causal in (False, True):
        rq, rk = rr.operands(q, kn, kc, sl, cos, sin, bt, causal, False)
        for b, L0 in enumerate((14, 48)):
            for i in range(Sq):
                assert (rq[b, i] == rr.rotate(q[b, i], cos, sin, [L0 + (i if causal else 0)])).all()
            for t in range(Sn):
                assert (rk[b, t] == rr.rotate(kn[b, t], cos, sin, [L0 + t])).all()
        assert (rq[..., 16:] == q[..., 16:]).all()


@pytest.mark.parametrize("operand,tdt", [("bf16", torch.bfloat16), ("fp16", torch.float16)])
def test_round_operand_is_torchs_cast(operand, tdt):
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.standard_normal(20000) * 3, rng.standard_normal(2000) * 1e-6, [0.0, 1.0, -1.0, 1 + 2.0 ** -9, 1 + 3 * 2.0 ** -9,
                                                                                           1 + 2.0 ** -12, 1 + 3 * 2.0 ** -12]])
    x = x.astype(np.float32).astype(np.float64)  # fp32 values: torch rounds them once
    want = torch.tensor(x, dtype=torch.float32).to(tdt).double().numpy()
    assert (rr.round_operand(x, operand) == want).all()
    assert (rr.ulp(np.array([1.0, 1.5, 2.0, 0.75]), operand) == np.array([1.0, 1.0, 2.0, 0.5]) * 2.0 ** -(rr.SIG_BITS[operand] - 1)).all()


def test_whole_call_composes_with_the_plain_references():
    rng = np.random.default_rng(9)
    B, Sq, Sn, H, Hkv, D, ps = 2, 2, 2, 4, 2, 32, 16
    q, kn, vn = rng.standard_normal((B, Sq, H, D)), rng.standard_normal((B, Sn, Hkv, D)), rng.standard_normal((B, Sn, Hkv, D))
    kc, vc = rng.standard_normal((6, ps, Hkv, D)), rng.standard_normal((6, ps, Hkv, D))
    bt = rng.permutation(6).reshape(2, 3)
    cos, sin = _tables(rng, 64, 16)
    sl = [0, 14]
    o, lse, kc2, vc2 = rr.forward(q, kc, vc, sl, cos, sin, bt, kn, vn, causal=True, interleaved=True, operand="fp16")
    rq, rk = rr.operands(q, kn, kc, sl, cos, sin, bt, True, True)
    o2, lse2, kc3, vc3 = paged_ref.forward(rr.round_operand(rq, "fp16"), kc, vc, sl, bt, rr.round_operand(rk, "fp16"), vn, True)
    assert (o == o2).all() and (lse == lse2).all() and (kc2 == kc3).all() and (vc2 == vc3).all()
    assert (kc2[bt[1, 0], 14] == rr.round_operand(rk[1, 0], "fp16")).all() and (vc2[bt[1, 0], 14] == vn[1, 0]).all()  # V is not rotated
    # packed with equal lengths = the batched call
    cu = [0, 2, 4]
    op, lp, kcp, vcp = rr.forward_packed(q.reshape(4, H, D), kc, vc, cu, 2, sl, cos, sin, bt, kn.reshape(4, Hkv, D), vn.reshape(4, Hkv, D),
                                         causal=True, interleaved=True, operand="fp16")
    assert (op.reshape(B, Sq, H, D) == o).all() and (kcp == kc2).all() and (vcp == vc2).all()
    assert (lp.reshape(H, B, Sq).transpose(1, 0, 2) == lse).all()
    assert varlen_paged_ref.covered(cu, 4, 2).all()
