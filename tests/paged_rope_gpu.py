"""Helpers shared by tests/test_gpu_paged_rope.py and tests/test_gpu_varlen_paged_rope.py: rotary tables, the parent sequence (operands
rotated on the GPU by ops.rope_rotate, then the existing entries), and the format bounds of a rotated element."""
from __future__ import annotations

import numpy as np
import torch

import paged_rope_ref as rr

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def i32(vals):
    return torch.tensor(np.asarray(vals), dtype=torch.int32, device="cuda")


def tables(seqlen_ro, rotary_dim, dtype, seed, pad=0):
    """cos / sin [seqlen_ro, rotary_dim / 2] of random angles in `dtype` (fp32 or the operand type); pad > 0: rows of a wider buffer (a
    row stride that is not the row length)"""
    ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, (seqlen_ro, rotary_dim // 2))
    res = []
    for f in (np.cos, np.sin):
        t = torch.zeros(seqlen_ro, rotary_dim // 2 + pad, dtype=dtype, device="cuda")
        t[:, :rotary_dim // 2] = torch.tensor(f(ang), dtype=torch.float32, device="cuda").to(dtype)
        res.append(t[:, :rotary_dim // 2])
    return res


def rotate_by_ops(um, x, pos, cos, sin, interleaved):
    """the parent commit's rotation: x [B, S, h, D] (or packed [T, h, D] with pos [T]) rotated at pos [B, S] by ops.rope_rotate on the
    GPU -- per-sequence fp32 tables gathered at the (clamped) positions and pair-duplicated, x as a strided BHSD view, only the
    [:rotary_dim] slice rotated, the non-interleaved form through the column permutation into pairs and back.  Returns x's layout."""
    packed = x.dim() == 3
    if packed:
        x, pos = x[None], np.asarray(pos)[None]
    B, S, h, D = x.shape
    rd = 2 * cos.shape[1]
    p = torch.tensor(np.minimum(np.asarray(pos, np.int64), cos.shape[0] - 1), device="cuda")
    c = cos.float()[p].repeat_interleave(2, dim=-1).contiguous()  # [B, S, rd], pair-duplicated
    s = sin.float()[p].repeat_interleave(2, dim=-1).contiguous()
    xv = x.transpose(1, 2)[..., :rd]  # strided BHSD view of the rotary slice
    if not interleaved:
        perm = torch.stack([torch.arange(rd // 2), torch.arange(rd // 2) + rd // 2], 1).reshape(-1).cuda()
        xv = xv[..., perm].contiguous()
    y = um.ops.rope_rotate(xv, c, s)  # dense [B, h, S, rd]
    if not interleaved:
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(rd, device="cuda")
        y = y[..., inv]
    out = x.clone()
    out[..., :rd] = y.transpose(1, 2)
    return out[0] if packed else out


def rotation_bound(x, rotary_dim, interleaved, operand):
    """the issue's bound on |got - fp64| of a rotated element: half an ulp of the operand type at the pair's magnitude plus the fp32
    arithmetic; 0 on the pass-through tail (those elements are copied)"""
    m = rr.pair_magnitude(x, rotary_dim, interleaved)
    return 1.001 * 2.0 ** -8 * m if operand == "bf16" else np.where(m > 0, 1.001 * 2.0 ** -11 * m + 2.0 ** -25, 0.0)


def fp32_slack(x, rotary_dim, interleaved, operand):
    """the part of rotation_bound above half an ulp at the pair's magnitude: what the fp32 arithmetic may move a value by.  A 16-bit
    rounding tie closer to the fp64 value than this may round either way."""
    m = rr.pair_magnitude(x, rotary_dim, interleaved)
    return 0.001 * 2.0 ** -8 * m if operand == "bf16" else np.where(m > 0, 0.001 * 2.0 ** -11 * m + 2.0 ** -25, 0.0)


def check_rotated_rows(got, exact, src, rotary_dim, interleaved, operand, tag):
    """got: rows read back from the GPU (fp64 view of 16-bit values); exact: the fp64 rotation of src"""
    err = np.abs(got - exact)
    bound = rotation_bound(src, rotary_dim, interleaved, operand)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{tag}: rotated rows max err {float(err.max()) if err.size else 0.0:.3e}, worst err / bound {worst:.3f}")
    assert (err <= bound).all(), (tag, float(err.max()), worst)
