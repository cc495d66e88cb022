"""Packed variable-length attention on the 16-bit MFMA kernels: `umfa::varlen_forward` / `umfa::varlen_backward` custom ops (fake
implementations + autograd registered, so torch.compile(fullgraph=True) keeps them as single graph nodes) and `varlen_attention`, the
differentiable entry with the arguments and results of torch.nn.attention.varlen.varlen_attn.

Layout: query [T_q, H, D], key / value [T_k, H_kv, D] (H a multiple of H_kv: grouped-query attention), cu_seq_q / cu_seq_k device int32
[N + 1] of cumulative offsets; sequence n owns rows cu[n] .. cu[n+1]-1.  Strided views with a contiguous head_dim and token / head strides
that are multiples of 8 elements (qkv[:, 0] of a [T, 3, H, D] projection) go to the kernels without a copy.  Causal is bottom-right
aligned per sequence (query i sees key j iff j <= i + L_k - L_q), flash-attention's varlen convention.  The offsets never leave the
device: no call synchronises, and a captured graph follows their contents on replay.

Sliding window: `window_size=(left, right)`, flash-attention's convention, bottom-right per sequence -- query i sees key j iff
j >= i + (L_k - L_q) - left (left >= 0) and j <= i + (L_k - L_q) + right (right >= 0); -1 is unbounded on that side and causal sets
right = 0.  `umfa::varlen_window_forward` / `umfa::varlen_window_backward` run it; a window that bounds nothing (left >= max_k,
right >= max_q, or -1) takes the unwindowed ops, bit for bit.

Scope: fp16 / bf16 device tensors, head_dim 64 / 128.  Anything else raises ValueError: there is no fall-back.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops

VARLEN_HEAD_DIMS = (64, 128)
_DTYPES = (torch.float16, torch.bfloat16)


def _kernel_view(t: torch.Tensor) -> torch.Tensor:
    """t itself when the kernels can read it (contiguous head_dim, token / head strides multiples of 8, 16-byte aligned), else a copy"""
    s = t.stride()
    if s[2] == 1 and s[0] % 8 == 0 and s[1] % 8 == 0 and s[0] >= t.shape[2] and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def _check(query, key, value, cu_seq_q, cu_seq_k):
    ok = (query.dim() == 3 and key.dim() == 3 and value.dim() == 3 and query.is_cuda and key.is_cuda and value.is_cuda
          and query.dtype in _DTYPES and key.dtype == query.dtype and value.dtype == query.dtype
          and key.shape == value.shape and query.shape[2] == key.shape[2] and query.shape[2] in VARLEN_HEAD_DIMS
          and key.shape[1] > 0 and query.shape[1] % key.shape[1] == 0)
    if not ok:
        raise ValueError("varlen_attention: needs device fp16 / bf16 tensors query [T_q, H, D], key / value [T_k, H_kv, D] with H % H_kv == 0 "
                         f"and head_dim 64 or 128 (got {tuple(query.shape)} {query.dtype}, {tuple(key.shape)}, {tuple(value.shape)})")
    for name, cu in (("cu_seq_q", cu_seq_q), ("cu_seq_k", cu_seq_k)):
        if cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 1 or not cu.is_cuda:
            raise ValueError(f"varlen_attention: {name} must be a 1-D device int32 tensor of N + 1 offsets")
    if cu_seq_q.numel() != cu_seq_k.numel():
        raise ValueError("varlen_attention: cu_seq_q and cu_seq_k must hold the same number of sequences")


@torch.library.custom_op("umfa::varlen_forward", mutates_args=(), device_types="cuda")
def varlen_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seq_q: torch.Tensor, cu_seq_k: torch.Tensor, max_q: int,
                   max_k: int, is_causal: bool, scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """O [T_q, H, D] (q's dtype) and the fp32 log-sum-exp [H, T_q] (umfa_varlen_attention_forward_stream)."""
    return ops.varlen_attention_forward(_kernel_view(q), _kernel_view(k), _kernel_view(v), cu_seq_q.contiguous(), cu_seq_k.contiguous(),
                                        int(max_q), int(max_k), scale=float(scale), causal=bool(is_causal))


@varlen_forward.register_fake
def _(q, k, v, cu_seq_q, cu_seq_k, max_q, max_k, is_causal, scale):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_backward", mutates_args=(), device_types="cuda")
def varlen_backward(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, lse: torch.Tensor,
                    cu_seq_q: torch.Tensor, cu_seq_k: torch.Tensor, max_q: int, max_k: int, is_causal: bool,
                    scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """dQ [T_q, H, D], dK / dV [T_k, H_kv, D] in the operand dtype (umfa_varlen_attention_backward_stream)."""
    return ops.varlen_attention_backward(dout.to(q.dtype).contiguous(), _kernel_view(q), _kernel_view(k), _kernel_view(v), out.contiguous(),
                                         lse.contiguous(), cu_seq_q.contiguous(), cu_seq_k.contiguous(), int(max_q), int(max_k),
                                         scale=float(scale), causal=bool(is_causal))


@varlen_backward.register_fake
def _(dout, q, k, v, out, lse, cu_seq_q, cu_seq_k, max_q, max_k, is_causal, scale):
    return q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape)


def _setup_context(ctx, inputs, output):
    q, k, v, cu_seq_q, cu_seq_k, max_q, max_k, is_causal, scale = inputs
    out, lse = output
    ctx.save_for_backward(q, k, v, out, lse, cu_seq_q, cu_seq_k)
    ctx.max_q, ctx.max_k, ctx.is_causal, ctx.scale = int(max_q), int(max_k), bool(is_causal), float(scale)


def _backward(ctx, dout, dlse):
    q, k, v, out, lse, cu_seq_q, cu_seq_k = ctx.saved_tensors
    dq, dk, dv = torch.ops.umfa.varlen_backward(dout, q, k, v, out, lse, cu_seq_q, cu_seq_k, ctx.max_q, ctx.max_k, ctx.is_causal, ctx.scale)
    return dq, dk, dv, None, None, None, None, None, None


varlen_forward.register_autograd(_backward, setup_context=_setup_context)


@torch.library.custom_op("umfa::varlen_window_forward", mutates_args=(), device_types="cuda")
def varlen_window_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seq_q: torch.Tensor, cu_seq_k: torch.Tensor, max_q: int,
                          max_k: int, is_causal: bool, scale: float, window_left: int,
                          window_right: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_forward with a sliding window (umfa_varlen_attention_forward_window_stream)."""
    return ops.varlen_attention_forward(_kernel_view(q), _kernel_view(k), _kernel_view(v), cu_seq_q.contiguous(), cu_seq_k.contiguous(),
                                        int(max_q), int(max_k), scale=float(scale), causal=bool(is_causal),
                                        window=(int(window_left), int(window_right)))


@varlen_window_forward.register_fake
def _(q, k, v, cu_seq_q, cu_seq_k, max_q, max_k, is_causal, scale, window_left, window_right):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_window_backward", mutates_args=(), device_types="cuda")
def varlen_window_backward(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, lse: torch.Tensor,
                           cu_seq_q: torch.Tensor, cu_seq_k: torch.Tensor, max_q: int, max_k: int, is_causal: bool, scale: float,
                           window_left: int, window_right: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """varlen_backward with a sliding window (umfa_varlen_attention_backward_window_stream)."""
    return ops.varlen_attention_backward(dout.to(q.dtype).contiguous(), _kernel_view(q), _kernel_view(k), _kernel_view(v), out.contiguous(),
                                         lse.contiguous(), cu_seq_q.contiguous(), cu_seq_k.contiguous(), int(max_q), int(max_k),
                                         scale=float(scale), causal=bool(is_causal), window=(int(window_left), int(window_right)))


@varlen_window_backward.register_fake
def _(dout, q, k, v, out, lse, cu_seq_q, cu_seq_k, max_q, max_k, is_causal, scale, window_left, window_right):
    return q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape)


def _setup_context_window(ctx, inputs, output):
    _setup_context(ctx, inputs[:9], output)
    ctx.window = (int(inputs[9]), int(inputs[10]))


def _backward_window(ctx, dout, dlse):
    q, k, v, out, lse, cu_seq_q, cu_seq_k = ctx.saved_tensors
    dq, dk, dv = torch.ops.umfa.varlen_window_backward(dout, q, k, v, out, lse, cu_seq_q, cu_seq_k, ctx.max_q, ctx.max_k, ctx.is_causal,
                                                       ctx.scale, *ctx.window)
    return dq, dk, dv, None, None, None, None, None, None, None, None


varlen_window_forward.register_autograd(_backward_window, setup_context=_setup_context_window)


def _window(window_size, is_causal: bool, max_q: int, max_k: int) -> Tuple[int, int]:
    """window_size normalised as the C entries do it: causal sets right = 0, a side that cannot bound any row (left >= max_k,
    right >= max_q) is -1; a value below -1 is a ValueError"""
    try:
        left, right = (int(w) for w in window_size)
    except (TypeError, ValueError):
        raise ValueError(f"varlen_attention: window_size must be a pair of ints (got {window_size!r})") from None
    if left < -1 or right < -1:
        raise ValueError(f"varlen_attention: window_size values must be >= -1 (-1: unbounded), got {(left, right)}")
    if is_causal:
        right = 0
    if left >= max_k:
        left = -1
    if right >= max_q:
        right = -1
    return left, right


def varlen_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, cu_seq_q: torch.Tensor, cu_seq_k: torch.Tensor,
                     max_q: int, max_k: int, is_causal: bool = False, *, scale: Optional[float] = None, return_lse: bool = False,
                     window_size: Tuple[int, int] = (-1, -1)):
    """softmax(q k^T scale [bottom-right causal]) v per packed sequence -- differentiable in query, key and value.  Returns O [T_q, H, D]
    in query's dtype, or (O, LSE [H, T_q] fp32, natural log) with return_lse.  A row that sees no key (L_k = 0, causal with L_q > L_k,
    or outside its window) gives O = 0 and LSE = -inf.  max_q / max_k: the longest query / key sequence (host ints; rows past them are
    not computed).  window_size: (left, right) sliding window, flash-attention's convention (see the module docstring).
    Raises ValueError outside the kernels' scope (see the module docstring)."""
    _check(query, key, value, cu_seq_q, cu_seq_k)
    left, right = _window(window_size, bool(is_causal), int(max_q), int(max_k))
    sm = float(scale) if scale is not None else float(query.shape[-1]) ** -0.5
    if left == -1 and right in (-1, 0):  # no band: the unwindowed kernels ((-1, 0) is bottom-right causal)
        out, lse = torch.ops.umfa.varlen_forward(query, key, value, cu_seq_q, cu_seq_k, int(max_q), int(max_k), right == 0, sm)
    else:
        out, lse = torch.ops.umfa.varlen_window_forward(query, key, value, cu_seq_q, cu_seq_k, int(max_q), int(max_k), bool(is_causal), sm,
                                                        left, right)
    return (out, lse) if return_lse else out
